"""Threshold hillslopes on the device (include/soil_hip.h: soil_slope_limit, soil_slope_limit_batch; soil.slope_limit /
slope_limit_batch, ErosionBatch.slope_limited / evolve_limited), every cell bit for bit against the Jacobi restatement
of tests/slope_limit_ref.py, the small cases against its Dijkstra as well.  Everything compared is a float32 word, the
NaN words included: there is no tolerance anywhere.  The inputs are those of tests/test_slope_limit_abi.py, which holds
the two restatements to each other and every input to its share of lowered cells.

  shapes     1x1, 1x7, 5x1; 63x65, 64x64, 65x129, 130x67: ragged tiles on either axis, exactly one tile, a one-cell
             sliver of a tile; D4 and D8, anisotropic scales, scalar slope and slope plane, with and without excess
  reach      a single pit in a 200x200 plateau, mid-tile and in a tile corner: its cone crosses three tiles each way
  launches   a serpentine corridor between NaN walls on 130x130, across the whole grid and wound inside bands a tile
             wide (2000 cells of it in one tile: the inner cap), in child processes with one and with 1000 launches a
             look: convergence, the launch bound, the looks
  hostile    NaN voids and walls, +-0, denormal heights and steps, +-inf, +-3e38, slope entries NaN / negative / +inf /
             0, a scalar slope of 0 — on tile corners, tile edges and in the apron of a neighbouring tile
  batches    B = 3 of 65x129 (the plateau pit beside two smooth models) with a pair of scales per model, every slice
             against its single call; the corridor, and a hostile model, between two benign ones; B = 5 of 130x67: not
             cut into chunks
  batch class  ErosionBatch.slope_limited, evolve_limited against the composition, evolve as it was
  alignment  planes 4 bytes off their alignment (the kernel has no vector-load path; the scalar path must not care)
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import slope_limit_ref as ref
from slope_limit_ref import D4, D8
from util import product_param, script_param, terrain, to_gpu, to_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_CHECK = int(os.environ.get("SOIL_SLOPE_LIMIT_PER_CHECK", "3"))   # launches a look at the "changed" word (docs/KNOBS.md)


def bound(tiles, per_check=PER_CHECK):
    """The launches no legal input exceeds (csrc/slope_limit.hip), and the overshoot of the last group."""
    return tiles * (4 * 64 + 16) + 2 + per_check - 1


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    assert got.shape == want.shape, what
    bad = _bits(got) != _bits(want)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d words differ, first at %s: %r vs %r" % (what, bad.sum(), bad.size, at, got[at], want[at]))


def _slope(slope):
    return to_gpu(slope) if isinstance(slope, np.ndarray) else slope


def _run(h, scale, slope, edge, excess=False, batch=False):
    from soillib_amd import soil
    fn = soil.slope_limit_batch if batch else soil.slope_limit
    out = fn(to_gpu(h), scale, _slope(slope), edge, excess)
    return tuple(to_np(t) for t in out) if excess else to_np(out)


def _check_case(key, dijkstra=False):
    from soillib_amd import soil
    h, scale, slope, edge = ref.case(key)
    want = ref.reference(key)
    got, ex = _run(h, scale, slope, edge, excess=True)
    info = soil.slope_limit_info()
    _same(got, want, "%r" % (key,))
    _same(ex, ref.excess(h, want), "%r: excess" % (key,))
    H, W = h.shape
    tiles = -(-H // 64) * -(-W // 64)
    assert info["tiles"] == tiles and info["models"] == 1
    assert PER_CHECK <= info["launches"] == PER_CHECK * info["looks"] <= bound(tiles)
    _same(_run(h, scale, slope, edge), want, "%r without excess" % (key,))
    if dijkstra:
        _same(got, ref.dijkstra(h, scale, slope, edge), "%r against Dijkstra" % (key,))
    return info


# ------------------------------------------------------------------ plain shapes

@pytest.mark.parametrize("plane", [False, True])
@pytest.mark.parametrize("edge", [D4, D8])
@pytest.mark.parametrize("shape", ref.TERRAIN_SHAPES)
def test_terrain_shapes(hip, shape, edge, plane):
    _check_case(("terrain", shape, edge, plane), dijkstra=shape == (63, 65))


@pytest.mark.parametrize("edge", [D4, D8])
@pytest.mark.parametrize("shape", ref.TINY_SHAPES)
def test_tiny_shapes(hip, shape, edge):
    _check_case(("tiny", shape, edge), dijkstra=True)


# ------------------------------------------------------------------ reach across tiles

@pytest.mark.parametrize("corner", [False, True])
def test_a_single_pit_in_a_plateau_reaches_across_tiles(hip, corner):
    """Every tile holds its constraints in the first launch and none of them is inert: the dirty marks carry the cone
    through tiles in which nothing moved at first, one ring of tiles a launch."""
    key = ("reach", corner)
    info = _check_case(key)
    h, want = ref.case(key)[0], ref.reference(key)
    assert (want < h).sum() == h.size - 1, "the cone takes the whole grid"
    assert info["looks"] >= 2, "the first launches moved tiles: a second look had to follow"


# ------------------------------------------------------------------ the serpentine, in child processes

def _child_main(path):
    from soillib_amd import soil
    out = {}
    for name in ("serpentine", "banded"):
        out[name] = _run(*ref.case((name,)))
        info = soil.slope_limit_info()
        out[name + "_info"] = np.array([info[k] for k in ("launches", "tiles", "models", "looks")])
    np.savez(path, **out)


@pytest.mark.parametrize("per_check", [1, 1000])
def test_the_serpentine_corridor_over_many_launches(hip, tmp_path, per_check):
    """Two ways of more than 8000 cells: one over seams in series (every corridor row crosses the grid), one wound
    inside bands a tile wide, some 2000 cells of it inside one tile — many times the inner cap, with nothing moving in
    the tiles around.  The call converges, the launches stay under the documented bound, and the looks are what the
    knob implies — one a launch with SOIL_SLOPE_LIMIT_PER_CHECK=1; with 1000, more than the launches that move
    anything, the first look sees a change and the second none."""
    path = str(tmp_path / "serpentine.npz")
    env = dict(os.environ)
    env["SOIL_SLOPE_LIMIT_PER_CHECK"] = str(per_check)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, "%s\n%s" % (r.stdout[-3000:], r.stderr[-3000:])
    got = np.load(path)
    for name in ("serpentine", "banded"):
        want = ref.reference((name,))
        assert (want < ref.case((name,))[0]).sum() > 8000
        _same(got[name], want, "%s, %d launches a look" % (name, per_check))
        launches, tiles, models, looks = got[name + "_info"].tolist()
        print("%s: %d launches, %d looks at %d a look" % (name, launches, looks, per_check))
        assert (tiles, models) == (9, 1) and launches == per_check * looks
        assert launches <= bound(9, per_check)
        if per_check == 1:
            assert 20 <= launches < 1000, "tens of launches in series, and fewer than the other case's launches a look"
        else:
            assert looks == 2


# ------------------------------------------------------------------ hostile cells

@pytest.mark.parametrize("name", sorted(ref.hostile_cases()), ids=lambda n: n.replace(" ", "_"))
def test_hostile_cells(hip, name):
    _check_case(("hostile", name))


def test_planes_off_their_alignment(hip):
    from soillib_amd import _abi
    key = ("terrain", (65, 129), D8, True)
    h, scale, slope, edge = ref.case(key)
    H, W = h.shape

    def shifted(arr=None):
        flat = np.zeros(H * W + 4, np.float32)
        if arr is not None:
            flat[1:1 + H * W] = arr.reshape(-1)
        buf = to_gpu(flat)
        assert buf.ptr % 16 == 0
        return buf, buf.ptr + 4
    (hb, hp), (sb, sp), (ob, op), (eb, ep) = shifted(h), shifted(slope), shifted(), shifted()
    import ctypes as C
    sc = (C.c_float * 2)(*scale)
    _abi.check(hip.soil_slope_limit(op, ep, hp, sp, 0.0, H, W, sc, edge, _abi.stream()))
    want = ref.reference(key)
    _same(to_np(ob)[1:1 + H * W].reshape(H, W), want, "out 4 bytes off")
    _same(to_np(eb)[1:1 + H * W].reshape(H, W), ref.excess(h, want), "excess 4 bytes off")


# ------------------------------------------------------------------ batches

@pytest.mark.parametrize("plane", [False, True])
@pytest.mark.parametrize("edge", [D4, D8])
def test_a_batch_of_three_with_a_pair_of_scales_each(hip, edge, plane):
    from soillib_amd import soil
    hs, scales, sl = ref.pit_batch()
    slope = sl if plane else 1.0
    singles, launches = [], []
    for b in range(3):
        singles.append(_run(hs[b], scales[b], slope[b] if plane else slope, edge, excess=True))
        launches.append(soil.slope_limit_info()["launches"])
        _same(singles[b][0], ref.jacobi(hs[b], scales[b], slope[b] if plane else slope, edge), "model %d alone" % b)
    got, ex = _run(hs, scales, slope, edge, excess=True, batch=True)
    info = soil.slope_limit_info()
    for b in range(3):
        _same(got[b], singles[b][0], "model %d of the batch" % b)
        _same(ex[b], singles[b][1], "model %d of the batch: excess" % b)
    print("launches alone %r, together %d" % (launches, info["launches"]))
    assert info["models"] == 3 and info["tiles"] == 6
    # the launches of the model that needs most (a tile may or may not see what its neighbour wrote in the same launch:
    # a launch more or less), not the sum
    assert info["launches"] <= max(launches) + PER_CHECK and info["launches"] < sum(launches)
    # one scale pair for all
    got1 = _run(hs, scales[0], slope, edge, batch=True)
    for b in range(3):
        _same(got1[b], ref.jacobi(hs[b], scales[0], slope[b] if plane else slope, edge), "one pair, model %d" % b)


def test_a_model_that_needs_many_more_launches_between_two_that_need_few(hip):
    """The corridor between two smooth models: one changed word serves the batch, so the launches go on for as long as
    any model moves — those of the corridor alone, not those of the last model, and not the sum."""
    from soillib_amd import soil
    h, scale, slope, edge = ref.serpentine_case()
    benign = ref.smooth(130, 130, 6)
    launches = []
    for m in (benign, h):
        _run(m, scale, slope, edge)
        launches.append(soil.slope_limit_info()["launches"])
    got = _run(np.stack([benign, h, benign]), scale, slope, edge, batch=True)
    info = soil.slope_limit_info()
    print("launches alone %r, together %d" % (launches, info["launches"]))
    _same(got[1], ref.reference(("serpentine",)), "the corridor in the middle")
    want = ref.jacobi(benign, scale, slope, edge)
    _same(got[0], want, "the model before")
    _same(got[2], want, "the model after")
    # (a tile may or may not see what its neighbour wrote in the same launch: the count is not the same to the launch)
    assert launches[0] + 20 <= info["launches"] <= launches[1] + launches[1] // 4 + PER_CHECK


def test_a_hostile_model_between_two_benign_ones(hip):
    cases = ref.hostile_cases()
    benign = ref.smooth(130, 130, 5)
    for name in ("inf", "nan", "slope 0"):
        h, scale, slope, edge = cases[name]
        hs = np.stack([benign, h, benign])
        got = _run(hs, scale, slope, edge, batch=True)
        _same(got[1], ref.reference(("hostile", name)), "the hostile model %r" % name)
        want = ref.jacobi(benign, scale, slope, edge)
        _same(got[0], want, "the model before %r" % name)
        _same(got[2], want, "the model after %r" % name)
        assert np.isfinite(got[0]).all()


def test_a_batch_of_five_is_one_call_whatever_the_chunk_knob_says(hip, monkeypatch):
    """The entry never cuts a batch into chunks (a model's offset is taken in int64 in the kernel): the info call
    reports all five models, also under a SOIL_FLOW_BATCH_CELLS that would cut the chunking entries."""
    from soillib_amd import soil
    monkeypatch.setenv("SOIL_FLOW_BATCH_CELLS", str(130 * 67))
    H, W = 130, 67
    hs = np.stack([ref.smooth(H, W, 20 + b) for b in range(5)])
    got = _run(hs, ref.SCALES, ref.TERRAIN_SLOPE, D8, batch=True)
    info = soil.slope_limit_info()
    assert info["models"] == 5 and info["tiles"] == 6
    for b in range(5):
        _same(got[b], ref.jacobi(hs[b], ref.SCALES, ref.TERRAIN_SLOPE, D8), "model %d" % b)


# ------------------------------------------------------------------ through the batch object

def test_the_batch_methods(hip, oracle):
    """ErosionBatch.slope_limited is slope_limit_batch of its height; evolve_limited is stream_power, then
    slope_limit_batch, then diffuse_batch, bit for bit; evolve is what it was; the batch's planes stay as they are."""
    from soillib_amd import silt, soil
    from soillib_amd.erosion import ErosionBatch
    B, H, W = 3, 64, 64
    prm = product_param(script_param(oracle.default_param()))
    prm.maxage = 32
    scales = [(20.0 / H * (1 + b), 20.0 / W, 4.0) for b in range(B)]
    layers = np.stack([terrain(oracle, H, W, seed=3.0 + 5.0 * b, sediment=0.05, rng_seed=b) for b in range(B)])
    splane = to_gpu(np.random.default_rng(4).uniform(0.05, 0.3, (B, H, W)).astype(np.float32))
    for scale in ((20.0 / H, 20.0 / W, 4.0), scales):
        bt = ErosionBatch(B, H, W, scale, prm, 256, [11 + 7 * b for b in range(B)])
        bt.set_layers(to_gpu(layers))
        silt.set(bt.rainfall, 1.0)
        bt.step()
        before = {n: to_np(getattr(bt, n)).copy() for n in ("height", "layers", "rainfall")}
        pairs = [list(s[:2]) for s in scales] if scale is scales else list(scale[:2])
        per_model = pairs if scale is scales else [pairs] * B
        for slope, edge in ((0.1, None), (splane, soil.d4)):
            got, ex = (to_np(t) for t in bt.slope_limited(slope, edge=edge, excess=True))
            e = D8 if edge is None else D4
            for b in range(B):
                s = to_np(slope)[b] if slope is splane else slope
                want = ref.jacobi(before["height"][b], per_model[b], s, e)
                _same(got[b], want, "slope_limited, model %d" % b)
                _same(ex[b], ref.excess(before["height"][b], want), "slope_limited excess, model %d" % b)
            assert 0.0 < ref.lowered_share(before["height"], got) < 1.0
        for kw in (dict(), dict(m=0.4, edge=soil.d4, first_axis=1)):
            sp = {k: v for k, v in kw.items() if k != "first_axis"}
            carved = bt.stream_power(25.0, 1e-3, **sp)
            # evolve, as before this method existed
            want = to_np(soil.diffuse_batch(carved, pairs, 25.0, kappa=0.02, border="fixed", first_axis=kw.get("first_axis", 0)))
            _same(to_np(bt.evolve(25.0, 1e-3, kappa=0.02, **kw)), want, "evolve(%r)" % sorted(kw))
            for slope in (0.1, splane):
                limited = soil.slope_limit_batch(carved, pairs, slope, kw.get("edge", soil.d8))
                want_l = to_np(soil.diffuse_batch(limited, pairs, 25.0, kappa=0.02, border="fixed", first_axis=kw.get("first_axis", 0)))
                got = to_np(bt.evolve_limited(25.0, 1e-3, slope, kappa=0.02, **kw))
                _same(got, want_l, "evolve_limited(%r)" % sorted(kw))
                assert (to_np(limited) < to_np(carved)).any() and (_bits(got) != _bits(want)).any(), "the threshold binds"
        for n, v in before.items():
            _same(to_np(getattr(bt, n)).reshape(v.shape), v, "the batch's %s is not touched" % n)


if __name__ == "__main__":
    _child_main(sys.argv[1])
