"""Exact multiple-flow accumulation on the device (include/soil_hip.h: soil_mfd_weights, soil_mfd_accumulate and their
_batch forms; soil.mfd_weights / mfd_accumulate, ErosionBatch.drainage_mfd), every cell word for word against the numpy
restatement of tests/mfd_ref.py: the shares (float32), out64 (float64) and out (float32), the NaN words included.
There is no tolerance anywhere but in the one statistical test.  The Gibbs weights of the restatement come from the
device's own rw_exp2 (soil_selftest_math op 12), the powers from its sp_pow (soil_selftest_math64 op 0).

  shapes     1x1, 5x7, 64x64, 65x65 (four tiles, a corner seam), 66x130, 130x66, 129x129; D4 and D8;
             T in {1, 10, 1e4}, p in {0, 1, 1.1, 4}
  flats      a filled DEM with and without `dist`
  hostile    NaN, +-inf, +-3e38 and +-0 heights on seams and corners; NaN, +-inf and +-0 sources
  chains     the serpentine through every cell of one tile (sixteen times the inner cap), a serpentine over 129x129,
             a staircase through a tile corner, and a long chain that leaves its tile through the corner
             (the diagonal wake-up)
  calls      planes 4 bytes off their alignment, a second stream, SOIL_MFD_PER_CHECK 1 and 7 in child processes
  batches    3 x 65 x 70 with a pair of scales per model and a hostile model between two benign ones; 65 540 models
             of 2 x 3
  statistics the library's own random_weighted + accumulate, K = 1024 at 48 x 48
  batch class  ErosionBatch.drainage_mfd against the composed single calls
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mfd_ref as ref
from mfd_ref import D4, D8
from util import product_param, script_param, terrain, to_gpu, to_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_CHECK = int(os.environ.get("SOIL_MFD_PER_CHECK", "4"))   # launches a look at the "changed" word (docs/KNOBS.md)
SHAPES = [(1, 1), (5, 7), (64, 64), (65, 65), (66, 130), (130, 66), (129, 129)]
SCALE = (1.5, 2.0)
KINDS = [dict(T=1.0), dict(T=10.0), dict(T=1e4), dict(p=0.0, scale=SCALE), dict(p=1.0, scale=SCALE),
         dict(p=1.1, scale=SCALE), dict(p=4.0, scale=SCALE)]


def bound(tiles, per_check=PER_CHECK):
    """The launches no input exceeds (csrc/mfd.hip), and the overshoot of the last group."""
    return tiles * (4 * 64 + 16) + 2 + per_check - 1


def dev_exp2(a, b):
    """rw_exp2(a, b) on the device, element by element (soil_selftest_math op 12)."""
    from soillib_amd import _abi
    a = np.ascontiguousarray(np.broadcast_to(a, np.broadcast(a, b).shape), np.float32)
    b = np.ascontiguousarray(np.broadcast_to(b, a.shape), np.float32)
    ga, gb, out = to_gpu(a.ravel()), to_gpu(b.ravel()), to_gpu(np.zeros(a.size, np.float32))
    _abi.check(_abi.lib().soil_selftest_math(out.c_ptr, ga.c_ptr, gb.c_ptr, a.size, 12, _abi.stream()))
    return to_np(out).reshape(a.shape)


def dev_pow(S, e):
    """sp_pow(S, e) on the device (soil_selftest_math64 op 0)."""
    from soillib_amd import _abi, silt
    S, e = np.ascontiguousarray(S, np.float64), np.ascontiguousarray(e, np.float64)
    out = silt.tensor(silt.float64, silt.shape(S.size), silt.gpu)
    a, b = to_gpu(S.reshape(-1)), to_gpu(e.reshape(-1))
    _abi.check(_abi.lib().soil_selftest_math64(out.c_ptr, a.c_ptr, b.c_ptr, S.size, 0, _abi.stream()))
    return to_np(out).reshape(S.shape)


def want_weights(h, edge, kind, dist=None):
    return ref.weights(h, edge, dist=dist, exp2=dev_exp2, pow_=dev_pow, **kind)


def _opt(a):
    return None if a is None else to_gpu(a)


def run(h, source, edge, kind, dist=None):
    """(weights, out64, out) of the device for numpy planes, (H, W) or (B, H, W)."""
    from soillib_amd import soil
    batch = h.ndim == 3
    wf, af = (soil.mfd_weights_batch, soil.mfd_accumulate_batch) if batch else (soil.mfd_weights, soil.mfd_accumulate)
    gh, gs, gd = to_gpu(h), _opt(source), _opt(dist)
    w = to_np(wf(gh, edge, dist=gd, **kind))
    a64 = to_np(af(gh, gs, edge, dist=gd, double=True, **kind))
    a32 = to_np(af(gh, gs, edge, dist=gd, **kind))
    return w, a64, a32


def check(h, source, edge, kind, dist=None, what="", want=None):
    """One model against the restatement (or a closed form `want`); returns the call's info."""
    from soillib_amd import soil
    w, a64, a32 = run(h, source, edge, kind, dist)
    info = soil.mfd_info()
    ww = want_weights(h, edge, kind, dist)
    ref.same(w, ww, "%s: weights" % what)
    if want is None:
        want = ref.accumulate(ww, source)[0]
    ref.same(a64, want, "%s: out64" % what)
    ref.same(a32, want.astype(np.float32), "%s: out" % what)
    H, W = h.shape
    tiles = -(-H // 64) * -(-W // 64)
    assert info["tiles"] == tiles and info["models"] == 1
    assert PER_CHECK <= info["launches"] == PER_CHECK * info["looks"] <= bound(tiles)
    return info


# ------------------------------------------------------------------ shapes, edges, kinds

@pytest.mark.parametrize("edge", [D4, D8])
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes(hip, shape, edge):
    h = ref.fractal(*shape, seed=3 + shape[0])
    src = np.random.default_rng(shape[1]).random(shape).astype(np.float32)
    for i, kind in enumerate(KINDS):
        check(h, src if i % 2 else None, edge, kind, what="%r %r" % (shape, kind))


def test_the_power_function_is_the_pow_the_restatement_assumes(hip):
    S = np.array([0.5, 1.0, 2.0, 1e-3, 37.5, np.inf])
    for p in (0.0, 1.0, 1.1, 4.0):
        got = dev_pow(S, np.full(S.shape, p))
        assert np.allclose(got[:-1], np.power(S[:-1], p), rtol=1e-14) and got[-1] == (1.0 if p == 0 else np.inf)


# ------------------------------------------------------------------ flats

@pytest.mark.parametrize("edge", [D4, D8])
def test_a_filled_dem_with_and_without_dist(hip, edge):
    from soillib_amd import soil
    h = ref.fractal(66, 130, seed=11, amplitude=60.0)
    h[30, 70] = np.nan
    filled_t = soil.fill_depressions(to_gpu(h), edge)
    filled, dist = to_np(filled_t), to_np(soil.flat_distance(filled_t, edge))
    assert (dist > 0).sum() > 20, "the fill made flats"
    for kind in (dict(T=10.0), dict(p=1.1, scale=SCALE)):
        check(filled, None, edge, kind, what="filled, no dist")
        check(filled, None, edge, kind, dist=dist, what="filled, dist")
    w = want_weights(filled, edge, dict(T=10.0), dist)
    term = ~(w != 0).any(0)
    nan = np.isnan(filled)
    beside = nan.copy()
    for k in range(ref.k_of(edge)):
        beside |= ref.shifted(nan, k, False)
    border = np.zeros_like(term)
    border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
    assert (term <= (border | beside)).all()


# ------------------------------------------------------------------ hostile cells

@pytest.mark.parametrize("edge", [D4, D8])
@pytest.mark.parametrize("shape", [(70, 66), (129, 129)])
def test_hostile_cells(hip, shape, edge):
    h, src = ref.hostile(*shape), ref.hostile_source(*shape)
    for kind in (dict(T=10.0), dict(T=1.0), dict(p=0.0, scale=SCALE), dict(p=4.0, scale=SCALE)):
        check(h, src, edge, kind, what="hostile %r %r" % (shape, kind))
    check(h, src, edge, dict(T=0.0), what="T = 0", want=ref._start(src.astype(np.float64))[1:-1, 1:-1].copy())
    cold = want_weights(ref.fractal(*shape), edge, dict(T=1e-3))
    assert (cold.sum(0) == 0).mean() > 0.5, "Z overflows at a small T: terminals"
    check(ref.fractal(*shape), None, edge, dict(T=1e-3), what="T = 1e-3")


# ------------------------------------------------------------------ chains

def test_the_serpentine_in_one_tile(hip):
    """4096 cells in a row inside one tile, sixteen times the inner cap: the tile stops at the cap sixteen times and has
    to mark itself dirty each time, nothing around it moves."""
    h, dist, pos = ref.snake(64, 64)
    info = check(h, None, D4, dict(T=10.0), dist=dist, what="serpentine", want=pos.astype(np.float64))
    assert info["launches"] >= 17


def test_a_serpentine_over_129_by_129(hip):
    h, dist, pos = ref.snake(129, 129)
    info = check(h, None, D4, dict(T=10.0), dist=dist, what="serpentine 129", want=pos.astype(np.float64))
    assert info["launches"] >= 129 * 129 // 256


def test_a_staircase_through_a_tile_corner(hip):
    """(63, 63) -> (64, 64): the chain leaves a tile through its corner."""
    h, dist = ref.staircase(129, 129, 129)
    want = ref.accumulate(ref.weights(h, D8, T=10.0, dist=dist))[0]
    assert want[100, 100] == 101.0 and want[127, 128] == 130.0
    check(h, None, D8, dict(T=10.0), dist=dist, what="staircase")


def test_the_diagonal_wake_up(hip):
    """ref.corner_chain: a pulse crosses the first tile in sixteen launches and leaves it through its corner; the
    diagonal tile is quiet by then and nothing but the diagonal neighbour's mark wakes it
    (tests/test_mfd_abi.py shows that a wake-up from four neighbours loses this input)."""
    h, dist, src, want = ref.corner_chain()
    info = check(h, src, D8, dict(T=10.0), dist=dist, what="corner chain", want=want)
    assert info["launches"] >= 20


# ------------------------------------------------------------------ alignment, streams, knobs

def test_planes_off_their_alignment(hip):
    from soillib_amd import _abi
    H, W, K = 65, 70, 8
    h, src = ref.fractal(H, W, seed=9), np.random.default_rng(1).random((H, W)).astype(np.float32)
    dist = np.zeros((H, W), np.int32)

    def shifted(arr, n=H * W, dtype=np.float32):
        flat = np.zeros(n * (2 if dtype == np.float64 else 1) + 4, np.float32 if dtype != np.int32 else np.int32)
        if arr is not None:
            flat[1:1 + n] = arr.reshape(-1)
        buf = to_gpu(flat)
        assert buf.ptr % 16 == 0
        return buf, buf.ptr + 4
    (hb, hp), (sb, sp), (db, dp) = shifted(h), shifted(src), shifted(dist, dtype=np.int32)
    (wb, wp), (ob, op), (o64b, o64p) = shifted(None, K * H * W), shifted(None), shifted(None, dtype=np.float64)
    sc = (C.c_float * 2)(*SCALE)
    o64p += 4                                                          # (a double plane: 8 bytes off its 16)
    _abi.check(hip.soil_mfd_weights(wp, hp, dp, 1, 1.1, H, W, sc, D8, _abi.stream()))
    _abi.check(hip.soil_mfd_accumulate(op, o64p, hp, sp, dp, 1, 1.1, H, W, sc, D8, _abi.stream()))
    ww = want_weights(h, D8, dict(p=1.1, scale=SCALE), dist)
    want = ref.accumulate(ww, src)[0]
    ref.same(to_np(wb)[1:1 + K * H * W].reshape(K, H, W), ww, "weights 4 bytes off")
    ref.same(to_np(ob)[1:1 + H * W].reshape(H, W), want.astype(np.float32), "out 4 bytes off")
    ref.same(to_np(o64b)[2:2 + 2 * H * W].view(np.float64).reshape(H, W), want, "out64 8 bytes off")


def test_on_a_second_stream(hip):
    import torch
    from soillib_amd import _abi
    h = ref.fractal(66, 130, seed=5)
    small = ref.fractal(5, 7, seed=5)
    s = torch.cuda.Stream()
    _abi.set_stream(s.cuda_stream)
    try:
        for plane in (h, small, h):
            check(plane, None, D8, dict(T=10.0), what="second stream")
    finally:
        _abi.set_stream(0)


def _child_main(path):
    from soillib_amd import soil
    out = {}
    h, dist, _ = ref.snake(64, 64)
    for name, (plane, d) in (("snake", (h, dist)), ("terrain", (ref.fractal(130, 66, seed=2), None))):
        out[name] = to_np(soil.mfd_accumulate(to_gpu(plane), None, D4 if d is not None else D8, T=10.0, dist=_opt(d), double=True))
        info = soil.mfd_info()
        out[name + "_info"] = np.array([info[k] for k in ("launches", "tiles", "models", "looks")])
    np.savez(path, **out)


@pytest.mark.parametrize("per_check", [1, 7])
def test_launches_per_look(hip, tmp_path, per_check):
    path = str(tmp_path / "mfd.npz")
    env = dict(os.environ)
    env["SOIL_MFD_PER_CHECK"] = str(per_check)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, "%s\n%s" % (r.stdout[-3000:], r.stderr[-3000:])
    got = np.load(path)
    ref.same(got["snake"], ref.snake(64, 64)[2].astype(np.float64), "serpentine, %d a look" % per_check)
    h = ref.fractal(130, 66, seed=2)
    ref.same(got["terrain"], ref.accumulate(want_weights(h, D8, dict(T=10.0)))[0], "terrain, %d a look" % per_check)
    launches, tiles, models, looks = got["snake_info"]
    assert (tiles, models) == (1, 1) and launches == per_check * looks
    # sixteen capped launches move the tile; the group of launches after the group with the sixteenth sees no move
    assert launches == per_check * (-(-16 // per_check) + 1) <= bound(1, per_check)
    launches, tiles, models, looks = got["terrain_info"]
    assert (tiles, models) == (6, 1) and per_check * looks == launches <= bound(6, per_check)


def test_the_info_against_the_shape(hip):
    from soillib_amd import soil
    info = check(ref.fractal(130, 200, seed=4), None, D8, dict(T=10.0), what="130 x 200")
    assert info["tiles"] == 12
    level = np.zeros((70, 70), np.float32)
    info = check(level, None, D8, dict(T=10.0), what="level: nothing is sent")
    assert info["launches"] == PER_CHECK and info["looks"] == 1, "every tile inert: the first look sees no move"
    assert soil.mfd_info() == info


# ------------------------------------------------------------------ batches

def test_a_batch_with_a_pair_of_scales_per_model_and_a_hostile_model(hip):
    from soillib_amd import soil
    H, W = 65, 70
    hs = np.stack([ref.fractal(H, W, seed=21), ref.hostile(H, W), ref.fractal(H, W, seed=22)])
    src = np.stack([np.random.default_rng(b).random((H, W)).astype(np.float32) for b in range(3)])
    src[1] = ref.hostile_source(H, W)
    scales = [(1.0, 1.0), (1.5, 0.5), (0.25, 3.0)]
    for edge, kind in ((D8, dict(p=1.1, scale=scales)), (D4, dict(p=4.0, scale=scales)), (D8, dict(T=10.0)),
                       (D8, dict(p=1.1, scale=scales[1]))):
        w, a64, a32 = run(hs, src, edge, kind)
        info = soil.mfd_info()
        assert info["models"] == 3 and info["tiles"] == 4 and info["launches"] <= bound(4)
        most = 0
        for b in range(3):
            one = dict(kind)
            if "scale" in kind and kind["scale"] is scales:
                one["scale"] = scales[b]
            sw, s64, s32 = run(hs[b], src[b], edge, one)
            most = max(most, soil.mfd_info()["launches"])
            ref.same(w[b], sw, "weights, model %d" % b)
            ref.same(a64[b], s64, "out64, model %d" % b)
            ref.same(a32[b], s32, "out, model %d" % b)
            ref.same(s64, ref.accumulate(want_weights(hs[b], edge, one), src[b])[0], "the single call, model %d" % b)
        assert info["launches"] == most, "the launches of a batch are those of the model that needs most"


def test_more_models_than_a_grid_axis_takes(hip):
    B = 65540
    base = np.array([[3.0, 2.0, 1.0], [2.5, 1.5, 0.0]], np.float32)
    hs = np.repeat(base[None], B, axis=0)
    marks = (0, 1, 65534, 65535, 65536, B - 1)
    for i, b in enumerate(marks):
        hs[b] = base * (i + 2) + np.arange(6, dtype=np.float32).reshape(2, 3) * (i % 2)
    w, a64, a32 = run(hs, None, D8, dict(T=1.0))
    for b in marks + (7, 40000):
        ww = want_weights(hs[b], D8, dict(T=1.0))
        ref.same(w[b], ww, "weights, model %d" % b)
        ref.same(a64[b], ref.accumulate(ww)[0], "out64, model %d" % b)
    same = np.ones(B, bool)
    same[list(marks)] = False
    assert (ref.bits64(a64[same]) == ref.bits64(a64[7])).all() and (ref.bits32(a32[same]) == ref.bits32(a32[7])).all()


# ------------------------------------------------------------------ the Monte-Carlo mean of the library's own multiflow

def test_the_mean_of_random_weighted_accumulations_lies_around_it(hip):
    """K = 1024 graphs of soil.random_weighted, each accumulated by soil.accumulate: at most 0.5 % of the cells lie more
    than 6 sample standard errors from mfd_accumulate, and cells of zero sample variance agree to 1e-6 relative."""
    from soillib_amd import silt, soil
    n, K, T = 48, 1024, 10.0
    h = to_gpu(ref.fractal(n, n, seed=7))
    one = silt.tensor(silt.float32, silt.shape(n, n), silt.gpu)
    silt.set(one, 1.0)
    s, ss = np.zeros((n, n)), np.zeros((n, n))
    for k in range(K):
        a = to_np(soil.accumulate(soil.random_weighted(h, D8, 1234, k, T), one, D8)).astype(np.float64)
        s += a
        ss += a * a
    mean = s / K
    var = np.maximum(ss - K * mean * mean, 0) / (K - 1)
    exact = to_np(soil.mfd_accumulate(h, None, D8, T=T, double=True))
    still = var == 0
    assert (np.abs(mean[still] - exact[still]) <= 1e-6 * np.abs(exact[still])).all()
    z = np.abs(mean[~still] - exact[~still]) / np.sqrt(var[~still] / K)
    print("greatest deviation %.2f standard errors, %d of %d cells beyond 6" % (z.max(), (z > 6).sum(), z.size))
    assert (z > 6).sum() <= 0.005 * n * n


# ------------------------------------------------------------------ through the batch object

def test_drainage_mfd_is_the_composed_single_calls(hip, oracle):
    from soillib_amd import silt, soil
    from soillib_amd.erosion import ErosionBatch
    B, H, W = 3, 64, 70
    prm = product_param(script_param(oracle.default_param()))
    prm.maxage = 32
    scales = [(20.0 / H * (1 + b), 20.0 / W, 4.0) for b in range(B)]
    layers = np.stack([terrain(oracle, H, W, seed=3.0 + 5.0 * b, sediment=0.05, rng_seed=b) for b in range(B)])
    src = np.random.default_rng(3).random((B, H, W)).astype(np.float32)
    for scale in ((20.0 / H, 20.0 / W, 4.0), scales):
        bt = ErosionBatch(B, H, W, scale, prm, 256, [11 + 7 * b for b in range(B)])
        bt.set_layers(to_gpu(layers))
        silt.set(bt.rainfall, 1.0)
        bt.step()
        before = {n: to_np(getattr(bt, n)).copy() for n in ("height", "layers", "rainfall")}
        pair = lambda b: list(scales[b][:2]) if scale is scales else list(scale[:2])
        for kw, edge in ((dict(T=10.0), D8), (dict(p=1.1), D4)):
            for conditioned, source in ((True, None), (False, src)):
                got = to_np(bt.drainage_mfd(source=_opt(source), edge=None if edge == D8 else soil.d4,
                                            conditioned=conditioned, **kw))
                for b in range(B):
                    hb = to_gpu(before["height"][b])
                    dist = None
                    if conditioned:
                        hb = soil.fill_depressions(hb, edge)
                        dist = soil.flat_distance(hb, edge)
                    one = dict(kw, scale=pair(b)) if "p" in kw else kw
                    want = to_np(soil.mfd_accumulate(hb, None if source is None else to_gpu(source[b]), edge, dist=dist, **one))
                    ref.same(got[b], want, "drainage_mfd(%r, conditioned=%r), model %d" % (kw, conditioned, b))
        for n, v in before.items():
            assert (to_np(getattr(bt, n)) == v).all(), "the batch's %s is not touched" % n


if __name__ == "__main__":
    _child_main(sys.argv[1])
