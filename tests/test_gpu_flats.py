"""Flats and filled lakes on the device (include/soil_hip.h: "flow graphs: conditioning"; soil.flat_distance,
flat_receivers, resolve_flats and their _batch forms), every cell, bit for bit, against the numpy restatements of
tests/flats_ref.py, under D4 and D8 throughout.  Everything compared is an int32: there is no tolerance anywhere.

  shapes         1x1, 1x200, 200x1, 3x3, 63x65, 64x64, 65x129, 130x70, 200x200: one tile, ragged tiles, seams in both
                 directions, a 4x4 tile grid
  constructions  an all-level plane; NaN blocks over a tile corner and NaN cells on seams; a closed depression and
                 single pits (-1); two terraces; flats that touch only diagonally; mixed +-0; +-inf; denormals; a
                 quantised DEM before and after the oracle's fill; a serpentine corridor of pitch 2 at 130x130 (a
                 distance in the thousands over seams in series) under SOIL_FLATS_PER_CHECK 1 and 3 in child processes
  receivers      each construction against the rule; in place; a plane 4 bytes off its alignment; hostile graph entries;
                 a dist plane of another height
  end to end     fill_depressions -> steepest -> resolve_flats -> flow_paths / accumulate at 200x200
  batches        B = 1, 3, 17 at 65x129, one model the corridor: slices against the single calls, and the launches of
                 a batch the largest of its models', not their sum
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import flats_ref as ref
from flats_ref import D4, D8
from util import to_gpu, to_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 200), (200, 1), (3, 3), (63, 65), (64, 64), (65, 129), (130, 70), (200, 200)]
EDGES = [D4, D8]
PER_CHECK = int(os.environ.get("SOIL_FLATS_PER_CHECK", "3"))      # launches a look at the "changed" word (docs/KNOBS.md)


_same = ref.same                          # (shared with tests/test_gpu_cpp_ops.py)


@functools.lru_cache(maxsize=None)
def _heights(H, W):
    return ref.constructions(H, W)


@functools.lru_cache(maxsize=None)
def _want(H, W, edge):
    """The restatement's distances of every construction at one shape, made once and left unchanged."""
    out = {}
    for name, h in _heights(H, W):
        out[name] = ref.distance_bfs(h, edge)
        out[name].setflags(write=False)
    return out


def _distance(h, edge):
    from soillib_amd import soil
    return to_np(soil.flat_distance(to_gpu(h), edge))


def _receivers(g, h, d, edge):
    from soillib_amd import soil
    return to_np(soil.flat_receivers(to_gpu(g), to_gpu(h), to_gpu(d), edge))


# ------------------------------------------------------------------ the distance

@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("edge", EDGES)
def test_distance_of_every_construction(hip, H, W, edge):
    from soillib_amd import soil
    for name, h in _heights(H, W):
        _same(_distance(h, edge), _want(H, W, edge)[name], "%s at %dx%d edge %d" % (name, H, W, edge))
        info = soil.flat_distance_info()
        assert info["tiles"] == -(-H // 64) * -(-W // 64) and info["models"] == 1
        assert info["launches"] == PER_CHECK * info["looks"] >= PER_CHECK


@pytest.mark.parametrize("edge", EDGES)
def test_diagonal_flats_differ_between_d4_and_d8(hip, edge):
    h = ref.diagonal_flats(130, 70)
    got = _distance(h, edge)
    inner = (h == 2.0)
    inner[:3, :] = inner[-4:, :] = inner[:, :3] = inner[:, -4:] = False
    assert ((got[inner] == -1).all()) == (edge == D4) and inner.any()
    _same(got, ref.distance_relax(h, edge), "diagonal flats against the second restatement")


@functools.lru_cache(maxsize=None)
def _quantised(oracle, H, W, edge):
    q = ref.quantised(oracle, H, W)
    return q, oracle.fill_depressions(q, edge)


@pytest.mark.parametrize("H,W", [(130, 70), (200, 200)])
@pytest.mark.parametrize("edge", EDGES)
def test_a_quantised_dem_before_and_after_the_fill(hip, oracle, H, W, edge):
    for what, h in zip(("before", "after"), _quantised(oracle, H, W, edge)):
        want = ref.distance_relax(h, edge)
        assert (want > 1).any(), "natural flats more than one cell deep"
        _same(_distance(h, edge), want, "quantised DEM %s the fill, %dx%d edge %d" % (what, H, W, edge))
        if what == "after":
            assert (want >= 0).all()
        graph = oracle.steepest(h, edge)
        _same(_receivers(graph, h, want, edge), ref.receivers(graph, h, want, edge), "its receivers, %s" % what)


# ------------------------------------------------------------------ the serpentine, in child processes

def _child_main(path):
    from soillib_amd import soil
    out = {}
    for edge in EDGES:
        out["d%d" % edge] = _distance(ref.serpentine(130, 130), edge)
        out["info%d" % edge] = np.array([soil.flat_distance_info()[k] for k in ("launches", "tiles", "models", "looks")])
    np.savez(path, **out)


@functools.lru_cache(maxsize=None)
def _serpentine_want(edge):
    return ref.distance_bfs(ref.serpentine(130, 130), edge)


@pytest.mark.parametrize("per_check", ["1", "3"])
def test_the_serpentine_corridor_over_many_launches(hip, tmp_path, per_check):
    """A distance in the thousands, over seams in series: the launch loop and its looks at the flag, with one and with
    three launches a look.  The launches stay far below the cap, 9 * (4 * 64 + 16) + 16."""
    path = str(tmp_path / "serpentine.npz")
    env = dict(os.environ)
    env["SOIL_FLATS_PER_CHECK"] = per_check
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, "%s\n%s" % (r.stdout[-3000:], r.stderr[-3000:])
    got = np.load(path)
    for edge in EDGES:
        want = _serpentine_want(edge)
        assert want.max() > 8000 and (want >= 0).all()
        _same(got["d%d" % edge], want, "serpentine edge %d, %s launches a look" % (edge, per_check))
        launches, tiles, models, looks = got["info%d" % edge].tolist()
        assert (tiles, models) == (9, 1) and launches == int(per_check) * looks
        assert 64 <= launches <= 9 * (4 * 64 + 16) + 16, "every corridor row crosses seams: launches in series"


# ------------------------------------------------------------------ receivers

@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("edge", EDGES)
def test_receivers_of_every_construction_out_of_place_and_in_place(hip, H, W, edge):
    from soillib_amd import _abi
    none = np.full((H, W), -1, np.int32)
    hostile = ref.hostile_graph(H, W)
    for name, h in _heights(H, W):
        dist = _want(H, W, edge)[name]
        for gname, g in (("all -1", none), ("hostile", hostile)):
            want = ref.receivers(g, h, dist, edge)
            what = "%s, graph %s, %dx%d edge %d" % (name, gname, H, W, edge)
            _same(_receivers(g, h, dist, edge), want, what)
            if gname == "all -1":
                assert ((want >= 0) == (dist > 0)).all(), "every cell with a distance above 0 has a receiver"
        gg, hh, dd = to_gpu(hostile), to_gpu(h), to_gpu(dist)
        _abi.check(hip.soil_flat_receivers(gg.c_ptr, gg.c_ptr, hh.c_ptr, dd.c_ptr, H, W, edge, _abi.stream()))
        _same(to_np(gg), ref.receivers(hostile, h, dist, edge), "%s in place, %dx%d edge %d" % (name, H, W, edge))


@pytest.mark.parametrize("edge", EDGES)
def test_receivers_with_planes_off_their_alignment_and_a_foreign_dist(hip, edge):
    from soillib_amd import _abi, silt
    H, W = 65, 129
    h = ref.terraces(H, W)
    dist = ref.distance_bfs(h, edge)
    g = ref.hostile_graph(H, W)
    want = ref.receivers(g, h, dist, edge)

    def shifted(arr, dtype):
        buf = silt.tensor(dtype, silt.shape(H * W + 4), silt.gpu)
        assert buf.ptr % 16 == 0
        view = silt.tensor.from_device(buf.ptr + 4, dtype, silt.shape(H, W), keepalive=buf)
        arr = np.ascontiguousarray(arr)
        _abi.check(hip.soil_memcpy_h2d(view.c_ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes, _abi.stream()))
        _abi.check(hip.soil_stream_synchronize(_abi.stream()))
        return view

    for off in range(4):                                           # each plane in turn 4 bytes off, the others aligned
        planes = [shifted(a, t) if i == off else to_gpu(a)
                  for i, (a, t) in enumerate(((g, silt.int32), (g, silt.int32), (h, silt.float32), (dist, silt.int32)))]
        _abi.check(hip.soil_flat_receivers(*[p.c_ptr for p in planes], H, W, edge, _abi.stream()))
        _same(to_np(planes[0]), want, "plane %d off its alignment" % off)
    hs = shifted(h, silt.float32)
    ds = silt.tensor(silt.int32, silt.shape(H, W), silt.gpu)
    _abi.check(hip.soil_flat_distance(ds.c_ptr, hs.c_ptr, H, W, edge, _abi.stream()))
    _same(to_np(ds), dist, "the distance of a height plane off its alignment")
    # a dist plane from another height: the level plane's distances on the terraces — what qualifies by the rule is
    # taken, everything else stays as it was
    foreign = ref.distance_bfs(ref.level(H, W), edge)
    want = ref.receivers(g, h, foreign, edge)
    assert (want == g).sum() > (g >= 0).sum(), "entries left unchanged although in < 0 and dist > 0"
    _same(_receivers(g, h, foreign, edge), want, "a foreign dist")
    other = (foreign + 1000).astype(np.int32)                      # no neighbour is one step closer: nothing changes
    other[::2] += 7
    _same(_receivers(g, h + np.float32(1.0), other, edge), ref.receivers(g, h + np.float32(1.0), other, edge), "another foreign dist")


# ------------------------------------------------------------------ end to end on the device

@pytest.mark.parametrize("edge", EDGES)
def test_a_filled_dem_drains_to_the_border(hip, oracle, edge):
    from soillib_amd import silt, soil
    S = 200
    dem = oracle.noise(S, S, seed=3.0, ext=(float(S), float(S))) * np.float32(100.0)
    filled = soil.fill_depressions(to_gpu(dem), edge)
    plain = soil.steepest(filled, edge)
    graph = soil.resolve_flats(filled, edge)
    _same(to_np(graph), to_np(soil.resolve_flats(filled, edge, plain)), "resolve_flats with the graph given")
    f = to_np(filled)
    dist = ref.distance_relax(f, edge)
    _same(to_np(graph), ref.receivers(to_np(plain), f, dist, edge), "resolve_flats against the restatement")
    terminal, steps, _ = (to_np(t) if t is not None else None for t in soil.flow_paths(graph, edge))
    assert (terminal >= 0).all() and (steps >= 0).all(), "no cell at -1: the patched graph is acyclic"
    tx, ty = terminal // S, terminal % S
    assert ((tx == 0) | (tx == S - 1) | (ty == 0) | (ty == S - 1)).all(), "every terminal is on the border"
    ones = silt.tensor(silt.float32, silt.shape(S, S), silt.gpu)
    silt.set(ones, 1.0)
    ends = np.unique(terminal)

    def drained(g):
        acc = to_np(soil.accumulate(g, ones, edge)).reshape(-1)
        return float(acc[ends].astype(np.float64).sum())

    assert drained(graph) == float(S * S), "upstream area over the terminals is every cell (40 000 < 2^24: exact)"
    assert drained(plain) < float(S * S), "without resolve_flats the lakes keep their cells"


# ------------------------------------------------------------------ batches

@functools.lru_cache(maxsize=None)
def _models(B, H, W):
    pool = [h for _, h in _heights(H, W)]
    hs = [pool[(3 * b) % len(pool)] for b in range(B)]
    hs[B // 2] = ref.serpentine(H, W)                               # one model holds the corridor, the others are benign
    return np.stack(hs)


@pytest.mark.parametrize("B", [1, 3, 17])
@pytest.mark.parametrize("edge", EDGES)
def test_a_batch_is_its_models_side_by_side(hip, B, edge):
    from soillib_amd import soil
    H, W = 65, 129
    hs = _models(B, H, W)
    singles, launches = [], []
    for b in range(B):
        singles.append(_distance(hs[b], edge))
        launches.append(soil.flat_distance_info()["launches"])
        _same(singles[b], ref.distance_bfs(hs[b], edge), "model %d alone" % b)
    hb = to_gpu(hs)
    dist = soil.flat_distance_batch(hb, edge)
    info = soil.flat_distance_info()
    _same(to_np(dist), np.stack(singles), "the batch's distances against the single calls")
    assert info["models"] == B and info["tiles"] == 2 * 3
    assert all(n % PER_CHECK == 0 for n in launches), "a call's launches come PER_CHECK a look"
    assert info["launches"] == max(launches), "the launches of a batch: the largest of its models', not their sum"
    assert B == 1 or info["launches"] < sum(launches)
    g = np.stack([ref.hostile_graph(H, W, seed=b) for b in range(B)])
    want = np.stack([_receivers(g[b], hs[b], singles[b], edge) for b in range(B)])
    _same(to_np(soil.flat_receivers_batch(to_gpu(g), hb, dist, edge)), want, "the batch's receivers")
    _same(want, np.stack([ref.receivers(g[b], hs[b], singles[b], edge) for b in range(B)]), "and the restatement")
    own = to_np(soil.resolve_flats_batch(hb, edge))
    for b in range(B):
        _same(own[b], to_np(soil.resolve_flats(to_gpu(hs[b]), edge)), "resolve_flats_batch, model %d" % b)


if __name__ == "__main__":
    _child_main(sys.argv[1])
