"""Stream order and channel segments on the device (include/soil_hip.h: soil_stream_order, soil_stream_order_batch;
soillib_amd.soil.stream_order / stream_segments / stream_magnitude and their _batch forms, ErosionBatch.stream_order /
stream_segments), word for word against tests/stream_order_ref.py, which restates the definition by level sets and not
the passes: every plane is int32 (the lengths and magnitudes float32 bit patterns), there is no tolerance anywhere, and
the level count of every call is the reference's.

  shapes     (1, 1), (1, 7), (5, 8), (13, 21); (12, 20) the 16-byte init; (7, 64) the dyadic tree of order 7; (3, 261),
             (5, 1028) two work-groups along a row — the seed pass reads donors across the boundary —; (67, 131);
             (1027, 2051) above the engine's work-group cap for the oracle's noise graph and the chain
  graphs     a chain through every cell (order 1, one level), a comb (order 2), the dyadic tree with its closed form,
             junctions of mixed donor orders placed by hand, cells with all K donors, cycles with trees draining into
             them, hostile entries, a stop on a junction's donor, a channel mask with holes, areas with NaN and +-inf,
             the CPU oracle's steepest graphs of a noise DEM, numpy's steepest graph of a terrain with plateaus
  calls      D4 and D8 (a D8 graph under D4), every optional input given and NULL, each output alone and all together,
             planes 4 bytes off their alignment
  batches    3 x 12 x 20 with a different level count per model and a hostile one in the middle; 5 x 8 x 12 in chunks of
             2 + 2 + 1; work-group counts 1, 3, 64 and 64-bit offsets in child processes; SOIL_STREAM_ORDER_NARROW=0
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import flow_paths_ref as fref
import paths_cap_ref as cap
import stream_order_ref as ref
from stream_order_ref import D4, D8
from util import product_param, script_param, terrain, to_gpu, to_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 7), (5, 8), (13, 21), (12, 20), (3, 261), (5, 1028), (67, 131)]


def _info():
    from soillib_amd import soil
    return soil.stream_order_info()


def _rounds(H, W):
    return len(bin(H * W - 1)) - 2 if H * W > 1 else 0


def _opt(a):
    return None if a is None else to_gpu(a)


def _call(dims, graph, edge, channel=None, area=None, threshold=None, stop=None, want=ref.OUTPUTS):
    """The planes named in `want` of one call through the module's one entry point, as numpy arrays."""
    from soillib_amd import soil
    got = soil._stream_order("test", dims, to_gpu(graph), edge, _opt(channel), _opt(area), threshold, _opt(stop), want)
    return {k: to_np(v) for k, v in got.items()}


@functools.lru_cache(maxsize=None)
def _cases(H, W, edge):
    out = ref.cases(H, W, edge)
    for c in out.values():
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _want(H, W, edge, name):
    return ref.by_levels(edge=edge, **_cases(H, W, edge)[name])


# ------------------------------------------------------------------ against the reference

@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("edge", [D4, D8])
def test_single_grid_against_the_reference(hip, H, W, edge):
    for name, c in _cases(H, W, edge).items():
        what = "%s %dx%d edge %d" % (name, H, W, edge)
        got = _call(2, edge=edge, **c)
        ref.same(got, _want(H, W, edge, name), what, _info()["levels"])
        i = _info()
        vec = int(W % 4 == 0)
        assert (i["chunks"], i["vec_chunks"], i["idx64_chunks"], i["rounds"]) == (1, vec, 0, _rounds(H, W)), what


@pytest.mark.parametrize("edge", [D4, D8])
def test_the_dyadic_tree_of_order_seven(hip, edge):
    g, order, donors = ref.dyadic(6)
    assert g.shape == (7, 64)
    got = _call(2, g, edge)
    assert (got["order"] == order).all() and (got["donors"] == donors).all(), "the closed form"
    ref.same(got, ref.by_levels(g, edge), "dyadic (7, 64)", _info()["levels"])
    assert _info()["levels"] == 7 == got["order"].max()


@pytest.mark.parametrize("edge", [D4, D8])
def test_junctions_of_mixed_orders(hip, edge):
    got = _call(2, ref.mixed(), edge)
    for at, o in ref.MIXED_ORDERS.items():
        assert got["order"][at] == o, (at, o)
    for at, d in ref.MIXED_DONORS.items():
        assert got["donors"][at] == d, (at, d)
    assert _info()["levels"] == 3


@pytest.mark.parametrize("H,W", [(13, 21), (12, 20), (67, 131)])
@pytest.mark.parametrize("edge", [D4, D8])
def test_the_oracles_steepest_graphs(hip, oracle, H, W, edge):
    """The CPU oracle's steepest graph of a noise DEM: every cell a channel; the cells draining three or more; those
    under a mask with holes and stops on junction donors; and a D8 graph read under D4."""
    g = oracle.steepest(ref.noise_height(oracle, H, W), edge)
    area = ref.upstream_count(g, edge)
    for kw in (dict(), dict(area=area, threshold=3.0),
               dict(channel=ref.holes(H, W), area=area, threshold=2.0, stop=ref.junction_stop(g, edge))):
        got = _call(2, g, edge, **kw)
        ref.same(got, ref.by_levels(g, edge, **kw), "oracle.steepest %dx%d edge %d %s" % (H, W, edge, sorted(kw)),
                 _info()["levels"])
    if edge == D8:
        ref.same(_call(2, g, D4), ref.by_levels(g, D4), "a D8 graph under D4", _info()["levels"])
        assert (ref.by_levels(g, D4)["order"] != ref.by_levels(g, D8)["order"]).any()


def test_above_the_work_group_cap(hip, oracle):
    """(1027, 2051): more blocks of 256 cells than work-groups of a round: the oracle's noise graph with the lower half
    of the DEM as channels (the negated height as `area`), the chain through every cell, and the chain with a
    junction two rows down, whose order 2 reaches the foot only in the last round."""
    H, W = 1027, 2051
    assert cap.above(H * W)
    h = ref.noise_height(oracle, H, W)
    g = oracle.steepest(h, D8)
    kw = dict(area=-h, threshold=-float(np.median(h)))
    want = ref.by_levels(g, D8, **kw)
    assert want["levels"] >= 4 and 0.3 < (want["order"] > 0).mean() < 0.7
    ref.same(_call(2, g, D8, **kw), want, "noise above the cap", _info()["levels"])
    assert _info() == dict(chunks=1, vec_chunks=0, idx64_chunks=0, rounds=22, levels=want["levels"])
    chain = fref.serpentine(H, W)
    got = _call(2, chain, D4, want=("order", "link_foot"))
    assert (got["order"] == 1).all() and got["link_foot"].sum() == 1 and got["link_foot"][H - 1, W - 1] == 1
    assert _info()["levels"] == 1
    chain[0, 0] = W                                                # ref.cases' chain_join
    got = _call(2, chain, D4, want=("order",))
    want = np.full((H, W), 2, np.int32)
    want[:2] = 1
    want[1, 0] = 2
    assert (got["order"] == want).all() and _info()["levels"] == 2 and H * W - 2 * W > 1 << 21


def test_without_narrowing_the_work_set(hip, monkeypatch):
    """SOIL_STREAM_ORDER_NARROW=0 (read per call): every channel cell stays in every closure's work set; the same
    words and the same level count."""
    monkeypatch.setenv("SOIL_STREAM_ORDER_NARROW", "0")
    for H, W, name in ((67, 131, "descent"), (12, 20, "chain_join"), (13, 21, "cycles_area"), (12, 20, "mixed")):
        ref.same(_call(2, edge=D8, **_cases(H, W, D8)[name]), _want(H, W, D8, name), "%s, not narrowed" % name,
                 _info()["levels"])
    g = ref.dyadic(6)[0]
    ref.same(_call(2, g, D4), ref.by_levels(g, D4), "dyadic, not narrowed", _info()["levels"])


# ------------------------------------------------------------------ call variants

def _planes_of_three():
    """Three models of (12, 20) with 3, 2 and 1 levels under D4 and D8 alike: the hand-placed junctions, a hostile
    graph, the chain; and every optional input."""
    H, W = 12, 20
    cs = _cases(H, W, D8)
    graph = np.stack([cs["mixed"]["graph"], cs["hostile"]["graph"], cs["chain"]["graph"]])
    channel = np.stack([ref.holes(H, W), np.ones((H, W), np.int32), ref.holes(H, W)[::-1].copy()])
    area = np.stack([ref.area_plane(H, W, b) for b in range(3)])
    stop = np.stack([cs["descent_all"]["stop"], fref.stop_planes(H, W)[1][1], cs["comb_stop"]["stop"]])
    return graph, channel, area, stop


def test_every_optional_input_and_each_output_alone(hip):
    from soillib_amd import _abi, silt
    graph, channel, area, stop = _planes_of_three()
    B, H, W = graph.shape
    gg, gc, ga, gs = to_gpu(graph), to_gpu(channel), to_gpu(area), to_gpu(stop)
    new = lambda shape: silt.tensor(silt.int32, silt.shape(*shape), silt.gpu)   # noqa: E731
    ptr = lambda t: None if t is None else t.c_ptr                # noqa: E731
    for with_c, with_a, with_s in [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)]:
        kw = dict(channel=channel if with_c else None, area=area if with_a else None, threshold=4.0,
                  stop=stop if with_s else None)
        want = ref.batch(ref.by_levels, graph, D8, **kw)
        for which in [(k,) for k in range(5)] + [(0, 1, 2, 3, 4), (2, 4)]:
            outs = [new((B, H, W)) if k in which else None for k in range(5)]
            _abi.check(hip.soil_stream_order_batch(*[ptr(o) for o in outs], gg.c_ptr, ptr(gc) if with_c else None,
                                                   ptr(ga) if with_a else None, 4.0, ptr(gs) if with_s else None,
                                                   B, H, W, D8, _abi.stream()))
            got = {name: to_np(o) for name, o in zip(ref.OUTPUTS, outs) if o is not None}
            ref.same(got, want, "batch, inputs %r outputs %r" % ((with_c, with_a, with_s), which), _info()["levels"])
            b = len(which) % 3                                    # the single grid on one model's slices
            outs = [new((H, W)) if k in which else None for k in range(5)]
            at = lambda t: C.c_void_p(t.ptr + 4 * b * H * W)      # noqa: E731
            _abi.check(hip.soil_stream_order(*[ptr(o) for o in outs], at(gg), at(gc) if with_c else None,
                                             at(ga) if with_a else None, 4.0, at(gs) if with_s else None, H, W, D8,
                                             _abi.stream()))
            got = {name: to_np(o) for name, o in zip(ref.OUTPUTS, outs) if o is not None}
            one = ref.by_levels(graph[b], D8, kw["channel"] if kw["channel"] is None else channel[b],
                                kw["area"] if kw["area"] is None else area[b], 4.0, kw["stop"] if kw["stop"] is None else stop[b])
            ref.same(got, one, "single model %d, outputs %r" % (b, which), _info()["levels"])
            ref.same(got, {k: v[b] for k, v in want.items() if k != "levels"}, "the batch's slice")


def test_planes_off_their_16_bytes(hip):
    """Every plane 4 bytes past a 16-byte boundary, W % 4 == 0: the scalar init takes the call and gives what the
    16-byte form gives; so does one input plane off alone."""
    from soillib_amd import _abi, silt
    graph, channel, area, stop = _planes_of_three()
    B, H, W = graph.shape
    want = ref.batch(ref.by_levels, graph, D8, channel, area, 4.0, stop)

    def shifted(arr, dtype):
        buf = silt.tensor(dtype, silt.shape(B * H * W + 4), silt.gpu)
        assert buf.ptr % 16 == 0
        view = silt.tensor.from_device(buf.ptr + 4, dtype, silt.shape(B, H, W), keepalive=buf)
        if arr is not None:
            arr = np.ascontiguousarray(arr)
            _abi.check(hip.soil_memcpy_h2d(view.c_ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes, _abi.stream()))
            _abi.check(hip.soil_stream_synchronize(_abi.stream()))
        return view

    planes = (graph, channel, area, stop)
    dtypes = (silt.int32, silt.int32, silt.float32, silt.int32)
    off = [shifted(p, d) for p, d in zip(planes, dtypes)]
    on = [to_gpu(p) for p in planes]
    outs = [shifted(None, silt.int32) for _ in range(5)]
    for which, vec in (((0, 1, 2, 3), 0), ((0,), 0), ((1,), 0), ((2,), 0), ((3,), 0), ((), 1)):
        g, c, a, s = [off[i] if i in which else on[i] for i in range(4)]
        _abi.check(hip.soil_stream_order_batch(*[o.c_ptr for o in outs], g.c_ptr, c.c_ptr, a.c_ptr, 4.0, s.c_ptr, B, H, W,
                                               D8, _abi.stream()))
        ref.same({k: to_np(o) for k, o in zip(ref.OUTPUTS, outs)}, want, "planes %r off their 16 bytes" % (which,),
                 _info()["levels"])
        assert _info()["chunks"] == 1 and _info()["vec_chunks"] == vec, which


# ------------------------------------------------------------------ batches

def test_a_batch_is_its_single_calls_slice_for_slice(hip):
    """3 x 12 x 20: a different graph and level count per model, a hostile model between two benign ones."""
    graph, channel, area, stop = _planes_of_three()
    for edge in (D4, D8):
        for kw in (dict(), dict(channel=channel, area=area, threshold=4.0, stop=stop)):
            want = ref.batch(ref.by_levels, graph, edge, **kw)
            got = _call(3, graph, edge, **kw)
            ref.same(got, want, "batch edge %d %s" % (edge, sorted(kw)), _info()["levels"])
            assert got["channel_graph"].max() < graph[0].size, "channel_graph holds indices within the model"
            levels = []
            for b in range(3):
                one = _call(2, graph[b], edge, **{k: (v if k == "threshold" else v[b]) for k, v in kw.items()})
                levels.append(_info()["levels"])
                ref.same({k: v[b] for k, v in got.items()}, one, "model %d against the single call" % b)
            assert max(levels) == want["levels"]
            if not kw:
                assert levels == [3, 2, 1], levels


def _five(H=8, W=12):
    cs = _cases(H, W, D8)
    graph = np.stack([cs[k]["graph"] for k in ("descent", "hostile", "cycles", "chain", "comb")])
    area = np.stack([ref.area_plane(H, W, 10 + b) for b in range(5)])
    stop = np.stack([cs["comb_stop"]["stop"]] * 5)
    return graph, area, stop


CHILD_ENVS = {
    "cells": {},                                                  # SOIL_FLOW_BATCH_CELLS: set by the child
    "groups1": {"SOIL_PATHS_GROUPS": "1"},
    "groups3": {"SOIL_PATHS_GROUPS": "3"},
    "groups64": {"SOIL_PATHS_GROUPS": "64"},
    "idx64": {"SOIL_PATHS_IDX64": "1"},
}
CHILD_SINGLE = [(5, 1028, "descent_all"), (67, 131, "descent"), (13, 21, "cycles")]


def _child_main(path, chunked):
    """The child of test_chunks_and_launch_shapes: B = 5 at (8, 12), with `chunked` as 2 + 2 + 1; three single grids."""
    out = {}
    if chunked:
        os.environ["SOIL_FLOW_BATCH_CELLS"] = str(2 * 8 * 12 + 8 * 12 // 2)
    graph, area, stop = _five()
    for tag, kw in (("plain", dict()), ("all", dict(area=area, threshold=4.0, stop=stop))):
        got = _call(3, graph, D8, **kw)
        i = _info()
        for k, v in got.items():
            out["batch_%s_%s" % (tag, k)] = v
        out["batch_%s_info" % tag] = np.array([i[k] for k in ("chunks", "vec_chunks", "idx64_chunks", "rounds", "levels")])
    os.environ.pop("SOIL_FLOW_BATCH_CELLS", None)
    for H, W, name in CHILD_SINGLE:
        got = _call(2, edge=D8, **_cases(H, W, D8)[name])
        for k, v in got.items():
            out["%dx%d_%s" % (H, W, k)] = v
        out["%dx%d_levels" % (H, W)] = np.array([_info()["levels"]])
    np.savez(path, **out)


@pytest.mark.parametrize("name", sorted(CHILD_ENVS))
def test_chunks_and_launch_shapes(hip, tmp_path, name):
    """A fresh child process under SOIL_FLOW_BATCH_CELLS (5 x 8 x 12 in chunks of 2 + 2 + 1 models), SOIL_PATHS_GROUPS
    = 1, 3 and 64 and SOIL_PATHS_IDX64 = 1: the reference's words whatever the path, and the info record."""
    path = str(tmp_path / "stream_order.npz")
    env = dict(os.environ)
    for k in ("SOIL_FLOW_BATCH_CELLS", "SOIL_PATHS_LIST_FROM", "SOIL_PATHS_IDX64", "SOIL_PATHS_GROUPS",
              "SOIL_STREAM_ORDER_NARROW"):
        env.pop(k, None)
    env.update(CHILD_ENVS[name])
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path, name], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=280)
    assert r.returncode == 0, "%s\n%s" % (r.stdout[-3000:], r.stderr[-3000:])
    got = np.load(path)
    chunks = 3 if name == "cells" else 1
    graph, area, stop = _five()
    for tag, kw in (("plain", dict()), ("all", dict(area=area, threshold=4.0, stop=stop))):
        want = ref.batch(ref.by_levels, graph, D8, **kw)
        info = got["batch_%s_info" % tag].tolist()
        ref.same({k: got["batch_%s_%s" % (tag, k)] for k in ref.OUTPUTS}, want, "5 x 8 x 12 %s under %s" % (tag, name),
                 info[4])
        assert info[:4] == [chunks, chunks, chunks if name == "idx64" else 0, _rounds(8, 12)], info
        for b in range(5):                                        # ... against the single calls
            kb = {k: (v if k == "threshold" else v[b]) for k, v in kw.items()}
            ref.same({k: got["batch_%s_%s" % (tag, k)][b] for k in ref.OUTPUTS}, _call(2, graph[b], D8, **kb),
                     "model %d against the single call" % b)
    for H, W, case in CHILD_SINGLE:
        ref.same({k: got["%dx%d_%s" % (H, W, k)] for k in ref.OUTPUTS}, _want(H, W, D8, case),
                 "%dx%d %s under %s" % (H, W, case, name), int(got["%dx%d_levels" % (H, W)][0]))


# ------------------------------------------------------------------ segments, magnitude, the batch's methods

@pytest.mark.parametrize("H,W", [(7, 13), (12, 20), (67, 131)])
@pytest.mark.parametrize("edge", [D4, D8])
def test_segments_and_magnitude(hip, H, W, edge):
    from soillib_amd import soil
    scale = (0.5, 1.25)
    for name in ("mixed", "descent", "descent_area", "comb_holes", "comb_stop"):
        c = _cases(H, W, edge).get(name)
        if c is None:
            continue
        planes = ref.by_levels(edge=edge, **c)
        args = (to_gpu(c["graph"]), edge, _opt(c["channel"]), _opt(c["area"]), c["threshold"], _opt(c["stop"]))
        for by in ("link", "order"):
            for sc in (scale, None):
                got = soil.stream_segments(*args, scale=sc, by=by)
                want = ref.segments(planes, edge, sc, by)
                what = "%s %dx%d edge %d by %s" % (name, H, W, edge, by)
                assert (to_np(got[0]) == want[0]).all(), what
                fref.same_words(tuple(None if g is None else to_np(g) for g in got[1:]), want[1:], what)
                off = want[0] == 0                                # a non-channel cell is its own foot at distance 0
                assert (to_np(got[1])[off] == np.arange(H * W).reshape(H, W)[off]).all() and (to_np(got[2])[off] == 0).all()
        mag = to_np(soil.stream_magnitude(*args))
        assert mag.dtype == np.float32 and (mag.view(np.uint32) == ref.magnitude(planes).view(np.uint32)).all(), name
    order, donors = soil.stream_order(to_gpu(_cases(H, W, edge)["descent"]["graph"]), edge, donors=True)
    want = _want(H, W, edge, "descent")
    assert (to_np(order) == want["order"]).all() and (to_np(donors) == want["donors"]).all()
    assert (to_np(soil.stream_order(to_gpu(_cases(H, W, edge)["descent"]["graph"]), edge)) == want["order"]).all()


def test_segments_and_magnitude_of_a_batch(hip):
    from soillib_amd import soil
    graph, channel, area, stop = _planes_of_three()
    graph = graph[[0, 2, 0]]                                      # (the hostile model has cycles: accumulate's business)
    scales = [(1.0, 2.0), (0.5, 0.5), (3.0, 1.0)]
    args = (to_gpu(graph), D8, to_gpu(channel), to_gpu(area), 4.0, to_gpu(stop))
    planes = [ref.by_levels(graph[b], D8, channel[b], area[b], 4.0, stop[b]) for b in range(3)]
    for by in ("link", "order"):
        got = [to_np(t) for t in soil.stream_segments_batch(*args, scale=scales, by=by)]
        for b in range(3):
            want = ref.segments(planes[b], D8, scales[b], by)
            assert (got[0][b] == want[0]).all()
            fref.same_words(tuple(g[b] for g in got[1:]), want[1:], "model %d by %s" % (b, by))
    mag = to_np(soil.stream_magnitude_batch(*args))
    for b in range(3):
        assert (mag[b].view(np.uint32) == ref.magnitude(planes[b]).view(np.uint32)).all()
    o, d = soil.stream_order_batch(*args, donors=True)
    assert (to_np(o) == np.stack([p["order"] for p in planes])).all() and (to_np(d) == np.stack([p["donors"] for p in planes])).all()


def test_the_batch_methods_are_the_module_calls(hip, oracle):
    from soillib_amd import silt, soil
    from soillib_amd.erosion import ErosionBatch
    B, H, W = 3, 32, 32
    p = product_param(script_param(oracle.default_param()))
    p.maxage = 64
    scale = (20.0 / H, 20.0 / W, 4.0)
    layers = np.stack([terrain(oracle, H, W, seed=3.0 + 5.0 * b, sediment=0.05, rng_seed=b) for b in range(B)])
    bt = ErosionBatch(B, H, W, scale, p, 256, [11 + 7 * b for b in range(B)])
    bt.set_layers(to_gpu(layers))
    silt.set(bt.rainfall, 1.0)
    bt.step()
    names = ("layers",) + ErosionBatch.PLANES_1 + ErosionBatch.PLANES_2
    before = {n: to_np(getattr(bt, n)).copy() for n in names}
    for edge in (D4, D8):
        _, graph = soil.condition_batch(bt.height, edge)
        area = soil.accumulate_batch(graph, to_gpu(np.ones((B, H, W), np.float32)), edge)
        order, donors = bt.stream_order(6.0, edge=edge, donors=True)
        want = soil.stream_order_batch(graph, edge, None, area, 6.0, None, True)
        assert (to_np(order) == to_np(want[0])).all() and (to_np(donors) == to_np(want[1])).all()
        restated = ref.batch(ref.by_levels, to_np(graph), edge, None, to_np(area), 6.0)
        ref.same(dict(order=to_np(order), donors=to_np(donors)), restated, "ErosionBatch.stream_order", _info()["levels"])
        assert restated["levels"] >= 2 and (restated["order"] == 0).any()
        given = bt.stream_order(2.0, edge=edge, graph=graph, area=area)
        assert (to_np(given) == to_np(soil.stream_order_batch(graph, edge, None, area, 2.0))).all()
        for by in ("link", "order"):
            got = bt.stream_segments(6.0, edge=edge, by=by)
            want = soil.stream_segments_batch(graph, edge, None, area, 6.0, None, scale[:2], by)
            for g, w in zip(got, want):
                assert (to_np(g).view(np.uint32) == to_np(w).view(np.uint32)).all(), by
    for n in names:
        assert (to_np(getattr(bt, n)).view(np.uint32) == before[n].view(np.uint32)).all(), n


# ------------------------------------------------------------------ refusals

def test_refusals_leave_the_planes_untouched(hip):
    from soillib_amd import _abi
    B, H, W = 2, 5, 8
    outs = [to_gpu(np.full((B, H, W), -77, np.int32)) for _ in range(5)]
    g = to_gpu(np.full((B, H, W), -1, np.int32))
    a = to_gpu(np.zeros((B, H, W), np.float32))
    st = _abi.stream()
    one, many = hip.soil_stream_order, hip.soil_stream_order_batch
    o = [t.c_ptr for t in outs]

    def refused(name, rc):
        assert rc == _abi.SOIL_ERR_INVALID_ARGUMENT, name
        assert _abi.last_error().startswith(name + ": "), (name, _abi.last_error())

    refused("stream_order", one(*o, None, None, a.c_ptr, 1.0, None, H, W, D8, st))
    refused("stream_order", one(None, None, None, None, None, g.c_ptr, None, None, 1.0, None, H, W, D8, st))
    refused("stream_order", one(*o, g.c_ptr, None, a.c_ptr, float("nan"), None, H, W, D8, st))
    refused("stream_order", one(*o, g.c_ptr, None, None, 1.0, None, H, W, 2, st))
    refused("stream_order", one(o[0], o[0], None, None, None, g.c_ptr, None, None, 1.0, None, H, W, D8, st))
    refused("stream_order", one(g.c_ptr, None, None, None, None, g.c_ptr, None, None, 1.0, None, H, W, D8, st))
    for b, h, w in ((0, H, W), (B, 0, W), (B, H, -3), (B, 1 << 16, 1 << 16)):
        refused("stream_order_batch", many(*o, g.c_ptr, None, a.c_ptr, 1.0, None, b, h, w, D8, st))
    refused("stream_order_batch", many(*o[:4], a.c_ptr, g.c_ptr, None, a.c_ptr, 1.0, None, B, H, W, D8, st))
    _abi.check(hip.soil_stream_synchronize(st))
    assert all((to_np(t) == -77).all() for t in outs) and (to_np(g) == -1).all() and (to_np(a) == 0).all()


if __name__ == "__main__":
    _child_main(sys.argv[1], sys.argv[2] == "cells")
