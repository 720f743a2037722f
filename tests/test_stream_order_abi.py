"""Stream order and channel segments without a device (include/soil_hip.h: soil_stream_order, soil_stream_order_batch,
soil_stream_order_info): the two restatements of tests/stream_order_ref.py against each other and against closed forms
and hand-placed junctions, that every built case is informative, the header against SIGNATURES, the surfaces, and every
refusal with its text before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import flow_paths_ref as fref
import stream_order_ref as ref
from stream_order_ref import D4, D8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_SHAPES = [(1, 1), (1, 7), (5, 8), (13, 21), (12, 20), (3, 261), (5, 1028), (67, 131)]   # tests/test_gpu_stream_order.py
NOISE_SHAPES = [(13, 21), (12, 20), (67, 131)]


def _same(a, b, what):
    for k in ref.OUTPUTS + ("levels",):
        assert np.array_equal(a[k], b[k]), (what, k)


# ---- the two restatements ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", GPU_SHAPES)
@pytest.mark.parametrize("edge", [D4, D8])
def test_the_levels_are_the_forest_rule_on_every_acyclic_case(H, W, edge):
    seen = 0
    for name, c in ref.cases(H, W, edge).items():
        if not ref.is_acyclic(edge=edge, **c):
            assert name.startswith(("cycles", "hostile")), name
            continue
        _same(ref.by_levels(edge=edge, **c), ref.by_walk(edge=edge, **c), "%s %dx%d edge %d" % (name, H, W, edge))
        seen += 1
    assert seen >= 3


@pytest.mark.parametrize("m", [1, 2, 3, 6])
@pytest.mark.parametrize("edge", [D4, D8])
def test_the_dyadic_tree_has_its_closed_form(m, edge):
    g, order, donors = ref.dyadic(m)
    assert g.shape == (m + 1, 1 << m)
    for fn in (ref.by_levels, ref.by_walk):
        got = fn(g, edge)
        assert np.array_equal(got["order"], order) and np.array_equal(got["donors"], donors)
        assert got["order"].max() == m + 1 == got["levels"]
        assert got["order"][m, 0] == m + 1 and got["channel_graph"][m, 0] == -1
    if m == 6:                                                     # (7, 64): off-tree cells, paths, both survivors
        assert order[3, 5] == 1 and donors[3, 5] == 0 and order[3, 4] == 3 and order[3, 3] == 3 and order[3, 8] == 4


@pytest.mark.parametrize("edge", [D4, D8])
def test_a_comb_has_order_two_and_a_chain_one_level(edge):
    for H, W in ((2, 2), (5, 8), (13, 21)):
        got = ref.by_levels(ref.comb(H, W), edge)
        want = np.ones((H, W), np.int32)
        want[1:, 0] = 2
        assert np.array_equal(got["order"], want) and got["levels"] == 2
        assert np.array_equal(got["link_foot"][:, 1], np.r_[0, np.ones(H - 1, np.int32)])   # (row 0 joins no junction)
        chain = ref.by_levels(fref.serpentine(H, W), edge)
        assert (chain["order"] == 1).all() and chain["levels"] == 1 and chain["link_foot"].sum() == 1
        assert chain["donors"].sum() == H * W - 1 and chain["donors"].max() == 1


@pytest.mark.parametrize("edge", [D4, D8])
def test_junctions_of_mixed_orders_by_hand(edge):
    """(2, 2, 1) -> 3, (3, 2, 2) -> 3, (2, 1, 1) -> 2, and a single donor keeps its order."""
    for fn in (ref.by_levels, ref.by_walk):
        got = fn(ref.mixed(), edge)
        for at, o in ref.MIXED_ORDERS.items():
            assert got["order"][at] == o, (at, o, got["order"][at])
        for at, d in ref.MIXED_DONORS.items():
            assert got["donors"][at] == d, (at, d)
        assert got["levels"] == 3
        # a link ends above every junction; a Strahler stream only where the order rises
        assert got["link_foot"][3, 3] == 1 and got["order_foot"][3, 3] == 0         # (4, 3) is a junction of order 3
        assert got["link_foot"][2, 2] == 1 and got["order_foot"][2, 2] == 1
        assert got["link_foot"][2, 9] == 1 and got["order_foot"][2, 9] == 0         # 2 into (2, 1, 1) -> 2
        assert got["link_foot"][6, 3] == 1 and got["order_foot"][6, 3] == 1         # the outlet
        assert got["link_foot"][4, 3] == 0 and got["order_foot"][5, 3] == 0
    stopped = ref.by_levels(ref.mixed(), edge, stop=ref.cases(7, 13, edge)["mixed_stop"]["stop"])
    assert stopped["order"][2, 3] == 2 and stopped["donors"][2, 3] == 2 and stopped["order"][2, 2] == 2
    assert stopped["channel_graph"][2, 2] == -1 and stopped["link_foot"][2, 2] == 1


def test_d4_ignores_diagonal_entries():
    g = fref.all_donors(5, 8, D8)
    d4, d8 = ref.by_levels(g, D4), ref.by_levels(g, D8)
    assert d8["donors"].max() == 8 and d4["donors"].max() == 4
    assert d8["order"][1, 1] == 2 == d4["order"][1, 1] and (d4["channel_graph"][0, 0], d8["channel_graph"][0, 0]) == (-1, 9)


def test_cycles_take_the_levels():
    """An isolated cycle has order 1; one that a tree drains into has the tree's order plus one all round."""
    g = ref.drawn([">v.", "^<<"])
    got = ref.by_levels(g, D8)
    assert got["order"].tolist() == [[2, 2, 1], [2, 2, 1]] and got["levels"] == 2
    assert ref.by_levels(ref.drawn([">v", "^<"]), D8)["order"].tolist() == [[1, 1], [1, 1]]
    assert not ref.is_acyclic(g, D8)
    big = ref.by_levels(fref.cycles(5, 8), D8)
    assert big["order"][0, 0] == 2 and big["order"][4, 0] == 2 and big["order"][2, 1] == 2 and big["order"][0, 7] == 1


def test_the_area_comparison_is_a_float_comparison():
    a = np.array([[np.nan, np.inf, -np.inf, 4.0, np.float32(4.0) - np.float32(4e-7), -0.0]], np.float32)
    g = np.full((1, 6), -1, np.int32)
    assert ref.by_levels(g, D8, area=a, threshold=4.0)["order"].tolist() == [[0, 1, 0, 1, 0, 0]]
    assert ref.by_levels(g, D8, area=a, threshold=-np.inf)["order"].tolist() == [[0, 1, 1, 1, 1, 1]]
    assert ref.by_levels(g, D8, area=a, threshold=0.0)["order"].tolist() == [[0, 1, 0, 1, 1, 1]]
    hole = ref.by_levels(ref.comb(3, 6), D8, channel=np.array([[1, 1, 0, 1, 1, 1]] * 3, np.int32))
    assert hole["channel_graph"][0].tolist() == [6, 0, -1, -1, 3, 4] and hole["order"][0].tolist() == [1, 1, 0, 1, 1, 1]
    assert hole["link_foot"][0].tolist() == [1, 0, 0, 1, 0, 0]      # above the junction (1, 0); where the stream leaves


# ---- the cases are informative -------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", NOISE_SHAPES)
@pytest.mark.parametrize("edge", [D4, D8])
def test_the_noise_graphs_have_three_orders_and_feet_of_both_kinds(oracle, H, W, edge):
    g = oracle.steepest(ref.noise_height(oracle, H, W), edge)
    got = ref.by_levels(g, edge)
    _same(got, ref.by_walk(g, edge), "oracle.steepest")
    assert len(np.unique(got["order"])) >= 3
    for k in ("link_foot", "order_foot"):
        assert set(np.unique(got[k]).tolist()) == {0, 1}, k
    assert (got["link_foot"] != got["order_foot"]).any()
    cut = ref.by_levels(g, edge, area=ref.upstream_count(g, edge), threshold=3.0)
    assert (cut["order"] == 0).any() and cut["order"].max() >= 2 and (cut["order"] != got["order"]).any()


@pytest.mark.parametrize("H,W", [(5, 8), (13, 21), (12, 20), (67, 131)])
def test_every_built_case_is_informative(H, W):
    cases = ref.cases(H, W, D8)
    assert {"chain", "comb", "comb_holes", "comb_stop", "hostile", "all_donors", "cycles", "descent_all"} <= set(cases)
    got = {k: ref.by_levels(edge=D8, **c) for k, c in cases.items()}
    assert got["chain"]["levels"] == 1 and got["comb"]["levels"] == 2 and got["descent"]["levels"] >= (3 if H * W > 200 else 2)
    for k in ("comb", "descent", "descent_all"):
        assert set(np.unique(got[k]["link_foot"]).tolist()) == {0, 1}, k
        assert set(np.unique(got[k]["order_foot"]).tolist()) == {0, 1}, k
    assert (got["descent"]["link_foot"] != got["descent"]["order_foot"]).any()
    assert (got["comb_holes"]["order"] == 0).any() and (got["comb_holes"]["order"] != got["comb"]["order"]).any()
    assert (got["comb_stop"]["order"] != got["comb"]["order"]).any()
    assert (got["descent_all"]["order"] == 0).any() and got["descent_all"]["order"].max() >= 2
    assert got["all_donors"]["donors"].max() == 8
    assert not ref.is_acyclic(edge=D8, **cases["cycles"]) and got["cycles"]["order"].max() >= 2
    if H >= 7 and W >= 13:
        assert got["mixed"]["levels"] == 3 and got["mixed_stop"]["order"][2, 3] == 2


def test_segments_and_magnitude_on_the_dyadic_tree():
    g, order, donors = ref.dyadic(3)
    planes = ref.by_levels(g, D8)
    o, seg, steps, length = ref.segments(planes, D8, (1.0, 2.0), "link")
    assert seg[0, 5] == 8 + 5 and steps[0, 5] == 1 and length[0, 5] == np.float32(1.0)   # the odd survivor below: a foot
    assert seg[2, 2] == 2 * 8 + 1 and steps[2, 2] == 1 and length[2, 2] == np.float32(2.0)
    o2, seg2, steps2, _ = ref.segments(planes, D8, None, "order")
    assert seg2[0, 1] == 8 + 1 and steps2[0, 1] == 1               # order 1 runs on through row 1's odd survivor
    assert seg2[0, 0] == 0 and steps2[0, 0] == 0                   # ... and ends at once above an even one
    assert seg2[2, 7] == 2 * 8 + 7 and order[2, 7] == 1            # an off-tree cell is its own stream
    mag = ref.magnitude(planes)
    assert mag[3, 0] == 8.0 and mag[1, 0] == 2.0 and mag[0, 3] == 1.0 and mag[2, 2] == 2.0 and mag[2, 7] == 1.0
    cut = ref.by_levels(g, D8, channel=(order > 1).astype(np.int32))
    assert ref.magnitude(cut)[0, 0] == 0.0 and ref.segments(cut, D8)[1][0, 3] == 3


# ---- the header, the bindings, the surfaces ------------------------------------------------------------------------

ENTRIES = {
    "soil_stream_order": "int32_t* order, int32_t* donors, int32_t* link_foot, int32_t* order_foot, int32_t* channel_graph, "
                         "const int32_t* graph, const int32_t* channel, const float* area, float threshold, "
                         "const int32_t* stop, int64_t H, int64_t W, int edge, void* stream",
    "soil_stream_order_batch": "int32_t* order, int32_t* donors, int32_t* link_foot, int32_t* order_foot, "
                               "int32_t* channel_graph, const int32_t* graph, const int32_t* channel, const float* area, "
                               "float threshold, const int32_t* stop, int64_t B, int64_t H, int64_t W, int edge, "
                               "void* stream",
    "soil_stream_order_info": "int64_t info[5]",
}
_CTYPES = {"int32_t*": C.c_void_p, "const int32_t*": C.c_void_p, "const float*": C.c_void_p, "void*": C.c_void_p,
           "float": C.c_float, "int64_t": C.c_int64, "int": C.c_int}


def _squash(s):
    return re.sub(r"\s+", " ", s).strip()


def test_the_header_declares_the_entries_and_signatures_match_it():
    from soillib_amd import _abi
    text = open(os.path.join(ROOT, "include", "soil_hip.h")).read()
    for name, args in ENTRIES.items():
        m = re.search(r"int %s\((.*?)\);" % name, text, re.S)
        assert m, name
        assert _squash(m.group(1)) == args
        if name.endswith("_info"):
            assert _abi.SIGNATURES[name] == (C.c_int, [C.POINTER(C.c_int64)])
            continue
        want = [_CTYPES[a.rsplit(" ", 1)[0]] for a in args.split(", ")]
        assert _abi.SIGNATURES[name] == (C.c_int, want), name
    flat = _squash(re.sub(r"\n \* ?", "\n", text))
    for phrase in ("word for word those of soil_flow_paths", "a NaN area fails", "donors[n] is the number of channel-graph edges",
                   "J_k = the cells of M_1 with at least two donors in M_k", "the largest k with n in M_k",
                   "iff two donors are in M_k", "one donor is in M_{k+1}", "Cycles are allowed",
                   "link_foot[n] = 1 iff", "order_foot[n] = 1 iff", "-1 elsewhere", "Every output may be NULL, not all",
                   "floor(log2(H * W)) + 1", "SYNCHRONISE THE STREAM", "a NaN `threshold` with `area` given"):
        assert phrase in flat, phrase


def test_the_library_binds_the_entries_and_the_build_has_the_source():
    from soillib_amd import _abi, build
    lib = _abi.lib()
    for name in ENTRIES:
        assert hasattr(lib, name), name
    found = [s for s in build.SOURCES if "int soil_stream_order(" in open(os.path.join(build.CSRC, s)).read()]
    assert found == ["stream_order.hip"]
    source = open(os.path.join(build.CSRC, "stream_order.hip")).read()
    assert "atomicMax" in source and "WS_STREAM_ORDER" in source and "ptr_rounds" in source
    assert "stream_order" not in open(os.path.join(ROOT, "include", "soil.hpp")).read()
    assert "SOIL_STREAM_ORDER_NARROW" in open(os.path.join(ROOT, "docs", "KNOBS.md")).read()


def test_the_surfaces():
    import soillib
    from soillib_amd import soil
    from soillib_amd.erosion import ErosionBatch, ErosionModel
    for name in ("stream_order", "stream_order_batch", "stream_order_info", "stream_segments", "stream_segments_batch",
                 "stream_magnitude", "stream_magnitude_batch"):
        assert callable(getattr(soil, name)) and getattr(soillib, name) is getattr(soil, name), name
    for name in ("stream_order", "stream_segments"):
        assert callable(getattr(ErosionBatch, name)) and not hasattr(ErosionModel, name), name
    assert "its own foot at" in soil.stream_segments.__doc__ and "order == 0" in soil.stream_segments.__doc__


def test_the_info_record_is_all_zero_before_a_call_and_needs_no_device():
    from soillib_amd import _abi, soil
    assert _abi.lib().soil_stream_order_info(None) == _abi.SOIL_ERR_INVALID_ARGUMENT
    assert _abi.last_error() == "stream_order_info: null info"
    import threading
    seen = []
    t = threading.Thread(target=lambda: seen.append(soil.stream_order_info()))   # a thread that never made a call
    t.start()
    t.join()
    assert seen == [dict(chunks=0, vec_chunks=0, idx64_chunks=0, rounds=0, levels=0)]


# ---- refusals of the two entries, without a device -----------------------------------------------------------------

def _calls():
    """(what, the text after the entry's name, single-grid call or None, batch call): each breaks one rule; the
    pointers stand for planes of 4 x 4 cells (never read)."""
    from soillib_amd import _abi
    lib = _abi.lib()
    cells = 3 * 16 * 4
    o, d, lf, of, cg, g, ch, a, s = (C.c_void_p(1 << 20 + i) for i in range(9))   # far apart
    inside = lambda p, off: C.c_void_p(p.value + off)              # noqa: E731
    nan = float("nan")

    def one(outs, ins, H=4, W=4, edge=D8, th=1.0):
        return lambda: lib.soil_stream_order(*outs, *ins[:3], th, ins[3], H, W, edge, None)

    def many(outs, ins, B=3, H=4, W=4, edge=D8, th=1.0):
        return lambda: lib.soil_stream_order_batch(*outs, *ins[:3], th, ins[3], B, H, W, edge, None)
    outs, ins = (o, d, lf, of, cg), (g, ch, a, s)
    none = (None,) * 5
    only = lambda i, p: tuple(p if k == i else None for k in range(5))   # noqa: E731
    big = 1 << 16
    no_out = "no output asked for (order, donors, link_foot, order_foot and channel_graph are all null)"
    shape_text = "a model must have 1..2^31-1 cells (int32 graph)"
    alias = "an output aliases an input plane"
    out = [
        ("null graph", "null graph", one(outs, (None, ch, a, s)), many(outs, (None, ch, a, s))),
        ("no output", no_out, one(none, ins), many(none, (g, None, None, None))),
        ("H = 0", "empty grid", one(outs, ins, H=0), many(outs, ins, H=0)),
        ("W = 0", "empty grid", one(outs, ins, W=0, edge=D4), many(outs, ins, W=0, edge=D4)),
        ("W < 0", "empty grid", one(only(1, d), ins, W=-2), many(only(1, d), ins, W=-2)),
        ("H W > INT32_MAX", shape_text, one(outs, ins, H=big, W=big), many(outs, ins, B=1, H=big, W=big // 2)),
        ("edge 2", "invalid edge enumerator", one(outs, ins, edge=2), many(outs, ins, edge=2)),
        ("edge -1", "invalid edge enumerator", one(outs, ins, edge=-1), many(outs, ins, edge=-1)),
        ("B = 0", "B must be >= 1", None, many(outs, ins, B=0)),
        ("B < 0", "B must be >= 1", None, many(outs, ins, B=-3)),
        ("NaN threshold", "threshold is NaN", one(outs, ins, th=nan), many(outs, ins, th=nan)),
        ("order is graph", alias, one((g, d, lf, of, cg), ins), many((g, d, lf, of, cg), ins)),
        ("donors is channel", alias, one(only(1, ch), ins), many(only(1, ch), ins)),
        ("link_foot is area", alias, one(only(2, a), ins), many(only(2, a), ins)),
        ("order_foot inside stop", alias, one(only(3, inside(s, 60)), ins), many(only(3, inside(s, cells - 4)), ins)),
        ("channel_graph ends inside graph", alias, one(only(4, inside(g, -60)), ins), many(only(4, inside(g, 4 - cells)), ins)),
        ("order is donors", "two outputs overlap", one((o, o, None, None, None), ins), many((o, inside(o, cells - 4), lf, of, cg), ins)),
        ("the feet overlap", "two outputs overlap", one((None, None, lf, inside(lf, 60), None), ins),
         many((None, None, lf, inside(lf, 4 - cells), None), ins)),
        ("channel_graph is order", "two outputs overlap", one((o, d, lf, of, o), ins), many((o, d, lf, of, o), ins)),
    ]
    return out


def test_every_refusal_names_its_entry_and_has_its_text():
    from soillib_amd import _abi
    for what, text, single, batch in _calls():
        for name, call in (("stream_order", single), ("stream_order_batch", batch)):
            if call is None:
                continue
            assert call() == _abi.SOIL_ERR_INVALID_ARGUMENT, (what, name)
            assert _abi.last_error() == "%s: %s" % (name, text), (what, name, _abi.last_error())


def test_a_nan_threshold_without_an_area_and_planes_side_by_side_pass_the_checks():
    """Such calls get as far as looking for a device."""
    from soillib_amd import _abi
    lib = _abi.lib()
    if lib.soil_device_count() > 0:
        pytest.skip("a HIP device is present")
    p = [C.c_void_p((1 << 20) + 64 * i) for i in range(9)]          # nine planes of 4 x 4 cells, back to back
    nan = float("nan")
    assert lib.soil_stream_order(*p[:5], p[5], p[6], None, nan, p[8], 4, 4, D8, None) == _abi.SOIL_ERR_NO_DEVICE
    assert lib.soil_stream_order(*p[:5], p[5], p[6], p[7], 1.0, p[8], 4, 4, D4, None) == _abi.SOIL_ERR_NO_DEVICE
    for i in range(5):                                             # each output alone, every optional input NULL
        outs = [p[i] if k == i else None for k in range(5)]
        assert lib.soil_stream_order(*outs, p[5], None, None, 0.0, None, 4, 4, D8, None) == _abi.SOIL_ERR_NO_DEVICE
        assert lib.soil_stream_order_batch(*outs, p[5], None, None, 0.0, None, 1, 4, 4, D8, None) == _abi.SOIL_ERR_NO_DEVICE


# ---- the ValueErrors of the Python layer: before any device work ---------------------------------------------------

def _host(dtype, shape):
    from soillib_amd import silt
    return silt.tensor._wrap_numpy(np.zeros(shape, dtype))


def test_the_module_functions_refuse():
    from soillib_amd import soil
    g2, g3 = _host(np.int32, (4, 3)), _host(np.int32, (5, 4, 3))
    v2, v3 = _host(np.float32, (4, 3)), _host(np.float32, (5, 4, 3))
    for fn, args, kw, match in [
            (soil.stream_order, (g3, soil.d8), {}, r"stream_order: graph: expected a \(H, W\)"),
            (soil.stream_order, (v2, soil.d8), {}, "stream_order: graph: expected an int32"),
            (soil.stream_order, (g2, 2), {}, "stream_order: edge"),
            (soil.stream_order, (g2, soil.d8), dict(channel=v2), "stream_order: channel: expected an int32"),
            (soil.stream_order, (g2, soil.d8), dict(area=g2, threshold=1.0), "stream_order: area: expected a float32"),
            (soil.stream_order, (g2, soil.d8), dict(area=v2), "stream_order: area needs a threshold"),
            (soil.stream_order, (g2, soil.d8), dict(threshold=2.0), "stream_order: threshold needs an area"),
            (soil.stream_order, (g2, soil.d8), dict(area=v2, threshold=float("nan")), "stream_order: threshold is NaN"),
            (soil.stream_order, (g2, soil.d8), dict(stop=_host(np.int32, (3, 4))), "stream_order: stop"),
            (soil.stream_order_batch, (g2, soil.d8), {}, r"stream_order_batch: graph: expected a \(B, H, W\)"),
            (soil.stream_order_batch, (g3, soil.d8), dict(area=v2, threshold=1.0), "stream_order_batch: area"),
            (soil.stream_segments, (g2, soil.d8), dict(by="basin"), "stream_segments: by must be 'link' or 'order'"),
            (soil.stream_segments, (g2, "d8"), {}, "stream_segments: edge"),
            (soil.stream_segments_batch, (g3, soil.d8), dict(channel=g2), "stream_segments_batch: channel"),
            (soil.stream_magnitude, (g3, soil.d8), {}, "stream_magnitude: graph"),
            (soil.stream_magnitude_batch, (g3, soil.d8), dict(stop=v3), "stream_magnitude_batch: stop")]:
        with pytest.raises(ValueError, match=match):
            fn(*args, **kw)


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the refusal came after the planes were touched (%s)" % name)


def test_the_batch_methods_refuse():
    from soillib_amd.erosion import ErosionBatch
    good, value = _host(np.int32, (5, 4, 3)), _host(np.float32, (5, 4, 3))
    for method in ("stream_order", "stream_segments"):
        for args, kw in (((float("nan"),), {}), (("3",), {}), ((2.0,), dict(edge=2)), ((2.0,), dict(kind="direction")),
                         ((2.0,), dict(graph=value)), ((2.0,), dict(graph=good, area=good)),
                         ((2.0,), dict(graph=_host(np.int32, (5, 3, 4))))):
            bt = ErosionBatch.__new__(ErosionBatch)
            bt.B, bt.H, bt.W = 5, 4, 3
            bt.scale, bt.scales = [1.0, 1.0, 1.0], None
            bt.height = _Untouchable()
            with pytest.raises(ValueError, match=r"ErosionBatch\.%s" % method):
                getattr(bt, method)(*args, **kw)
