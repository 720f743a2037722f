"""Downstream walks along a receiver graph (include/soil_hip.h: "flow graphs: downstream"; soil_flow_paths,
soil_flow_paths_batch), what can be checked without a GPU: the two numpy restatements of the definition against each
other and against hand-computed cases, the header, the bound symbols and the surfaces, every refusal of the two
entries with the entry's name in the message, SOIL_ERR_NO_DEVICE for a well-formed call, and the ValueErrors of the
Python layer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import flow_paths_ref as ref
from flow_paths_ref import D4, D8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = np.uint32(ref.NAN_WORD)
SHAPES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 4), (4, 3), (7, 9), (37, 53)]


def _equal(a, b, what):
    for x, y, name in zip(a, b, ("terminal", "steps", "length")):
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape, (what, name)
            assert (ref.words(x) == ref.words(y)).all(), "%s: %s differs" % (what, name)


# ---- (ii) equals (i) -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("edge", [D4, D8])
def test_the_two_restatements_agree_on_the_built_graphs(H, W, edge):
    scale = (0.25, 3.0)
    for name, graph in ref.built_graphs(H, W, edge):
        stops = ref.stop_planes(H, W) if (H, W) != (37, 53) or name in ("cycles", "hostile") else [("none", None)]
        for sname, stop in stops:
            _equal(ref.walk_doubling(graph, edge, scale, stop), ref.walk_serial(graph, edge, scale, stop),
                   "%s, stop %s, %dx%d edge %d" % (name, sname, H, W, edge))


@pytest.mark.parametrize("H,W", [(7, 9), (20, 24)])
@pytest.mark.parametrize("edge", [D4, D8])
@pytest.mark.parametrize("plateaus", [False, True])
def test_the_two_restatements_agree_on_downhill_graphs(H, W, edge, plateaus):
    h = ref.terrain(H, W, 3, plateaus)
    for seed in (None, 11):
        graph = ref.descent(h, edge, seed)
        got = ref.walk_doubling(graph, edge, (1e-3, 1e3))
        _equal(got, ref.walk_serial(graph, edge, (1e-3, 1e3)), "descent seed %r" % (seed,))
        assert (got[0] >= 0).all(), "a downhill graph has no cycle"
        assert (graph.reshape(-1)[got[0].reshape(-1)] == -1).all(), "every terminal is a cell without a receiver"


def test_the_batch_helper_walks_model_by_model():
    graphs = np.stack([ref.serpentine(4, 5), ref.cycles(4, 5), ref.hostile(4, 5, 2)])
    scales = [(1.0, 1.0), (0.25, 3.0), (2.0, 0.5)]
    got = ref.walk_batch(ref.walk_doubling, graphs, D8, scales)
    for b in range(3):
        _equal([o[b] for o in got], ref.walk_serial(graphs[b], D8, scales[b]), "model %d" % b)


# ---- hand-computed cases pin (i) -------------------------------------------------------------------------------

def _f32(*v):
    return np.array(v, np.float32)


def test_a_chain_of_five():
    g = np.array([[1, 2, 3, 4, -1]], np.int32)
    for edge in (D4, D8):
        t, s, l = ref.walk_serial(g, edge, (7.0, 0.5))          # column steps: sy
        assert t.tolist() == [[4, 4, 4, 4, 4]] and s.tolist() == [[4, 3, 2, 1, 0]]
        assert (l == _f32(2.0, 1.5, 1.0, 0.5, 0.0)).all() and l.dtype == np.float32 and t.dtype == s.dtype == np.int32


def test_a_diagonal_step_is_an_edge_under_d8_and_none_under_d4():
    # 0 -> 4 (diagonal) -> 7 (a row step) -> 8 (a column step); every other cell -1
    g = np.full((3, 3), -1, np.int32)
    g[0, 0], g[1, 1], g[2, 1] = 4, 7, 8
    t, s, l = ref.walk_serial(g, D8, (3.0, 4.0))                 # dd = 5
    assert t[0, 0] == 8 and s[0, 0] == 3 and l[0, 0] == np.float32(3.0 + 4.0 + 5.0)
    assert t[1, 1] == 8 and s[1, 1] == 2 and l[1, 1] == np.float32(7.0)
    t, s, l = ref.walk_serial(g, D4, (3.0, 4.0))
    assert t[0, 0] == 0 and s[0, 0] == 0 and l[0, 0] == 0.0      # the same entry is no edge: a terminal
    assert t[1, 1] == 8 and s[1, 1] == 2


def test_a_two_cell_cycle_with_one_feeder():
    g = np.array([[1, 2, 1, -1, 3]], np.int32)                   # 0 -> 1 <-> 2; 3 a terminal; 4 -> 3
    t, s, l = ref.walk_serial(g, D8, (1.0, 1.0))
    assert t.tolist() == [[-1, -1, -1, 3, 3]] and s.tolist() == [[-1, -1, -1, 0, 1]]
    assert (l.view(np.uint32) == np.array([[NAN, NAN, NAN, 0, np.float32(1).view(np.uint32)]], np.uint32)).all()
    stop = np.array([[0, 0, 5, 0, 0]], np.int32)                 # a stop cell on the cycle makes it resolve
    t, s, _ = ref.walk_serial(g, D8, None, stop)
    assert t.tolist() == [[2, 2, 2, 3, 3]] and s.tolist() == [[2, 1, 0, 0, 1]]


def test_a_stop_cell_in_mid_chain():
    g = np.array([[1, 2, 3, 4, -1]], np.int32)
    stop = np.array([[0, 0, 1, 0, 0]], np.int32)
    t, s, l = ref.walk_serial(g, D4, (1.0, 2.0), stop)
    assert t.tolist() == [[2, 2, 2, 4, 4]] and s.tolist() == [[2, 1, 0, 1, 0]]
    assert (l == _f32(4.0, 2.0, 0.0, 2.0, 0.0)).all()


def test_grids_one_and_two_cells_wide():
    g = np.array([[1], [2], [-1], [2]], np.int32)                # W = 1: row steps only
    t, s, l = ref.walk_serial(g, D8, (0.5, 9.0))
    assert t.reshape(-1).tolist() == [2, 2, 2, 2] and s.reshape(-1).tolist() == [2, 1, 0, 1]
    assert (l.reshape(-1) == _f32(1.0, 0.5, 0.0, 0.5)).all()
    # W = 2: cell 1 = (0, 1) -> 2 = (1, 0) is a diagonal, although the indices are neighbours; 2 -> 3 a column step
    g = np.array([[-1, 2], [3, -1]], np.int32)
    t, s, l = ref.walk_serial(g, D8, (3.0, 4.0))
    assert t.tolist() == [[0, 3], [3, 3]] and s.tolist() == [[0, 2], [1, 0]] and l[0, 1] == np.float32(9.0)
    t, s, _ = ref.walk_serial(g, D4, None)
    assert t.tolist() == [[0, 1], [3, 3]] and s.tolist() == [[0, 0], [1, 0]]
    # cell 1 = (0, 1) -> 3 - 1 = 2 is no wrap-around neighbour of (0, 1)'s "right": index 2 is (1, 0)
    g = np.array([[1, 2, -1]], np.int32).reshape(1, 3)
    assert ref.walk_serial(g, D4)[0].tolist() == [[2, 2, 2]]


def test_entries_that_are_no_edge():
    H, W = 3, 4
    for bad in (-1, 5, 3, 11, 7, H * W, H * W + 5, -7, ref.INT32_MIN, ref.INT32_MAX):
        g = np.full((H, W), -1, np.int64)
        g[1, 1] = bad                                            # cell 5: itself, non-neighbours, other numberings
        t, s, _ = ref.walk_serial(g.astype(np.int32), D8)
        assert t[1, 1] == 5 and s[1, 1] == 0, bad


def test_the_length_rounds_once_from_fp64():
    # 3 row steps of 0.1f: (double)0.1f * 3 rounded to float, not 0.1f + 0.1f + 0.1f in float
    g = np.array([[1], [2], [3], [-1]], np.int32)
    l = ref.walk_serial(g, D8, (0.1, 1.0))[2]
    assert l[0, 0] == np.float32(np.float64(np.float32(0.1)) * 3.0)
    dd = np.sqrt(np.float64(np.float32(1e-3)) ** 2 + np.float64(np.float32(1e3)) ** 2)
    g = np.array([[-1, 0], [1, -1]], np.int32)                   # 2 = (1, 0) -> 1 = (0, 1): a diagonal
    assert ref.walk_serial(g, D8, (1e-3, 1e3))[2][1, 0] == np.float32(dd + np.float64(np.float32(1e3)))


# ---- the header, the symbols, the surfaces ---------------------------------------------------------------------

ENTRIES = {
    "soil_flow_paths": "int32_t* terminal, int32_t* steps, float* length, const int32_t* graph, const int32_t* stop, "
                       "int64_t H, int64_t W, int edge, const float scale[2], void* stream",
    "soil_flow_paths_batch": "int32_t* terminal, int32_t* steps, float* length, const int32_t* graph, "
                             "const int32_t* stop, int64_t B, int64_t H, int64_t W, int edge, const float* scales, "
                             "int64_t n_scales, void* stream",
}


def _squash(s):
    return re.sub(r"\s+", " ", s).strip()


def test_the_header_declares_the_entries_and_states_the_contract():
    text = open(os.path.join(ROOT, "include", "soil_hip.h")).read()
    for name, args in ENTRIES.items():
        m = re.search(r"int %s\((.*?)\);" % name, text, re.S)
        assert m, name
        assert _squash(m.group(1)) == args
    flat = _squash(re.sub(r"\n \* ?", "\n", text))
    for phrase in ("(float)(((double)n_row * sx + (double)n_col * sy) + (double)n_diag * dd)", "0x7fc00000",
                   "stop[n] != 0 is a terminal", "INT32_MIN", "H * W - 1 edges", "SOIL_FLOW_BATCH_CELLS",
                   "do not synchronise", "all three outputs null", "n_scales not 1 or B"):
        assert phrase in flat, phrase


def test_the_library_binds_the_entries_and_the_build_has_the_source():
    from soillib_amd import _abi, build
    lib = _abi.lib()
    i64, vp, cint, fp = C.c_int64, C.c_void_p, C.c_int, C.POINTER(C.c_float)
    assert _abi.SIGNATURES["soil_flow_paths"] == (cint, [vp, vp, vp, vp, vp, i64, i64, cint, fp, vp])
    assert _abi.SIGNATURES["soil_flow_paths_batch"] == (cint, [vp, vp, vp, vp, vp, i64, i64, i64, cint, fp, i64, vp])
    for name in ENTRIES:
        assert hasattr(lib, name), name
    found = [s for s in build.SOURCES if "int soil_flow_paths(" in open(os.path.join(build.CSRC, s)).read()]
    assert found == ["flow_paths.hip"]
    graph = open(os.path.join(build.CSRC, "graph.hip")).read()
    assert "flow_paths" not in graph, "the kernels of graph.hip stay as they are"


def test_the_surfaces():
    import soillib
    from soillib_amd import soil
    from soillib_amd.erosion import ErosionBatch, ErosionModel
    for name in ("flow_paths", "basins", "flow_length", "watershed", "flow_paths_batch", "basins_batch",
                 "flow_length_batch"):
        assert callable(getattr(soil, name)) and getattr(soillib, name) is getattr(soil, name), name
    for name in ("basins", "flow_length"):
        assert callable(getattr(ErosionBatch, name)) and not hasattr(ErosionModel, name), name
    text = open(os.path.join(ROOT, "include", "soil.hpp")).read()
    for name in ("flow_paths", "basins", "flow_length", "flow_paths_batch", "basins_batch", "flow_length_batch"):
        assert re.search(r"inline [^;{]*\b%s\(" % name, text), name
    assert "soil_flow_paths(" in text and "soil_flow_paths_batch(" in text
    knobs = open(os.path.join(ROOT, "docs", "KNOBS.md")).read()
    assert "SOIL_PATHS_LIST_FROM" in knobs and "SOIL_PATHS_IDX64" in knobs
    for method in (ErosionBatch.basins, ErosionBatch.flow_length):
        assert "edge" in method.__code__.co_varnames[:method.__code__.co_argcount]


def test_the_call_info_needs_no_device():
    from soillib_amd import _abi, soil
    assert _abi.lib().soil_flow_paths_info(None) == _abi.SOIL_ERR_INVALID_ARGUMENT
    assert _abi.last_error().startswith("flow_paths_info: ")
    assert sorted(soil.flow_paths_info()) == ["chunks", "idx64_chunks", "rounds", "vec_chunks"]


# ---- refusals of the two entries, without a device -------------------------------------------------------------

def _calls():
    """(what, single-grid call or None, batch call): each breaks one rule; `p` stands for a tensor (never read)."""
    from soillib_amd import _abi
    lib = _abi.lib()
    p = C.c_void_p(4096)
    sc = (C.c_float * 6)(1, 1, 1, 1, 1, 1)
    one, many = lib.soil_flow_paths, lib.soil_flow_paths_batch
    big = 1 << 16
    out = [
        ("null graph", lambda: one(p, p, p, None, p, 4, 4, D8, sc, None), lambda: many(p, p, p, None, p, 3, 4, 4, D8, sc, 3, None)),
        ("no output", lambda: one(None, None, None, p, p, 4, 4, D8, sc, None),
         lambda: many(None, None, None, p, None, 3, 4, 4, D8, sc, 1, None)),
        ("length without scale", lambda: one(None, None, p, p, None, 4, 4, D8, None, None),
         lambda: many(p, p, p, p, None, 3, 4, 4, D8, None, 1, None)),
        ("H = 0", lambda: one(p, None, None, p, None, 0, 4, D8, None, None), lambda: many(p, None, None, p, None, 3, 0, 4, D8, None, 1, None)),
        ("W = 0", lambda: one(p, None, None, p, None, 4, 0, D4, None, None), lambda: many(p, None, None, p, None, 3, 4, 0, D4, None, 1, None)),
        ("W < 0", lambda: one(p, None, None, p, None, 4, -2, D4, None, None), lambda: many(p, None, None, p, None, 3, 4, -2, D4, None, 1, None)),
        ("H W > INT32_MAX", lambda: one(p, None, None, p, None, big, big, D8, None, None),
         lambda: many(p, None, None, p, None, 1, big, big // 2, D8, None, 1, None)),
        ("edge 2", lambda: one(p, None, None, p, None, 4, 4, 2, None, None), lambda: many(p, None, None, p, None, 3, 4, 4, 2, None, 1, None)),
        ("edge -1", lambda: one(p, None, None, p, None, 4, 4, -1, None, None), lambda: many(p, None, None, p, None, 3, 4, 4, -1, None, 1, None)),
        ("B = 0", None, lambda: many(p, None, None, p, None, 0, 4, 4, D8, None, 1, None)),
        ("B < 0", None, lambda: many(p, None, None, p, None, -3, 4, 4, D8, None, 1, None)),
        ("n_scales 2 of 3", None, lambda: many(None, None, p, p, None, 3, 4, 4, D8, sc, 2, None)),
        ("n_scales 0", None, lambda: many(None, None, p, p, None, 3, 4, 4, D8, sc, 0, None)),
        ("n_scales 4 of 3", None, lambda: many(p, None, None, p, None, 3, 4, 4, D8, sc, 4, None)),
    ]
    return out


def test_every_refusal_names_its_entry():
    from soillib_amd import _abi
    for what, single, batch in _calls():
        for name, call in (("flow_paths", single), ("flow_paths_batch", batch)):
            if call is None:
                continue
            assert call() == _abi.SOIL_ERR_INVALID_ARGUMENT, (what, name)
            assert _abi.last_error().startswith(name + ": "), (what, name, _abi.last_error())


def test_a_well_formed_call_fails_loudly_without_a_device():
    from soillib_amd import _abi
    lib = _abi.lib()
    if lib.soil_device_count() > 0:
        pytest.skip("a HIP device is present")
    p = C.c_void_p(4096)
    sc = (C.c_float * 6)(1, 1, 1, 1, 1, 1)
    assert lib.soil_flow_paths(p, p, p, p, p, 4, 4, D8, sc, None) == _abi.SOIL_ERR_NO_DEVICE
    assert lib.soil_flow_paths(p, None, None, p, None, 4, 4, D4, None, None) == _abi.SOIL_ERR_NO_DEVICE
    assert lib.soil_flow_paths_batch(p, p, p, p, p, 3, 4, 4, D8, sc, 3, None) == _abi.SOIL_ERR_NO_DEVICE
    assert lib.soil_flow_paths_batch(None, p, None, p, None, 3, 4, 4, D8, None, 1, None) == _abi.SOIL_ERR_NO_DEVICE


# ---- the ValueErrors of the Python layer: before any device work -----------------------------------------------

def _host(dtype, shape):
    from soillib_amd import silt
    return silt.tensor._wrap_numpy(np.zeros(shape, dtype))


def _module_refusals():
    from soillib_amd import soil
    g2, g3 = _host(np.int32, (4, 3)), _host(np.int32, (5, 4, 3))
    return [
        (soil.flow_paths, (g3, soil.d8), {}, r"flow_paths: graph: expected a \(H, W\)"),
        (soil.flow_paths, (_host(np.float32, (4, 3)), soil.d8), {}, "flow_paths: graph: expected an int32"),
        (soil.flow_paths, (np.zeros((4, 3), np.int32), soil.d8), {}, "flow_paths: graph"),
        (soil.flow_paths, (g2, 2), {}, "flow_paths: edge"),
        (soil.flow_paths, (g2, soil.d8), dict(stop=_host(np.int32, (3, 4))), "flow_paths: stop"),
        (soil.flow_paths, (g2, soil.d8), dict(stop=_host(np.float32, (4, 3))), "flow_paths: stop"),
        (soil.flow_paths, (g2, soil.d8), dict(scale=[1.0]), "flow_paths: scale"),
        (soil.flow_paths, (g2, soil.d8), dict(scale=3.0), "flow_paths: scale"),
        (soil.basins, (g3, soil.d4), {}, "basins: graph"),
        (soil.basins, (g2, "d8"), {}, "basins: edge"),
        (soil.flow_length, (g2, soil.d8, [1.0, 2.0, 3.0]), {}, "flow_length: scale"),
        (soil.flow_length, (g2, soil.d8, ["a", "b"]), {}, "flow_length: scale"),
        (soil.watershed, (g3, soil.d8, [(0, 0)]), {}, "watershed: graph"),
        (soil.watershed, (g2, soil.d8, []), {}, "watershed: cells"),
        (soil.watershed, (g2, soil.d8, [(4, 0)]), {}, "watershed: cells"),
        (soil.watershed, (g2, soil.d8, [(0, -1)]), {}, "watershed: cells"),
        (soil.watershed, (g2, soil.d8, 5), {}, "watershed: cells"),
        (soil.flow_paths_batch, (g2, soil.d8), {}, r"flow_paths_batch: graph: expected a \(B, H, W\)"),
        (soil.flow_paths_batch, (_host(np.float32, (5, 4, 3)), soil.d8), {}, "flow_paths_batch: graph"),
        (soil.flow_paths_batch, (g3, 7), {}, "flow_paths_batch: edge"),
        (soil.flow_paths_batch, (g3, soil.d8), dict(stop=_host(np.int32, (4, 4, 3))), "flow_paths_batch: stop"),
        (soil.flow_paths_batch, (g3, soil.d8), dict(scale=[[1.0, 1.0]] * 4), "flow_paths_batch: scale"),
        (soil.basins_batch, (g2, soil.d8), {}, "basins_batch: graph"),
        (soil.basins_batch, (g3, soil.d8), dict(stop=g2), "basins_batch: stop"),
        (soil.flow_length_batch, (g3, soil.d8, [1.0]), {}, "flow_length_batch: scale"),
        (soil.flow_length_batch, (g3, soil.d8, [[1.0, 1.0, 1.0]] * 5), {}, "flow_length_batch: scale"),
        (soil.flow_length_batch, (g3, soil.d8, 1.0), {}, "flow_length_batch: scale"),
    ]


def test_the_module_functions_refuse():
    for fn, args, kw, match in _module_refusals():
        with pytest.raises(ValueError, match=match):
            fn(*args, **kw)


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the refusal came after the planes were touched (%s)" % name)


def _batch_without_a_device(B=5, scales=None):
    from soillib_amd.erosion import ErosionBatch
    bt = ErosionBatch.__new__(ErosionBatch)
    bt.B, bt.H, bt.W = B, 4, 3
    bt.seeds = list(range(B))
    bt.scale, bt.scales = ([1.0, 1.0, 1.0], None) if scales is None else (None, scales)
    bt.height = _Untouchable()
    return bt


def _batch_refusals():
    """(method, the stub's scales, args, kw, match)."""
    good = _host(np.int32, (5, 4, 3))
    out = []
    for method in ("basins", "flow_length"):
        for kw in (dict(graph=_host(np.int32, (5, 3, 4))), dict(graph=_host(np.float32, (5, 4, 3))), dict(graph=3),
                   dict(graph=good, stop=_host(np.int32, (4, 4, 3))), dict(graph=good, stop=_host(np.float32, (5, 4, 3))),
                   dict(graph=good, stop=1), dict(graph=good, edge=2), dict(edge="d4")):
            out.append((method, None, (), kw, r"ErosionBatch\.%s" % method))
    for scales in ([[1.0, 1.0, 1.0]] * 4, [[1.0, 1.0]] * 5, [[1.0, 1.0, "z"]] * 5):
        out.append(("flow_length", scales, (good,), {}, r"ErosionBatch\.flow_length"))
    return out


def test_the_batch_methods_refuse():
    for method, scales, args, kw, match in _batch_refusals():
        with pytest.raises(ValueError, match=match):
            getattr(_batch_without_a_device(scales=scales), method)(*args, **kw)
