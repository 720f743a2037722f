"""Downstream sums along a receiver graph and the implicit stream-power step (include/soil_hip.h: "flow graphs:
downstream sums"; soil_downstream, soil_stream_power and their _batch forms), what can be checked without a GPU: the
two numpy restatements of tests/downstream_ref.py against each other, hand-computed cases that pin the definition,
identities that tie it to soil_flow_paths' restatement, the header, the bound symbols and the surfaces, every refusal
of the four entries with the entry's name in the message, SOIL_ERR_NO_DEVICE for a well-formed call, and the
ValueErrors of the Python layer.

The bound between the restatements.  solve_doubling and solve_serial associate the same sum differently.  With
a, b, t >= 0 and finite every term is non-negative, nothing cancels, and each of the two carries a relative error
below 3 H W 2^-53 (at most H W - 1 edges, a product and a sum per edge, a coefficient's rounding) — below 2^-25 for
H W <= 2^20, a small fraction of a float32's half ulp — so their float32 results differ by at most 1 ulp (the two
fp64 values may lie on the two sides of a rounding boundary).  With signed coefficients a sum can cancel to any
relative error: only the sets of resolved cells are compared."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import downstream_ref as dref
import flow_paths_ref as ref
from flow_paths_ref import D4, D8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 4), (4, 3), (7, 9), (37, 53)]


def _draws(H, W, seed, signed=False):
    """a, b, t planes and stream-power planes of a (H, W) grid."""
    r = np.random.default_rng([seed, H, W])
    lo = -1.0 if signed else 0.0
    a, b, t = (r.uniform(lo, 1.0, (H, W)).astype(np.float32) for _ in range(3))
    height = (r.random((H, W)) * 100.0).astype(np.float32)
    erosivity = np.exp(r.uniform(np.log(1e-6), np.log(1e3), (H, W))).astype(np.float32)
    uplift = (r.random((H, W)) * 0.01).astype(np.float32)
    return a, b, t, (height, erosivity, uplift, 3.5)


def _close(got, want, what, ulps):
    assert (got[2] == want[2]).all(), "%s: the resolved cells differ" % what
    if ulps is not None:
        d = dref.ulps32(got[0], want[0])
        assert d.max() <= ulps, "%s: %d ulps at cell %d" % (what, d.max(), d.argmax())
        unresolved = ~got[2]
        assert (dref.words(got[0])[unresolved] == dref.NAN32).all() and (dref.words(got[1])[unresolved] == dref.NAN64).all()


# ---- (i) against (ii) ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("edge", [D4, D8])
def test_the_two_restatements_agree_on_the_built_graphs(H, W, edge):
    a, b, t, power = _draws(H, W, 1)
    sa, sb, st, _ = _draws(H, W, 2, signed=True)
    for name, graph in ref.built_graphs(H, W, edge):
        stops = ref.stop_planes(H, W) if (H, W) != (37, 53) or name == "cycles" else [("none", None)]
        for sname, stop in stops:
            what = "%s, stop %s, %dx%d edge %d" % (name, sname, H, W, edge)
            args = (graph, edge)
            _close(dref.solve_doubling(*args, a, b, t, (0.25, 3.0), stop), dref.solve_serial(*args, a, b, t, (0.25, 3.0), stop),
                   what + ", a b t", 1)
            _close(dref.solve_doubling(*args, stop=stop), dref.solve_serial(*args, stop=stop), what + ", all null", 0)
            _close(dref.solve_doubling(*args, scale=(0.25, 3.0), stop=stop, power=power),
                   dref.solve_serial(*args, scale=(0.25, 3.0), stop=stop, power=power), what + ", stream power", 1)
            _close(dref.solve_doubling(*args, sa, sb, st, (0.25, 3.0), stop), dref.solve_serial(*args, sa, sb, st, (0.25, 3.0), stop),
                   what + ", signed", None)


@pytest.mark.parametrize("H,W", [(7, 9), (20, 24)])
@pytest.mark.parametrize("edge", [D4, D8])
def test_the_two_restatements_agree_on_downhill_graphs(H, W, edge):
    a, b, t, power = _draws(H, W, 3)
    h = ref.terrain(H, W, 3)
    for seed in (None, 11):
        graph = ref.descent(h, edge, seed)
        got = dref.solve_doubling(graph, edge, a, b, t, (1e-3, 1e3))
        _close(got, dref.solve_serial(graph, edge, a, b, t, (1e-3, 1e3)), "descent seed %r" % (seed,), 1)
        assert got[2].all(), "a downhill graph has no cycle"
        pw = (h, power[1], power[2], power[3])
        _close(dref.solve_doubling(graph, edge, scale=(0.5, 2.0), power=pw), dref.solve_serial(graph, edge, scale=(0.5, 2.0), power=pw),
               "descent seed %r, stream power" % (seed,), 1)


def test_the_batch_helper_solves_model_by_model():
    graphs = np.stack([ref.serpentine(4, 5), ref.cycles(4, 5), ref.hostile(4, 5, 2)])
    a = np.stack([_draws(4, 5, 10 + i)[0] for i in range(3)])
    scales = [(1.0, 1.0), (0.25, 3.0), (2.0, 0.5)]
    got = dref.solve_batch(dref.solve_doubling, graphs, D8, a=a, scale=scales)
    for i in range(3):
        one = dref.solve_doubling(graphs[i], D8, a=a[i], scale=scales[i])
        assert all((dref.words(g[i]) == dref.words(o)).all() for g, o in zip(got[:2], one[:2])) and (got[2][i] == one[2]).all()


# ---- hand-computed cases pin (i) and (ii) ----------------------------------------------------------------------

def _both(*args, **kw):
    one, two = dref.solve_doubling(*args, **kw), dref.solve_serial(*args, **kw)
    for x, y in zip(one, two):
        assert (dref.words(x) == dref.words(y)).all() if x.dtype != bool else (x == y).all()
    assert one[0].dtype == np.float32 and one[1].dtype == np.float64 and one[2].dtype == bool
    return one


def _f32(*v):
    return np.array(v, np.float32)


def test_a_chain_of_five_with_b_one_half():
    g = np.array([[1, 2, 3, 4, -1]], np.int32)
    b = np.full((1, 5), 0.5, np.float32)
    t = _f32(0, 0, 0, 0, 8).reshape(1, 5)
    for edge in (D4, D8):
        out, out64, final = _both(g, edge, b=b, t=t)             # x = 1 + x[r] / 2 from x[4] = 8
        assert out.tolist() == [[2.375, 2.75, 3.5, 5.0, 8.0]] and (out64 == out).all() and final.all()
        out, _, _ = _both(g, edge, a=_f32(4, 4, 4, 4, 4).reshape(1, 5), b=b, t=t, scale=(7.0, 0.25))   # column steps: sy
        assert out.tolist() == [[2.375, 2.75, 3.5, 5.0, 8.0]]


def test_a_diagonal_step_is_an_edge_under_d8_and_none_under_d4():
    g = np.full((3, 3), -1, np.int32)
    g[0, 0], g[1, 1], g[2, 1] = 4, 7, 8                          # 0 -> 4 (diagonal) -> 7 (a row step) -> 8 (a column step)
    t = np.arange(9, dtype=np.float32).reshape(3, 3) * 100
    out, _, _ = _both(g, D8, t=t, scale=(3.0, 4.0))              # dd = 5
    assert out[0, 0] == 5.0 + 3.0 + 4.0 + 800.0 and out[1, 1] == 807.0 and out[2, 1] == 804.0
    out, _, _ = _both(g, D4, t=t, scale=(3.0, 4.0))
    assert out[0, 0] == 0.0 and out[1, 1] == 807.0               # the same entry is no edge: cell 0 keeps its t


def test_a_stop_cell_in_mid_chain():
    g = np.array([[1, 2, 3, 4, -1]], np.int32)
    stop = np.array([[0, 0, 1, 0, 0]], np.int32)
    out, _, final = _both(g, D4, t=_f32(1, 2, 10, 3, 20).reshape(1, 5), stop=stop)
    assert out.tolist() == [[12.0, 11.0, 10.0, 21.0, 20.0]] and final.all()


def test_a_two_cell_cycle_with_one_feeder():
    g = np.array([[1, 2, 1, -1, 3]], np.int32)                   # 0 -> 1 <-> 2; 3 a terminal; 4 -> 3
    out, out64, final = _both(g, D8, t=_f32(0, 0, 0, 6, 0).reshape(1, 5))
    assert final.tolist() == [[False, False, False, True, True]]
    assert dref.words(out).tolist() == [[0x7fc00000] * 3 + [int(np.float32(6).view(np.uint32)), int(np.float32(7).view(np.uint32))]]
    assert (dref.words(out64)[0, :3] == dref.NAN64).all() and out64[0, 3:].tolist() == [6.0, 7.0]
    stop = np.array([[0, 0, 5, 0, 0]], np.int32)                 # a stop cell on the cycle makes it resolve
    assert _both(g, D8, stop=stop)[0].tolist() == [[2.0, 1.0, 0.0, 0.0, 1.0]]


def test_a_grid_one_cell_wide():
    g = np.array([[1], [2], [-1], [2]], np.int32)                # W = 1: row steps only
    out, _, _ = _both(g, D8, scale=(0.5, 9.0))
    assert out.reshape(-1).tolist() == [1.0, 0.5, 0.0, 0.5]


def test_a_nan_is_the_canonical_word_and_spreads_upstream():
    g = np.array([[1, 2, 3, -1, 3]], np.int32)
    bits = _f32(1, np.nan, 1, 1, 1).reshape(1, 5).view(np.uint32).copy()
    bits[0, 1] |= np.uint32(0x12345)                             # a NaN with a payload
    out, out64, final = _both(g, D8, a=bits.view(np.float32))
    assert final.all() and dref.words(out).tolist()[0][:2] == [0x7fc00000] * 2 and out[0, 2:].tolist() == [1.0, 0.0, 1.0]
    assert (dref.words(out64)[0, :2] == dref.NAN64).all()


def test_one_stream_power_cell_by_hand():
    g = np.array([[1, -1]], np.int32)                            # a column step of length sy = 4
    h, k, u = _f32(10, 2).reshape(1, 2), _f32(0.5, 77).reshape(1, 2), _f32(1.25, 99).reshape(1, 2)
    out, out64, _ = dref.solve_doubling(g, D8, scale=(9.0, 4.0), power=(h, k, u, 2.0))
    F = np.float64(0.5) * 2.0 / 4.0                              # 0.25
    want = (10.0 + 2.0 * 1.25) / (1.0 + F) + (F / (1.0 + F)) * 2.0          # A0 + B0 h'[r]
    assert out64[0, 0] == want and out[0, 0] == np.float32(want) and abs(want - 10.4) < 1e-14
    assert out64[0, 1] == 2.0, "the terminal is the base level: neither lifted nor eroded"
    serial = dref.solve_serial(g, D8, scale=(9.0, 4.0), power=(h, k, u, 2.0))
    assert abs(serial[1][0, 0] - 10.4) < 1e-14 and serial[0][0, 0] == out[0, 0]
    same = dref.solve_doubling(g, D8, scale=(9.0, 4.0), power=(h, k, None, 0.0))      # dt = 0: the heights
    assert (same[1] == h).all()


# ---- identities with the walks of flow_paths_ref ---------------------------------------------------------------

@pytest.mark.parametrize("H,W", [(5, 1), (3, 4), (7, 9), (20, 24)])
@pytest.mark.parametrize("edge", [D4, D8])
def test_identities_with_the_walk(H, W, edge):
    cells = np.arange(H * W, dtype=np.float32).reshape(H, W)
    zeros, ones = np.zeros((H, W), np.float32), np.ones((H, W), np.float32)
    for name, graph in ref.built_graphs(H, W, edge):
        for sname, stop in ref.stop_planes(H, W):
            what = "%s, stop %s" % (name, sname)
            terminal, steps, length = ref.walk_doubling(graph, edge, (0.25, 8.0), stop)
            ok = terminal >= 0
            out, out64, final = dref.solve_doubling(graph, edge, stop=stop)
            assert (final == ok).all() and (out[ok] == steps[ok]).all() and (out64[ok] == steps[ok]).all(), what
            out = dref.solve_doubling(graph, edge, t=cells, a=zeros, stop=stop)[0]
            assert (out[ok] == terminal[ok]).all(), what
            with_b = dref.solve_doubling(graph, edge, t=cells, b=ones, scale=(0.25, 8.0), stop=stop)
            without = dref.solve_doubling(graph, edge, t=cells, scale=(0.25, 8.0), stop=stop)
            assert all((dref.words(p) == dref.words(q)).all() for p, q in zip(with_b[:2], without[:2])), what
            if edge == D4:                                       # dyadic scales, no diagonal: every partial sum is exact
                out = dref.solve_doubling(graph, edge, scale=(0.25, 8.0), stop=stop)[0]
                assert (dref.words(out) == ref.words(length)).all(), what


# ---- the header, the symbols, the surfaces ---------------------------------------------------------------------

ENTRIES = {
    "soil_downstream": "float* out, double* out64, const int32_t* graph, const float* a, const float* b, const float* t, "
                       "const int32_t* stop, int64_t H, int64_t W, int edge, const float scale[2], void* stream",
    "soil_downstream_batch": "float* out, double* out64, const int32_t* graph, const float* a, const float* b, "
                             "const float* t, const int32_t* stop, int64_t B, int64_t H, int64_t W, int edge, "
                             "const float* scales, int64_t n_scales, void* stream",
    "soil_stream_power": "float* out, double* out64, const float* height, const int32_t* graph, const float* erosivity, "
                         "const float* uplift, const int32_t* stop, int64_t H, int64_t W, int edge, const float scale[2], "
                         "double dt, void* stream",
    "soil_stream_power_batch": "float* out, double* out64, const float* height, const int32_t* graph, "
                               "const float* erosivity, const float* uplift, const int32_t* stop, int64_t B, int64_t H, "
                               "int64_t W, int edge, const float* scales, int64_t n_scales, double dt, void* stream",
    "soil_downstream_info": "int64_t info[4]",
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
    for phrase in ("x[n] = a[n] * L(n) + b[n] * x[r(n)]", "A <- A + (B * A_p)", "B <- B * B_p", "__dmul_rn, __dadd_rn",
                   "0x7fc00000 / 0x7ff8000000000000", "one definite bit pattern", "b == NULL gives the bits of b == 1.0",
                   "F = ((double)erosivity[n] * dt) / L", "B0 = F / d", "slope exponent n = 1 only",
                   "A terminal keeps (double)height[n]", "an output that aliases an input plane",
                   "a scale entry that is not a positive finite float", "SOIL_FLOW_BATCH_CELLS", "do not synchronise"):
        assert phrase in flat, phrase


def test_the_library_binds_the_entries_and_the_build_has_the_source():
    from soillib_amd import _abi, build
    lib = _abi.lib()
    i64, vp, cint, fp, dbl = C.c_int64, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_double
    assert _abi.SIGNATURES["soil_downstream"] == (cint, [vp] * 7 + [i64, i64, cint, fp, vp])
    assert _abi.SIGNATURES["soil_downstream_batch"] == (cint, [vp] * 7 + [i64, i64, i64, cint, fp, i64, vp])
    assert _abi.SIGNATURES["soil_stream_power"] == (cint, [vp] * 7 + [i64, i64, cint, fp, dbl, vp])
    assert _abi.SIGNATURES["soil_stream_power_batch"] == (cint, [vp] * 7 + [i64, i64, i64, cint, fp, i64, dbl, vp])
    assert _abi.SIGNATURES["soil_downstream_info"] == (cint, [C.POINTER(i64)])
    for name in ENTRIES:
        assert hasattr(lib, name), name
    found = [s for s in build.SOURCES if "int soil_downstream(" in open(os.path.join(build.CSRC, s)).read()]
    assert found == ["downstream.hip"]
    common = open(os.path.join(build.CSRC, "common.hpp")).read()
    assert "WS_DOWNSTREAM" in common and "WS_DOWNSTREAM" in open(os.path.join(build.CSRC, "downstream.hip")).read()


def test_the_surfaces():
    import soillib
    from soillib_amd import soil
    from soillib_amd.erosion import ErosionBatch, ErosionModel
    for name in ("downstream", "downstream_batch", "stream_power", "stream_power_batch", "erosivity", "chi",
                 "downstream_info"):
        assert callable(getattr(soil, name)) and getattr(soillib, name) is getattr(soil, name), name
    for name in ("downstream", "stream_power"):
        assert callable(getattr(ErosionBatch, name)) and not hasattr(ErosionModel, name), name
    text = open(os.path.join(ROOT, "include", "soil.hpp")).read()
    for name in ("downstream", "downstream_batch", "stream_power", "stream_power_batch"):
        assert re.search(r"inline [^;{]*\b%s\(" % name, text), name
        assert "soil_%s(" % name in text, name
    knobs = open(os.path.join(ROOT, "docs", "KNOBS.md")).read()
    # (read in the driver the entries share with soil_flow_paths, csrc/flow_paths.hpp, or in the host helpers that
    # driver shares with the other flow solvers, csrc/flow_host.hpp)
    for knob, where in (("SOIL_PATHS_LIST_FROM", "flow_paths.hpp"), ("SOIL_PATHS_IDX64", "flow_host.hpp"),
                        ("SOIL_FLOW_BATCH_CELLS", "flow_host.hpp"), ("SOIL_PATHS_GROUPS", "flow_paths.hpp")):
        line = [l for l in knobs.splitlines() if l.startswith("| `%s` " % knob)]
        assert len(line) == 1 and "soillib_amd/csrc/" + where in line[0] and "soil_downstream" in line[0], knob
    source = open(os.path.join(ROOT, "soillib_amd", "csrc", "downstream.hip")).read()
    assert '#include "flow_paths.hpp"' in source and "ptr_run(WS_DOWNSTREAM" in source


def test_the_call_info_needs_no_device():
    from soillib_amd import _abi, soil
    assert _abi.lib().soil_downstream_info(None) == _abi.SOIL_ERR_INVALID_ARGUMENT
    assert _abi.last_error().startswith("downstream_info: ")
    assert sorted(soil.downstream_info()) == ["chunks", "idx64_chunks", "rounds", "vec_chunks"]


# ---- refusals of the four entries, without a device ------------------------------------------------------------

def _p(k):
    """A stand-in for a tensor (never read): planes a MiB apart, so that none overlaps another."""
    return C.c_void_p(k << 20)


def _entries():
    """name -> call(over), `over` a dict of the arguments to replace in a well-formed call of (B, H, W) = (3, 4, 4)."""
    from soillib_amd import _abi
    lib = _abi.lib()
    sc = (C.c_float * 6)(1, 2, 1, 2, 1, 2)
    base = dict(out=_p(1), out64=_p(2), graph=_p(4), stop=_p(5), B=3, H=4, W=4, edge=D8, scale=sc, n=3, dt=1.5)
    sums = dict(base, a=_p(6), b=_p(7), t=_p(8))
    power = dict(base, height=_p(6), erosivity=_p(7), uplift=_p(8))

    def call(fn, names, defaults):
        def go(over=()):
            v = dict(defaults, **dict(over))
            return fn(*[v[k] for k in names], None)
        return go
    head_s, head_p = ["out", "out64", "graph", "a", "b", "t", "stop"], ["out", "out64", "height", "graph", "erosivity", "uplift", "stop"]
    return {
        "downstream": call(lib.soil_downstream, head_s + ["H", "W", "edge", "scale"], sums),
        "downstream_batch": call(lib.soil_downstream_batch, head_s + ["B", "H", "W", "edge", "scale", "n"], sums),
        "stream_power": call(lib.soil_stream_power, head_p + ["H", "W", "edge", "scale", "dt"], power),
        "stream_power_batch": call(lib.soil_stream_power_batch, head_p + ["B", "H", "W", "edge", "scale", "n", "dt"], power),
    }


def _bad_scale(*v):
    return (C.c_float * 6)(*v)


COMMON = [("null graph", dict(graph=None)), ("both outputs null", dict(out=None, out64=None)),
          ("out is the graph", dict(out=_p(4))), ("out64 is the stop plane", dict(out64=_p(5))),
          ("out inside the third float plane", dict(out=C.c_void_p((8 << 20) + 16))),
          ("out64 is the first float plane", dict(out64=_p(6))), ("out overlaps out64", dict(out=C.c_void_p((2 << 20) + 8))),
          ("H = 0", dict(H=0)), ("W = 0", dict(W=0)), ("W < 0", dict(W=-2)), ("H W > INT32_MAX", dict(H=1 << 16, W=1 << 15)),
          ("edge 2", dict(edge=2)), ("edge -1", dict(edge=-1))]
BATCH = [("B = 0", dict(B=0)), ("B < 0", dict(B=-3)), ("n_scales 2 of 3", dict(n=2)), ("n_scales 0", dict(n=0)),
         ("n_scales 4 of 3", dict(n=4))]
POWER = [("null height", dict(height=None)), ("null erosivity", dict(erosivity=None)), ("null scale", dict(scale=None)),
         ("scale 0", dict(scale=_bad_scale(0, 1, 1, 1, 1, 1))), ("scale < 0", dict(scale=_bad_scale(1, -1, 1, 1, 1, 1))),
         ("scale inf", dict(scale=_bad_scale(float("inf"), 1, 1, 1, 1, 1))),
         ("scale NaN", dict(scale=_bad_scale(1, float("nan"), 1, 1, 1, 1))),
         ("dt < 0", dict(dt=-1e-9)), ("dt inf", dict(dt=float("inf"))), ("dt NaN", dict(dt=float("nan")))]
POWER_BATCH = [("a later model's scale 0", dict(scale=_bad_scale(1, 1, 1, 1, 0, 1)))]


def _cases(name):
    cases = COMMON + (BATCH if name.endswith("_batch") else []) + (POWER if name.startswith("stream") else [])
    return cases + (POWER_BATCH if name == "stream_power_batch" else [])


def test_every_refusal_names_its_entry():
    from soillib_amd import _abi
    for name, call in _entries().items():
        for what, over in _cases(name):
            assert call(over) == _abi.SOIL_ERR_INVALID_ARGUMENT, (what, name)
            assert _abi.last_error().startswith(name + ": "), (what, name, _abi.last_error())


def test_a_well_formed_call_fails_loudly_without_a_device():
    from soillib_amd import _abi
    if _abi.lib().soil_device_count() > 0:
        pytest.skip("a HIP device is present")
    for name, call in _entries().items():
        assert call() == _abi.SOIL_ERR_NO_DEVICE, name
        assert call(dict(out=None, stop=None)) == _abi.SOIL_ERR_NO_DEVICE, name
        assert call(dict(out64=None, dt=0.0)) == _abi.SOIL_ERR_NO_DEVICE, name
    sums = _entries()["downstream"]
    assert sums(dict(a=None, b=None, t=None, stop=None, scale=None)) == _abi.SOIL_ERR_NO_DEVICE
    assert _entries()["downstream_batch"](dict(scale=None, n=1)) == _abi.SOIL_ERR_NO_DEVICE
    assert _entries()["stream_power"](dict(uplift=None)) == _abi.SOIL_ERR_NO_DEVICE


# ---- the ValueErrors of the Python layer: before any device work -----------------------------------------------

def _host(dtype, shape):
    from soillib_amd import silt
    return silt.tensor._wrap_numpy(np.zeros(shape, dtype))


def _module_refusals():
    from soillib_amd import soil
    g2, g3 = _host(np.int32, (4, 3)), _host(np.int32, (5, 4, 3))
    f2, f3 = _host(np.float32, (4, 3)), _host(np.float32, (5, 4, 3))
    return [
        (soil.downstream, (g3, soil.d8), {}, r"downstream: graph: expected a \(H, W\)"),
        (soil.downstream, (f2, soil.d8), {}, "downstream: graph: expected an int32"),
        (soil.downstream, (np.zeros((4, 3), np.int32), soil.d8), {}, "downstream: graph"),
        (soil.downstream, (g2, 2), {}, "downstream: edge"),
        (soil.downstream, (g2, soil.d8), dict(a=_host(np.float32, (3, 4))), "downstream: a"),
        (soil.downstream, (g2, soil.d8), dict(b=g2), "downstream: b: expected a float32"),
        (soil.downstream, (g2, soil.d8), dict(terminal=f3), "downstream: terminal"),
        (soil.downstream, (g2, soil.d8), dict(stop=f2), "downstream: stop"),
        (soil.downstream, (g2, soil.d8), dict(scale=[1.0]), "downstream: scale"),
        (soil.downstream, (g2, soil.d8), dict(scale=[[1.0, 1.0]] * 2), "downstream: scale"),
        (soil.downstream_batch, (g2, soil.d8), {}, r"downstream_batch: graph: expected a \(B, H, W\)"),
        (soil.downstream_batch, (g3, 7), {}, "downstream_batch: edge"),
        (soil.downstream_batch, (g3, soil.d8), dict(a=f2), "downstream_batch: a"),
        (soil.downstream_batch, (g3, soil.d8), dict(stop=_host(np.int32, (4, 4, 3))), "downstream_batch: stop"),
        (soil.downstream_batch, (g3, soil.d8), dict(scale=[[1.0, 1.0]] * 4), "downstream_batch: scale"),
        (soil.stream_power, (f2, g3, f2, soil.d8, (1.0, 1.0), 1.0), {}, "stream_power: graph"),
        (soil.stream_power, (g2, g2, f2, soil.d8, (1.0, 1.0), 1.0), {}, "stream_power: height"),
        (soil.stream_power, (None, g2, f2, soil.d8, (1.0, 1.0), 1.0), {}, "stream_power: height is required"),
        (soil.stream_power, (f2, g2, None, soil.d8, (1.0, 1.0), 1.0), {}, "stream_power: erosivity is required"),
        (soil.stream_power, (f2, g2, f3, soil.d8, (1.0, 1.0), 1.0), {}, "stream_power: erosivity"),
        (soil.stream_power, (f2, g2, f2, "d8", (1.0, 1.0), 1.0), {}, "stream_power: edge"),
        (soil.stream_power, (f2, g2, f2, soil.d8, None, 1.0), {}, "stream_power: scale"),
        (soil.stream_power, (f2, g2, f2, soil.d8, (1.0, 0.0), 1.0), {}, "stream_power: scale entries"),
        (soil.stream_power, (f2, g2, f2, soil.d8, (1.0, float("inf")), 1.0), {}, "stream_power: scale entries"),
        (soil.stream_power, (f2, g2, f2, soil.d8, (1.0, 1.0), -1.0), {}, "stream_power: dt"),
        (soil.stream_power, (f2, g2, f2, soil.d8, (1.0, 1.0), float("nan")), {}, "stream_power: dt"),
        (soil.stream_power, (f2, g2, f2, soil.d8, (1.0, 1.0), "1"), {}, "stream_power: dt"),
        (soil.stream_power, (f2, g2, f2, soil.d8, (1.0, 1.0), 1.0), dict(uplift=g2), "stream_power: uplift"),
        (soil.stream_power_batch, (f3, g3, f3, soil.d8, [[1.0, 1.0]] * 4, 1.0), {}, "stream_power_batch: scale"),
        (soil.stream_power_batch, (f3, g3, f3, soil.d8, None, 1.0), {}, "stream_power_batch: scale"),
        (soil.stream_power_batch, (f3, g3, f2, soil.d8, (1.0, 1.0), 1.0), {}, "stream_power_batch: erosivity"),
        (soil.stream_power_batch, (f3, g3, f3, soil.d8, [[1.0, 1.0]] * 4 + [[1.0, -2.0]], 1.0), {}, "stream_power_batch: scale entries"),
        (soil.chi, (g3, f2, soil.d8, (1.0, 1.0)), {}, "chi: graph"),
        (soil.chi, (g2, g2, soil.d8, (1.0, 1.0)), {}, "chi: area"),
        (soil.erosivity, (g2, 1.0, 0.5), {}, "erosivity: area"),
    ]


def test_the_module_functions_refuse():
    for fn, args, kw, match in _module_refusals():
        with pytest.raises(ValueError, match=match):
            fn(*args, **kw)


def test_a_numpy_scalar_is_a_number():
    """A dt that is a numbers.Real and no bool (a numpy scalar as much as a float) passes the scalar check: with host
    tensors the call then fails at the device check only.  What is no finite number >= 0 is refused with the same
    text whatever its type."""
    from soillib_amd import _abi, soil
    g2, g3 = _host(np.int32, (4, 3)), _host(np.int32, (5, 4, 3))
    f2, f3 = _host(np.float32, (4, 3)), _host(np.float32, (5, 4, 3))
    for name, fn, f, g in (("stream_power", soil.stream_power, f2, g2), ("stream_power_batch", soil.stream_power_batch, f3, g3)):
        for dt in (np.float32(1), np.int64(1), np.float64(1), 1, 1.0):
            with pytest.raises(_abi.SoilError, match="mismatch_host"):
                fn(f, g, f, soil.d8, (1.0, 1.0), dt)
        for dt in (True, "1", float("nan"), float("inf"), -1.0, -1, np.float32("nan"), np.float32("inf"), np.float32(-1),
                   np.int64(-1), np.bool_(True)):
            with pytest.raises(ValueError) as e:
                fn(f, g, f, soil.d8, (1.0, 1.0), dt)
            assert str(e.value) == "%s: dt must be a finite number >= 0, got %r" % (name, dt)


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
    good, plane = _host(np.int32, (5, 4, 3)), _host(np.float32, (5, 4, 3))
    out = []
    for kw in (dict(graph=_host(np.int32, (5, 3, 4))), dict(graph=plane), dict(graph=good, a=good),
               dict(graph=good, b=_host(np.float32, (4, 4, 3))), dict(graph=good, terminal=3.0),
               dict(graph=good, stop=plane), dict(graph=good, edge=2), dict(edge="d4")):
        out.append(("downstream", None, (), kw, r"ErosionBatch\.downstream"))
    out.append(("downstream", [[1.0, 1.0, 1.0]] * 4, (good,), {}, r"ErosionBatch\.downstream"))
    for args, kw in (((-1.0, 1e-4), {}), ((float("nan"), 1e-4), {}), ((1.0, -1e-4), {}), ((1.0, "k"), {}),
                     ((1.0, 1e-4), dict(m=float("inf"))), ((1.0, 1e-4), dict(kind="direction")),
                     ((1.0, 1e-4), dict(edge=2)), ((1.0, 1e-4), dict(kind="random_weighted")),
                     ((1.0, 1e-4), dict(kind="random_weighted", T=1.0, offset=-1)), ((1.0, 1e-4), dict(uplift=good)),
                     ((1.0, 1e-4), dict(uplift=_host(np.float32, (5, 3, 4))))):
        out.append(("stream_power", None, args, kw, r"ErosionBatch\.stream_power"))
    return out


def test_the_batch_methods_refuse():
    for method, scales, args, kw, match in _batch_refusals():
        with pytest.raises(ValueError, match=match):
            getattr(_batch_without_a_device(scales=scales), method)(*args, **kw)
