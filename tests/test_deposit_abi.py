"""The stream-power step with sediment deposition (include/soil_hip.h: "flow graphs: erosion-deposition";
soil_stream_power_deposit and its _batch form), what can be checked without a GPU: the two restatements of
tests/deposit_ref.py against each other, the identity with the stream-power step, hand-computed cases that pin the
definition, the convergence of the iteration (a condition on the inputs: asserted on the restatement), the header, the
bound symbols and the surfaces, every refusal with the entry's name in the message, SOIL_ERR_NO_DEVICE for a
well-formed call, and the ValueErrors of the Python layer.

The bound between the restatements.  solve_serial sums q upstream in fp64; solve_iterated rounds q to float32 and adds
in float32, as the device does.  At cell n with A_n cells upstream and Qabs_n the upstream sum of |q|, the float32 sum
is off by at most A_n 2^-24 Qabs_n (A_n - 1 additions, each off by half an ulp of a partial sum that is at most Qabs_n,
and q's own rounding).  It enters A0 as g dQs / d with g = G / A_n: at most G 2^-24 Qabs_n / d.  Down the graph
dx_n = dA0_n + B0_n dx_r, and since (1 + g) / d = 1 - B0 the weights (prod of B0 above j) / d_j along a path sum to at
most 1 / (1 + g) <= 1: dx <= G 2^-24 max Qabs after one iteration.  The error feeds back through q with the
iteration's contraction, which test_the_iteration_contracts holds below 0.8: a factor 1 / (1 - 0.8) = 5.  So
    |x_iterated - x_serial| <= 5 G 2^-24 max Qabs
(the fp64 roundings of either are 2^-29 of that).  It is a worst case — every rounding aligned; the tests print what
they see, some thousand times less.  For flux, the same sum once more: A_n (2^-24 Qabs_n + the bound on x)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import deposit_ref as dep
import downstream_ref as dref
import flow_paths_ref as ref
from flow_paths_ref import D4, D8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_EROSION, M_AREA = 2e-2, 0.5


@functools.lru_cache(maxsize=None)
def _case(oracle_, H, W, edge, G):
    """The downhill graph of terrain * 10 and the planes of a step on it: height, graph, area, erosivity, deposition,
    uplift."""
    h = (ref.terrain(H, W, 2) * 10).astype(np.float32)
    g = ref.descent(h, edge)
    area = oracle_.accumulate(g, np.ones((H, W), np.float32), edge)
    k = (K_EROSION * area.astype(np.float64) ** M_AREA).astype(np.float32)
    d = (np.float32(G) / area).astype(np.float32)
    u = (np.random.default_rng([H, W]).random((H, W)) * 0.01).astype(np.float32)
    for p in (h, g, area, k, d, u):
        p.setflags(write=False)
    return h, g, area, k, d, u


# ---- (i) against (ii) ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", [(12, 20), (13, 21), (48, 64)])
@pytest.mark.parametrize("edge", [D4, D8])
def test_the_two_restatements_agree_on_downhill_graphs(oracle, H, W, edge):
    G, dt, iters = 1.0, 10.0, 6
    h, g, area, k, d, u = _case(oracle, H, W, edge, G)
    for uplift in (None, u):
        a = dep.solve_iterated(oracle, g, edge, h, k, d, (0.3, 0.7), dt, uplift, iters)
        b = dep.solve_serial(g, edge, h, k, d, (0.3, 0.7), dt, uplift, iters)
        assert a["final"].all() and b["final"].all(), "a downhill graph resolves every cell"
        is_edge, _, lifted, *_ = dep.coefficients(g, edge, h, k, d, uplift, (0.3, 0.7), dt)
        q_abs = np.abs(dep.make_q(is_edge, lifted, b["out64"].reshape(-1))).reshape(H, W)
        Qabs = oracle.accumulate(g, q_abs, edge).astype(np.float64)
        bound = 5.0 * G * 2.0 ** -24 * Qabs.max()
        seen = np.abs(a["out64"] - b["out64"]).max()
        ulp = 2.0 ** -23 * np.abs(h).max()
        print("%dx%d edge %d uplift %r: the restatements differ by %.3g at most, bound %.3g (%.1f and %.1f float32 ulps "
              "of the highest cell)" % (H, W, edge, uplift is not None, seen, bound, seen / ulp, bound / ulp))
        assert seen <= bound
        # out: the float32 roundings of two values that close, half an ulp of the value each
        assert (np.abs(a["out"].astype(np.float64) - b["out"]) <= bound + 2.0 ** -23 * np.abs(b["out64"])).all()
        flux_bound = area * (2.0 ** -24 * Qabs + bound) + 2.0 ** -23 * np.abs(b["flux"])
        assert (np.abs(a["flux"].astype(np.float64) - b["flux"]) <= flux_bound).all()
        assert abs(a["residual"] - b["residual"]) <= 2 * bound


@pytest.mark.parametrize("iters", [1, 2, 5])
def test_a_zero_deposition_plane_gives_the_stream_power_step(oracle, iters):
    for H, W in ((12, 20), (13, 21)):
        for edge in (D4, D8):
            h, _, _, k, _, u = _case(oracle, H, W, edge, 1.0)
            zero = np.zeros((H, W), np.float32)
            for name, graph in ref.built_graphs(H, W, edge) + [("descent", _case(oracle, H, W, edge, 1.0)[1])]:
                for uplift in (None, u):
                    got = dep.solve_iterated(oracle, graph, edge, h, k, zero, (0.3, 0.7), 3.5, uplift, iters)
                    want = dref.solve_doubling(graph, edge, scale=(0.3, 0.7), power=(h, k, uplift, 3.5))
                    dref.same_words((got["out"], got["out64"]), want, "%s %dx%d edge %d" % (name, H, W, edge))
                    assert (got["final"] == want[2]).all()


# ---- by hand ---------------------------------------------------------------------------------------------------

def _f32(*v):
    return np.array(v, np.float32)


class _Spy:
    """An oracle whose accumulate remembers what it was asked and what it said."""

    def __init__(self, oracle_):
        self.oracle, self.calls = oracle_, []

    def accumulate(self, graph, source, edge, decay=None):
        out = self.oracle.accumulate(graph, source, edge, decay)
        self.calls.append((source.copy(), out.copy()))
        return out


def test_a_head_cell_has_no_upstream_share_in_any_iteration(oracle):
    H, W = 12, 20
    h, g, area, k, d, u = _case(oracle, H, W, D8, 2.0)
    spy = _Spy(oracle)
    dep.solve_iterated(spy, g, D8, h, k, d, (0.3, 0.7), 10.0, u, 5)
    heads = area == 1.0
    assert heads.any() and len(spy.calls) == 5                   # iterations 2 .. 5 and the flux
    for q, Qs in spy.calls:
        Qup = Qs.astype(np.float64) - q.astype(np.float64)
        assert (Qup[heads] == 0.0).all() and (q[heads] != 0).any()


def test_a_two_cell_chain_by_hand(oracle):
    """Cell 0 drains into cell 1, a terminal.  A head: Qup == 0 in every iteration, so every iterate is
    x0 = ((1 + g) b + F h1) / (1 + F + g) — reached at once, the residual of a second iteration is 0 — and the flux at
    the terminal is what the head lost."""
    graph = np.array([[1, -1]], np.int32)
    height, k, g = _f32(8.0, 2.0), _f32(0.5, 9.0), _f32(0.25, 7.0)
    dt, sy = 2.0, 0.5
    F = 0.5 * dt / sy                                            # a column step: L = sy
    d = (1.0 + F) + 0.25
    x0 = ((1.25 * 8.0) + (0.25 * 0.0)) / d + (F / d) * 2.0
    for iters in (1, 2, 4):
        got = dep.solve_iterated(oracle, graph, D4, height, k, g, (3.0, sy), dt, None, iters)
        assert got["out64"].tolist() == [[x0, 2.0]]
        assert got["residual"] == (abs(x0 - 8.0) if iters == 1 else 0.0)
        assert got["flux"].tolist() == [[np.float32(8.0 - x0)] * 2]
    serial = dep.solve_serial(graph, D4, height, k, g, (3.0, sy), dt, None, 3)
    assert serial["out64"].tolist() == [[x0, 2.0]]


def test_a_three_cell_chain_by_hand(oracle):
    """0 -> 1 -> 2, the last a terminal, row steps of length sx = 2, uplift on.  Iteration 1 is the stream-power step
    with d = 1 + F + g and (1 + g) b; iteration 2 gives cell 1 the share g1 q0 of what cell 0 lost in iteration 1."""
    graph = np.array([[1], [2], [-1]], np.int32)
    height, k, g, u = _f32(10.0, 6.0, 1.0), _f32(1.0, 3.0, 5.0), _f32(0.5, 0.125, 9.0), _f32(0.25, 0.5, 100.0)
    dt, sx = 4.0, 2.0
    F = [1.0 * dt / sx, 3.0 * dt / sx]
    d = [(1.0 + F[0]) + 0.5, (1.0 + F[1]) + 0.125]
    b = [10.0 + dt * 0.25, 6.0 + dt * 0.5]
    B0 = [F[0] / d[0], F[1] / d[1]]
    # iteration 1: Qup = 0
    x1 = ((1.125 * b[1]) + (0.125 * 0.0)) / d[1] + B0[1] * 1.0
    x0 = ((1.5 * b[0]) + (0.5 * 0.0)) / d[0] + B0[0] * x1
    got = dep.solve_iterated(oracle, graph.reshape(3, 1), D4, height.reshape(3, 1), k.reshape(3, 1), g.reshape(3, 1),
                             (sx, 1.0), dt, u.reshape(3, 1), 1)
    assert np.allclose(got["out64"].reshape(-1), [x0, x1, 1.0], rtol=2 ** -50, atol=0)
    assert got["out64"][2, 0] == 1.0, "the terminal is neither lifted nor eroded"
    # iteration 2: q from iteration 1, rounded to float32; cell 1 has cell 0 upstream
    q0 = float(np.float32(b[0] - got["out64"][0, 0]))
    y1 = ((1.125 * b[1]) + (0.125 * q0)) / d[1] + B0[1] * 1.0
    y0 = ((1.5 * b[0]) + (0.5 * 0.0)) / d[0] + B0[0] * y1
    got2 = dep.solve_iterated(oracle, graph.reshape(3, 1), D4, height.reshape(3, 1), k.reshape(3, 1), g.reshape(3, 1),
                              (sx, 1.0), dt, u.reshape(3, 1), 2)
    assert np.allclose(got2["out64"].reshape(-1), [y0, y1, 1.0], rtol=2 ** -50, atol=0)
    assert y1 > x1, "deposition raises the cell below an eroding one"
    assert got2["residual"] == max(abs(got2["out64"][i, 0] - got["out64"][i, 0]) for i in range(3))
    q = [np.float32(b[0] - got2["out64"][0, 0]), np.float32(b[1] - got2["out64"][1, 0])]
    assert got2["flux"].reshape(-1).tolist() == [q[0], q[0] + q[1], q[0] + q[1]]


def test_a_terminal_s_flux_is_the_sum_of_its_basin_s_q(oracle):
    H, W = 13, 21
    h, g, area, k, d, u = _case(oracle, H, W, D8, 1.0)
    got = dep.solve_iterated(oracle, g, D8, h, k, d, (0.3, 0.7), 10.0, None, 4)
    is_edge, _, b, *_ = dep.coefficients(g, D8, h, k, d, None, (0.3, 0.7), 10.0)
    q = dep.make_q(is_edge, b, got["out64"].reshape(-1)).astype(np.float64)
    terminal = ref.walk_serial(g, D8)[0].reshape(-1)
    assert (q[~is_edge] == 0).all()
    for t in np.flatnonzero(~is_edge):
        basin = q[terminal == t]
        want = basin.sum()
        # a float32 sum of len(basin) terms against the fp64 one: half an ulp of a partial sum per addition
        assert abs(float(got["flux"].reshape(-1)[t]) - want) <= len(basin) * 2.0 ** -24 * np.abs(basin).sum() + 1e-30


def test_a_void_is_nan_with_everything_upstream_and_no_flux_goes_wrong(oracle):
    H, W = 12, 20
    h, g, area, k, d, u = _case(oracle, H, W, D8, 1.0)
    h = h.copy()
    at = int(np.argmax(np.where((area > 4) & (g >= 0), area, 0)))
    h.reshape(-1)[at] = np.nan
    got = dep.solve_iterated(oracle, g, D8, h, k, d, (0.3, 0.7), 10.0, None, 3)
    marks = np.zeros((H, W), np.float32)
    marks.reshape(-1)[at] = 1
    way = dref.solve_doubling(g, D8, a=marks, t=marks)[1] != 0           # the sum of the marks on the way down
    assert (np.isnan(got["out64"]) == way).all() and way.sum() > 4
    assert np.isfinite(got["flux"]).all() and np.isfinite(got["residual"])


# ---- convergence: a condition on the inputs --------------------------------------------------------------------

@pytest.mark.parametrize("G", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("dt", [10.0, 1000.0])
def test_the_iteration_contracts(oracle, G, dt):
    """residual(k + 1) < 0.8 residual(k) from k = 2 until the residual first falls below 1e-5 of the terrain's range,
    D8 and D4 (a prototype: ratios of 0.04 to 0.73, floors of 3e-8 to 5e-7 on a range of 75)."""
    H, W = 48, 64
    for edge in (D8, D4):
        h, g, area, k, d, u = _case(oracle, H, W, edge, G)
        floor = 1e-5 * float(h.max() - h.min())
        r = dep.solve_iterated(oracle, g, edge, h, k, d, (1.0, 1.0), dt, None, 24)["residuals"]
        print("G %g dt %g edge %d: residuals %s" % (G, dt, edge, " ".join("%.2g" % v for v in r)))
        below = [i for i, v in enumerate(r) if v < floor]
        assert below, "the residual never fell below %g" % floor
        for i in range(1, below[0]):                                  # r[i] is residual(i + 1)
            assert r[i + 1] < 0.8 * r[i], (i + 1, r[i], r[i + 1])


# ---- the header, the symbols, the surfaces ---------------------------------------------------------------------

HEAD = ("float* out, double* out64, float* flux, double* residual, const float* height, const int32_t* graph, "
        "const float* erosivity, const float* deposition, const float* uplift, ")
ENTRIES = {
    "soil_stream_power_deposit": HEAD + "int64_t H, int64_t W, int edge, const float scale[2], double dt, int iters, void* stream",
    "soil_stream_power_deposit_batch": HEAD + ("int64_t B, int64_t H, int64_t W, int edge, const float* scales, "
                                               "int64_t n_scales, double dt, int iters, void* stream"),
    "soil_stream_power_deposit_info": "int64_t info[4]",
}


def _squash(s):
    return re.sub(r"\s+", " ", s).strip()


def test_the_header_declares_the_entries_and_states_the_contract():
    text = open(os.path.join(ROOT, "include", "soil_hip.h")).read()
    assert "flow graphs: erosion-deposition" in text
    for name, args in ENTRIES.items():
        m = re.search(r"int %s\((.*?)\);" % name, text, re.S)
        assert m, name
        assert _squash(m.group(1)) == args
    flat = _squash(re.sub(r"\n \* ?", "\n", text))
    for phrase in ("dh/dt = u - K A^m S + (G / A) * Qs", "d = (1.0 + F) + g", "g = (double)deposition[n]",
                   "Qup = (double)Qs[n] - (double)q[n]", "A0 = (((1.0 + g) * b) + (g * Qup)) / d",
                   "the bits soil_accumulate(graph, q, no decay) gives", "There is no `stop` plane",
                   "With `deposition` all zeros the result is the bits of soil_stream_power",
                   "a fixed count keeps the result one definite bit pattern", "The self-implicit term",
                   "a null `deposition`, iters < 1", "Nothing synchronises", "as integers",
                   "info[0] kernel launches, info[1] chunks, info[2] iterations run, info[3] bytes of scratch"):
        assert phrase in flat, phrase


def test_the_library_binds_the_entries_and_the_build_has_the_source():
    from soillib_amd import _abi, build
    lib = _abi.lib()
    i64, vp, cint, fp, dbl = C.c_int64, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_double
    assert _abi.SIGNATURES["soil_stream_power_deposit"] == (cint, [vp] * 9 + [i64, i64, cint, fp, dbl, cint, vp])
    assert _abi.SIGNATURES["soil_stream_power_deposit_batch"] == (cint, [vp] * 9 + [i64, i64, i64, cint, fp, i64, dbl, cint, vp])
    assert _abi.SIGNATURES["soil_stream_power_deposit_info"] == (cint, [C.POINTER(i64)])
    for name in ENTRIES:
        assert hasattr(lib, name), name
    found = [s for s in build.SOURCES if "int soil_stream_power_deposit(" in open(os.path.join(build.CSRC, s)).read()]
    assert len(found) == 1
    common = open(os.path.join(build.CSRC, "common.hpp")).read()
    source = open(os.path.join(build.CSRC, found[0])).read()
    for slot in ("WS_DEPOSIT", "WS_DEPOSIT_RAKE", "WS_DEPOSIT_PLANES"):
        assert slot in common and slot in source, slot
    assert "int rake_accumulate(" in common and "ptr_run(WS_DEPOSIT" in source and "ptr_chunk(" in source


def test_the_surfaces():
    import soillib
    from soillib_amd import soil
    from soillib_amd.erosion import ErosionBatch, ErosionModel
    for name in ("stream_power_deposit", "stream_power_deposit_batch", "deposition", "stream_power_deposit_info"):
        assert callable(getattr(soil, name)) and getattr(soillib, name) is getattr(soil, name), name
    assert callable(ErosionBatch.stream_power_deposit) and not hasattr(ErosionModel, "stream_power_deposit")
    text = open(os.path.join(ROOT, "include", "soil.hpp")).read()
    assert "deposit" not in text, "nothing new is named in soil.hpp"


def test_the_call_info_needs_no_device():
    from soillib_amd import _abi, soil
    assert _abi.lib().soil_stream_power_deposit_info(None) == _abi.SOIL_ERR_INVALID_ARGUMENT
    assert _abi.last_error().startswith("stream_power_deposit_info: ")
    assert sorted(soil.stream_power_deposit_info()) == ["chunks", "iters", "launches", "scratch_bytes"]


# ---- refusals, without a device --------------------------------------------------------------------------------

def _p(k):
    """A stand-in for a tensor (never read): planes a MiB apart, so that none overlaps another."""
    return C.c_void_p(k << 20)


def _entries():
    """name -> call(over), `over` a dict of the arguments to replace in a well-formed call of (B, H, W) = (3, 4, 4)."""
    from soillib_amd import _abi
    lib = _abi.lib()
    sc = (C.c_float * 6)(1, 2, 1, 2, 1, 2)
    base = dict(out=_p(1), out64=_p(2), flux=_p(3), residual=_p(4), height=_p(5), graph=_p(6), erosivity=_p(7),
                deposition=_p(8), uplift=_p(9), B=3, H=4, W=4, edge=D8, scale=sc, n=3, dt=1.5, iters=4)
    head = ["out", "out64", "flux", "residual", "height", "graph", "erosivity", "deposition", "uplift"]

    def call(fn, names):
        def go(over=()):
            v = dict(base, **dict(over))
            return fn(*[v[k] for k in names], None)
        return go
    return {
        "stream_power_deposit": call(lib.soil_stream_power_deposit, head + ["H", "W", "edge", "scale", "dt", "iters"]),
        "stream_power_deposit_batch": call(lib.soil_stream_power_deposit_batch,
                                           head + ["B", "H", "W", "edge", "scale", "n", "dt", "iters"]),
    }


def _bad_scale(*v):
    return (C.c_float * 6)(*v)


REFUSED = [("null graph", dict(graph=None)), ("both outputs null", dict(out=None, out64=None)),
           ("out is the graph", dict(out=_p(6))), ("out64 is the height", dict(out64=_p(5))),
           ("out inside the uplift", dict(out=C.c_void_p((9 << 20) + 16))), ("out overlaps out64", dict(out=C.c_void_p((2 << 20) + 8))),
           ("out is the deposition", dict(out=_p(8))), ("out64 is the deposition", dict(out64=_p(8))),
           ("H = 0", dict(H=0)), ("W = 0", dict(W=0)), ("W < 0", dict(W=-2)), ("H W > INT32_MAX", dict(H=1 << 16, W=1 << 15)),
           ("edge 2", dict(edge=2)), ("edge -1", dict(edge=-1)),
           ("null height", dict(height=None)), ("null erosivity", dict(erosivity=None)), ("null scale", dict(scale=None)),
           ("scale 0", dict(scale=_bad_scale(0, 1, 1, 1, 1, 1))), ("scale < 0", dict(scale=_bad_scale(1, -1, 1, 1, 1, 1))),
           ("scale inf", dict(scale=_bad_scale(float("inf"), 1, 1, 1, 1, 1))),
           ("scale NaN", dict(scale=_bad_scale(1, float("nan"), 1, 1, 1, 1))),
           ("dt < 0", dict(dt=-1e-9)), ("dt inf", dict(dt=float("inf"))), ("dt NaN", dict(dt=float("nan"))),
           ("null deposition", dict(deposition=None)), ("iters 0", dict(iters=0)), ("iters < 0", dict(iters=-3)),
           ("flux is the graph", dict(flux=_p(6))), ("flux is the deposition", dict(flux=_p(8))),
           ("flux is out", dict(flux=_p(1))), ("flux inside out64", dict(flux=C.c_void_p((2 << 20) + 64))),
           ("flux is the uplift", dict(flux=_p(9))), ("residual is the height", dict(residual=_p(5))),
           ("residual inside out", dict(residual=C.c_void_p((1 << 20) + 8))), ("residual is out64", dict(residual=_p(2))),
           ("residual inside flux", dict(residual=C.c_void_p((3 << 20) + 16))), ("residual is the erosivity", dict(residual=_p(7)))]
BATCH = [("B = 0", dict(B=0)), ("B < 0", dict(B=-3)), ("n_scales 2 of 3", dict(n=2)), ("n_scales 0", dict(n=0)),
         ("n_scales 4 of 3", dict(n=4)), ("a later model's scale 0", dict(scale=_bad_scale(1, 1, 1, 1, 0, 1)))]


def _cases(name):
    return REFUSED + (BATCH if name.endswith("_batch") else [])


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
        assert call(dict(out=None, flux=None, residual=None)) == _abi.SOIL_ERR_NO_DEVICE, name
        assert call(dict(out64=None, uplift=None, dt=0.0, iters=1)) == _abi.SOIL_ERR_NO_DEVICE, name


# ---- the ValueErrors of the Python layer: before any device work -----------------------------------------------

def _host(dtype, shape):
    from soillib_amd import silt
    return silt.tensor._wrap_numpy(np.zeros(shape, dtype))


def _module_refusals():
    from soillib_amd import soil
    g2, g3 = _host(np.int32, (4, 3)), _host(np.int32, (5, 4, 3))
    f2, f3 = _host(np.float32, (4, 3)), _host(np.float32, (5, 4, 3))
    one, many = soil.stream_power_deposit, soil.stream_power_deposit_batch
    ok = (1.0, 1.0)
    return [
        (one, (f2, g3, f2, f2, soil.d8, ok, 1.0), {}, "stream_power_deposit: graph"),
        (one, (g2, g2, f2, f2, soil.d8, ok, 1.0), {}, "stream_power_deposit: height"),
        (one, (None, g2, f2, f2, soil.d8, ok, 1.0), {}, "stream_power_deposit: height is required"),
        (one, (f2, g2, None, f2, soil.d8, ok, 1.0), {}, "stream_power_deposit: erosivity is required"),
        (one, (f2, g2, f2, None, soil.d8, ok, 1.0), {}, "stream_power_deposit: deposition is required"),
        (one, (f2, g2, f2, f3, soil.d8, ok, 1.0), {}, "stream_power_deposit: deposition"),
        (one, (f2, g2, f2, g2, soil.d8, ok, 1.0), {}, "stream_power_deposit: deposition"),
        (one, (f2, g2, f2, f2, "d8", ok, 1.0), {}, "stream_power_deposit: edge"),
        (one, (f2, g2, f2, f2, soil.d8, None, 1.0), {}, "stream_power_deposit: scale"),
        (one, (f2, g2, f2, f2, soil.d8, (1.0, 0.0), 1.0), {}, "stream_power_deposit: scale entries"),
        (one, (f2, g2, f2, f2, soil.d8, ok, -1.0), {}, "stream_power_deposit: dt"),
        (one, (f2, g2, f2, f2, soil.d8, ok, float("nan")), {}, "stream_power_deposit: dt"),
        (one, (f2, g2, f2, f2, soil.d8, ok, 1.0), dict(uplift=g2), "stream_power_deposit: uplift"),
        (one, (f2, g2, f2, f2, soil.d8, ok, 1.0), dict(iters=0), "stream_power_deposit: iters"),
        (one, (f2, g2, f2, f2, soil.d8, ok, 1.0), dict(iters=2.0), "stream_power_deposit: iters"),
        (one, (f2, g2, f2, f2, soil.d8, ok, 1.0), dict(iters=True), "stream_power_deposit: iters"),
        (many, (f3, g2, f3, f3, soil.d8, ok, 1.0), {}, r"stream_power_deposit_batch: graph: expected a \(B, H, W\)"),
        (many, (f3, g3, f3, f2, soil.d8, ok, 1.0), {}, "stream_power_deposit_batch: deposition"),
        (many, (f3, g3, f3, f3, soil.d8, [[1.0, 1.0]] * 4, 1.0), {}, "stream_power_deposit_batch: scale"),
        (many, (f3, g3, f3, f3, soil.d8, [[1.0, 1.0]] * 4 + [[1.0, -2.0]], 1.0), {}, "stream_power_deposit_batch: scale entries"),
        (many, (f3, g3, f3, f3, soil.d8, ok, 1.0), dict(iters=-1), "stream_power_deposit_batch: iters"),
        (soil.deposition, (g2, 1.0), {}, "deposition: area"),
        (soil.deposition, (f2, -1.0), {}, "deposition: G"),
        (soil.deposition, (f2, float("nan")), {}, "deposition: G"),
    ]


def test_the_module_functions_refuse():
    for fn, args, kw, match in _module_refusals():
        with pytest.raises(ValueError, match=match):
            fn(*args, **kw)


def test_a_numpy_scalar_is_a_number():
    """dt as a numpy float or integer, iters as a numpy integer: past the scalar checks, refused at the device check
    only (the tensors are host tensors).  What is no number, or out of range, is refused with the same text whatever
    its type."""
    from soillib_amd import _abi, soil
    g2, g3 = _host(np.int32, (4, 3)), _host(np.int32, (5, 4, 3))
    f2, f3 = _host(np.float32, (4, 3)), _host(np.float32, (5, 4, 3))
    for name, fn, f, g in (("stream_power_deposit", soil.stream_power_deposit, f2, g2),
                           ("stream_power_deposit_batch", soil.stream_power_deposit_batch, f3, g3)):
        for dt, iters in ((np.float32(1), np.int64(2)), (np.int64(1), np.int32(2)), (1.0, np.uint8(2)), (np.float64(1), 2)):
            with pytest.raises(_abi.SoilError, match="mismatch_host"):
                fn(f, g, f, f, soil.d8, (1.0, 1.0), dt, iters=iters)
        for dt in (True, "1", float("nan"), float("inf"), -1.0, np.float32("nan"), np.float32(-1), np.int64(-1)):
            with pytest.raises(ValueError) as e:
                fn(f, g, f, f, soil.d8, (1.0, 1.0), dt)
            assert str(e.value) == "%s: dt must be a finite number >= 0, got %r" % (name, dt)
        for iters in (True, "2", 2.0, np.float32(2), 0, np.int64(0), -1, 2 ** 31, np.int64(2 ** 31), float("nan")):
            with pytest.raises(ValueError) as e:
                fn(f, g, f, f, soil.d8, (1.0, 1.0), 1.0, iters=iters)
            assert str(e.value) == "%s: iters must be an integer >= 1, got %r" % (name, iters)
    with pytest.raises(_abi.SoilError, match="mismatch_host"):
        soil.deposition(f2, np.float32(1))
    for G in (True, "1", float("nan"), -1.0, np.float32(-1)):
        with pytest.raises(ValueError) as e:
            soil.deposition(f2, G)
        assert str(e.value) == "deposition: G must be a finite number >= 0, got %r" % (G,)


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
    for args, kw in (((-1.0, 1e-4), {}), ((float("nan"), 1e-4), {}), ((1.0, -1e-4), {}), ((1.0, "k"), {}),
                     ((1.0, 1e-4), dict(m=float("inf"))), ((1.0, 1e-4), dict(G=-1.0)), ((1.0, 1e-4), dict(G=None)),
                     ((1.0, 1e-4), dict(G=float("inf"))), ((1.0, 1e-4), dict(iters=0)), ((1.0, 1e-4), dict(iters=1.5)),
                     ((1.0, 1e-4), dict(kind="direction")), ((1.0, 1e-4), dict(edge=2)),
                     ((1.0, 1e-4), dict(kind="random_weighted")),
                     ((1.0, 1e-4), dict(kind="random_weighted", T=1.0, offset=-1)), ((1.0, 1e-4), dict(uplift=good)),
                     ((1.0, 1e-4), dict(uplift=_host(np.float32, (5, 3, 4))))):
        out.append(("stream_power_deposit", None, args, kw, r"ErosionBatch\.stream_power_deposit"))
    out.append(("stream_power_deposit", [[1.0, 1.0, 1.0]] * 4, (1.0, 1e-4), {}, r"ErosionBatch\.stream_power_deposit"))
    for kw in (dict(G=-0.5), dict(G="1"), dict(G=True), dict(G=1.0, iters=0), dict(G=1.0, iters=None)):
        out.append(("evolve", None, (1.0, 1e-4), dict(kw, kappa=0.1), r"ErosionBatch\.evolve: (G|iters)"))
    return out


def test_the_batch_methods_refuse():
    for method, scales, args, kw, match in _batch_refusals():
        with pytest.raises(ValueError, match=match):
            getattr(_batch_without_a_device(scales=scales), method)(*args, **kw)


def test_evolve_without_G_builds_the_argument_list_it_builds_today(monkeypatch):
    """evolve(...) without G: stream_power with today's positional arguments, then diffuse_batch of its result with
    today's; with G: stream_power_deposit in its place, the rest the same."""
    from soillib_amd import soil
    from soillib_amd.erosion import ErosionBatch
    bt = _batch_without_a_device()
    calls = []
    monkeypatch.setattr(ErosionBatch, "stream_power", lambda self, *a, **k: calls.append(("stream_power", a, k)) or "carved")
    monkeypatch.setattr(ErosionBatch, "stream_power_deposit",
                        lambda self, *a, **k: calls.append(("stream_power_deposit", a, k)) or "filled")
    monkeypatch.setattr(soil, "diffuse_batch", lambda *a, **k: calls.append(("diffuse_batch", a, k)) or "out")
    assert bt.evolve(2.0, 1e-3, 0.4, 0.25, None, "random_weighted", soil.d4, 1.5, 3, 1) == "out"
    assert calls == [("stream_power", (2.0, 1e-3, 0.4, "random_weighted", soil.d4, 1.5, 3, None), {}),
                     ("diffuse_batch", ("carved", [1.0, 1.0], 2.0, 0.25), dict(border="fixed", first_axis=1))]
    del calls[:]
    assert bt.evolve(2.0, 1e-3, kappa=0.25) == "out"
    assert calls == [("stream_power", (2.0, 1e-3, 0.5, "steepest", None, None, 0, None), {}),
                     ("diffuse_batch", ("carved", [1.0, 1.0], 2.0, 0.25), dict(border="fixed", first_axis=0))]
    del calls[:]
    assert bt.evolve(2.0, 1e-3, kappa=0.25, G=1.5, iters=3) == "out"
    assert calls == [("stream_power_deposit", (2.0, 1e-3, 0.5, 1.5, 3, "steepest", None, None, 0, None), {}),
                     ("diffuse_batch", ("filled", [1.0, 1.0], 2.0, 0.25), dict(border="fixed", first_axis=0))]
