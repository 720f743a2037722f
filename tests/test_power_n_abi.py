"""The stream-power step with a slope exponent above 1 (include/soil_hip.h: "flow graphs: slope exponents above 1";
soil_stream_power_n and its _batch form), what can be checked without a GPU: the restatement solve_iterated of
tests/power_n_ref.py against the per-cell bisection solve_exact on a conditioned terrain with a filled lake, the
convergence that comparison rests on, the stall of the same iteration started from the old heights, hand-computed
cases, the header, the bound symbols and the surfaces, every refusal with the entry's name in the message,
SOIL_ERR_NO_DEVICE for a well-formed call, and the ValueErrors of the Python layer.

The bounds.  The defect of a cell is f = x - b + kd S^n with S = (x - x[r]) / L.  The solver reaches x through the
linearised equation (1 + F) x = b + c + F x[r], F = n kd S^(n-1) / L, whose terms it rounds: each of the handful of
operations of a cell is off by at most 2^-53 of its result, the solve's A + B x[r] adds two more, and evaluating f
itself on the rounded x moves it by (1 + F) half-ulps of x and F of x[r].  So |f| is a small multiple of 2^-52 of the
largest of |x|, |b|, kd S^n, F |x| and F |x[r]|; the multiple is measured on the restatement once it has converged,
printed, and held with a factor of 4 for the order of the roundings (profiles/stream_power_n/checks.txt has the
figures: 7.25 at the most, so 29).

Against solve_exact: a defect f at a cell moves its height by f / (1 + F), and a receiver's error reaches the cell
with the factor F / (1 + F) < 1, so along a way of `depth` edges the errors add up to at most depth times the largest
f / (1 + F); the bisection's own x[r] + s L is off by an ulp of x per cell in the same way.  Added to that, the distance
of the iterate from its fixed point: the last change, which the issue found within a factor of two of the true error
where the iteration is slow — and where Newton converges it is far below it."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import downstream_ref as dref
import flats_ref
import flow_paths_ref as ref
import power_n_ref as pn
from flow_paths_ref import D4, D8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 24, 36
SCALE, DT = (1.0, 1.5), 50.0
DEFECT_MULTIPLE = 29.0                                        # 4 x the 7.25 measured below
# (Kc, n) -> the Newton steps after which the restatement's last change is below 1e-9 of the height range, raised case
# by case until it was, and one more: the step that brings the quadratic phase down to the rounding floor
ITERS = {(0.02, 1.5): 6, (0.02, 2.0): 7, (0.02, 3.0): 10, (2.0, 1.5): 7, (2.0, 2.0): 10, (2.0, 3.0): 23}


@functools.lru_cache(maxsize=None)
def _terrain(oracle_):
    """A noise terrain x 100 with a basin pressed into it, conditioned for D8 on the CPU: the filled surface, its
    steepest graph with the flats routed (flats_ref), the drainage area and a uniform uplift."""
    dem = (oracle_.noise(H, W, seed=5.0, ext=(float(H), float(W))) * 100).astype(np.float32)
    dem[8:16, 10:24] -= np.float32(40.0)                      # the fill makes a lake of it
    filled = oracle_.fill_depressions(dem, D8)
    g = oracle_.steepest(filled, D8)
    g = flats_ref.receivers(g, filled, flats_ref.distance_bfs(filled, D8), D8)
    area = oracle_.accumulate(g, np.ones((H, W), np.float32), D8)
    u = np.full((H, W), 0.01, np.float32)
    for p in (filled, g, area, u):
        p.setflags(write=False)
    return filled, g, area, u


def _erosivity(area, Kc):
    return (Kc * area.astype(np.float64) ** 0.5).astype(np.float32)


# ---- the terrain is what the cases need --------------------------------------------------------------------------

def test_the_terrain_has_a_filled_lake_and_drains_off_the_grid(oracle):
    filled, g, area, u = _terrain(oracle)
    r = g.reshape(-1)
    has = r >= 0
    level = has & (filled.reshape(-1) == filled.reshape(-1)[np.where(has, r, 0)])
    print("level edges %d, terminals %d, range %g .. %g" % (level.sum(), (~has).sum(), filled.min(), filled.max()))
    assert level.sum() >= 30, "at least 30 cells whose old slope to the receiver is 0"
    assert not flats_ref.interior_terminals(g).any() and dref.solve_doubling(g, D8)[2].all()
    for Kc, order in ((0.02, 1.0), (2.0, 100.0)):
        mid = float(np.median(_erosivity(area, Kc))) * DT / 1.0
        assert order / 3 <= mid <= order * 3, "K dt / L of order %g, got a median of %g" % (order, mid)


# ---- (i) against (ii) --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1.5, 2.0, 3.0])
@pytest.mark.parametrize("Kc", [0.02, 2.0])
def test_the_restatement_reaches_the_exact_heights(oracle, Kc, n):
    filled, g, area, u = _terrain(oracle)
    k = _erosivity(area, Kc)
    span = float(filled.max() - filled.min())
    iters = ITERS[(Kc, n)]
    it = pn.solve_iterated(g, D8, filled, k, SCALE, DT, n, u, None, iters)
    exact, depth = pn.solve_exact(g, D8, filled, k, SCALE, DT, n, u)
    assert it["final"].all() and np.isfinite(exact).all()
    # the condition on the iteration count: it is examined, not assumed
    res = it["residuals"]
    print("Kc %g n %g: residuals %s" % (Kc, n, " ".join("%.2g" % v for v in res)))
    assert it["residual"] < 1e-9 * span, "the restatement has not converged after %d steps" % iters
    # acceptance: the defect of every cell
    miss, largest, F = pn.defect(it["out64"], g, D8, filled, k, SCALE, DT, n, u)
    unit = 2.0 ** -52 * largest
    multiple = float((miss[unit > 0] / unit[unit > 0]).max())
    print("Kc %g n %g: the defect is %.2f x 2^-52 of the largest term at most (held: %g), %.3g absolute" % (
        Kc, n, multiple, DEFECT_MULTIPLE, miss.max()))
    assert (miss <= DEFECT_MULTIPLE * unit).all()
    # against the bisection
    bound = 2.0 * it["residual"] + depth * float((DEFECT_MULTIPLE * unit / (1.0 + F)).max()) + \
        depth * 2.0 ** -52 * float(np.abs(exact).max())
    seen = float(np.abs(it["out64"] - exact).max())
    print("Kc %g n %g: %.3g from the exact heights at most, bound %.3g, the longest way %d edges" % (Kc, n, seen, bound, depth))
    assert seen <= bound
    # erosion only: nothing rises above its lifted height, and the step is not the n = 1 step
    lifted = filled.astype(np.float64) + DT * u
    assert (it["out64"] <= lifted).all()
    assert np.abs(it["out64"] - dref.solve_doubling(g, D8, scale=SCALE, power=(filled, k, u, DT))[1]).max() > 1e-3 * span


@pytest.mark.parametrize("n", [1.5, 2.0, 3.0])
@pytest.mark.parametrize("Kc", [0.02, 2.0])
def test_from_the_old_heights_the_same_iteration_stalls(oracle, Kc, n):
    """Why the start is the n = 1 solve: the tangent of S^n at S = 0 is flat, so a lake's level cells learn of the
    outlet one cell per step.  After the steps that bring the library's iteration to the rounding floor, the one
    started from the old heights is still many orders above it — and its last change, printed beside the true error,
    is far above 1e-9 of the range too: a caller who reads the residual sees the stall."""
    filled, g, area, u = _terrain(oracle)
    k = _erosivity(area, Kc)
    span = float(filled.max() - filled.min())
    iters = ITERS[(Kc, n)]
    exact, _ = pn.solve_exact(g, D8, filled, k, SCALE, DT, n, u)
    ours = pn.solve_iterated(g, D8, filled, k, SCALE, DT, n, u, None, iters)
    old = pn.solve_iterated(g, D8, filled, k, SCALE, DT, n, u, None, iters, from_old=True)
    err_ours, err_old = float(np.abs(ours["out64"] - exact).max()), float(np.abs(old["out64"] - exact).max())
    print("Kc %g n %g, %d steps: from the n = 1 solve %.3g off (last change %.3g), from the old heights %.3g off (last "
          "change %.3g)" % (Kc, n, iters, err_ours, ours["residual"], err_old, old["residual"]))
    assert old["residual"] > 1e-9 * span and err_old > 1e3 * err_ours and err_old > 1e-6 * span


# ---- by hand ---------------------------------------------------------------------------------------------------

def _f32(*v):
    return np.array(v, np.float32)


def test_a_two_cell_chain_by_hand():
    """Cell 0 drains into cell 1, a terminal, along a column step of length sy.  n = 2: s + C s^2 = R has the root
    s = (sqrt(1 + 4 C R) - 1) / (2 C); x^0 is the n = 1 step, the first Newton step is written out."""
    graph = np.array([[1, -1]], np.int32)
    height, k, u = _f32(8.0, 2.0), _f32(0.5, 9.0), _f32(0.25, 100.0)
    dt, sy = 2.0, 0.5
    b, kd = 8.0 + dt * 0.25, 0.5 * dt
    F0 = kd / sy
    x0 = b / (1.0 + F0) + (F0 / (1.0 + F0)) * 2.0
    assert pn.solve_iterated(graph, D4, height, k, (3.0, sy), dt, 1.0, u)["out64"].tolist() == [[x0, 2.0]]
    S = (x0 - 2.0) / sy
    F = ((2.0 * kd) / sy) * S
    c = (kd * 1.0) * (S * S)
    x1 = (b + c) / (1.0 + F) + (F / (1.0 + F)) * 2.0
    got = pn.solve_iterated(graph, D4, height, k, (3.0, sy), dt, 2.0, u, None, 1)
    assert got["out64"].tolist() == [[x1, 2.0]] and got["residual"] == abs(x1 - x0)
    assert got["out64"][0, 1] == 2.0, "the terminal is neither lifted nor eroded"
    Cq, R = kd / sy, (b - 2.0) / sy
    root = 2.0 + sy * (np.sqrt(1.0 + 4.0 * Cq * R) - 1.0) / (2.0 * Cq)
    done = pn.solve_iterated(graph, D4, height, k, (3.0, sy), dt, 2.0, u, None, 8)
    assert abs(done["out64"][0, 0] - root) <= 4 * 2.0 ** -52 * root and done["residual"] <= 2.0 ** -50 * root
    assert abs(pn.solve_exact(graph, D4, height, k, (3.0, sy), dt, 2.0, u)[0][0, 0] - root) <= 4 * 2.0 ** -52 * root
    # pow=None is n == 2: the same words
    assert pn.solve_iterated(graph, D4, height, k, (3.0, sy), dt, 2.0, u, None, 8, pow=None)["out64"].tolist() == done["out64"].tolist()


def test_a_receiver_that_is_not_below_takes_no_erosion_and_a_stop_is_a_terminal():
    graph = np.array([[1, 2, -1]], np.int32)
    height, k = _f32(3.0, 5.0, 1.0), _f32(1.0, 1.0, 1.0)
    got = pn.solve_iterated(graph, D4, height, k, (1.0, 1.0), 0.0, 2.5, None, None, 3)
    assert got["out64"].tolist() == [[3.0, 5.0, 1.0]], "dt = 0: the heights"
    # cell 0 lies below its receiver, cell 1: in every iterate S = 0, so x = b = its own height plus the uplift
    u = _f32(0.5, 0.0, 0.0)
    # (cell 1 has no erosivity and keeps its 5; the n = 1 start pulls cell 0 up towards it, the Newton steps do not)
    got = pn.solve_iterated(graph, D4, height, _f32(1.0, 0.0, 1.0), (1.0, 1.0), 2.0, 2.5, u, None, 4)
    assert got["out64"].tolist() == [[4.0, 5.0, 1.0]]
    assert pn.solve_iterated(graph, D4, height, _f32(1.0, 0.0, 1.0), (1.0, 1.0), 2.0, 1.0, u)["out64"][0, 0] == 4.0 / 3.0 + (2.0 / 3.0) * 5.0
    stop = np.array([[0, 1, 0]], np.int32)
    got = pn.solve_iterated(graph, D4, height, k, (1.0, 1.0), 2.0, 2.5, u, stop, 4)
    assert got["out64"][0, 1] == 5.0 and got["final"].all()


def test_n_equal_one_is_the_stream_power_step_and_a_void_reaches_everything_upstream(oracle):
    filled, g, area, u = _terrain(oracle)
    k = _erosivity(area, 0.02)
    one = pn.solve_iterated(g, D8, filled, k, SCALE, DT, 1.0, u, None, 5)
    want = dref.solve_doubling(g, D8, scale=SCALE, power=(filled, k, u, DT))
    dref.same_words((one["out"], one["out64"]), want, "n = 1")
    assert one["residual"] == 0 and one["residuals"] == []
    h = filled.copy()
    at = int(np.argmax(np.where((area > 4) & (g >= 0), area, 0)))
    h.reshape(-1)[at] = np.nan
    got = pn.solve_iterated(g, D8, h, k, SCALE, DT, 2.0, u, None, 4)
    marks = np.zeros((H, W), np.float32)
    marks.reshape(-1)[at] = 1
    way = dref.solve_doubling(g, D8, a=marks, t=marks)[1] != 0
    assert (np.isnan(got["out64"]) == way).all() and way.sum() > 4 and np.isfinite(got["residual"])


# ---- the header, the symbols, the surfaces ---------------------------------------------------------------------

HEAD = ("float* out, double* out64, double* residual, const float* height, const int32_t* graph, "
        "const float* erosivity, const float* uplift, const int32_t* stop, ")
ENTRIES = {
    "soil_stream_power_n": HEAD + ("int64_t H, int64_t W, int edge, const float scale[2], double dt, double n, int iters, "
                                   "void* stream"),
    "soil_stream_power_n_batch": HEAD + ("int64_t B, int64_t H, int64_t W, int edge, const float* scales, "
                                         "int64_t n_scales, double dt, double n, int iters, void* stream"),
    "soil_stream_power_n_info": "int64_t info[4]",
    "soil_selftest_math64": "double* out, const double* a, const double* b, int64_t n, int op, void* stream",
}


def _squash(s):
    return re.sub(r"\s+", " ", s).strip()


def test_the_header_declares_the_entries_and_states_the_contract():
    text = open(os.path.join(ROOT, "include", "soil_hip.h")).read()
    assert "flow graphs: slope exponents above 1" in text
    assert text.index("flow graphs: erosion-deposition") < text.index("flow graphs: slope exponents above 1")
    for name, args in ENTRIES.items():
        m = re.search(r"int %s\((.*?)\);" % name, text, re.S)
        assert m, name
        assert _squash(m.group(1)) == args
    flat = _squash(re.sub(r"\n \* ?", "\n", text))
    for phrase in ("dh/dt = u - K A^m S^n", "S^n ~ (1 - n) S_j^n + n S_j^(n-1) S", "d = x[i] - x[r]",
                   "S = d <= 0 ? 0.0 : d / L", "P = n == 2 ? S : pow(S, n - 1)", "kd = (double)erosivity[i] * dt",
                   "F = ((n * kd) / L) * P", "c = (kd * (n - 1)) * (P * S)", "D = 1.0 + F ; A = (b + c) / D ; B = F / D",
                   "x^0 = the solve of soil_stream_power on the same arguments", "The start is the n = 1 solve",
                   "one cell per iteration", "takes no erosion in that step", "n < 1 is out of scope on purpose",
                   "soil_selftest_math64 op 0", "n == 1.0 runs soil_stream_power's single solve and nothing else",
                   "an n that is not finite, n < 1 or n > 16, iters < 1", "as integers", "Nothing synchronises",
                   "info[0] kernel launches, info[1] chunks, info[2] iterations run (0 for n == 1), info[3] bytes of scratch"):
        assert phrase in flat, phrase
    assert "soil_stream_power_n below iterates on this solve" in flat, "soil_stream_power's own text points here"


def test_the_library_binds_the_entries_and_the_build_has_the_source():
    from soillib_amd import _abi, build
    lib = _abi.lib()
    i64, vp, cint, fp, dbl = C.c_int64, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_double
    assert _abi.SIGNATURES["soil_stream_power_n"] == (cint, [vp] * 8 + [i64, i64, cint, fp, dbl, dbl, cint, vp])
    assert _abi.SIGNATURES["soil_stream_power_n_batch"] == (cint, [vp] * 8 + [i64, i64, i64, cint, fp, i64, dbl, dbl, cint, vp])
    assert _abi.SIGNATURES["soil_stream_power_n_info"] == (cint, [C.POINTER(i64)])
    assert _abi.SIGNATURES["soil_selftest_math64"] == (cint, [vp, vp, vp, i64, cint, vp])
    for name in ENTRIES:
        assert hasattr(lib, name), name
    found = [s for s in build.SOURCES if "int soil_stream_power_n(" in open(os.path.join(build.CSRC, s)).read()]
    assert found == ["downstream.hip"]
    common = open(os.path.join(build.CSRC, "common.hpp")).read()
    source = open(os.path.join(build.CSRC, found[0])).read()
    for slot in ("WS_POWER_N", "WS_POWER_N_ITERATE"):
        assert slot in common and slot in source, slot
    # one power function, in a header the kernel and the selftest both include; the engine's rounds as they are
    math = open(os.path.join(build.CSRC, "soil_math.hpp")).read()
    runtime = open(os.path.join(build.CSRC, "runtime.hip")).read()
    assert math.count("double sp_pow(double S, double e)") == 1
    assert "sp_pow(" in source and "sp_pow(" in runtime and "pow(" not in source.replace("sp_pow(", "")
    assert "k_pn_init<K, true>" in source and "down_launch_round<true>" in source and "k_dep_final<<<" in source


def test_the_surfaces():
    import inspect
    import soillib
    from soillib_amd import soil
    from soillib_amd.erosion import ErosionBatch
    for name in ("stream_power_n", "stream_power_n_batch", "stream_power_n_info"):
        assert callable(getattr(soil, name)) and getattr(soillib, name) is getattr(soil, name), name
    for fn in (soil.stream_power_n, soil.stream_power_n_batch):
        assert list(inspect.signature(fn).parameters) == ["height", "graph", "erosivity", "edge_", "scale", "dt", "n", "uplift",
                                                          "stop", "iters", "double", "residual"]
        assert inspect.signature(fn).parameters["iters"].default == 12
    sp = inspect.signature(ErosionBatch.stream_power).parameters
    assert list(sp)[-3:] == ["n", "iters", "residual"] and (sp["n"].default, sp["iters"].default, sp["residual"].default) == (1.0, 12, False)
    ev = inspect.signature(ErosionBatch.evolve).parameters
    assert list(ev)[-1] == "n" and ev["n"].default == 1.0
    assert "stream_power_n" not in open(os.path.join(ROOT, "include", "soil.hpp")).read(), "nothing new is named in soil.hpp"
    for fn in (soil.stream_power, ErosionBatch.stream_power):
        assert "slope exponent 1)" not in fn.__doc__


def test_the_call_info_needs_no_device():
    from soillib_amd import _abi, soil
    assert _abi.lib().soil_stream_power_n_info(None) == _abi.SOIL_ERR_INVALID_ARGUMENT
    assert _abi.last_error().startswith("stream_power_n_info: ")
    assert sorted(soil.stream_power_n_info()) == ["chunks", "iters", "launches", "scratch_bytes"]


# ---- refusals, without a device --------------------------------------------------------------------------------

def _p(k):
    """A stand-in for a tensor (never read): planes a MiB apart, so that none overlaps another."""
    return C.c_void_p(k << 20)


def _entries():
    """name -> call(over), `over` a dict of the arguments to replace in a well-formed call of (B, H, W) = (3, 4, 4)."""
    from soillib_amd import _abi
    lib = _abi.lib()
    sc = (C.c_float * 6)(1, 2, 1, 2, 1, 2)
    base = dict(out=_p(1), out64=_p(2), residual=_p(3), height=_p(4), graph=_p(5), erosivity=_p(6), uplift=_p(7),
                stop=_p(8), B=3, H=4, W=4, edge=D8, scale=sc, ns=3, dt=1.5, n=2.0, iters=4)
    head = ["out", "out64", "residual", "height", "graph", "erosivity", "uplift", "stop"]

    def call(fn, names):
        def go(over=()):
            v = dict(base, **dict(over))
            return fn(*[v[k] for k in names], None)
        return go
    return {
        "stream_power_n": call(lib.soil_stream_power_n, head + ["H", "W", "edge", "scale", "dt", "n", "iters"]),
        "stream_power_n_batch": call(lib.soil_stream_power_n_batch,
                                     head + ["B", "H", "W", "edge", "scale", "ns", "dt", "n", "iters"]),
    }


def _bad_scale(*v):
    return (C.c_float * 6)(*v)


REFUSED = [  # everything soil_stream_power refuses
           ("null graph", dict(graph=None)), ("both outputs null", dict(out=None, out64=None)),
           ("out is the graph", dict(out=_p(5))), ("out64 is the height", dict(out64=_p(4))),
           ("out inside the uplift", dict(out=C.c_void_p((7 << 20) + 16))), ("out overlaps out64", dict(out=C.c_void_p((2 << 20) + 8))),
           ("out is the stop plane", dict(out=_p(8))), ("out64 is the erosivity", dict(out64=_p(6))),
           ("H = 0", dict(H=0)), ("W = 0", dict(W=0)), ("W < 0", dict(W=-2)), ("H W > INT32_MAX", dict(H=1 << 16, W=1 << 15)),
           ("edge 2", dict(edge=2)), ("edge -1", dict(edge=-1)),
           ("null height", dict(height=None)), ("null erosivity", dict(erosivity=None)), ("null scale", dict(scale=None)),
           ("scale 0", dict(scale=_bad_scale(0, 1, 1, 1, 1, 1))), ("scale < 0", dict(scale=_bad_scale(1, -1, 1, 1, 1, 1))),
           ("scale inf", dict(scale=_bad_scale(float("inf"), 1, 1, 1, 1, 1))),
           ("scale NaN", dict(scale=_bad_scale(1, float("nan"), 1, 1, 1, 1))),
           ("dt < 0", dict(dt=-1e-9)), ("dt inf", dict(dt=float("inf"))), ("dt NaN", dict(dt=float("nan"))),
           # and the entries' own
           ("n NaN", dict(n=float("nan"))), ("n inf", dict(n=float("inf"))), ("n -inf", dict(n=float("-inf"))),
           ("n < 1", dict(n=0.999)), ("n 0", dict(n=0.0)), ("n < 0", dict(n=-2.0)), ("n > 16", dict(n=16.5)),
           ("iters 0", dict(iters=0)), ("iters < 0", dict(iters=-3)), ("iters 0 at n = 1", dict(iters=0, n=1.0)),
           ("residual is the graph", dict(residual=_p(5))), ("residual is the height", dict(residual=_p(4))),
           ("residual is the erosivity", dict(residual=_p(6))), ("residual is the uplift", dict(residual=_p(7))),
           ("residual is the stop plane", dict(residual=_p(8))), ("residual inside out", dict(residual=C.c_void_p((1 << 20) + 8))),
           ("residual is out64", dict(residual=_p(2))), ("residual inside out64", dict(residual=C.c_void_p((2 << 20) + 64)))]
BATCH = [("B = 0", dict(B=0)), ("B < 0", dict(B=-3)), ("n_scales 2 of 3", dict(ns=2)), ("n_scales 0", dict(ns=0)),
         ("n_scales 4 of 3", dict(ns=4)), ("a later model's scale 0", dict(scale=_bad_scale(1, 1, 1, 1, 0, 1)))]


def _cases(name):
    return REFUSED + (BATCH if name.endswith("_batch") else [])


def test_every_refusal_names_its_entry():
    from soillib_amd import _abi
    for name, call in _entries().items():
        for what, over in _cases(name):
            assert call(over) == _abi.SOIL_ERR_INVALID_ARGUMENT, (what, name)
            assert _abi.last_error().startswith(name + ": "), (what, name, _abi.last_error())
        assert call(dict(n=0.5)) == _abi.SOIL_ERR_INVALID_ARGUMENT
        assert "n < 1" in _abi.last_error() and "safeguarded solve per cell" in _abi.last_error(), _abi.last_error()


def test_a_well_formed_call_fails_loudly_without_a_device():
    from soillib_amd import _abi
    if _abi.lib().soil_device_count() > 0:
        pytest.skip("a HIP device is present")
    for name, call in _entries().items():
        assert call() == _abi.SOIL_ERR_NO_DEVICE, name
        assert call(dict(out=None, residual=None, stop=None)) == _abi.SOIL_ERR_NO_DEVICE, name
        assert call(dict(out64=None, uplift=None, dt=0.0, iters=1, n=1.0)) == _abi.SOIL_ERR_NO_DEVICE, name
        assert call(dict(n=16.0)) == _abi.SOIL_ERR_NO_DEVICE, name


def test_the_fp64_selftest_refuses_before_any_device_work():
    from soillib_amd import _abi
    lib = _abi.lib()
    for args in ((None, _p(2), _p(3), 4, 0), (_p(1), None, _p(3), 4, 0), (_p(1), _p(2), None, 4, 0),
                 (_p(1), _p(2), _p(3), 4, 1), (_p(1), _p(2), _p(3), 4, -1), (_p(1), _p(2), _p(3), 4, 12)):
        assert lib.soil_selftest_math64(*args, None) == _abi.SOIL_ERR_INVALID_ARGUMENT, args
        assert _abi.last_error().startswith("selftest_math64: "), _abi.last_error()


# ---- the ValueErrors of the Python layer: before any device work -----------------------------------------------

def _host(dtype, shape):
    from soillib_amd import silt
    return silt.tensor._wrap_numpy(np.zeros(shape, dtype))


def _module_refusals():
    from soillib_amd import soil
    g2, g3 = _host(np.int32, (4, 3)), _host(np.int32, (5, 4, 3))
    f2, f3 = _host(np.float32, (4, 3)), _host(np.float32, (5, 4, 3))
    one, many = soil.stream_power_n, soil.stream_power_n_batch
    ok = (1.0, 1.0)
    return [
        (one, (f2, g3, f2, soil.d8, ok, 1.0, 2.0), {}, "stream_power_n: graph"),
        (one, (g2, g2, f2, soil.d8, ok, 1.0, 2.0), {}, "stream_power_n: height"),
        (one, (None, g2, f2, soil.d8, ok, 1.0, 2.0), {}, "stream_power_n: height is required"),
        (one, (f2, g2, None, soil.d8, ok, 1.0, 2.0), {}, "stream_power_n: erosivity is required"),
        (one, (f2, g2, f3, soil.d8, ok, 1.0, 2.0), {}, "stream_power_n: erosivity"),
        (one, (f2, g2, f2, "d8", ok, 1.0, 2.0), {}, "stream_power_n: edge"),
        (one, (f2, g2, f2, soil.d8, None, 1.0, 2.0), {}, "stream_power_n: scale"),
        (one, (f2, g2, f2, soil.d8, (1.0, 0.0), 1.0, 2.0), {}, "stream_power_n: scale entries"),
        (one, (f2, g2, f2, soil.d8, ok, -1.0, 2.0), {}, "stream_power_n: dt"),
        (one, (f2, g2, f2, soil.d8, ok, float("nan"), 2.0), {}, "stream_power_n: dt"),
        (one, (f2, g2, f2, soil.d8, ok, 1.0, 2.0), dict(uplift=g2), "stream_power_n: uplift"),
        (one, (f2, g2, f2, soil.d8, ok, 1.0, 2.0), dict(stop=f2), "stream_power_n: stop"),
        (one, (f2, g2, f2, soil.d8, ok, 1.0, 2.0), dict(stop=g3), "stream_power_n: stop"),
        (one, (f2, g2, f2, soil.d8, ok, 1.0, 2.0), dict(iters=0), "stream_power_n: iters"),
        (one, (f2, g2, f2, soil.d8, ok, 1.0, 2.0), dict(iters=2.0), "stream_power_n: iters"),
        (one, (f2, g2, f2, soil.d8, ok, 1.0, 2.0), dict(iters=True), "stream_power_n: iters"),
        (many, (f3, g2, f3, soil.d8, ok, 1.0, 2.0), {}, r"stream_power_n_batch: graph: expected a \(B, H, W\)"),
        (many, (f3, g3, f2, soil.d8, ok, 1.0, 2.0), {}, "stream_power_n_batch: erosivity"),
        (many, (f3, g3, f3, soil.d8, [[1.0, 1.0]] * 4, 1.0, 2.0), {}, "stream_power_n_batch: scale"),
        (many, (f3, g3, f3, soil.d8, [[1.0, 1.0]] * 4 + [[1.0, -2.0]], 1.0, 2.0), {}, "stream_power_n_batch: scale entries"),
        (many, (f3, g3, f3, soil.d8, ok, 1.0, 2.0), dict(iters=-1), "stream_power_n_batch: iters"),
        (many, (f3, g3, f3, soil.d8, ok, 1.0, 0.5), {}, "stream_power_n_batch: n must be"),
    ]


def test_the_module_functions_refuse():
    for fn, args, kw, match in _module_refusals():
        with pytest.raises(ValueError, match=match):
            fn(*args, **kw)


def test_the_exponent_and_the_count_are_numbers_in_range():
    """n as a Python or numpy number in 1 .. 16 and iters as an integer: past the scalar checks, refused at the device
    check only (the tensors are host tensors).  Anything else is refused with one text whatever its type."""
    from soillib_amd import _abi, soil
    g2, g3 = _host(np.int32, (4, 3)), _host(np.int32, (5, 4, 3))
    f2, f3 = _host(np.float32, (4, 3)), _host(np.float32, (5, 4, 3))
    for name, fn, f, g in (("stream_power_n", soil.stream_power_n, f2, g2), ("stream_power_n_batch", soil.stream_power_n_batch, f3, g3)):
        for n, iters in ((1, 1), (1.0, np.int64(2)), (np.float32(2.5), np.uint8(3)), (np.int64(3), 8), (16, 2), (16.0, 2)):
            with pytest.raises(_abi.SoilError, match="mismatch_host"):
                fn(f, g, f, soil.d8, (1.0, 1.0), 1.0, n, iters=iters)
        for n in (True, "2", None, float("nan"), float("inf"), -float("inf"), 0.999, 0, -2.0, 16.001, 17, np.float32("nan"),
                  np.float64(0.5)):
            with pytest.raises(ValueError) as e:
                fn(f, g, f, soil.d8, (1.0, 1.0), 1.0, n)
            assert str(e.value) == ("%s: n must be a finite number in 1 .. 16 (a slope exponent below 1 needs a safeguarded "
                                    "solve per cell), got %r" % (name, n))
        for iters in (True, "2", 2.0, 0, np.int64(0), -1, 2 ** 31, float("nan")):
            with pytest.raises(ValueError) as e:
                fn(f, g, f, soil.d8, (1.0, 1.0), 1.0, 2.0, iters=iters)
            assert str(e.value) == "%s: iters must be an integer >= 1, got %r" % (name, iters)


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


def test_the_batch_methods_refuse():
    cases = [("stream_power", dict(n=0.5), r"ErosionBatch\.stream_power: n must be"),
             ("stream_power", dict(n=float("nan")), r"ErosionBatch\.stream_power: n must be"),
             ("stream_power", dict(n="2"), r"ErosionBatch\.stream_power: n must be"),
             ("stream_power", dict(n=17), r"ErosionBatch\.stream_power: n must be"),
             ("stream_power", dict(n=2.0, iters=0), r"ErosionBatch\.stream_power: iters"),
             ("stream_power", dict(n=2.0, iters=1.5), r"ErosionBatch\.stream_power: iters"),
             ("stream_power", dict(n=2.0, kind="direction"), r"ErosionBatch\.stream_power: kind"),
             ("evolve", dict(kappa=0.1, n=0.5), r"ErosionBatch\.evolve: n must be"),
             ("evolve", dict(kappa=0.1, n=True), r"ErosionBatch\.evolve: n must be"),
             ("evolve", dict(kappa=0.1, n=2.0, iters=0), r"ErosionBatch\.evolve: iters"),
             ("evolve", dict(kappa=0.1, n=2.0, G=1.0), r"ErosionBatch\.evolve: G \(deposition\) takes the slope exponent n = 1 only"),
             ("evolve", dict(kappa=0.1, n=1.5, G=0.0), r"ErosionBatch\.evolve: G \(deposition\) takes the slope exponent n = 1 only")]
    for method, kw, match in cases:
        with pytest.raises(ValueError, match=match):
            getattr(_batch_without_a_device(), method)(1.0, 1e-4, **kw)


def test_evolve_routes_by_the_exponent(monkeypatch):
    """evolve(n=1), the default: stream_power with today's positional arguments and no keyword; with n != 1 the same
    call with n and iters behind them; then diffuse_batch of the result either way."""
    from soillib_amd import soil
    from soillib_amd.erosion import ErosionBatch
    bt = _batch_without_a_device()
    calls = []
    monkeypatch.setattr(ErosionBatch, "stream_power", lambda self, *a, **k: calls.append(("stream_power", a, k)) or "carved")
    monkeypatch.setattr(ErosionBatch, "stream_power_deposit",
                        lambda self, *a, **k: calls.append(("stream_power_deposit", a, k)) or "filled")
    monkeypatch.setattr(soil, "diffuse_batch", lambda *a, **k: calls.append(("diffuse_batch", a, k)) or "out")
    for kw in ({}, dict(n=1.0), dict(n=1, iters=3)):
        del calls[:]
        assert bt.evolve(2.0, 1e-3, kappa=0.25, **kw) == "out"
        assert calls == [("stream_power", (2.0, 1e-3, 0.5, "steepest", None, None, 0, None), {}),
                         ("diffuse_batch", ("carved", [1.0, 1.0], 2.0, 0.25), dict(border="fixed", first_axis=0))]
    del calls[:]
    assert bt.evolve(2.0, 1e-3, 0.4, 0.25, None, "random_weighted", soil.d4, 1.5, 3, 1, None, 5, 2.5) == "out"
    assert calls == [("stream_power", (2.0, 1e-3, 0.4, "random_weighted", soil.d4, 1.5, 3, None, 2.5, 5), {}),
                     ("diffuse_batch", ("carved", [1.0, 1.0], 2.0, 0.25), dict(border="fixed", first_axis=1))]
    del calls[:]
    assert bt.evolve(2.0, 1e-3, kappa=0.25, G=1.5, iters=3, n=1.0) == "out"
    assert calls[0] == ("stream_power_deposit", (2.0, 1e-3, 0.5, 1.5, 3, "steepest", None, None, 0, None), {})
