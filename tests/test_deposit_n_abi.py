"""The erosion-deposition step at a slope exponent above 1 (include/soil_hip.h: "flow graphs: erosion-deposition at
slope exponents above 1"; soil_stream_power_deposit_n and its _batch form), what can be checked without a GPU: the
restatement solve_iterated of tests/deposit_n_ref.py on a conditioned terrain with a filled lake — where its iteration
ends, and the defect of the nonlinear equation there —, its bit identities with the restatements of the two steps it
joins, one diverging case that pins the documented limit, hand-computed cases, the header, the bound symbols and the
surfaces, every refusal with the entry's name in the message, SOIL_ERR_NO_DEVICE for a well-formed call, and the
ValueErrors and call order of the Python layer.

Where the iteration ends.  On this terrain, with K dt / L of order 1, the last change does NOT fall below 1e-9 of the
height range in any of the six cases: it falls geometrically (a factor of 0.3 to 0.75 an iteration) and then stops at
one value, 3e-7 to 2e-6 on heights that span 95, from which no further iteration moves it — the float32 floor of Qs
the header of soil_stream_power_deposit describes: Qs is rounded to 2^-24 of itself and enters a cell's A as
g Qs / D.  The unit is therefore FLOOR = max over the cells of 2^-24 Qs g / D at the returned iterate, the test asserts
that the residual has stopped (four more iterations leave it within a factor of two) at a small multiple of it, and
the multiple is measured, printed and held with a factor of 4, as tests/test_power_n_abi.py holds its defect.

The defect of the nonlinear equation, Qs re-summed in fp64, has the same origin without the division: the float32
rounding of q and of the partial sums of Qs, times g.  Its unit is max 2^-24 Qs g; measured, printed, held at 4 x."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import deposit_n_ref as dn
import deposit_ref as dep
import downstream_ref as dref
import flats_ref
import power_n_ref as pn
from flow_paths_ref import D4, D8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 24, 36
SCALE, DT = (1.0, 1.5), 50.0
# (n, G) -> the iterations after which the restatement's last change has stopped falling (Kc = 0.02), found case by
# case on the restatement and one more
ITERS = {(1.5, 0.5): 15, (1.5, 1.0): 32, (2.0, 0.5): 18, (2.0, 1.0): 43, (3.0, 0.5): 21, (3.0, 1.0): 54}
FLOOR_MULTIPLE = 4 * 8.9                                      # 4 x the 8.9 measured below (n = 3, G = 1)
DEFAULT_ITERS = 28                                            # the table it was chosen from
DEFECT_MULTIPLE = 4 * 1.2                                     # 4 x the 1.2 measured below (n = 3, G = 0.5)


@functools.lru_cache(maxsize=None)
def _terrain(oracle_):
    """tests/test_power_n_abi.py's terrain: noise x 100 with a basin pressed into it, conditioned for D8 on the CPU —
    the filled surface, its steepest graph with the flats routed, the drainage area and a uniform uplift."""
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


def _deposition(area, G):
    return (np.float32(G) / area).astype(np.float32)


def test_the_terrain_has_a_filled_lake_and_the_two_regimes(oracle):
    filled, g, area, u = _terrain(oracle)
    r = g.reshape(-1)
    has = r >= 0
    level = has & (filled.reshape(-1) == filled.reshape(-1)[np.where(has, r, 0)])
    assert level.sum() >= 30 and dref.solve_doubling(g, D8)[2].all() and not flats_ref.interior_terminals(g).any()
    for Kc, order in ((0.02, 1.0), (2.0, 100.0)):
        mid = float(np.median(_erosivity(area, Kc))) * DT / 1.0
        assert order / 3 <= mid <= order * 3, "K dt / L of order %g, got a median of %g" % (order, mid)


# ---- where the iteration ends, and the defect there --------------------------------------------------------------

@pytest.mark.parametrize("G", [0.5, 1.0])
@pytest.mark.parametrize("n", [1.5, 2.0, 3.0])
def test_the_iteration_stops_at_the_float32_floor_and_the_defect_there(oracle, n, G):
    filled, g, area, u = _terrain(oracle)
    k, d = _erosivity(area, 0.02), _deposition(area, G)
    span = float(filled.max() - filled.min())
    iters = ITERS[(n, G)]
    it = dn.solve_iterated(oracle, g, D8, filled, k, d, SCALE, DT, n, u, iters + 4, every=True)
    res = it["residuals"]
    at = it["steps"][iters - 1]
    assert at["final"].all() and np.isfinite(at["out64"]).all()
    print("n %g G %g: residuals %s" % (n, G, " ".join("%.2g" % v for v in res)))
    # the unit of the floor at the iterate returned after `iters`
    is_edge, rc, L, h, kd, b = pn.planes(g, D8, filled, k, SCALE, DT, u)
    x = at["out64"].reshape(-1)
    gg = dep._f64(d, H * W)
    Qs = np.abs(at["flux"].reshape(-1).astype(np.float64))
    S = np.where(x - x[rc] <= 0, 0.0, (x - x[rc]) / L)
    D = (1.0 + ((n * kd) / L) * np.power(S, n - 1.0)) + gg
    floor = float(np.where(is_edge, 2.0 ** -24 * Qs * gg / D, 0.0).max())
    print("n %g G %g: after %d iterations the last change is %.3g = %.1f x the floor unit %.3g (held: %g), %.3g of the "
          "range" % (n, G, iters, res[iters - 1], res[iters - 1] / floor, floor, FLOOR_MULTIPLE, res[iters - 1] / span))
    # which of the two the restatement shows: it does not reach 1e-9 of the range, it stops at the floor
    assert min(res) > 1e-9 * span, "the float32 floor lies above 1e-9 of the range on this terrain"
    assert res[iters - 1] <= FLOOR_MULTIPLE * floor
    assert all(0.5 * res[iters - 1] <= v <= 2.0 * res[iters - 1] for v in res[iters:]), "it has stopped"
    assert res[iters // 3] > 30 * res[iters - 1], "and it fell on the way there"
    # the defect of the nonlinear equation, Qs re-summed in fp64
    miss, _ = dn.defect(at["out64"], g, D8, filled, k, d, SCALE, DT, n, u)
    unit = float(np.where(is_edge, 2.0 ** -24 * Qs * gg, 0.0).max())
    print("n %g G %g: the defect is %.3g at most = %.1f x 2^-24 max Qs g = %.3g (held: %g)" % (
        n, G, miss.max(), miss.max() / unit, unit, DEFECT_MULTIPLE))
    assert miss.max() <= DEFECT_MULTIPLE * unit
    # deposition: somewhere the surface ends above the plain n step's
    plain = pn.solve_iterated(g, D8, filled, k, SCALE, DT, n, u, None, iters)["out64"]
    assert (at["out64"] - plain).max() > 1e-3 * span


def test_outside_the_domain_the_residual_grows(oracle):
    """n = 3, G = 4, K dt / L of order 100: the change of iteration 12 exceeds that of iteration 4 (here by many orders)
    while every value stays finite — the documented limit; nothing but the residual says so."""
    filled, g, area, u = _terrain(oracle)
    it = dn.solve_iterated(oracle, g, D8, filled, _erosivity(area, 2.0), _deposition(area, 4.0), SCALE, DT, 3.0, u, 12)
    res = it["residuals"]
    print("n 3 G 4 Kc 2: residuals %s" % " ".join("%.2g" % v for v in res))
    assert res[11] > res[3] and res[11] > 1e3 * float(filled.max() - filled.min())
    assert np.isfinite(it["out64"]).all() and it["final"].all()


# ---- the bit identities of the restatement ----------------------------------------------------------------------

@pytest.mark.parametrize("n", [1.5, 2.0, 3.0])
def test_zero_deposition_is_the_slope_exponent_step(oracle, n):
    filled, g, area, u = _terrain(oracle)
    k, zero = _erosivity(area, 0.02), np.zeros((H, W), np.float32)
    for uplift, iters in ((u, 1), (None, 3), (u, 6)):
        got = dn.solve_iterated(oracle, g, D8, filled, k, zero, SCALE, DT, n, uplift, iters)
        want = pn.solve_iterated(g, D8, filled, k, SCALE, DT, n, uplift, None, iters)
        pn.same_words(got, want, "zero deposition, n %g iters %d" % (n, iters))
        assert got["residuals"] == want["residuals"]


def test_n_equal_one_is_the_deposit_step(oracle):
    filled, g, area, u = _terrain(oracle)
    k, d = _erosivity(area, 0.02), _deposition(area, 1.0)
    for uplift, iters in ((u, 1), (None, 4)):
        got = dn.solve_iterated(oracle, g, D8, filled, k, d, SCALE, DT, 1.0, uplift, iters)
        want = dep.solve_iterated(oracle, g, D8, filled, k, d, SCALE, DT, uplift, iters)
        dep.same_words(got, want, "n = 1, iters %d" % iters)
    # its start is b, not the solve: with one iteration Qs is +0 everywhere and the flux is what that one solve removed
    one = dn.solve_iterated(oracle, g, D8, filled, k, d, SCALE, DT, 1.0, u, 1)
    lifted = np.where(g >= 0, filled.astype(np.float64) + DT * u.astype(np.float64), filled)
    assert one["residual"] == np.abs(one["out64"] - lifted).max() > 0


# ---- by hand ---------------------------------------------------------------------------------------------------

def _f32(*v):
    return np.array(v, np.float32)


def test_a_two_cell_chain_by_hand(oracle):
    """Cell 0 drains into cell 1, a terminal, along a column step of length sy; nothing drains into cell 0, so Qup is
    0 in every iteration.  n = 2: x^0 is the n = 1 step without deposition, the first iteration is written out."""
    graph = np.array([[1, -1]], np.int32)
    height, k, u, d = _f32(8.0, 2.0), _f32(0.5, 9.0), _f32(0.25, 100.0), _f32(0.75, 5.0)
    dt, sy, g = 2.0, 0.5, 0.75
    b, kd = 8.0 + dt * 0.25, 0.5 * dt
    F0 = kd / sy
    x0 = b / (1.0 + F0) + (F0 / (1.0 + F0)) * 2.0
    S = (x0 - 2.0) / sy
    F = ((2.0 * kd) / sy) * S
    c = (kd * 1.0) * (S * S)
    D = (1.0 + F) + g
    q0 = float(np.float32(b - x0))
    assert q0 - q0 == 0.0                                     # Qs = q, Qup = 0
    x1 = ((((1.0 + g) * b) + (g * 0.0)) + c) / D + (F / D) * 2.0
    got = dn.solve_iterated(oracle, graph, D4, height, k, d, (3.0, sy), dt, 2.0, u, 1)
    assert got["out64"].tolist() == [[x1, 2.0]] and got["residual"] == abs(x1 - x0)
    assert got["flux"].tolist() == [[np.float32(b - x1)] * 2], "what cell 0 lost reaches the terminal"
    # the fixed point: s + C s^2 = R with C = kd / (1 + g) / sy ... written as a quadratic in the height itself
    done = dn.solve_iterated(oracle, graph, D4, height, k, d, (3.0, sy), dt, 2.0, u, 10)
    x = done["out64"][0, 0]
    s = (x - 2.0) / sy
    assert abs((x - b) + kd * s * s - g * (b - x)) <= 8 * 2.0 ** -52 * b and done["residual"] <= 2.0 ** -50 * b
    assert x > pn.solve_iterated(graph, D4, height, k, (3.0, sy), dt, 2.0, u, None, 10)["out64"][0, 0], "deposition"
    # pow=None is n == 2: the same words
    assert dn.solve_iterated(oracle, graph, D4, height, k, d, (3.0, sy), dt, 2.0, u, 10, pow=None)["out64"].tolist() == done["out64"].tolist()


def test_a_y_of_three_cells_by_hand(oracle):
    """A 2 x 3 grid, D8: cells 0 and 2 drain diagonally into cell 4, which drains along its row into cell 3, a
    terminal; cells 1 and 5 are terminals too.  Qup of cell 4 is what 0 and 2 lost in x^0, and the iteration written
    out with the association of the rounds: x[0] = (A0 + B0 A4) + (B0 B4) h3."""
    graph = np.array([[4, -1, 4], [-1, 3, -1]], np.int32)
    height = _f32(9.0, 0.0, 7.0, 1.0, 4.0, 0.0)
    k, d = _f32(0.5, 0.0, 0.25, 0.0, 1.0, 0.0), _f32(0.5, 0.0, 0.5, 0.0, 0.25, 0.0)
    dt, n, scale = 2.0, 2.0, (1.0, 0.5)
    sx, sy, dd = dref.path_scale(scale)
    L = {0: dd, 2: dd, 4: sy}
    rcv = {0: 4, 2: 4, 4: 3}
    h = height.astype(np.float64)
    # x^0: soil_stream_power's solve with the same association
    A, B = {}, {}
    for i in (0, 2, 4):
        F = (float(k[i]) * dt) / L[i]
        A[i], B[i] = h[i] / (1.0 + F), F / (1.0 + F)
    x0 = {3: h[3], 4: A[4] + B[4] * h[3]}
    for i in (0, 2):
        x0[i] = (A[i] + B[i] * A[4]) + (B[i] * B[4]) * h[3]
    assert dn.solve_iterated(oracle, graph, D8, height, k, np.zeros(6, np.float32), scale, dt, 1.0, None, 1)["out64"].reshape(-1)[[0, 2, 4]].tolist() == [x0[0], x0[2], x0[4]]
    q = {i: np.float32(h[i] - x0[i]) for i in (0, 2, 4)}
    qplane = np.zeros((2, 3), np.float32)
    for i in q:
        qplane.reshape(-1)[i] = q[i]
    Qs = oracle.accumulate(graph, qplane, D8).reshape(-1)
    Qup = {i: float(Qs[i]) - float(q[i]) for i in q}
    assert Qup[0] == 0.0 and Qup[2] == 0.0
    assert abs(Qup[4] - (float(q[0]) + float(q[2]))) <= 2.0 ** -22 * float(Qs[4]) and Qup[4] > 1.0, "Qup is visible"
    for i in (0, 2, 4):
        S = (x0[i] - x0[rcv[i]]) / L[i]
        assert S > 0
        kd = float(k[i]) * dt
        F = ((n * kd) / L[i]) * S
        c = (kd * (n - 1.0)) * (S * S)
        g = float(d[i])
        D = (1.0 + F) + g
        A[i], B[i] = ((((1.0 + g) * h[i]) + (g * Qup[i])) + c) / D, F / D
    want = {4: A[4] + B[4] * h[3]}
    for i in (0, 2):
        want[i] = (A[i] + B[i] * A[4]) + (B[i] * B[4]) * h[3]
    got = dn.solve_iterated(oracle, graph, D8, height, k, d, scale, dt, n, None, 1)
    assert got["out64"].reshape(-1).tolist() == [want[0], 0.0, want[2], 1.0, want[4], 0.0]
    assert got["residual"] == max(abs(want[i] - x0[i]) for i in want)
    # without cell 4's share of what came from upstream it would lie lower by g Qup / D
    without = dn.solve_iterated(oracle, graph, D8, height, k, _f32(0.5, 0.0, 0.5, 0.0, 0.0, 0.0), scale, dt, n, None, 1)
    assert got["out64"][1, 1] > without["out64"][1, 1]


# ---- the header, the symbols, the surfaces ---------------------------------------------------------------------

HEAD = ("float* out, double* out64, float* flux, double* residual, const float* height, const int32_t* graph, "
        "const float* erosivity, const float* deposition, const float* uplift, ")
ENTRIES = {
    "soil_stream_power_deposit_n": HEAD + ("int64_t H, int64_t W, int edge, const float scale[2], double dt, double n, "
                                           "int iters, void* stream"),
    "soil_stream_power_deposit_n_batch": HEAD + ("int64_t B, int64_t H, int64_t W, int edge, const float* scales, "
                                                 "int64_t n_scales, double dt, double n, int iters, void* stream"),
    "soil_stream_power_deposit_n_info": "int64_t info[4]",
}


def _squash(s):
    return re.sub(r"\s+", " ", s).strip()


def test_the_header_declares_the_entries_and_states_the_contract():
    text = open(os.path.join(ROOT, "include", "soil_hip.h")).read()
    assert "flow graphs: erosion-deposition at slope exponents above 1" in text
    assert text.index("flow graphs: slope exponents above 1") < text.index("flow graphs: erosion-deposition at slope exponents above 1")
    for name, args in ENTRIES.items():
        m = re.search(r"int %s\((.*?)\);" % name, text, re.S)
        assert m, name
        assert _squash(m.group(1)) == args
    flat = _squash(re.sub(r"\n \* ?", "\n", text[text.index("flow graphs: erosion-deposition at slope exponents above 1"):]))
    for phrase in ("dh/dt = u - K A^m S^n + (G / A) * Qs", "S^n ~ (1 - n) S_j^n + n S_j^(n-1) S",
                   "x - b = -k dt S^n + g (Qup + b - x)", "There is no `stop` plane",
                   "x^0 = the solve of soil_stream_power on the same arguments with stop == NULL",
                   "q[i] = (float)(b - x[i])", "Qup = (double)Qs[i] - (double)q[i]", "d = x[i] - x[r]",
                   "S = d <= 0 ? 0.0 : d / L", "P = n == 2 ? S : pow(S, n - 1)", "kd = (double)erosivity[i] * dt",
                   "F = ((n * kd) / L) * P", "c = (kd * (n - 1)) * (P * S)", "g = (double)deposition[i]",
                   "D = (1.0 + F) + g", "A = ((((1.0 + g) * b) + (g * Qup)) + c) / D ; B = F / D",
                   "the bits of soil_stream_power_n with stop == NULL at the same `iters`", "but for b == -0.0",
                   "n == 1.0 runs soil_stream_power_deposit's iterations and nothing else", "x^0 = b, not the solve",
                   "THE ITERATION HAS A DOMAIN", "No damping is added", "the residual grows", "the caller must read it",
                   "soil_selftest_math64 op 0", "an n that is not finite, n < 1 or n > 16", "a null `deposition`, iters < 1",
                   "info[0] kernel launches, info[1] chunks, info[2] iterations run, info[3] bytes of scratch"):
        assert phrase in flat, phrase


def test_the_library_binds_the_entries_and_the_build_has_the_source():
    from soillib_amd import _abi, build
    lib = _abi.lib()
    i64, vp, cint, fp, dbl = C.c_int64, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_double
    assert _abi.SIGNATURES["soil_stream_power_deposit_n"] == (cint, [vp] * 9 + [i64, i64, cint, fp, dbl, dbl, cint, vp])
    assert _abi.SIGNATURES["soil_stream_power_deposit_n_batch"] == (cint, [vp] * 9 + [i64, i64, i64, cint, fp, i64, dbl, dbl, cint, vp])
    assert _abi.SIGNATURES["soil_stream_power_deposit_n_info"] == (cint, [C.POINTER(i64)])
    for name in ENTRIES:
        assert hasattr(lib, name), name
    found = [s for s in build.SOURCES if "int soil_stream_power_deposit_n(" in open(os.path.join(build.CSRC, s)).read()]
    assert found == ["downstream.hip"]
    source = open(os.path.join(build.CSRC, found[0])).read()
    # one init kernel of its own, on the short band, in both forms of the one launcher; the rest as it is
    assert "k_dn_init<K, true>, k_dn_init<K, false>, pn_init_grid(" in source and source.count("sp_pow(") == 2
    assert "pow(" not in source.replace("sp_pow(", "")
    for shared in ("k_dep_q<K, true, false>", "rake_accumulate(", "solve_pass(", "iter_setup(", "k_dep_final<<<"):
        assert shared in source, shared
    assert "stream_power_deposit_n" not in open(os.path.join(ROOT, "include", "soil.hpp")).read(), "nothing new is named in soil.hpp"


def test_the_surfaces():
    import inspect
    import soillib
    from soillib_amd import soil
    from soillib_amd.erosion import ErosionBatch
    for name in ("stream_power_deposit_n", "stream_power_deposit_n_batch", "stream_power_deposit_n_info"):
        assert callable(getattr(soil, name)) and getattr(soillib, name) is getattr(soil, name), name
    for fn in (soil.stream_power_deposit_n, soil.stream_power_deposit_n_batch):
        assert list(inspect.signature(fn).parameters) == ["height", "graph", "erosivity", "deposition", "edge_", "scale", "dt",
                                                          "n", "uplift", "iters", "double", "flux", "residual"]
        assert inspect.signature(fn).parameters["iters"].default == soil.DEPOSIT_N_ITERS == DEFAULT_ITERS
    sp = inspect.signature(ErosionBatch.stream_power_deposit_n).parameters
    assert list(sp) == ["self", "dt", "K", "m", "G", "n", "iters", "kind", "edge", "T", "offset", "uplift", "flux", "residual"]
    assert (sp["m"].default, sp["G"].default, sp["n"].default, sp["iters"].default) == (0.5, 1.0, 2.0, None)
    ev = inspect.signature(ErosionBatch.evolve_deposit).parameters
    assert list(ev)[:9] == ["self", "dt", "K", "G", "n", "m", "kappa", "critical_slope", "uplift"]
    assert all(ev[k].default is inspect.Parameter.empty for k in ("dt", "K", "G", "n"))
    # the methods that refuse G with n != 1 say where that step is
    for fn in (ErosionBatch.evolve, soil.stream_power_deposit):
        assert "stream_power_deposit_n" in fn.__doc__ and "no counterpart" not in fn.__doc__


def test_the_call_info_needs_no_device():
    from soillib_amd import _abi, soil
    assert _abi.lib().soil_stream_power_deposit_n_info(None) == _abi.SOIL_ERR_INVALID_ARGUMENT
    assert _abi.last_error().startswith("stream_power_deposit_n_info: ")
    assert sorted(soil.stream_power_deposit_n_info()) == ["chunks", "iters", "launches", "scratch_bytes"]


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
                deposition=_p(8), uplift=_p(9), B=3, H=4, W=4, edge=D8, scale=sc, ns=3, dt=1.5, n=2.0, iters=4)
    head = ["out", "out64", "flux", "residual", "height", "graph", "erosivity", "deposition", "uplift"]

    def call(fn, names):
        def go(over=()):
            v = dict(base, **dict(over))
            return fn(*[v[k] for k in names], None)
        return go
    return {
        "stream_power_deposit_n": call(lib.soil_stream_power_deposit_n, head + ["H", "W", "edge", "scale", "dt", "n", "iters"]),
        "stream_power_deposit_n_batch": call(lib.soil_stream_power_deposit_n_batch,
                                             head + ["B", "H", "W", "edge", "scale", "ns", "dt", "n", "iters"]),
    }


def _bad_scale(*v):
    return (C.c_float * 6)(*v)


REFUSED = [  # everything soil_stream_power refuses (there is no stop plane)
           ("null graph", dict(graph=None)), ("both outputs null", dict(out=None, out64=None)),
           ("out is the graph", dict(out=_p(6))), ("out64 is the height", dict(out64=_p(5))),
           ("out inside the uplift", dict(out=C.c_void_p((9 << 20) + 16))), ("out overlaps out64", dict(out=C.c_void_p((2 << 20) + 8))),
           ("out64 is the erosivity", dict(out64=_p(7))),
           ("H = 0", dict(H=0)), ("W = 0", dict(W=0)), ("W < 0", dict(W=-2)), ("H W > INT32_MAX", dict(H=1 << 16, W=1 << 15)),
           ("edge 2", dict(edge=2)), ("edge -1", dict(edge=-1)),
           ("null height", dict(height=None)), ("null erosivity", dict(erosivity=None)), ("null scale", dict(scale=None)),
           ("scale 0", dict(scale=_bad_scale(0, 1, 1, 1, 1, 1))), ("scale < 0", dict(scale=_bad_scale(1, -1, 1, 1, 1, 1))),
           ("scale inf", dict(scale=_bad_scale(float("inf"), 1, 1, 1, 1, 1))),
           ("scale NaN", dict(scale=_bad_scale(1, float("nan"), 1, 1, 1, 1))),
           ("dt < 0", dict(dt=-1e-9)), ("dt inf", dict(dt=float("inf"))), ("dt NaN", dict(dt=float("nan"))),
           # the deposit entries' own
           ("null deposition", dict(deposition=None)), ("out is the deposition", dict(out=_p(8))),
           ("out64 inside the deposition", dict(out64=C.c_void_p((8 << 20) + 8))),
           ("iters 0", dict(iters=0)), ("iters < 0", dict(iters=-3)), ("iters 0 at n = 1", dict(iters=0, n=1.0)),
           ("flux is the graph", dict(flux=_p(6))), ("flux is the deposition", dict(flux=_p(8))),
           ("flux is out", dict(flux=_p(1))), ("flux inside out64", dict(flux=C.c_void_p((2 << 20) + 64))),
           ("flux is the uplift", dict(flux=_p(9))), ("flux is the height", dict(flux=_p(5))),
           ("residual is the height", dict(residual=_p(5))), ("residual is the graph", dict(residual=_p(6))),
           ("residual is the erosivity", dict(residual=_p(7))), ("residual is the deposition", dict(residual=_p(8))),
           ("residual inside flux", dict(residual=C.c_void_p((3 << 20) + 16))), ("residual is out64", dict(residual=_p(2))),
           ("residual inside out", dict(residual=C.c_void_p((1 << 20) + 8))),
           # and the slope exponent's
           ("n NaN", dict(n=float("nan"))), ("n inf", dict(n=float("inf"))), ("n -inf", dict(n=float("-inf"))),
           ("n < 1", dict(n=0.999)), ("n 0", dict(n=0.0)), ("n < 0", dict(n=-2.0)), ("n > 16", dict(n=16.5))]
BATCH = [("B = 0", dict(B=0)), ("B < 0", dict(B=-3)), ("n_scales 2 of 3", dict(ns=2)), ("n_scales 0", dict(ns=0)),
         ("n_scales 4 of 3", dict(ns=4)), ("a later model's scale 0", dict(scale=_bad_scale(1, 1, 1, 1, 0, 1)))]


def test_every_refusal_names_its_entry():
    from soillib_amd import _abi
    for name, call in _entries().items():
        for what, over in REFUSED + (BATCH if name.endswith("_batch") else []):
            assert call(over) == _abi.SOIL_ERR_INVALID_ARGUMENT, (what, name)
            assert _abi.last_error().startswith(name + ": "), (what, name, _abi.last_error())
        assert call(dict(n=0.5)) == _abi.SOIL_ERR_INVALID_ARGUMENT
        assert "n < 1" in _abi.last_error() and "safeguarded solve per cell" in _abi.last_error(), _abi.last_error()
        assert call(dict(deposition=None)) == _abi.SOIL_ERR_INVALID_ARGUMENT and "null deposition" in _abi.last_error()


def test_a_well_formed_call_fails_loudly_without_a_device():
    from soillib_amd import _abi
    if _abi.lib().soil_device_count() > 0:
        pytest.skip("a HIP device is present")
    for name, call in _entries().items():
        assert call() == _abi.SOIL_ERR_NO_DEVICE, name
        assert call(dict(out=None, flux=None, residual=None)) == _abi.SOIL_ERR_NO_DEVICE, name
        assert call(dict(out64=None, uplift=None, dt=0.0, iters=1, n=1.0)) == _abi.SOIL_ERR_NO_DEVICE, name
        assert call(dict(n=16.0)) == _abi.SOIL_ERR_NO_DEVICE, name


# ---- the ValueErrors of the Python layer: before any device work -----------------------------------------------

def _host(dtype, shape):
    from soillib_amd import silt
    return silt.tensor._wrap_numpy(np.zeros(shape, dtype))


def _module_refusals():
    from soillib_amd import soil
    g2, g3 = _host(np.int32, (4, 3)), _host(np.int32, (5, 4, 3))
    f2, f3 = _host(np.float32, (4, 3)), _host(np.float32, (5, 4, 3))
    one, many = soil.stream_power_deposit_n, soil.stream_power_deposit_n_batch
    ok = (1.0, 1.0)
    return [
        (one, (f2, g3, f2, f2, soil.d8, ok, 1.0, 2.0), {}, "stream_power_deposit_n: graph"),
        (one, (g2, g2, f2, f2, soil.d8, ok, 1.0, 2.0), {}, "stream_power_deposit_n: height"),
        (one, (None, g2, f2, f2, soil.d8, ok, 1.0, 2.0), {}, "stream_power_deposit_n: height is required"),
        (one, (f2, g2, None, f2, soil.d8, ok, 1.0, 2.0), {}, "stream_power_deposit_n: erosivity is required"),
        (one, (f2, g2, f2, None, soil.d8, ok, 1.0, 2.0), {}, "stream_power_deposit_n: deposition is required"),
        (one, (f2, g2, f2, f3, soil.d8, ok, 1.0, 2.0), {}, "stream_power_deposit_n: deposition"),
        (one, (f2, g2, f2, f2, "d8", ok, 1.0, 2.0), {}, "stream_power_deposit_n: edge"),
        (one, (f2, g2, f2, f2, soil.d8, None, 1.0, 2.0), {}, "stream_power_deposit_n: scale"),
        (one, (f2, g2, f2, f2, soil.d8, (1.0, 0.0), 1.0, 2.0), {}, "stream_power_deposit_n: scale entries"),
        (one, (f2, g2, f2, f2, soil.d8, ok, -1.0, 2.0), {}, "stream_power_deposit_n: dt"),
        (one, (f2, g2, f2, f2, soil.d8, ok, 1.0, 2.0), dict(uplift=g2), "stream_power_deposit_n: uplift"),
        (one, (f2, g2, f2, f2, soil.d8, ok, 1.0, 2.0), dict(iters=0), "stream_power_deposit_n: iters"),
        (one, (f2, g2, f2, f2, soil.d8, ok, 1.0, 2.0), dict(iters=2.0), "stream_power_deposit_n: iters"),
        (one, (f2, g2, f2, f2, soil.d8, ok, 1.0, 0.5), {}, "stream_power_deposit_n: n must be"),
        (one, (f2, g2, f2, f2, soil.d8, ok, 1.0, float("nan")), {}, "stream_power_deposit_n: n must be"),
        (one, (f2, g2, f2, f2, soil.d8, ok, 1.0, 16.5), {}, "stream_power_deposit_n: n must be"),
        (one, (f2, g2, f2, f2, soil.d8, ok, 1.0, "2"), {}, "stream_power_deposit_n: n must be"),
        (many, (f3, g2, f3, f3, soil.d8, ok, 1.0, 2.0), {}, r"stream_power_deposit_n_batch: graph: expected a \(B, H, W\)"),
        (many, (f3, g3, f3, f2, soil.d8, ok, 1.0, 2.0), {}, "stream_power_deposit_n_batch: deposition"),
        (many, (f3, g3, f3, f3, soil.d8, [[1.0, 1.0]] * 4, 1.0, 2.0), {}, "stream_power_deposit_n_batch: scale"),
        (many, (f3, g3, f3, f3, soil.d8, ok, 1.0, 2.0), dict(iters=-1), "stream_power_deposit_n_batch: iters"),
        (many, (f3, g3, f3, f3, soil.d8, ok, 1.0, 0.5), {}, "stream_power_deposit_n_batch: n must be"),
    ]


def test_the_module_functions_refuse_and_take_numbers_in_range():
    from soillib_amd import _abi, soil
    for fn, args, kw, match in _module_refusals():
        with pytest.raises(ValueError, match=match):
            fn(*args, **kw)
    # past the scalar checks a host tensor is refused at the device check only
    f2, g2 = _host(np.float32, (4, 3)), _host(np.int32, (4, 3))
    for n, iters in ((1, 1), (np.float32(2.5), np.uint8(3)), (16.0, 2)):
        with pytest.raises(_abi.SoilError, match="mismatch_host"):
            soil.stream_power_deposit_n(f2, g2, f2, f2, soil.d8, (1.0, 1.0), 1.0, n, iters=iters)


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


def test_the_batch_methods_refuse_and_evolve_still_refuses_G_with_n():
    step, full = "stream_power_deposit_n", "evolve_deposit"
    cases = [(step, (1.0, 1e-4), dict(n=0.5), r"ErosionBatch\.stream_power_deposit_n: n must be"),
             (step, (1.0, 1e-4), dict(n="2"), r"ErosionBatch\.stream_power_deposit_n: n must be"),
             (step, (1.0, 1e-4), dict(G=-1.0), r"ErosionBatch\.stream_power_deposit_n: G"),
             (step, (1.0, 1e-4), dict(G=float("nan")), r"ErosionBatch\.stream_power_deposit_n: G"),
             (step, (1.0, 1e-4), dict(iters=0), r"ErosionBatch\.stream_power_deposit_n: iters"),
             (step, (1.0, 1e-4), dict(iters=1.5), r"ErosionBatch\.stream_power_deposit_n: iters"),
             (step, (-1.0, 1e-4), {}, r"ErosionBatch\.stream_power_deposit_n: dt"),
             (step, (1.0, 1e-4), dict(kind="direction"), r"ErosionBatch\.stream_power_deposit_n: kind"),
             (full, (1.0, 1e-4, 1.0, 0.5), dict(kappa=0.1), r"ErosionBatch\.evolve_deposit: n must be"),
             (full, (1.0, 1e-4, -1.0, 2.0), dict(kappa=0.1), r"ErosionBatch\.evolve_deposit: G"),
             (full, (1.0, 1e-4, 1.0, 2.0), dict(kappa=0.1, iters=0), r"ErosionBatch\.evolve_deposit: iters"),
             (full, (1.0, 1e-4, 1.0, 2.0), {}, r"ErosionBatch\.evolve_deposit: "),
             (full, (1.0, 1e-4, 1.0, 2.0), dict(kappa=0.1, critical_slope=-1.0), r"ErosionBatch\.evolve_deposit: slope"),
             (full, (1.0, 1e-4, 1.0, 2.0), dict(kappa=0.1, first_axis=2), r"ErosionBatch\.evolve_deposit: "),
             ("evolve", (1.0, 1e-4), dict(kappa=0.1, n=2.0, G=1.0), r"ErosionBatch\.evolve: G \(deposition\) takes the slope exponent n = 1 only"),
             ("evolve_limited", (1.0, 1e-4, 0.5), dict(kappa=0.1, n=2, G=1), r"ErosionBatch\.evolve_limited: G \(deposition\) takes the slope exponent n = 1 only")]
    for method, args, kw, match in cases:
        with pytest.raises(ValueError, match=match):
            getattr(_batch_without_a_device(), method)(*args, **kw)


def test_the_call_order_of_the_batch_methods(monkeypatch):
    """stream_power_deposit_n: conditioned() -> drainage(graph=g) -> erosivity and deposition -> the batch entry with the
    arguments in its order.  evolve_deposit: that step, the collapse where a critical slope is given, the diffusion."""
    from soillib_amd import silt, soil
    from soillib_amd.erosion import ErosionBatch
    calls = []
    log = lambda name, ret: (lambda *a, **k: calls.append((name, a, k)) or ret)
    bt = _batch_without_a_device(B=2)
    monkeypatch.setattr(ErosionBatch, "conditioned", lambda self, *a, **k: calls.append(("conditioned", a, k)) or ("filled", "graph"))
    monkeypatch.setattr(ErosionBatch, "drainage", lambda self, *a, **k: calls.append(("drainage", a, k)) or "area")
    monkeypatch.setattr(soil, "erosivity", log("erosivity", "k"))
    monkeypatch.setattr(soil, "deposition", lambda area, G, cell: calls.append(("deposition", (area, G), {})) or "d")
    monkeypatch.setattr(soil, "stream_power_deposit_n_batch", log("entry", "stepped"))
    monkeypatch.setattr(silt.tensor, "gpu", lambda self: self)
    assert bt.stream_power_deposit_n(2.0, 1e-3, 0.4, 1.5, 2.5, 7, "steepest", soil.d4, None, 0, None, True, True) == "stepped"
    assert calls == [("conditioned", ("steepest", soil.d4, None, 0), {}), ("drainage", (), dict(graph="graph", edge=soil.d4)),
                     ("erosivity", ("area", 1e-3, 0.4), {}), ("deposition", ("area", 1.5), {}),
                     ("entry", ("filled", "graph", "k", "d", soil.d4, [1.0, 1.0], 2.0, 2.5, None, 7, False, True, True), {})]
    del calls[:]
    assert bt.stream_power_deposit_n(2.0, 1e-3) == "stepped"
    assert calls[-1] == ("entry", ("filled", "graph", "k", "d", soil.d8, [1.0, 1.0], 2.0, 2.0, None, soil.DEPOSIT_N_ITERS,
                                   False, False, False), {})
    # evolve_deposit
    monkeypatch.setattr(ErosionBatch, "stream_power_deposit_n", lambda self, *a, **k: calls.append(("step", a, k)) or "carved")
    monkeypatch.setattr(soil, "slope_limit_batch", log("slope_limit_batch", "limited"))
    monkeypatch.setattr(soil, "diffuse_batch", log("diffuse_batch", "out"))
    del calls[:]
    assert bt.evolve_deposit(2.0, 1e-3, 1.5, 2.5, kappa=0.25) == "out"
    assert calls == [("step", (2.0, 1e-3, 0.5, 1.5, 2.5, None, "steepest", None, None, 0, None), {}),
                     ("diffuse_batch", ("carved", [1.0, 1.0], 2.0, 0.25), dict(border="fixed", first_axis=0))]
    del calls[:]
    assert bt.evolve_deposit(2.0, 1e-3, 1.5, 2.5, 0.4, 0.25, 0.7, None, 9, "random_weighted", soil.d4,
                             1.5, 3, 1) == "out"
    assert calls == [("step", (2.0, 1e-3, 0.4, 1.5, 2.5, 9, "random_weighted", soil.d4, 1.5, 3, None), {}),
                     ("slope_limit_batch", ("carved", [1.0, 1.0], 0.7, soil.d4), {}),
                     ("diffuse_batch", ("limited", [1.0, 1.0], 2.0, 0.25), dict(border="fixed", first_axis=1))]
