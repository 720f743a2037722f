"""Exact multiple-flow accumulation (include/soil_hip.h: soil_mfd_weights, soil_mfd_accumulate, their _batch forms,
soil_mfd_info), what can be checked without a GPU: the header, the symbols and the surfaces; every refusal with the
entry's name, through C and through Python; and the numpy restatement of tests/mfd_ref.py — which the GPU tests hold the
kernels to, bit for bit — against a dense fp64 solve, against closed forms, against the oracle's accumulation on
single-receiver terrains, against itself under the kernel's tile schedule, on hostile cells, and against the
Monte-Carlo mean of the reference algorithm (the oracle's random_weighted + accumulate)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import flats_ref
import mfd_ref as ref
from mfd_ref import D4, D8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_HEAD = "float* weights, const float* height, const int32_t* dist, int kind, double param, "
A_HEAD = "float* out, double* out64, const float* height, const float* source, const int32_t* dist, int kind, double param, "
ONE = "int64_t H, int64_t W, const float scale[2], int edge, void* stream"
MANY = "int64_t B, int64_t H, int64_t W, const float* scales, int64_t n_scales, int edge, void* stream"
ENTRIES = {"soil_mfd_weights": W_HEAD + ONE, "soil_mfd_weights_batch": W_HEAD + MANY,
           "soil_mfd_accumulate": A_HEAD + ONE, "soil_mfd_accumulate_batch": A_HEAD + MANY,
           "soil_mfd_info": "int64_t info[4]"}


def _mass_tol(steps, total):
    """How far the terminals' sum of a unit source may lie from the number of cells: a cell's K shares are K roundings of
    at most 2^-25 each, so it passes on its value times 1 +- K 2^-25 <= 1 +- 2^-22, over ways of at most `steps` cells
    (the sweeps the Jacobi iteration took); the fp64 sums add nothing at this scale."""
    return steps * 2.0 ** -22 * total


def _squash(s):
    return re.sub(r"\s+", " ", s).strip()


# ---- the header, the symbols, the surfaces ---------------------------------------------------------------------

def test_the_header_declares_the_entries_and_states_the_definition():
    text = open(os.path.join(ROOT, "include", "soil_hip.h")).read()
    assert text.index("flow graphs: exact multiple-flow accumulation") < text.index("int soil_mfd_weights(") < \
        text.index("- stencils */")
    for name, args in ENTRIES.items():
        m = re.search(r"int %s\((.*?)\);" % name, text, re.S)
        assert m, name
        assert _squash(m.group(1)) == args
    flat = _squash(re.sub(r"\n \* ?", "\n", text))
    for phrase in ("a[n] = source[n] + sum over donors d of w(d -> n) a[d]", "diff = h[n] (-) h[k]",
                   "P_k = rw_exp2(diff, c_k)", "P_k = (float) sp_pow((double)diff / L_k, p)", "soil_selftest_math op 12",
                   "soil_selftest_math64 op 0", "Z = ((P_0 + P_1) + ...) in fp32", "A cell sends iff Z is finite and > 0",
                   "w_k = P_k / Z, one IEEE fp32 division", "the rule of soil_flat_receivers",
                   "strictly lowers the pair (height, dist)", "s = s + a[k] * (double)w", "A zero share is skipped",
                   "canonical quiet NaN", "does not depend on the schedule", "SOIL_MFD_PER_CHECK", "tiles * 272 + 2",
                   "never a property of the input", "planar (K, H, W) float32", "T = 0 makes every cell a terminal"):
        assert phrase in flat, phrase


def test_the_library_binds_the_entries_and_the_build_has_the_source():
    from soillib_amd import _abi, build
    from test_abi_symbols import declared_symbols
    lib = _abi.lib()
    assert set(declared_symbols()) == set(_abi.SIGNATURES), set(declared_symbols()) ^ set(_abi.SIGNATURES)
    for name in ENTRIES:
        assert name in _abi.SIGNATURES and hasattr(lib, name), name
    found = [s for s in build.SOURCES if "int soil_mfd_accumulate(" in open(os.path.join(build.CSRC, s)).read()]
    assert found == ["mfd.hip"]
    source = open(os.path.join(build.CSRC, "mfd.hip")).read()
    assert "WS_MFD" in open(os.path.join(build.CSRC, "common.hpp")).read() and "WS_MFD" in source
    # the weights of random_weighted, the same inline functions; the rounded operations by name; the derived bound
    for piece in ("rw_exp2(", "rw_const(", "rw_temperature_ok(", "sp_pow(", "__fdiv_rn(", "__dmul_rn(", "__dadd_rn(",
                  "The launch bound.", "4 * kMT + kMT * kMT / kMInner"):
        assert piece in source, piece
    graph = open(os.path.join(build.CSRC, "graph.hip")).read()
    assert "inline RwConst rw_const" not in graph and "inline RwConst rw_const" in open(
        os.path.join(build.CSRC, "soil_math.hpp")).read(), "one definition of the constants"


def test_the_call_info_needs_no_device():
    from soillib_amd import _abi, soil
    assert _abi.lib().soil_mfd_info(None) == _abi.SOIL_ERR_INVALID_ARGUMENT
    assert _abi.last_error().startswith("mfd_info: ")
    assert sorted(soil.mfd_info()) == ["launches", "looks", "models", "tiles"]


def test_the_surfaces():
    import soillib
    from soillib_amd import soil
    from soillib_amd.erosion import ErosionBatch
    for name in ("mfd_weights", "mfd_weights_batch", "mfd_accumulate", "mfd_accumulate_batch", "mfd_info"):
        assert callable(getattr(soil, name)) and getattr(soillib, name) is getattr(soil, name), name
    for fn in (soil.mfd_weights, soil.mfd_weights_batch):
        assert list(inspect.signature(fn).parameters) == ["height", "edge_", "T", "p", "scale", "dist"]
    for fn in (soil.mfd_accumulate, soil.mfd_accumulate_batch):
        p = inspect.signature(fn).parameters
        assert list(p) == ["height", "source", "edge_", "T", "p", "scale", "dist", "double"]
        assert p["double"].default is False and p["T"].default is None and p["p"].default is None
    p = inspect.signature(ErosionBatch.drainage_mfd).parameters
    assert list(p) == ["self", "T", "p", "source", "edge", "conditioned"] and p["conditioned"].default is True
    assert "mfd" not in open(os.path.join(ROOT, "include", "soil.hpp")).read(), "nothing new is named in soil.hpp"
    assert "SOIL_MFD_PER_CHECK" in open(os.path.join(ROOT, "docs", "KNOBS.md")).read()


# ---- refusals, without a device --------------------------------------------------------------------------------

def _p(k):
    """A stand-in for a tensor (never read): planes 16 MiB apart, so that none overlaps another."""
    return C.c_void_p(k << 24)


def _entries():
    from soillib_amd import _abi
    lib = _abi.lib()
    sc = (C.c_float * 6)(1, 2, 1, 2, 1, 2)
    base = dict(weights=_p(1), out=_p(1), out64=_p(2), height=_p(3), source=_p(4), dist=_p(5), kind=0, param=10.0, B=3,
                H=4, W=4, scale=sc, ns=3, edge=D8)

    def call(fn, names):
        def go(over=()):
            v = dict(base, **dict(over))
            return fn(*[v[k] for k in names], None)
        return go
    wh, ah = ["weights", "height", "dist", "kind", "param"], ["out", "out64", "height", "source", "dist", "kind", "param"]
    one, many = ["H", "W", "scale", "edge"], ["B", "H", "W", "scale", "ns", "edge"]
    return {"mfd_weights": call(lib.soil_mfd_weights, wh + one), "mfd_weights_batch": call(lib.soil_mfd_weights_batch, wh + many),
            "mfd_accumulate": call(lib.soil_mfd_accumulate, ah + one),
            "mfd_accumulate_batch": call(lib.soil_mfd_accumulate_batch, ah + many)}


def _sc(*v):
    return (C.c_float * 6)(*v)


POWER = dict(kind=1, param=1.1)
SHARED = [("null height", dict(height=None), "null tensor"),
          ("H = 0", dict(H=0), "empty grid"), ("W < 0", dict(W=-2), "empty grid"),
          ("H W > INT32_MAX", dict(H=1 << 16, W=1 << 15), "a model must have 1..2^31-1 cells"),
          ("edge 2", dict(edge=2), "invalid edge enumerator"), ("edge -1", dict(edge=-1), "invalid edge enumerator"),
          ("kind 2", dict(kind=2), "invalid kind enumerator"), ("kind -1", dict(kind=-1), "invalid kind enumerator"),
          ("T < 0", dict(param=-1.0), "T must be 0 or a normal positive float"),
          ("T NaN", dict(param=float("nan")), "T must be 0 or a normal positive float"),
          ("T inf", dict(param=float("inf")), "T must be 0 or a normal positive float"),
          ("T subnormal", dict(param=1e-40), "T must be 0 or a normal positive float"),
          ("p < 0", dict(kind=1, param=-0.5), "p must be a finite number in 0 .. 16"),
          ("p > 16", dict(kind=1, param=16.5), "p must be a finite number in 0 .. 16"),
          ("p NaN", dict(kind=1, param=float("nan")), "p must be a finite number in 0 .. 16"),
          ("p inf", dict(kind=1, param=float("inf")), "p must be a finite number in 0 .. 16"),
          ("power without a scale", dict(POWER, scale=None), "null scale"),
          ("power, scale 0", dict(POWER, scale=_sc(0, 1, 1, 1, 1, 1)), "a scale must be a positive finite float"),
          ("power, scale < 0", dict(POWER, scale=_sc(1, -1, 1, 1, 1, 1)), "a scale must be a positive finite float"),
          ("power, scale inf", dict(POWER, scale=_sc(float("inf"), 1, 1, 1, 1, 1)), "a scale must be a positive finite float"),
          ("power, scale NaN", dict(POWER, scale=_sc(1, float("nan"), 1, 1, 1, 1)), "a scale must be a positive finite float")]
WEIGHTS = [("null weights", dict(weights=None), "null tensor"),
           ("weights are the height", dict(weights=_p(3)), "an output aliases an input plane"),
           ("the height inside the 8 planes of the weights", dict(height=C.c_void_p((1 << 24) + 4 * 8 * 16 - 8)),
            "an output aliases an input plane"),
           ("weights are the dist", dict(weights=_p(5)), "an output aliases an input plane")]
ACCUMULATE = [("both outputs null", dict(out=None, out64=None), "both outputs are null"),
              ("out is the height", dict(out=_p(3)), "an output aliases an input plane"),
              ("out64 is the source", dict(out64=_p(4)), "an output aliases an input plane"),
              ("out inside the dist", dict(out=C.c_void_p((5 << 24) + 16)), "an output aliases an input plane"),
              ("out64 is out", dict(out64=_p(1)), "out and out64 overlap")]
BATCH = [("B = 0", dict(B=0), "B must be >= 1"), ("B < 0", dict(B=-3), "B must be >= 1"),
         ("n_scales 2 of 3", dict(ns=2), "n_scales must be 1 or B"), ("n_scales 0", dict(ns=0), "n_scales must be 1 or B"),
         ("power, a later model's scale 0", dict(POWER, scale=_sc(1, 1, 1, 1, 0, 1)), "a scale must be a positive finite float")]


def _cases(name):
    return SHARED + (WEIGHTS if "weights" in name else ACCUMULATE) + (BATCH if name.endswith("_batch") else [])


def test_every_refusal_names_its_entry_and_its_reason():
    """These come before the device check: the same answers with and without a device."""
    from soillib_amd import _abi
    for name, call in _entries().items():
        for what, over, text in _cases(name):
            assert call(over) == _abi.SOIL_ERR_INVALID_ARGUMENT, (what, name)
            assert _abi.last_error().startswith("%s: %s" % (name, text)), (what, name, _abi.last_error())


def test_a_well_formed_call_gets_as_far_as_the_device_check():
    from soillib_amd import _abi
    if _abi.lib().soil_device_count() > 0:
        pytest.skip("a HIP device is present")
    for name, call in _entries().items():
        for over in (dict(), dict(source=None, dist=None), dict(param=0.0), dict(scale=None, ns=1), dict(POWER),
                     dict(kind=1, param=0.0), dict(kind=1, param=16.0), dict(scale=_sc(0, 0, 0, 0, 0, 0)),
                     dict(out=None), dict(out64=None)):
            assert call(over) == _abi.SOIL_ERR_NO_DEVICE, (name, over, _abi.last_error())


def _host(dtype, shape):
    from soillib_amd import silt
    return silt.tensor._wrap_numpy(np.zeros(shape, dtype))


def test_the_module_refuses_before_any_device_work():
    from soillib_amd import soil
    f2, f3, g2, g3 = _host(np.float32, (4, 3)), _host(np.float32, (5, 4, 3)), _host(np.int32, (4, 3)), _host(np.int32, (5, 4, 3))
    ok = (1.0, 1.0)
    cases = []
    for w, a, h, other, i, io in ((soil.mfd_weights, soil.mfd_accumulate, f2, f3, g2, g3),
                                  (soil.mfd_weights_batch, soil.mfd_accumulate_batch, f3, f2, g3, g2)):
        wn, an = w.__name__, a.__name__
        cases += [(w, (other, D8), dict(T=1.0), wn + ": height: expected a"), (w, (i, D8), dict(T=1.0), wn + ": height: expected a float32"),
                  (w, (h, 3), dict(T=1.0), wn + ": edge must be d4 or d8"), (w, (h, D8), {}, wn + ": exactly one of T and p"),
                  (w, (h, D8), dict(T=1.0, p=1.0), wn + ": exactly one of T and p"),
                  (w, (h, D8), dict(T=-1.0), wn + ": T must be 0 or a normal positive float32"),
                  (w, (h, D8), dict(T=float("nan")), wn + ": T must be a finite number"),
                  (w, (h, D8), dict(T=True), wn + ": T must be a finite number"),
                  (w, (h, D8), dict(p=17, scale=ok), wn + ": p must be a finite number in 0 .. 16"),
                  (w, (h, D8), dict(p=-1, scale=ok), wn + ": p must be a finite number"),
                  (w, (h, D8), dict(p=1.0), wn + ": scale must be one"),
                  (w, (h, D8), dict(p=1.0, scale=(0.0, 1.0)), wn + ": scale entries must be positive"),
                  (w, (h, D8), dict(T=1.0, dist=h), wn + ": dist: expected an int32"),
                  (w, (h, D8), dict(T=1.0, dist=io), wn + ": dist: expected a tensor of shape"),
                  (a, (h, other, D8), dict(T=1.0), an + ": source: expected a tensor of shape"),
                  (a, (h, i, D8), dict(T=1.0), an + ": source: expected a float32"),
                  (a, (h, None, D8), {}, an + ": exactly one of T and p")]
    for fn, args, kw, text in cases:
        with pytest.raises(ValueError, match=re.escape(text)):
            fn(*args, **kw)


def test_drainage_mfd_refuses_and_composes(monkeypatch):
    from soillib_amd import soil
    from soillib_amd.erosion import ErosionBatch
    batch = ErosionBatch.__new__(ErosionBatch)
    batch.B, batch.H, batch.W, batch.scale, batch.scales = 2, 4, 3, [2.0, 3.0, 1.0], None
    batch.height = _host(np.float32, (2, 4, 3))
    for kw, text in ((dict(), "exactly one of T and p"), (dict(T=1.0, p=1.0), "exactly one of T and p"),
                     (dict(T=-1.0), "T must be 0 or a normal positive float32"), (dict(p=17), "p must be a finite number in 0 .. 16"),
                     (dict(T=1.0, edge=5), "edge must be d4 or d8"), (dict(T=1.0, source=_host(np.int32, (2, 4, 3))), "source must be")):
        with pytest.raises(ValueError, match="ErosionBatch.drainage_mfd: " + re.escape(text)):
            batch.drainage_mfd(**kw)
    calls = []
    monkeypatch.setattr(soil, "fill_depressions_batch", lambda h, e: calls.append(("fill", h, e)) or "filled")
    monkeypatch.setattr(soil, "flat_distance_batch", lambda h, e: calls.append(("dist", h, e)) or "dist")
    monkeypatch.setattr(soil, "mfd_accumulate_batch", lambda h, s, e, **kw: calls.append(("mfd", h, s, e, kw)) or "out")
    assert batch.drainage_mfd(T=10.0) == "out"
    assert calls == [("fill", batch.height, D8), ("dist", "filled", D8),
                     ("mfd", "filled", None, D8, dict(T=10.0, p=None, scale=None, dist="dist"))]
    del calls[:]
    assert batch.drainage_mfd(p=1.1, edge=D4, conditioned=False) == "out"
    assert calls == [("mfd", batch.height, None, D4, dict(T=None, p=1.1, scale=[2.0, 3.0], dist=None))]


# ---- the restatement against a dense solve ----------------------------------------------------------------------

@pytest.mark.parametrize("kind", [dict(T=10.0), dict(p=1.1, scale=(1.0, 2.0))], ids=["gibbs", "power"])
@pytest.mark.parametrize("n", [24, 48])
def test_the_restatement_is_the_solution_of_the_triangular_system(n, kind):
    """M = I - W^T is an M-matrix: its inverse is non-negative.  For two approximate solutions x (np.linalg.solve) and a
    (the restatement) with residuals r_x and r_a, M (a - x) = r_x - r_a, so |a - x| <= M^-1 (|r_x| + |r_a|) cell by
    cell.  A residual computed in fp64 is itself off by at most (K + 2) eps (|source| + |M| |v|); that goes into the
    right-hand side.  The bound is then solved for with the same factorisation and doubled for that solve's own error
    (its relative error is far below 1).  The prototype saw 1.4e-15 relative at 48 x 48."""
    w = ref.weights(ref.fractal(n, n), D8, **kind)
    a, sweeps = ref.accumulate(w)
    assert 5 < sweeps < n * n
    M, src = ref.dense(w), np.ones(n * n)
    x = np.linalg.solve(M, src)
    eps = np.finfo(np.float64).eps
    rho = sum(np.abs(src - M @ v) + 10 * eps * (np.abs(src) + np.abs(M) @ np.abs(v)) for v in (x, a.ravel()))
    tol = 2 * np.linalg.solve(M, rho)
    err = np.abs(a.ravel() - x)
    print("greatest error %.3g relative to the greatest value, greatest tolerance %.3g" % (err.max() / x.max(), (tol / x.max()).max()))
    assert (tol >= 0).all() and tol.max() < 1e-11 * x.max(), "the bound itself is tight"
    assert (err <= tol).all(), (err.max(), tol[err.argmax()])
    term = w.sum(0) == 0
    assert abs(a[term].sum() - n * n) < _mass_tol(sweeps, n * n), "the terminals keep what arrived: the sum of a unit source"


# ---- closed forms, and the oracle on single-receiver terrains ----------------------------------------------------

def _singles():
    """name -> (h, dist, edge, kind, closed form or None): terrains on which every sending cell has one receiver."""
    out = {}
    for name, kind in (("ramp T", dict(T=10.0)), ("ramp p", dict(p=1.1, scale=(1.0, 2.0)))):
        out[name] = (ref.ramp(9, 7), None, D4, kind, np.repeat(np.arange(1, 10, dtype=np.float64)[:, None], 7, axis=1))
    h, dist, pos = ref.snake(64, 64)
    out["serpentine"] = (h, dist, D4, dict(T=10.0), pos.astype(np.float64))
    h, dist = ref.staircase(20)
    want = np.ones((20, 20))
    want[np.arange(20), np.arange(20)] = np.arange(1, 21)
    want[18, 19] = 21.0                                               # the last step hands its 20 to the cell above it
    out["staircase"] = (h, dist, D8, dict(T=10.0), want)
    return out


@pytest.mark.parametrize("name", ["ramp T", "ramp p", "serpentine", "staircase"])
def test_closed_forms(name):
    h, dist, edge, kind, want = _singles()[name]
    w = ref.weights(h, edge, dist=dist, **kind)
    assert set(np.unique(w)) <= {0.0, 1.0} and (w.sum(0) <= 1).all(), "one receiver, share exactly 1"
    a, _ = (ref.accumulate_tiled(w)[:1] + (0,)) if name == "serpentine" else ref.accumulate(w)
    ref.same(a, want, name)
    if name.startswith("ramp"):
        assert (a.sum(0) == 45).all(), "integer column sums"


@pytest.mark.parametrize("name", ["ramp T", "serpentine", "staircase"])
def test_single_receiver_terrains_are_the_oracles_accumulation(oracle, name):
    """With one receiver a cell and an integer source every sum is exact in fp32 and fp64 alike: the words of the
    oracle's accumulate along the oracle's steepest graph (its flats routed by the numpy flat_receivers)."""
    h, dist, edge, kind, _ = _singles()[name]
    H, W = h.shape
    source = (1 + np.arange(H * W).reshape(H, W) % 5).astype(np.float32)
    graph = oracle.steepest(h, edge)
    if dist is not None:
        graph = flats_ref.receivers(graph, h, dist, edge)
    want = oracle.accumulate(graph, source, edge)
    w = ref.weights(h, edge, dist=dist, **kind)
    a = ref.accumulate_tiled(w, source)[0] if name == "serpentine" else ref.accumulate(w, source)[0]
    ref.same(a.astype(np.float32), want, name)


# ---- schedule independence ------------------------------------------------------------------------------------

def test_the_tile_schedule_gives_the_bits_of_whole_grid_jacobi():
    h = ref.fractal(130, 70)
    for edge, kind in ((D8, dict(T=10.0)), (D4, dict(p=1.1, scale=(1.0, 1.0)))):
        w = ref.weights(h, edge, **kind)
        a, sweeps = ref.accumulate(w)
        b, launches, runs = ref.accumulate_tiled(w)
        ref.same(b, a, "tiles against Jacobi")
        print("130 x 70: %d global sweeps; %d launches, %d tile runs" % (sweeps, launches, runs))
        assert 2 < launches <= 6 * 272 + 2 and runs <= 6 * launches


def test_the_serpentine_in_one_tile_takes_sixteen_capped_launches():
    h, dist, pos = ref.snake(64, 64)
    a, launches, runs = ref.accumulate_tiled(ref.weights(h, D4, T=10.0, dist=dist))
    assert (a == pos).all() and launches == runs == 4096 // 256 + 1


def test_the_diagonal_wake_up_is_needed():
    """ref.corner_chain under the tile schedule: with the eight-neighbour wake-up the closed form, with four the diagonal
    tile never hears of the pulse."""
    h, dist, src, want = ref.corner_chain()
    w = ref.weights(h, D8, T=10.0, dist=dist)
    got, launches, _ = ref.accumulate_tiled(w, src)
    ref.same(got, want, "corner chain")
    assert launches == 20, "sixteen for the serpentine, one each for the three tiles down the diagonal and beside it, one more"
    assert (ref.accumulate_tiled(w, src, wake=4)[0] != want).sum() >= 65, "the four-neighbour slip loses the diagonal"


# ---- hostile cells -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("edge", [D4, D8])
@pytest.mark.parametrize("kind", [dict(T=10.0), dict(T=1.0), dict(p=0.0, scale=(1.0, 1.0)), dict(p=4.0, scale=(1.0, 3.0))],
                         ids=["T10", "T1", "p0", "p4"])
def test_hostile_cells(edge, kind):
    """NaN heights, +-inf, +-3e38, +-0 plateaus; NaN, +-inf and +-0 sources.  The shares are never NaN, a cell that
    sends gives away 1 up to rounding, a NaN cell and every neighbour of one is a terminal, the iteration settles (the
    shares are a DAG), the tile schedule gives the same words, and a zero share beside an infinite donor is skipped."""
    h, src = ref.hostile(70, 66), ref.hostile_source(70, 66)
    w = ref.weights(h, edge, **kind)
    assert np.isfinite(w).all() and (w >= 0).all() and (w <= 1).all()
    total = w.astype(np.float64).sum(0)
    assert ((total == 0) | (np.abs(total - 1) < 1e-6)).all()
    nan = np.isnan(h)
    beside = np.zeros_like(nan)
    for k in range(ref.k_of(edge)):
        beside |= ref.shifted(nan, k, False)
    assert (total[nan | beside] == 0).all()
    a, _ = ref.accumulate(w, src)
    ref.same(ref.accumulate_tiled(w, src)[0], a, "tiles against Jacobi")
    assert (ref.bits64(a[np.isnan(a)]) == ref.QNAN64).all() and np.isnan(a).any() and np.isinf(a).any()
    lone = (ref.incoming(w) != 0).sum(0) == 0
    ref.same(a[lone & ~np.isnan(src)], src[lone & ~np.isnan(src)].astype(np.float64), "a cell without donors keeps its source")
    assert np.signbit(a[lone & (src == 0) & np.signbit(src)]).all(), "-0 stays -0"


def test_an_infinite_donor_beside_a_zero_share():
    """Three cells in a row, heights 2, 1, 0.5: the middle cell, with an infinite source, sends to the right only; its
    share towards the higher cell on its left is 0.  That cell keeps its finite value: inf * 0 would have made it NaN."""
    src = np.array([[1.0, np.inf, 1.0]], np.float32)
    for kind in (dict(T=1.0), dict(p=1.0, scale=(1.0, 1.0))):
        w = ref.weights(np.array([[2.0, 1.0, 0.5]], np.float32), D4, **kind)
        assert w[2, 0, 0] == 1.0 and w[2, 0, 1] == 1.0 and w[1, 0, 1] == 0.0
        a, _ = ref.accumulate(w, src)
        assert a[0, 0] == 1.0 and a[0, 1] == np.inf and a[0, 2] == np.inf


def test_z_overflow_at_a_small_temperature_is_a_terminal():
    h = ref.fractal(24, 24)
    cold = ref.weights(h, D8, T=1e-3)
    warm = ref.weights(h, D8, T=10.0)
    assert (cold.sum(0) == 0).sum() > (warm.sum(0) == 0).sum(), "drops of more than 88 T overflow Z: terminals"
    assert (ref.weights(h, D8, T=0.0) == 0).all(), "T = 0: every cell a terminal, as random_weighted has it"
    a, sweeps = ref.accumulate(cold)
    assert abs(a[cold.sum(0) == 0].sum() - 24 * 24) < _mass_tol(sweeps, 24 * 24)


@pytest.mark.parametrize("edge", [D4, D8])
def test_dist_routing_on_a_filled_dem_leaves_terminals_on_the_border_or_beside_nan(oracle, edge):
    h = ref.fractal(40, 44, seed=11, amplitude=60.0)
    h[20, 20] = np.nan
    filled = oracle.fill_depressions(h, edge)
    dist = flats_ref.distance_bfs(filled, edge)
    raw = ref.weights(filled, edge, T=10.0)
    w = ref.weights(filled, edge, T=10.0, dist=dist)
    assert ((raw != 0).any(0) <= (w != 0).any(0)).all() and (dist > 0).sum() > 10, "the fill made flats, dist routes them"
    term = ~(w != 0).any(0)
    nan = np.isnan(filled)
    beside = nan.copy()
    for k in range(ref.k_of(edge)):
        beside |= ref.shifted(nan, k, False)
    border = np.zeros_like(term)
    border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
    assert (term <= (border | beside)).all(), np.argwhere(term & ~(border | beside))[:5]
    assert ((raw.sum(0) == 0) & ~(border | beside)).any(), "without dist the filled lakes are terminals"
    a, sweeps = ref.accumulate(w)
    live = ~nan
    assert abs(a[term & live].sum() - live.sum()) < _mass_tol(sweeps, live.sum())


# ---- the statistical link to the reference algorithm ---------------------------------------------------------------

@pytest.mark.parametrize("T", [10.0, 1.0])
def test_the_monte_carlo_mean_of_the_reference_algorithm_lies_around_it(oracle, T):
    """K = 2048 graphs of the oracle's random_weighted (one seed, offsets 0 .. K - 1), each accumulated by the oracle: the
    share of cells whose mean lies more than 6 sample standard errors from the exact accumulation is at most 0.5 %, and
    cells of zero sample variance agree to 1e-6 relative.  Observed on this terrain (profiles/mfd/checks.txt): no cell
    beyond 6; the greatest deviation 4.07 standard errors at T = 10 and 4.54 at T = 1."""
    n, K = 48, 2048
    h = ref.fractal(n, n, seed=7)
    one = np.ones((n, n), np.float32)
    s = np.zeros((n, n))
    ss = np.zeros((n, n))
    for k in range(K):
        a = oracle.accumulate(oracle.random_weighted(h, D8, 1234, k, T), one, D8).astype(np.float64)
        s += a
        ss += a * a
    mean = s / K
    var = np.maximum(ss - K * mean * mean, 0) / (K - 1)
    se = np.sqrt(var / K)
    exact, _ = ref.accumulate(ref.weights(h, D8, T=T))
    still = var == 0
    assert (np.abs(mean[still] - exact[still]) <= 1e-6 * np.abs(exact[still])).all()
    z = np.abs(mean[~still] - exact[~still]) / se[~still]
    print("T = %g: greatest deviation %.2f standard errors, %d of %d cells beyond 6; median relative MC error %.3g" % (
        T, z.max(), (z > 6).sum(), z.size, np.median(np.abs(mean - exact) / exact)))
    assert (z > 6).sum() <= 0.005 * n * n
