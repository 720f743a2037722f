"""Hillslope diffusion (include/soil_hip.h: "hillslope diffusion"; soil_diffuse, soil_diffuse_batch), what can be
checked without a GPU: the two numpy restatements of tests/diffuse_ref.py against each other and against the
properties of the scheme, hand-computed cases that pin the definition, the header, the bound symbols and the
surfaces, every refusal of the two entries with the entry's name in the message, SOIL_ERR_NO_DEVICE for a well-formed
call, and the ValueErrors of the Python layer.

The bounds.  solve_sweeps and solve_dense solve the same diagonally dominant M-matrix systems (condition number at
most 1 + 4 w) by two backward-stable algorithms in fp64: their fp64 results differ by a relative 1e-11 at the very
most for w <= 1e4, five orders below a float32's half ulp, so their float32 results differ by at most 1 ulp (the two
fp64 values may lie on the two sides of a rounding boundary).  Conservation with border = 0: every column of a
sweep's matrix sums to 1 exactly in exact arithmetic; the bound (H + W) (1 + w) 2^-52 sum|h| is a loose backward-error
bound for the two solves."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import diffuse_ref as dref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (13, 21), (64, 65)]
WS = [1e-3, 0.3, 7.0, 1e4]
SCALE = (0.3, 0.7)


def _dt(w):
    """dt that makes kappa dt / s^2 == w (to rounding) along axis 0 with kappa = 1 and SCALE: the larger of the two."""
    return w * float(np.float32(SCALE[0])) ** 2


def _heights(H, W, seed=0):
    return (np.random.default_rng([seed, H, W]).standard_normal((H, W)) * 100.0).astype(np.float32)


def _mixed(H, W, seed=1):
    """Heights with void cells, a diffusivity plane, uplift and a fixed mask."""
    r = np.random.default_rng([seed, H, W])
    h = _heights(H, W, seed)
    h[r.random((H, W)) < 0.1] = np.nan
    k = r.uniform(0.1, 2.0, (H, W)).astype(np.float32)
    u = r.uniform(0.0, 0.5, (H, W)).astype(np.float32)
    fixed = (r.random((H, W)) < 0.1).astype(np.int32)
    return h, k, u, fixed


# ---- (i) against (ii), and the scheme's properties ---------------------------------------------------------------

@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("border", [0, 1])
def test_the_two_restatements_agree(H, W, border):
    h = _heights(H, W)
    hm, k, u, fixed = _mixed(H, W)
    for w in WS:
        for axis in (0, 1):
            a, b = dref.solve_sweeps(h, SCALE, _dt(w), kappa=1.0, border=border, first_axis=axis), \
                dref.solve_dense(h, SCALE, _dt(w), kappa=1.0, border=border, first_axis=axis)
            d = dref.ulps32(a[0], b[0])
            assert d.max() <= 1, "%dx%d w %g border %d axis %d: %d ulps" % (H, W, w, border, axis, d.max())
            a = dref.solve_sweeps(hm, SCALE, _dt(w), diffusivity=k, uplift=u, fixed=fixed, border=border, first_axis=axis)
            b = dref.solve_dense(hm, SCALE, _dt(w), diffusivity=k, uplift=u, fixed=fixed, border=border, first_axis=axis)
            assert (np.isnan(a[0]) == np.isnan(hm)).all() and (np.isnan(b[0]) == np.isnan(hm)).all()
            ok = ~np.isnan(hm)
            d = dref.ulps32(a[0][ok], b[0][ok]) if ok.any() else np.zeros(1, np.int64)
            assert d.max() <= 1, "%dx%d w %g border %d axis %d, every plane: %d ulps" % (H, W, w, border, axis, d.max())
            assert a[0].dtype == np.float32 and a[1].dtype == np.float64


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("border", [0, 1])
def test_the_maximum_principle(H, W, border):
    hm, k, _, fixed = _mixed(H, W, 2)
    for h, kw in ((_heights(H, W, 2), dict(kappa=1.0)), (hm, dict(diffusivity=k, fixed=fixed))):
        if np.isnan(h).all():
            continue
        lo, hi = np.nanmin(h), np.nanmax(h)
        for w in WS:
            for solve in (dref.solve_sweeps, dref.solve_dense):
                out, out64 = solve(h, SCALE, _dt(w), border=border, **kw)
                ok = ~np.isnan(h)
                assert (out[ok] >= lo).all() and (out[ok] <= hi).all(), (H, W, w, border, solve.__name__)
                if solve is dref.solve_sweeps:
                    assert (out64[ok] >= np.float64(lo)).all() and (out64[ok] <= np.float64(hi)).all(), "in fp64 too"


@pytest.mark.parametrize("H,W", SHAPES)
def test_the_sum_is_conserved_without_fixed_cells(H, W):
    h = _heights(H, W, 3)
    total, mass = math.fsum(h.astype(np.float64).reshape(-1)), math.fsum(np.abs(h.astype(np.float64)).reshape(-1))
    for w in WS:
        for axis in (0, 1):
            out64 = dref.solve_sweeps(h, SCALE, _dt(w), kappa=1.0, border=0, first_axis=axis)[1]
            bound = (H + W) * (1.0 + w) * 2.0 ** -52 * mass
            drift = abs(math.fsum(out64.reshape(-1)) - total)
            assert drift <= bound, "%dx%d w %g axis %d: the sum moved by %g, bound %g" % (H, W, w, axis, drift, bound)


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("border", [0, 1])
def test_fixed_cells_keep_their_bits_and_void_cells_are_nan(H, W, border):
    h, k, u, fixed = _mixed(H, W, 4)
    void, free = dref.kinds(h, fixed, border)
    for w in WS:
        out, out64 = dref.solve_sweeps(h, SCALE, _dt(w), diffusivity=k, uplift=u, fixed=fixed, border=border)
        held = ~void & ~free
        assert (dref.words(out[held]) == dref.words(h[held])).all() and (out64[held] == h[held].astype(np.float64)).all()
        assert (dref.words(out[void]) == dref.NAN32).all() and (dref.words(out64[void]) == dref.NAN64).all()
        assert not np.isnan(out[~void]).any() and not np.isnan(out64[~void]).any()


def test_a_wall_of_void_cells_separates_two_regions():
    H, W = 13, 21
    h = _heights(H, W, 5)
    h[:, 9] = np.nan                                                 # a wall from edge to edge
    h[6, 3] = np.nan
    other = h.copy()
    other[:, 10:] = _heights(H, W, 6)[:, 10:] * 3.0                  # the right side changes
    other[2, 15] = np.nan
    for w in (0.3, 1e4, 1e9):
        for axis in (0, 1):
            a = dref.solve_sweeps(h, SCALE, _dt(w), kappa=1.0, border=0, first_axis=axis)
            b = dref.solve_sweeps(other, SCALE, _dt(w), kappa=1.0, border=0, first_axis=axis)
            assert (dref.words(a[1][:, :9]) == dref.words(b[1][:, :9])).all(), "not one bit of the left side moved"
            assert (dref.words(a[1][:, 10:]) != dref.words(b[1][:, 10:])).any()


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("border", [0, 1])
def test_the_transpose_identity(H, W, border):
    h, k, u, fixed = _mixed(H, W, 7)
    t = lambda p: np.ascontiguousarray(p.T)
    for w in (0.3, 1e4, 1e9):
        a = dref.solve_sweeps(h, SCALE, _dt(w), diffusivity=k, uplift=u, fixed=fixed, border=border, first_axis=0)
        b = dref.solve_sweeps(t(h), SCALE[::-1], _dt(w), diffusivity=t(k), uplift=t(u), fixed=t(fixed), border=border, first_axis=1)
        dref.same_words([t(p) for p in b], a, "%dx%d w %g border %d" % (H, W, w, border))


@pytest.mark.parametrize("H,W", SHAPES)
def test_trivial_steps(H, W):
    h = _heights(H, W, 8)
    k = np.zeros((H, W), np.float32)
    for border in (0, 1):
        for kw in (dict(dt=0.0, kappa=3.0), dict(dt=5.0, kappa=0.0), dict(dt=5.0, diffusivity=k)):
            out, out64 = dref.solve_sweeps(h, SCALE, border=border, **kw)
            dref.same_words((out, out64), (h, h.astype(np.float64)), "%r border %d" % (sorted(kw), border))
        flat = np.full((H, W), np.float32(123.456), np.float32)
        for w in WS:
            out, out64 = dref.solve_sweeps(flat, SCALE, _dt(w), kappa=1.0, border=border)
            # the constant solves every sweep's system exactly; the fp64 solve is off by the relative 1e-11 at most of
            # the module's docstring, and a float32 value is the nearest float32 of everything that close to it
            assert (out == flat).all() and np.abs(out64 / np.float64(flat[0, 0]) - 1.0).max() <= 1e-11


# ---- hand-computed cases pin (i) and (ii) ------------------------------------------------------------------------

def test_a_line_of_three_by_hand():
    # 1 x 3, the middle cell fixed, w = 1 along the row: x0 = (3 + 9) / 2, x2 = (0 + 9) / 2
    h = np.array([[3.0, 9.0, 0.0]], np.float32)
    fixed = np.array([[0, 1, 0]], np.int32)
    for solve in (dref.solve_sweeps, dref.solve_dense):
        for axis in (0, 1):
            out, out64 = solve(h, (5.0, 1.0), 1.0, kappa=1.0, fixed=fixed, border=0, first_axis=axis)
            assert out64.tolist() == [[6.0, 9.0, 4.5]] and out.tolist() == [[6.0, 9.0, 4.5]], solve.__name__
    # all three free, w = 1: the recurrence written out
    out, out64 = dref.solve_sweeps(np.array([[0.0, 1.0, 6.0]], np.float32), (5.0, 1.0), 1.0, kappa=1.0, border=0)
    g0, e0 = 1.0 / 2.0, 0.0 / 2.0
    den1 = 3.0 - 1.0 * g0
    e1, g1 = (1.0 + 1.0 * e0) / den1, 1.0 / den1
    den2 = 2.0 - 1.0 * g1
    x2 = (6.0 + 1.0 * e1) / den2
    x1 = e1 + g1 * x2
    x0 = e0 + g0 * x1
    assert out64.tolist() == [[x0, x1, x2]] and np.abs(out64 - [[1.0, 2.0, 4.0]]).max() < 1e-14
    # border = 1 on a grid one cell high: every cell lies on the outermost row and stays
    out, out64 = dref.solve_sweeps(h, (5.0, 1.0), 1.0, kappa=1.0, border=1)
    assert (out == h).all()
    # uplift lifts free cells only, and dt u enters before the solve
    out, out64 = dref.solve_sweeps(h, (5.0, 1.0), 1.0, kappa=0.0, uplift=np.full((1, 3), 0.25, np.float32), fixed=fixed, border=0)
    assert out64.tolist() == [[3.25, 9.0, 0.25]]


def test_a_grid_of_two_by_two_by_hand():
    # w = 1 along both axes: a pair (a, b) becomes ((2a + b) / 3, (a + 2b) / 3); columns first, then rows
    h = np.array([[3.0, 6.0], [0.0, 3.0]], np.float32)
    for solve in (dref.solve_sweeps, dref.solve_dense):
        out, out64 = solve(h, (1.0, 1.0), 1.0, kappa=1.0, border=0)
        assert np.abs(out64 - [[3.0, 4.0], [2.0, 3.0]]).max() < 1e-14, solve.__name__
    out, out64 = dref.solve_sweeps(h, (1.0, 1.0), 1.0, kappa=1.0, border=0)
    assert out64.tolist() == [[3.0, 4.0], [2.0, 3.0]], "every intermediate is exact here"
    # anisotropic: sx = 2 makes w = 1/4 along axis 0; kappa = 4 with (2, 1) is w = (1, 4)
    a = dref.solve_sweeps(h, (2.0, 1.0), 1.0, kappa=4.0, border=0)[1]
    cols = np.array([[(2.0 * 3 + 0) / 3, (2.0 * 6 + 3) / 3], [(3 + 0.0) / 3, (6 + 2.0 * 3) / 3]])
    rows = np.array([[(5 * cols[0, 0] + 4 * cols[0, 1]) / 9, (4 * cols[0, 0] + 5 * cols[0, 1]) / 9],
                     [(5 * cols[1, 0] + 4 * cols[1, 1]) / 9, (4 * cols[1, 0] + 5 * cols[1, 1]) / 9]])
    assert np.abs(a - rows).max() < 1e-14
    assert dref.solve_sweeps(h, (1.0, 1.0), 1.0, kappa=1.0, border=1)[1].tolist() == h.tolist(), "2 x 2 is all border"


def test_the_batch_helper_solves_model_by_model():
    hs = np.stack([_heights(5, 6, i) for i in range(3)])
    scales = [(1.0, 1.0), (0.25, 3.0), (2.0, 0.5)]
    got = dref.solve_batch(dref.solve_sweeps, hs, scales, 2.0, kappa=0.5)
    for i in range(3):
        dref.same_words([g[i] for g in got], dref.solve_sweeps(hs[i], scales[i], 2.0, kappa=0.5), "model %d" % i)


# ---- the header, the symbols, the surfaces -----------------------------------------------------------------------

ENTRIES = {
    "soil_diffuse": "float* out, double* out64, const float* height, const float* diffusivity, const float* uplift, "
                    "const int32_t* fixed, int64_t H, int64_t W, const float scale[2], double kappa, double dt, "
                    "int border, int first_axis, void* stream",
    "soil_diffuse_batch": "float* out, double* out64, const float* height, const float* diffusivity, const float* uplift, "
                          "const int32_t* fixed, int64_t B, int64_t H, int64_t W, const float* scales, int64_t n_scales, "
                          "double kappa, double dt, int border, int first_axis, void* stream",
    "soil_diffuse_info": "int64_t info[4]",
}


def _squash(s):
    return re.sub(r"\s+", " ", s).strip()


def test_the_header_declares_the_entries_and_states_the_contract():
    text = open(os.path.join(ROOT, "include", "soil_hip.h")).read()
    assert "hillslope diffusion */" in text
    for name, args in ENTRIES.items():
        m = re.search(r"int %s\((.*?)\);" % name, text, re.S)
        assert m, name
        assert _squash(m.group(1)) == args
    flat = _squash(re.sub(r"\n \* ?", "\n", text))
    for phrase in ("locally one-dimensional backward Euler", "NOT Peaceman-Rachford", "positivity is worth more than second order",
                   "maximum principle", "w = (kf * dt) / ss", "kf = 0.5 * ((double)k[i] + (double)k[i+1])",
                   "b_i = (1.0 + p_i) + q_i", "den = b_i - p_i * g_{i-1}", "e_i = (d_i + p_i * e_{i-1}) / den",
                   "g_i = q_i / den", "x_i = e_i + g_i * x_{i+1}", "never multiplied by zero",
                   "(double)height[n] + dt * (double)uplift[n]", "0x7fc00000 / 0x7ff8000000000000",
                   "one definite bit pattern", "SOIL_FLOW_BATCH_CELLS", "do not synchronise", "16 bytes a cell"):
        assert phrase in flat, phrase


def test_the_library_binds_the_entries_and_the_build_has_the_source():
    from soillib_amd import _abi, build
    lib = _abi.lib()
    i64, vp, cint, fp, dbl = C.c_int64, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_double
    assert _abi.SIGNATURES["soil_diffuse"] == (cint, [vp] * 6 + [i64, i64, fp, dbl, dbl, cint, cint, vp])
    assert _abi.SIGNATURES["soil_diffuse_batch"] == (cint, [vp] * 6 + [i64, i64, i64, fp, i64, dbl, dbl, cint, cint, vp])
    assert _abi.SIGNATURES["soil_diffuse_info"] == (cint, [C.POINTER(i64)])
    for name in ENTRIES:
        assert hasattr(lib, name), name
    found = [s for s in build.SOURCES if "int soil_diffuse(" in open(os.path.join(build.CSRC, s)).read()]
    assert found == ["diffuse.hip"]
    assert "WS_DIFFUSE" in open(os.path.join(build.CSRC, "common.hpp")).read()
    assert lib.soil_abi_version() == 1


def test_the_surfaces():
    import soillib
    from soillib_amd import soil
    from soillib_amd.erosion import ErosionBatch, ErosionModel
    for name in ("diffuse", "diffuse_batch", "diffuse_info"):
        assert callable(getattr(soil, name)) and getattr(soillib, name) is getattr(soil, name), name
    for name in ("diffuse", "evolve"):
        assert callable(getattr(ErosionBatch, name)) and not hasattr(ErosionModel, name), name
    assert "soil_diffuse" not in open(os.path.join(ROOT, "include", "soil.hpp")).read(), "no C++ wrapper in this change"


def test_the_call_info_needs_no_device_and_is_zero_before_a_call():
    import threading
    from soillib_amd import _abi, soil
    assert _abi.lib().soil_diffuse_info(None) == _abi.SOIL_ERR_INVALID_ARGUMENT
    assert _abi.last_error().startswith("diffuse_info: ")
    seen = {}

    def fresh():                                                     # the record is per host thread: a new one has made no call
        seen.update(soil.diffuse_info())
    t = threading.Thread(target=fresh)
    t.start()
    t.join()
    assert seen == dict(launches=0, chunks=0, idx64_chunks=0, scratch_bytes=0)


# ---- refusals of the two entries, without a device ---------------------------------------------------------------

def _p(k):
    """A stand-in for a tensor (never read): planes a MiB apart, so that none overlaps another."""
    return C.c_void_p(k << 20)


def _entries():
    """name -> call(over), `over` a dict of the arguments to replace in a well-formed call of (B, H, W) = (3, 4, 4)."""
    from soillib_amd import _abi
    lib = _abi.lib()
    sc = (C.c_float * 6)(1, 2, 1, 2, 1, 2)
    base = dict(out=_p(1), out64=_p(2), height=_p(4), diffusivity=_p(5), uplift=_p(6), fixed=_p(7), B=3, H=4, W=4,
                scale=sc, n=3, kappa=0.5, dt=1.5, border=1, axis=0)

    def call(fn, names):
        def go(over=()):
            v = dict(base, **dict(over))
            return fn(*[v[k] for k in names], None)
        return go
    head = ["out", "out64", "height", "diffusivity", "uplift", "fixed"]
    tail = ["kappa", "dt", "border", "axis"]
    return {"diffuse": call(lib.soil_diffuse, head + ["H", "W", "scale"] + tail),
            "diffuse_batch": call(lib.soil_diffuse_batch, head + ["B", "H", "W", "scale", "n"] + tail)}


def _bad_scale(*v):
    return (C.c_float * 6)(*v)


COMMON = [("null height", dict(height=None)), ("both outputs null", dict(out=None, out64=None)),
          ("out is the height", dict(out=_p(4))), ("out64 is the diffusivity", dict(out64=_p(5))),
          ("out inside the uplift", dict(out=C.c_void_p((6 << 20) + 16))), ("out64 is the fixed mask", dict(out64=_p(7))),
          ("out overlaps out64", dict(out=C.c_void_p((2 << 20) + 8))), ("null scale", dict(scale=None)),
          ("H = 0", dict(H=0)), ("W = 0", dict(W=0)), ("W < 0", dict(W=-2)), ("H W > INT32_MAX", dict(H=1 << 16, W=1 << 15)),
          ("scale 0", dict(scale=_bad_scale(0, 1, 1, 1, 1, 1))), ("scale < 0", dict(scale=_bad_scale(1, -1, 1, 1, 1, 1))),
          ("scale inf", dict(scale=_bad_scale(float("inf"), 1, 1, 1, 1, 1))),
          ("scale NaN", dict(scale=_bad_scale(1, float("nan"), 1, 1, 1, 1))),
          ("dt < 0", dict(dt=-1e-9)), ("dt inf", dict(dt=float("inf"))), ("dt NaN", dict(dt=float("nan"))),
          ("kappa < 0 without a plane", dict(kappa=-1e-9, diffusivity=None)),
          ("kappa inf without a plane", dict(kappa=float("inf"), diffusivity=None)),
          ("kappa NaN without a plane", dict(kappa=float("nan"), diffusivity=None)),
          ("border 2", dict(border=2)), ("border -1", dict(border=-1)), ("first_axis 2", dict(axis=2)),
          ("first_axis -1", dict(axis=-1))]
BATCH = [("B = 0", dict(B=0)), ("B < 0", dict(B=-3)), ("n_scales 2 of 3", dict(n=2)), ("n_scales 0", dict(n=0)),
         ("n_scales 4 of 3", dict(n=4)), ("a later model's scale 0", dict(scale=_bad_scale(1, 1, 1, 1, 0, 1)))]


def _cases(name):
    return COMMON + (BATCH if name.endswith("_batch") else [])


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
        assert call(dict(out=None)) == _abi.SOIL_ERR_NO_DEVICE, name
        assert call(dict(out64=None, dt=0.0, border=0, axis=1)) == _abi.SOIL_ERR_NO_DEVICE, name
        assert call(dict(diffusivity=None, uplift=None, fixed=None, kappa=0.0)) == _abi.SOIL_ERR_NO_DEVICE, name
        assert call(dict(kappa=float("nan"))) == _abi.SOIL_ERR_NO_DEVICE, "%s: with a plane kappa is not read" % name
    assert _entries()["diffuse_batch"](dict(n=1)) == _abi.SOIL_ERR_NO_DEVICE


# ---- the ValueErrors of the Python layer: before any device work -------------------------------------------------

def _host(dtype, shape):
    from soillib_amd import silt
    return silt.tensor._wrap_numpy(np.zeros(shape, dtype))


def _module_refusals():
    from soillib_amd import soil
    g2, g3 = _host(np.int32, (4, 3)), _host(np.int32, (5, 4, 3))
    f2, f3 = _host(np.float32, (4, 3)), _host(np.float32, (5, 4, 3))
    one = (1.0, 1.0)
    return [
        (soil.diffuse, (f3, one, 1.0), dict(kappa=1.0), r"diffuse: height: expected a \(H, W\)"),
        (soil.diffuse, (g2, one, 1.0), dict(kappa=1.0), "diffuse: height: expected a float32"),
        (soil.diffuse, (np.zeros((4, 3), np.float32), one, 1.0), dict(kappa=1.0), "diffuse: height"),
        (soil.diffuse, (f2, one, 1.0), {}, "diffuse: exactly one of kappa and diffusivity"),
        (soil.diffuse, (f2, one, 1.0), dict(kappa=1.0, diffusivity=f2), "diffuse: exactly one of kappa and diffusivity"),
        (soil.diffuse, (f2, one, 1.0), dict(kappa=-1.0), "diffuse: kappa"),
        (soil.diffuse, (f2, one, 1.0), dict(kappa=float("inf")), "diffuse: kappa"),
        (soil.diffuse, (f2, one, 1.0), dict(kappa="1"), "diffuse: kappa"),
        (soil.diffuse, (f2, one, 1.0), dict(kappa=True), "diffuse: kappa"),
        (soil.diffuse, (f2, one, 1.0), dict(diffusivity=g2), "diffuse: diffusivity: expected a float32"),
        (soil.diffuse, (f2, one, 1.0), dict(diffusivity=_host(np.float32, (3, 4))), "diffuse: diffusivity"),
        (soil.diffuse, (f2, one, 1.0), dict(kappa=1.0, uplift=f3), "diffuse: uplift"),
        (soil.diffuse, (f2, one, 1.0), dict(kappa=1.0, fixed=f2), "diffuse: fixed: expected an int32"),
        (soil.diffuse, (f2, None, 1.0), dict(kappa=1.0), "diffuse: scale"),
        (soil.diffuse, (f2, [1.0], 1.0), dict(kappa=1.0), "diffuse: scale"),
        (soil.diffuse, (f2, [[1.0, 1.0]] * 2, 1.0), dict(kappa=1.0), "diffuse: scale"),
        (soil.diffuse, (f2, (1.0, 0.0), 1.0), dict(kappa=1.0), "diffuse: scale entries"),
        (soil.diffuse, (f2, (float("inf"), 1.0), 1.0), dict(kappa=1.0), "diffuse: scale entries"),
        (soil.diffuse, (f2, one, -1.0), dict(kappa=1.0), "diffuse: dt"),
        (soil.diffuse, (f2, one, float("nan")), dict(kappa=1.0), "diffuse: dt"),
        (soil.diffuse, (f2, one, "1"), dict(kappa=1.0), "diffuse: dt"),
        (soil.diffuse, (f2, one, 1.0), dict(kappa=1.0, border="open"), "diffuse: border"),
        (soil.diffuse, (f2, one, 1.0), dict(kappa=1.0, border=1), "diffuse: border"),
        (soil.diffuse, (f2, one, 1.0), dict(kappa=1.0, first_axis=2), "diffuse: first_axis"),
        (soil.diffuse, (f2, one, 1.0), dict(kappa=1.0, first_axis=True), "diffuse: first_axis"),
        (soil.diffuse_batch, (f2, one, 1.0), dict(kappa=1.0), r"diffuse_batch: height: expected a \(B, H, W\)"),
        (soil.diffuse_batch, (f3, [[1.0, 1.0]] * 4, 1.0), dict(kappa=1.0), "diffuse_batch: scale"),
        (soil.diffuse_batch, (f3, [[1.0, 1.0]] * 4 + [[1.0, -2.0]], 1.0), dict(kappa=1.0), "diffuse_batch: scale entries"),
        (soil.diffuse_batch, (f3, one, 1.0), dict(diffusivity=f2), "diffuse_batch: diffusivity"),
        (soil.diffuse_batch, (f3, one, 1.0), dict(kappa=1.0, fixed=g2), "diffuse_batch: fixed"),
        (soil.diffuse_batch, (f3, one, 1.0), {}, "diffuse_batch: exactly one"),
    ]


def test_the_module_functions_refuse():
    for fn, args, kw, match in _module_refusals():
        with pytest.raises(ValueError, match=match):
            fn(*args, **kw)


def test_a_numpy_scalar_is_a_number():
    """kappa and dt as numpy scalars: past the scalar checks, refused at the device check only (the tensors are host
    tensors).  What is no finite number >= 0 is refused with the same text whatever its type."""
    from soillib_amd import _abi, soil
    f2, f3 = _host(np.float32, (4, 3)), _host(np.float32, (5, 4, 3))
    for name, fn, f in (("diffuse", soil.diffuse, f2), ("diffuse_batch", soil.diffuse_batch, f3)):
        for kappa, dt in ((np.float32(0.5), np.float32(1)), (np.int64(1), np.int64(1)), (np.float64(0.5), 1), (0.5, 1.0)):
            with pytest.raises(_abi.SoilError, match="mismatch_host"):
                fn(f, (1.0, 1.0), dt, kappa=kappa)
        for bad in (True, "1", float("nan"), float("inf"), -1.0, np.float32("nan"), np.float32("inf"), np.float32(-1),
                    np.int64(-1), np.bool_(True)):
            with pytest.raises(ValueError) as e:
                fn(f, (1.0, 1.0), bad, kappa=0.5)
            assert str(e.value) == "%s: dt must be a finite number >= 0, got %r" % (name, bad)
            with pytest.raises(ValueError) as e:
                fn(f, (1.0, 1.0), 1.0, kappa=bad)
            assert str(e.value) == "%s: kappa must be a finite number >= 0, got %r" % (name, bad)


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
    mask, plane = _host(np.int32, (5, 4, 3)), _host(np.float32, (5, 4, 3))
    out = []
    for args, kw in (((-1.0,), dict(kappa=1.0)), ((float("nan"),), dict(kappa=1.0)), ((1.0,), {}),
                     ((1.0,), dict(kappa=1.0, diffusivity=plane)), ((1.0,), dict(kappa=-1.0)), ((1.0,), dict(kappa="k")),
                     ((1.0,), dict(diffusivity=mask)), ((1.0,), dict(diffusivity=_host(np.float32, (5, 3, 4)))),
                     ((1.0,), dict(kappa=1.0, uplift=mask)), ((1.0,), dict(kappa=1.0, fixed=plane)),
                     ((1.0,), dict(kappa=1.0, border="closed")), ((1.0,), dict(kappa=1.0, first_axis=3))):
        out.append(("diffuse", None, args, kw, r"ErosionBatch\.diffuse"))
    out.append(("diffuse", [[1.0, 1.0, 1.0]] * 4, (1.0,), dict(kappa=1.0), r"ErosionBatch\.diffuse"))
    for args, kw in (((-1.0, 1e-4), dict(kappa=1.0)), ((1.0, 1e-4), {}), ((1.0, 1e-4), dict(kappa=-2.0)),
                     ((1.0, -1e-4), dict(kappa=1.0)), ((1.0, 1e-4), dict(kappa=1.0, m=float("inf"))),
                     ((1.0, 1e-4), dict(kappa=1.0, kind="direction")), ((1.0, 1e-4), dict(kappa=1.0, edge=2)),
                     ((1.0, 1e-4), dict(kappa=1.0, kind="random_weighted")), ((1.0, 1e-4), dict(kappa=1.0, uplift=mask)),
                     ((1.0, 1e-4), dict(kappa=1.0, first_axis=2))):
        out.append(("evolve", None, args, kw, r"ErosionBatch\.evolve"))
    return out


def test_the_batch_methods_refuse():
    for method, scales, args, kw, match in _batch_refusals():
        with pytest.raises(ValueError, match=match):
            getattr(_batch_without_a_device(scales=scales), method)(*args, **kw)
