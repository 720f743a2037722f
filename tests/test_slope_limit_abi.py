"""Threshold hillslopes (include/soil_hip.h: soil_slope_limit, soil_slope_limit_batch, soil_slope_limit_info), what can
be checked without a GPU: the header, the symbols and the surfaces; every refusal with the entry's name in the message,
through C and through Python; the keyword plumbing of ErosionBatch.slope_limited and evolve_limited with stubs, and that
evolve makes the calls it made before; the two restatements of tests/slope_limit_ref.py against each other on every
input tests/test_gpu_slope_limit.py compares, and against cases computed by hand; and that every compared input is
informative — a terrain on which nothing or everything moves shows little."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import slope_limit_ref as ref
from slope_limit_ref import D4, D8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = "float* out, float* excess, const float* height, const float* slope_plane, double slope, "
ENTRIES = {
    "soil_slope_limit": HEAD + "int64_t H, int64_t W, const float scale[2], int edge, void* stream",
    "soil_slope_limit_batch": HEAD + "int64_t B, int64_t H, int64_t W, const float* scales, int64_t n_scales, int edge, "
                                     "void* stream",
    "soil_slope_limit_info": "int64_t info[4]",
}


def _squash(s):
    return re.sub(r"\s+", " ", s).strip()


def _f32(*v):
    return np.array(v, np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).tolist()


# ---- the header, the symbols, the surfaces ---------------------------------------------------------------------

def test_the_header_declares_the_entries_and_states_the_definition():
    text = open(os.path.join(ROOT, "include", "soil_hip.h")).read()
    assert text.index("flow graphs: conditioning") < text.index("int soil_slope_limit(") < text.index("- stencils */")
    for name, args in ENTRIES.items():
        m = re.search(r"int %s\((.*?)\);" % name, text, re.S)
        assert m, name
        assert _squash(m.group(1)) == args
    flat = _squash(re.sub(r"\n \* ?", "\n", text))
    for phrase in ("w[n] <= w[k] (+) c_k[n]", "c_k[n] = (float)((double)slope[n] * L_k)", "round to nearest, denormals kept",
                   "the slope of the cell being lowered", "w[n] <- cand if cand < w[n]", "in any order of updates",
                   "strict <", "c is never -0", "a NaN height is a void", "no limit at this cell",
                   "+-inf heights go through the arithmetic as they are", "a slope of 0 levels every connected component",
                   "SOIL_SLOPE_LIMIT_PER_CHECK", "+0 where the cell was not lowered", "synchronise the stream",
                   "those of the model that needs most", "never cut into chunks", "tiles * 272 + 2",
                   "with a plane the scalar is not read"):
        assert phrase in flat, phrase


def test_the_library_binds_the_entries_and_the_build_has_the_source():
    from soillib_amd import _abi, build
    lib = _abi.lib()
    i64, vp, cint, fp, dbl = C.c_int64, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_double
    assert _abi.SIGNATURES["soil_slope_limit"] == (cint, [vp, vp, vp, vp, dbl, i64, i64, fp, cint, vp])
    assert _abi.SIGNATURES["soil_slope_limit_batch"] == (cint, [vp, vp, vp, vp, dbl, i64, i64, i64, fp, i64, cint, vp])
    assert _abi.SIGNATURES["soil_slope_limit_info"] == (cint, [C.POINTER(i64)])
    for name in ENTRIES:
        assert hasattr(lib, name), name
    found = [s for s in build.SOURCES if "int soil_slope_limit(" in open(os.path.join(build.CSRC, s)).read()]
    assert found == ["slope_limit.hip"]
    source = open(os.path.join(build.CSRC, found[0])).read()
    common = open(os.path.join(build.CSRC, "common.hpp")).read()
    assert "WS_SLOPE_LIMIT" in common and "WS_SLOPE_LIMIT" in source
    # one kernel template over K, plane and batch; the rounded addition by name; the host helpers
    assert "template <int K, bool PLANE, bool BATCH>" in source and "__fadd_rn(" in source
    for helper in ("check_grid_batch(", "check_scales_positive(", "upload_scale_records(", "overlaps("):
        assert helper in source, helper


def test_the_call_info_needs_no_device():
    from soillib_amd import _abi, soil
    assert _abi.lib().soil_slope_limit_info(None) == _abi.SOIL_ERR_INVALID_ARGUMENT
    assert _abi.last_error().startswith("slope_limit_info: ")
    assert sorted(soil.slope_limit_info()) == ["launches", "looks", "models", "tiles"]


def test_the_surfaces():
    import soillib
    from soillib_amd import soil
    from soillib_amd.erosion import ErosionBatch
    for name in ("slope_limit", "slope_limit_batch", "slope_limit_info"):
        assert callable(getattr(soil, name)) and getattr(soillib, name) is getattr(soil, name), name
    for fn in (soil.slope_limit, soil.slope_limit_batch):
        p = inspect.signature(fn).parameters
        assert list(p) == ["height", "scale", "slope", "edge_", "excess"]
        assert p["edge_"].default is None and p["excess"].default is False
    p = inspect.signature(ErosionBatch.slope_limited).parameters
    assert list(p) == ["self", "slope", "edge", "excess"] and p["edge"].default is None and p["excess"].default is False
    ev = list(inspect.signature(ErosionBatch.evolve).parameters)
    lim = list(inspect.signature(ErosionBatch.evolve_limited).parameters)
    assert lim == ev[:3] + ["critical_slope"] + ev[3:], "evolve's arguments, the critical slope after dt and K"
    assert "removed, not deposited" in ErosionBatch.evolve_limited.__doc__
    assert "slope_limit" not in open(os.path.join(ROOT, "include", "soil.hpp")).read(), "nothing new is named in soil.hpp"
    assert "SOIL_SLOPE_LIMIT_PER_CHECK" in open(os.path.join(ROOT, "docs", "KNOBS.md")).read()


# ---- refusals, without a device --------------------------------------------------------------------------------

def _p(k):
    """A stand-in for a tensor (never read): planes a MiB apart, so that none overlaps another."""
    return C.c_void_p(k << 20)


def _entries():
    """name -> call(over), `over` a dict of the arguments to replace in a well-formed call of (B, H, W) = (3, 4, 4)."""
    from soillib_amd import _abi
    lib = _abi.lib()
    sc = (C.c_float * 6)(1, 2, 1, 2, 1, 2)
    base = dict(out=_p(1), excess=_p(2), height=_p(3), plane=None, slope=0.5, B=3, H=4, W=4, scale=sc, ns=3, edge=D8)
    head = ["out", "excess", "height", "plane", "slope"]

    def call(fn, names):
        def go(over=()):
            v = dict(base, **dict(over))
            return fn(*[v[k] for k in names], None)
        return go
    return {"slope_limit": call(lib.soil_slope_limit, head + ["H", "W", "scale", "edge"]),
            "slope_limit_batch": call(lib.soil_slope_limit_batch, head + ["B", "H", "W", "scale", "ns", "edge"])}


def _bad_scale(*v):
    return (C.c_float * 6)(*v)


REFUSED = [("null out", dict(out=None), "null tensor"), ("null height", dict(height=None), "null tensor"),
           ("null scale", dict(scale=None), "null scale"),
           ("H = 0", dict(H=0), "empty grid"), ("W = 0", dict(W=0), "empty grid"), ("W < 0", dict(W=-2), "empty grid"),
           ("H W > INT32_MAX", dict(H=1 << 16, W=1 << 15), "a model must have 1..2^31-1 cells"),
           ("edge 2", dict(edge=2), "invalid edge enumerator"), ("edge -1", dict(edge=-1), "invalid edge enumerator"),
           ("out is the height", dict(out=_p(3)), "an output aliases an input plane"),
           ("out inside the height", dict(out=C.c_void_p((3 << 20) + 16)), "an output aliases an input plane"),
           ("excess is the height", dict(excess=_p(3)), "an output aliases an input plane"),
           ("out is the slope plane", dict(plane=_p(1)), "an output aliases an input plane"),
           ("excess is the slope plane", dict(plane=_p(2)), "an output aliases an input plane"),
           ("excess is out", dict(excess=_p(1)), "out and excess overlap"),
           ("excess inside out", dict(excess=C.c_void_p((1 << 20) + 8)), "out and excess overlap"),
           ("scale 0", dict(scale=_bad_scale(0, 1, 1, 1, 1, 1)), "a scale must be a positive finite float"),
           ("scale < 0", dict(scale=_bad_scale(1, -1, 1, 1, 1, 1)), "a scale must be a positive finite float"),
           ("scale inf", dict(scale=_bad_scale(float("inf"), 1, 1, 1, 1, 1)), "a scale must be a positive finite float"),
           ("scale NaN", dict(scale=_bad_scale(1, float("nan"), 1, 1, 1, 1)), "a scale must be a positive finite float"),
           ("slope < 0", dict(slope=-1e-9), "slope must be finite and >= 0"),
           ("slope NaN", dict(slope=float("nan")), "slope must be finite and >= 0"),
           ("slope inf", dict(slope=float("inf")), "slope must be finite and >= 0"),
           ("slope -inf", dict(slope=float("-inf")), "slope must be finite and >= 0")]
BATCH = [("B = 0", dict(B=0), "B must be >= 1"), ("B < 0", dict(B=-3), "B must be >= 1"),
         ("n_scales 2 of 3", dict(ns=2), "n_scales must be 1 or B"), ("n_scales 0", dict(ns=0), "n_scales must be 1 or B"),
         ("n_scales 4 of 3", dict(ns=4), "n_scales must be 1 or B"),
         ("a later model's scale 0", dict(scale=_bad_scale(1, 1, 1, 1, 0, 1)), "a scale must be a positive finite float")]


def _cases(name):
    return REFUSED + (BATCH if name.endswith("_batch") else [])


def test_every_refusal_names_its_entry_and_its_reason():
    from soillib_amd import _abi
    for name, call in _entries().items():
        for what, over, text in _cases(name):
            assert call(over) == _abi.SOIL_ERR_INVALID_ARGUMENT, (what, name)
            assert _abi.last_error().startswith("%s: %s" % (name, text)), (what, name, _abi.last_error())


def test_with_a_plane_the_scalar_slope_is_not_read():
    """A well-formed call gets as far as the device check (SOIL_ERR_NO_DEVICE here, or it would touch the stand-in
    pointers): with a slope plane a scalar that would be refused alone is not looked at."""
    from soillib_amd import _abi
    if _abi.lib().soil_device_count() > 0:
        pytest.skip("a HIP device is present")
    for name, call in _entries().items():
        assert call() == _abi.SOIL_ERR_NO_DEVICE, name
        assert call(dict(excess=None, slope=0.0)) == _abi.SOIL_ERR_NO_DEVICE, name
        assert call(dict(slope=-0.0)) == _abi.SOIL_ERR_NO_DEVICE, name
        for bad in (-1.0, float("nan"), float("inf")):
            assert call(dict(plane=_p(4), slope=bad)) == _abi.SOIL_ERR_NO_DEVICE, (name, bad)
            assert call(dict(slope=bad)) == _abi.SOIL_ERR_INVALID_ARGUMENT, (name, bad)


def _host(dtype, shape):
    from soillib_amd import silt
    return silt.tensor._wrap_numpy(np.zeros(shape, dtype))


def _module_refusals():
    from soillib_amd import soil
    f2, f3, g2 = _host(np.float32, (4, 3)), _host(np.float32, (5, 4, 3)), _host(np.int32, (4, 3))
    one, many = soil.slope_limit, soil.slope_limit_batch
    ok = (1.0, 1.0)
    return [
        (one, (f3, ok, 0.5), {}, r"slope_limit: height: expected a \(H, W\)"),
        (one, (g2, ok, 0.5), {}, "slope_limit: height: expected a float32"),
        (one, (f2, ok, 0.5), dict(edge_=2), "slope_limit: edge"),
        (one, (f2, ok, 0.5), dict(edge_="d8"), "slope_limit: edge"),
        (one, (f2, None, 0.5), {}, "slope_limit: scale"),
        (one, (f2, (1.0, 0.0), 0.5), {}, "slope_limit: scale entries"),
        (one, (f2, (1.0, float("inf")), 0.5), {}, "slope_limit: scale entries"),
        (one, (f2, ok, -0.5), {}, "slope_limit: slope must be a finite number >= 0"),
        (one, (f2, ok, float("nan")), {}, "slope_limit: slope must be a finite number >= 0"),
        (one, (f2, ok, float("inf")), {}, "slope_limit: slope must be a finite number >= 0"),
        (one, (f2, ok, "0.5"), {}, "slope_limit: slope must be a finite number >= 0"),
        (one, (f2, ok, True), {}, "slope_limit: slope must be a finite number >= 0"),
        (one, (f2, ok, None), {}, "slope_limit: slope must be a finite number >= 0"),
        (one, (f2, ok, f3), {}, "slope_limit: slope: expected a tensor of shape"),
        (one, (f2, ok, g2), {}, "slope_limit: slope: expected a float32"),
        (many, (f2, ok, 0.5), {}, r"slope_limit_batch: height: expected a \(B, H, W\)"),
        (many, (f3, [[1.0, 1.0]] * 4, 0.5), {}, "slope_limit_batch: scale"),
        (many, (f3, [[1.0, 1.0]] * 4 + [[1.0, -2.0]], 0.5), {}, "slope_limit_batch: scale entries"),
        (many, (f3, ok, -1), {}, "slope_limit_batch: slope must be a finite number >= 0"),
        (many, (f3, ok, f2), {}, "slope_limit_batch: slope: expected a tensor of shape"),
        (many, (f3, ok, 0.5), dict(edge_=True), "slope_limit_batch: edge"),
    ]


def test_the_module_functions_refuse_before_any_device_work():
    from soillib_amd import _abi, soil
    for fn, args, kw, match in _module_refusals():
        with pytest.raises(ValueError, match=match):
            fn(*args, **kw)
    # well-formed arguments on host tensors get as far as the device check, numpy scalars included
    f2, f3 = _host(np.float32, (4, 3)), _host(np.float32, (5, 4, 3))
    for slope in (0, 0.0, -0.0, np.float32(0.5), np.int64(2), f2):
        with pytest.raises(_abi.SoilError, match="mismatch_host"):
            soil.slope_limit(f2, (1.0, 2.0), slope, soil.d4, True)
    with pytest.raises(_abi.SoilError, match="mismatch_host"):
        soil.slope_limit_batch(f3, [[1.0, 2.0]] * 5, f3)


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the refusal came after the planes were touched (%s)" % name)


def _batch_without_a_device(B=5, scales=None):
    from soillib_amd.erosion import ErosionBatch
    bt = ErosionBatch.__new__(ErosionBatch)
    bt.B, bt.H, bt.W = B, 4, 3
    bt.seeds = list(range(B))
    bt.scale, bt.scales = ([1.0, 2.0, 1.0], None) if scales is None else (None, scales)
    bt.height = _Untouchable()
    return bt


def test_the_batch_methods_refuse():
    f3, g3, small = _host(np.float32, (5, 4, 3)), _host(np.int32, (5, 4, 3)), _host(np.float32, (4, 4, 3))
    cases = [("slope_limited", (-1.0,), {}, r"ErosionBatch\.slope_limited: slope must be a finite number >= 0"),
             ("slope_limited", (float("nan"),), {}, r"ErosionBatch\.slope_limited: slope must be"),
             ("slope_limited", (float("inf"),), {}, r"ErosionBatch\.slope_limited: slope must be"),
             ("slope_limited", ("1",), {}, r"ErosionBatch\.slope_limited: slope must be"),
             ("slope_limited", (g3,), {}, r"ErosionBatch\.slope_limited: slope must be a float32 tensor"),
             ("slope_limited", (small,), {}, r"ErosionBatch\.slope_limited: slope must be a float32 tensor"),
             ("slope_limited", (0.5,), dict(edge=3), r"ErosionBatch\.slope_limited: edge"),
             ("evolve_limited", (1.0, 1e-4, -0.5), dict(kappa=0.1), r"ErosionBatch\.evolve_limited: slope must be"),
             ("evolve_limited", (1.0, 1e-4, g3), dict(kappa=0.1), r"ErosionBatch\.evolve_limited: slope must be a float32 tensor"),
             ("evolve_limited", (1.0, 1e-4, 0.5), dict(kappa=0.1, edge=9), r"ErosionBatch\.evolve_limited: edge"),
             ("evolve_limited", (1.0, 1e-4, 0.5), {}, r"ErosionBatch\.evolve_limited: exactly one of kappa and diffusivity"),
             ("evolve_limited", (-1.0, 1e-4, 0.5), dict(kappa=0.1), r"ErosionBatch\.evolve_limited: dt"),
             ("evolve_limited", (1.0, 1e-4, 0.5), dict(kappa=0.1, n=0.5), r"ErosionBatch\.evolve_limited: n must be"),
             ("evolve_limited", (1.0, 1e-4, 0.5), dict(kappa=0.1, n=2.0, G=1.0),
              r"ErosionBatch\.evolve_limited: G \(deposition\) takes the slope exponent n = 1 only"),
             ("evolve_limited", (1.0, 1e-4, 0.5), dict(kappa=0.1, kind="direction"), r"ErosionBatch\.evolve_limited: kind")]
    for method, args, kw, match in cases:
        with pytest.raises(ValueError, match=match):
            getattr(_batch_without_a_device(), method)(*args, **kw)
    bt = _batch_without_a_device(scales=[[1.0, 1.0, 1.0]] * 4)
    with pytest.raises(ValueError, match=r"ErosionBatch\.slope_limited: "):
        bt.slope_limited(0.5)
    assert f3 is not None


def test_slope_limited_and_evolve_limited_route_their_arguments(monkeypatch):
    """slope_limited: slope_limit_batch of the batch's height with its scale(s).  evolve_limited: evolve's first half
    with evolve's arguments, slope_limit_batch of the carved surface, diffuse_batch of the limited one.  evolve: the
    calls it made before this method existed, and no other."""
    from soillib_amd import soil
    from soillib_amd.erosion import ErosionBatch
    calls = []
    monkeypatch.setattr(ErosionBatch, "stream_power", lambda self, *a, **k: calls.append(("stream_power", a, k)) or "carved")
    monkeypatch.setattr(ErosionBatch, "stream_power_deposit",
                        lambda self, *a, **k: calls.append(("stream_power_deposit", a, k)) or "carved")
    monkeypatch.setattr(soil, "slope_limit_batch", lambda *a, **k: calls.append(("slope_limit_batch", a, k)) or "limited")
    monkeypatch.setattr(soil, "diffuse_batch", lambda *a, **k: calls.append(("diffuse_batch", a, k)) or "out")
    bt = _batch_without_a_device()
    bt.height = "height"
    plane = _host(np.float32, (5, 4, 3))
    assert bt.slope_limited(0.5) == "limited" and bt.slope_limited(plane, soil.d4, True) == "limited"
    assert calls == [("slope_limit_batch", ("height", [1.0, 2.0], 0.5, soil.d8, False), {}),
                     ("slope_limit_batch", ("height", [1.0, 2.0], plane, soil.d4, True), {})]
    per = _batch_without_a_device(B=2, scales=[[1.0, 2.0, 1.0], [3.0, 4.0, 1.0]])
    per.height = "height"
    del calls[:]
    per.slope_limited(np.float32(0.25))
    assert calls == [("slope_limit_batch", ("height", [[1.0, 2.0], [3.0, 4.0]], 0.25, soil.d8, False), {})]
    # evolve, without the new method: stream_power and diffuse_batch, nothing between them
    bt.height = _Untouchable()
    for kw in ({}, dict(n=1.0)):
        del calls[:]
        assert bt.evolve(2.0, 1e-3, kappa=0.25, **kw) == "out"
        assert calls == [("stream_power", (2.0, 1e-3, 0.5, "steepest", None, None, 0, None), {}),
                         ("diffuse_batch", ("carved", [1.0, 2.0], 2.0, 0.25), dict(border="fixed", first_axis=0))]
    del calls[:]
    assert bt.evolve(2.0, 1e-3, kappa=0.25, G=1.5, iters=3) == "out"
    assert [c[0] for c in calls] == ["stream_power_deposit", "diffuse_batch"]
    # evolve_limited: the same first half, then the threshold, then the diffusion of the limited surface
    del calls[:]
    assert bt.evolve_limited(2.0, 1e-3, 0.6, kappa=0.25) == "out"
    assert calls == [("stream_power", (2.0, 1e-3, 0.5, "steepest", None, None, 0, None), {}),
                     ("slope_limit_batch", ("carved", [1.0, 2.0], 0.6, soil.d8), {}),
                     ("diffuse_batch", ("limited", [1.0, 2.0], 2.0, 0.25), dict(border="fixed", first_axis=0))]
    del calls[:]
    assert bt.evolve_limited(2.0, 1e-3, plane, 0.4, 0.25, None, "random_weighted", soil.d4, 1.5, 3, 1, None, 5, 2.5) == "out"
    assert calls == [("stream_power", (2.0, 1e-3, 0.4, "random_weighted", soil.d4, 1.5, 3, None, 2.5, 5), {}),
                     ("slope_limit_batch", ("carved", [1.0, 2.0], plane, soil.d4), {}),
                     ("diffuse_batch", ("limited", [1.0, 2.0], 2.0, 0.25), dict(border="fixed", first_axis=1))]
    del calls[:]
    assert bt.evolve_limited(2.0, 1e-3, 0.6, kappa=0.25, G=1.5, iters=3) == "out"
    assert calls[0] == ("stream_power_deposit", (2.0, 1e-3, 0.5, 1.5, 3, "steepest", None, None, 0, None), {})
    assert [c[0] for c in calls] == ["stream_power_deposit", "slope_limit_batch", "diffuse_batch"]


# ---- the two restatements --------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ref.all_keys(), ids=lambda k: "-".join(str(v) for v in k).replace(" ", "_"))
def test_the_two_restatements_agree_on_every_input_of_the_gpu_file(key):
    h, scale, slope, edge = ref.case(key)
    want = ref.reference(key)
    assert ref.same_bits(ref.dijkstra(h, scale, slope, edge), want), key
    with np.errstate(invalid="ignore"):
        assert (want[~np.isnan(h)] <= h[~np.isnan(h)]).all() and (np.isnan(want) == np.isnan(h)).all()
    # a fixed point: one more sweep of either kind moves nothing
    assert ref.same_bits(ref.jacobi(want, scale, slope, edge), want)


def test_the_two_restatements_agree_on_the_batch_inputs():
    hs, scales, slope = ref.pit_batch()
    for b in range(3):
        for edge in (D4, D8):
            for s in (1.0, slope[b]):
                assert ref.same_bits(ref.dijkstra(hs[b], scales[b], s, edge), ref.jacobi(hs[b], scales[b], s, edge)), (b, edge)


# ---- every compared input is informative -----------------------------------------------------------------------

@pytest.mark.parametrize("plane", [False, True])
@pytest.mark.parametrize("edge", [D4, D8])
@pytest.mark.parametrize("shape", ref.TERRAIN_SHAPES)
def test_on_every_terrain_case_between_a_fifth_and_four_fifths_of_the_cells_are_lowered(shape, edge, plane):
    key = ("terrain", shape, edge, plane)
    share = ref.lowered_share(ref.case(key)[0], ref.reference(key))
    print("%r: %.3f of the cells lowered" % (key, share))
    assert 0.2 <= share <= 0.8


@pytest.mark.parametrize("name", sorted(ref.hostile_cases()))
def test_every_hostile_construction_changes_a_cell_and_leaves_one(name):
    h = ref.hostile_cases()[name][0]
    w = ref.reference(("hostile", name))
    with np.errstate(invalid="ignore"):
        lowered, kept = int((w < h).sum()), int((_bits_eq(w, h) & ~np.isnan(h)).sum())
    print("%s: %d lowered, %d kept" % (name, lowered, kept))
    assert lowered >= 1 and kept >= 1


def _bits_eq(a, b):
    return np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)


def test_the_hostile_values_sit_where_the_tiles_meet():
    cases = ref.hostile_cases()
    assert np.isnan(cases["nan"][0][63, 63]) and np.isnan(cases["nan"][0][64, 64]) and np.isnan(cases["nan"][0][0, 64])
    z = cases["zeros"][0]
    assert all(np.signbit(z[s]) and z[s] == 0 for s in ref.SPOTS) and (z == 0).sum() > 1000
    d = cases["denormal"][0]
    tiny = np.finfo(np.float32).tiny
    assert (np.abs(d[d != 0]) < tiny).all() and all(0 < c.max() < tiny for c in ref.steps(*cases["denormal"][2:0:-1], d.shape))
    i = cases["inf"][0]
    assert i[64, 64] == -np.inf and np.isposinf(i).sum() == 4 and (i == np.float32(3e38)).sum() == 3 and (i == np.float32(-3e38)).sum() == 1
    s = cases["slope entries"][2]
    assert np.isnan(s[63, 63]) and s[63, 64] == -1 and np.isposinf(s[64, 63]) and s[64, 64] == 0 and np.signbit(s[64, 30])
    # what a hostile slope entry does: the cell keeps its height
    w = ref.reference(("hostile", "slope entries"))
    h = cases["slope entries"][0]
    for at in ((63, 63), (63, 64), (64, 63), (30, 63)):
        assert w[at] == h[at], at
    assert (w[90:110, 60:70] == h[90:110, 60:70]).all() and (w[10:20, 60:70] == w[10:20, 60:70].min()).all()
    # a scalar slope of 0: every component level at its minimum
    h, w = cases["slope 0"][0], ref.reference(("hostile", "slope 0"))
    left = ~np.isnan(h[:, :64])
    assert (w[:, :64][left] == np.nanmin(h[:, :64])).all()
    assert len(np.unique(w[~np.isnan(w)])) == 2, "the two sides of the wall"


# ---- by hand ---------------------------------------------------------------------------------------------------

def _both(h, scale, slope, edge):
    a, b = ref.jacobi(h, scale, slope, edge), ref.dijkstra(h, scale, slope, edge)
    assert ref.same_bits(a, b)
    return a


@pytest.mark.parametrize("edge", [D4, D8])
def test_a_ramp_a_spike_and_a_pit_behind_a_wall_by_hand(edge):
    # 1 x 5: the steps along a row of cells are column steps, sy; slope 0.25 of sy = 1 is exact
    w = _both(_f32(0, 10, 20, 30, 40).reshape(1, 5), (7.0, 1.0), 0.25, edge)
    assert w.tolist() == [[0.0, 0.25, 0.5, 0.75, 1.0]]
    w = _both(_f32(0, 10, 20, 30, 40).reshape(5, 1), (2.0, 9.0), 0.25, edge)
    assert w.reshape(-1).tolist() == [0.0, 0.5, 1.0, 1.5, 2.0], "down a column of cells: row steps, sx"
    # a ramp that is gentle enough stays as it is, bit for bit
    h = _f32(0, 0.25, 0.5, 0.75).reshape(1, 4)
    assert ref.same_bits(_both(h, (1.0, 1.0), 0.25, edge), h)
    # a spike comes down to its lowest neighbour plus the shortest step
    h = np.zeros((3, 3), np.float32)
    h[1, 1] = 10
    w = _both(h, (1.0, 3.0), 1.0, edge)
    assert w[1, 1] == 1.0 and (np.delete(w.reshape(-1), 4) == 0).all()
    w = _both(h, (4.0, 3.0), 1.0, edge)
    assert w[1, 1] == 3.0
    # a pit in a plateau: a cone, cut by a NaN wall
    h = np.full((3, 7), 10, np.float32)
    h[1, 1] = 0
    h[:, 4] = np.nan
    w = _both(h, (1.0, 1.0), 1.0, edge)
    assert np.isnan(w[:, 4]).all() and (w[:, 5:] == 10).all(), "behind the wall nothing moves"
    if edge == D4:
        assert w[:, :4].tolist() == [[2, 1, 2, 3], [1, 0, 1, 2], [2, 1, 2, 3]]
    else:
        r2 = np.float32(np.sqrt(2.0))
        assert w[:, :4].tolist() == [[r2, 1, r2, np.float32(r2 + np.float32(1))], [1, 0, 1, 2], [r2, 1, r2, np.float32(r2 + np.float32(1))]]
    # the slope that binds an edge is the slope of the cell being lowered
    s = _f32(9, 0.5, 9, 2).reshape(1, 4)
    assert _both(_f32(0, 10, 0, 10).reshape(1, 4), (1.0, 1.0), s, edge).tolist() == [[0, 0.5, 0, 2]]


@pytest.mark.parametrize("edge", [D4, D8])
def test_signed_zeros_a_slope_of_zero_and_hostile_entries_by_hand(edge):
    nz, pz = np.float32(-0.0), np.float32(0.0)
    # a tie keeps the bits the cell has; a cell that is lowered to zero becomes +0, whichever zero lowered it
    w = _both(_f32(nz, pz, 1.0, nz).reshape(1, 4), (1.0, 1.0), 0.0, edge)
    assert _bits(w) == _bits(_f32(nz, pz, pz, nz).reshape(1, 4))
    w = _both(_f32(nz, 1.0).reshape(1, 2), (1.0, 1.0), 0.0, edge)
    assert _bits(w) == _bits(_f32(nz, pz).reshape(1, 2))
    # a scalar slope of -0 is 0; a plane entry of -0 too
    for s in (-0.0, _f32(nz, nz).reshape(1, 2)):
        assert _bits(_both(_f32(nz, 1.0).reshape(1, 2), (1.0, 1.0), s, edge)) == _bits(_f32(nz, pz).reshape(1, 2))
    # x + c = 0 with x = -c: +0 under round to nearest
    assert _bits(_both(_f32(-1.0, 5.0).reshape(1, 2), (1.0, 1.0), 1.0, edge)) == _bits(_f32(-1.0, pz).reshape(1, 2))
    # a slope of 0 levels every component to its minimum
    w = _both(_f32(3, 1, np.nan, 5, 4).reshape(1, 5), (1.0, 1.0), 0.0, edge)
    assert w[0, [0, 1, 3, 4]].tolist() == [1, 1, 4, 4] and np.isnan(w[0, 2])
    # a slope entry that is NaN, negative or +inf: the cell keeps its height and still binds its neighbours
    for bad in (np.nan, -1.0, np.inf, -np.inf):
        s = _f32(1, 1, bad, 1, 0).reshape(1, 5)
        assert _both(_f32(0, 10, 5, 10, 10).reshape(1, 5), (1.0, 1.0), s, edge).tolist() == [[0, 1, 5, 6, 6]], bad
    # +-inf heights go through the arithmetic
    w = _both(_f32(-np.inf, 3, np.nan, 7).reshape(1, 4), (1.0, 1.0), 1.0, edge)
    assert w[0, :2].tolist() == [-np.inf, -np.inf] and np.isnan(w[0, 2]) and w[0, 3] == 7
    assert _both(_f32(np.inf, 2).reshape(1, 2), (1.0, 1.0), 1.0, edge).tolist() == [[3, 2]]
    # beside a -inf cell a cell without a limit keeps its height: -inf + inf is NaN, and NaN lowers nobody
    s = _f32(1, np.nan, 1).reshape(1, 3)
    assert _both(_f32(-np.inf, 3, 9).reshape(1, 3), (1.0, 1.0), s, edge).tolist() == [[-np.inf, 3, 4]]
    # the step is one fp64 product rounded once: 0.1f * 0.7f in fp64, then to fp32 — not the fp32 product
    c = ref.steps(np.float32(0.1), (0.7, 0.7), (1, 1))[0][0, 0]
    assert c == np.float32(np.float64(np.float32(0.1)) * np.float64(np.float32(0.7)))
    # the excess: +0 where nothing moved, the height's NaN on voids
    h = _f32(0, 10, np.nan, nz, np.inf, np.inf).reshape(1, 6)
    w = _f32(0, 0.5, np.nan, nz, np.inf, 4).reshape(1, 6)
    assert _bits(ref.excess(h, w)) == _bits(_f32(pz, 9.5, np.nan, pz, pz, np.inf).reshape(1, 6))
