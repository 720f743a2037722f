"""Flow routing for batches of models (include/soil_hip.h: "flow graphs: batches of models"), what can be checked
without a GPU: the header's declarations and contract, the exported and bound symbols, the build's sources, the
Python surface and its refusals, and that the entries fail loudly without a device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    "soil_direction_batch": "int32_t* direction, const float* height, int64_t B, int64_t H, int64_t W, int edge, "
                            "void* stream",
    "soil_steepest_batch": "int32_t* graph, const float* height, int64_t B, int64_t H, int64_t W, int edge, "
                           "void* stream",
    "soil_random_weighted_batch": "int32_t* graph, const float* height, int64_t B, int64_t H, int64_t W, int edge, "
                                  "const uint64_t* seeds, uint64_t offset, float T, void* stream",
    "soil_slope_batch": "float* slope, const float* tensor, const int32_t* flow, int64_t B, int64_t H, int64_t W, "
                        "const float* scales, int64_t n_scales, void* stream",
    "soil_accumulate_batch": "float* out, const int32_t* graph, const float* source, const float* decay, int64_t B, "
                             "int64_t H, int64_t W, int edge, void* stream",
}
SINGLE = {"soil_direction_batch": "soil_direction", "soil_steepest_batch": "soil_steepest",
          "soil_random_weighted_batch": "soil_random_weighted", "soil_slope_batch": "soil_slope",
          "soil_accumulate_batch": "soil_accumulate"}


def _header():
    return open(os.path.join(ROOT, "include", "soil_hip.h")).read()


def _section():
    """The header from the new heading to the next one."""
    text = _header()
    m = re.search(r"/\* -+ flow graphs: batches of models \*/(.*?)/\* -{20,} [a-zA-Z]", text, re.S)
    assert m, "the heading 'flow graphs: batches of models' is missing from include/soil_hip.h"
    return m.group(1)


def _squash(s):
    return re.sub(r"\s+", " ", s).strip()


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_the_header_declares_the_entry_under_the_new_heading(name):
    section = _section()
    m = re.search(r"int %s\((.*?)\);" % name, section, re.S)
    assert m, "%s is not declared under the heading" % name
    assert _squash(m.group(1)) == ENTRIES[name]
    # each entry cites its single-grid counterpart in the comment in front of it
    before = section[:m.start()]
    comment = before[before.rindex("/*"):]
    assert re.search(r"\b%s\b" % SINGLE[name], comment), "%s does not cite %s" % (name, SINGLE[name])


def test_the_header_states_the_contract():
    text = _squash(re.sub(r"\n \* ?", "\n", _section()))
    for phrase in ("model-major", "model b of a plane starts at element b * H * W", "bit for bit",
                   "index WITHIN its own model", "handed to soil_accumulate",
                   "a neighbour off a model's edge does not exist", "is no edge",
                   "2 * (ceil(log2(H*W) / 2) + 1)", "not those of the stacked size",
                   "stream-ordered and do not synchronise", "soil_accumulate keeps its synchronisation",
                   "SOIL_ERR_INVALID_ARGUMENT", "SOIL_ERR_NO_DEVICE", "SOIL_FLOW_BATCH_CELLS",
                   "Results do not depend on the chunking"):
        assert phrase in text, phrase


def test_the_library_exports_and_binds_the_entries():
    from soillib_amd import _abi
    lib = _abi.lib()
    i64, vp, cint = C.c_int64, C.c_void_p, C.c_int
    want = {
        "soil_direction_batch": [vp, vp, i64, i64, i64, cint, vp],
        "soil_steepest_batch": [vp, vp, i64, i64, i64, cint, vp],
        "soil_random_weighted_batch": [vp, vp, i64, i64, i64, cint, C.POINTER(C.c_uint64), C.c_uint64, C.c_float, vp],
        "soil_slope_batch": [vp, vp, vp, i64, i64, i64, C.POINTER(C.c_float), i64, vp],
        "soil_accumulate_batch": [vp, vp, vp, vp, i64, i64, i64, cint, vp],
    }
    for name, args in want.items():
        assert hasattr(lib, name), name
        res, bound = _abi.SIGNATURES[name]
        assert res is cint and bound == args, name
        assert getattr(lib, name).argtypes == args


def test_the_kernels_are_in_a_built_source():
    from soillib_amd import build
    found = [src for src in build.SOURCES
             if "soil_accumulate_batch(" in open(os.path.join(build.CSRC, src)).read()]
    assert len(found) == 1, found
    text = open(os.path.join(build.CSRC, found[0])).read()
    for name in ENTRIES:
        assert re.search(r"^int %s\(" % name, text, re.M), name


def test_the_cpp_header_has_the_wrappers():
    text = open(os.path.join(ROOT, "include", "soil.hpp")).read()
    for name in ENTRIES:
        assert re.search(r"inline [^;{]*\b%s\(" % name[len("soil_"):], text), name
        assert name + "(" in text


def test_the_python_surface():
    import soillib
    from soillib_amd import soil
    from soillib_amd.erosion import ErosionBatch, ErosionModel
    for name in ("direction_batch", "steepest_batch", "random_weighted_batch", "slope_batch", "accumulate_batch"):
        assert callable(getattr(soil, name)) and getattr(soillib, name) is getattr(soil, name)
    for name in ("flow", "drainage", "flow_slope"):
        assert callable(getattr(ErosionBatch, name)), name
        assert not hasattr(ErosionModel, name), name


def test_the_knob_is_documented():
    assert "SOIL_FLOW_BATCH_CELLS" in open(os.path.join(ROOT, "docs", "KNOBS.md")).read()


# ---- refusals in Python: before any device work, on a batch without planes ----

class _Untouchable:
    """Stands for a plane the refusals must never reach."""

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


def _host_tensor(dtype, shape):
    import numpy as np
    from soillib_amd import silt
    return silt.tensor._wrap_numpy(np.zeros(shape, dtype))


FLOW = [dict(kind="steepest8"), dict(kind=None), dict(kind=1),
        dict(kind="random_weighted"), dict(kind="random_weighted", T=None),
        dict(kind="random_weighted", T=float("nan")),
        dict(kind="random_weighted", T=float("inf")), dict(kind="random_weighted", T="10"),
        dict(kind="random_weighted", T=True),
        dict(kind="random_weighted", T=10.0, offset=-1),
        dict(kind="random_weighted", T=10.0, offset=0.5),
        dict(edge=2), dict(edge="d8"), dict(kind="direction", edge=-1)]


@pytest.mark.parametrize("kw", FLOW)
def test_flow_refuses(kw):
    with pytest.raises(ValueError, match=r"ErosionBatch\.flow"):
        _batch_without_a_device().flow(**kw)


def _batch_refusals():
    """(method, the stub's scales, args, kw, match) of drainage() and flow_slope()."""
    import numpy as np
    good_g, good_f = _host_tensor(np.int32, (5, 4, 3)), _host_tensor(np.float32, (5, 4, 3))
    bad = [dict(graph=_host_tensor(np.int32, (4, 4, 3))), dict(graph=_host_tensor(np.int32, (5, 12))),
           dict(graph=_host_tensor(np.float32, (5, 4, 3))), dict(graph=np.zeros((5, 4, 3), np.int32)),
           dict(graph=good_g, source=_host_tensor(np.float32, (5, 4, 4))),
           dict(graph=good_g, source=_host_tensor(np.int32, (5, 4, 3))),
           dict(graph=good_g, source=good_f, decay=_host_tensor(np.float32, (5, 3, 4))),
           dict(graph=good_g, source=good_f, decay=1.0),
           dict(graph=good_g, source=good_f, edge=7)]
    out = [("drainage", None, (), kw, r"ErosionBatch\.drainage") for kw in bad]
    for graph in (_host_tensor(np.int32, (5, 3, 4)), _host_tensor(np.float32, (5, 4, 3)), 3):
        out.append(("flow_slope", None, (graph,), {}, r"ErosionBatch\.flow_slope"))
    for scales in ([[1.0, 1.0, 1.0]] * 4, [[1.0, 1.0, 1.0]] * 6, [[1.0, 1.0]] * 5, [[1.0, 1.0, "z"]] * 5):
        out.append(("flow_slope", scales, (good_g,), {}, r"ErosionBatch\.flow_slope"))
    return out


def _refuses(which):
    cases = [c for c in _batch_refusals() if c[0] == which]
    assert cases
    for method, scales, args, kw, match in cases:
        with pytest.raises(ValueError, match=match):
            getattr(_batch_without_a_device(scales=scales), method)(*args, **kw)


def test_drainage_refuses():
    _refuses("drainage")


def test_flow_slope_refuses():
    _refuses("flow_slope")


def _module_refusals():
    import numpy as np
    from soillib_amd import soil
    h = _host_tensor(np.float32, (5, 4, 3))
    g = _host_tensor(np.int32, (5, 4, 3))
    out = [(soil.random_weighted_batch, (h, soil.d8, [1, 2, 3, 4], 0, 10.0), {}, "random_weighted_batch: 4 seeds for 5 models")]
    for scale in ([1.0], [1.0, 1.0, 1.0], [[1.0, 1.0]] * 4, [[1.0, 1.0, 1.0]] * 5, 1.0, [["a", "b"]] * 5):
        out.append((soil.slope_batch, (h, g, scale), {}, "slope_batch"))
    out += [(soil.slope_batch, (h, _host_tensor(np.int32, (5, 3, 4)), [1.0, 1.0]), {}, "slope_batch: flow"),
            (soil.accumulate_batch, (g, _host_tensor(np.float32, (4, 4, 3)), soil.d8), {}, "accumulate_batch: field"),
            (soil.accumulate_batch, (g, h, soil.d8), dict(decay=_host_tensor(np.float32, (5, 4))), "accumulate_batch: decay")]
    for fn in (soil.steepest_batch, soil.direction_batch):
        out.append((fn, (_host_tensor(np.float32, (4, 3)), soil.d8), {}, r"\(B, H, W\)"))
    return out


def test_the_module_functions_refuse_wrong_counts_before_any_device_work():
    for fn, args, kw, match in _module_refusals():
        with pytest.raises(ValueError, match=match):
            fn(*args, **kw)


def test_the_entry_points_fail_loudly_without_a_device():
    from soillib_amd import _abi
    lib = _abi.lib()
    if lib.soil_device_count() > 0:
        pytest.skip("a HIP device is present")
    seeds = (C.c_uint64 * 2)(1, 2)
    scales = (C.c_float * 4)(1, 1, 1, 1)
    assert lib.soil_direction_batch(None, None, 2, 8, 8, _abi.D8, None) == _abi.SOIL_ERR_NO_DEVICE
    assert lib.soil_steepest_batch(None, None, 2, 8, 8, _abi.D8, None) == _abi.SOIL_ERR_NO_DEVICE
    assert lib.soil_random_weighted_batch(None, None, 2, 8, 8, _abi.D8, seeds, 0, 10.0, None) == _abi.SOIL_ERR_NO_DEVICE
    assert lib.soil_slope_batch(None, None, None, 2, 8, 8, scales, 2, None) == _abi.SOIL_ERR_NO_DEVICE
    assert lib.soil_accumulate_batch(None, None, None, None, 2, 8, 8, _abi.D8, None) == _abi.SOIL_ERR_NO_DEVICE


# ---- the temperature of random_weighted: refused before anything else, device or none (soil_hip.h) ----

def _with_temperature(lib, T):
    """(name, return code, last error) of the three entries that take a temperature, on null tensors."""
    seeds = (C.c_uint64 * 2)(1, 2)
    calls = {"soil_random_weighted": lambda: lib.soil_random_weighted(None, None, 8, 8, 1, 0, 0, T, None),
             "soil_random_weighted_batch": lambda: lib.soil_random_weighted_batch(None, None, 2, 8, 8, 1, seeds, 0, T, None),
             "soil_multiflow": lambda: lib.soil_multiflow(None, None, None, 8, 8, 1, 0, 0, 1, 2, 2, T, None)}
    return [(name, call(), lib.soil_last_error().decode()) for name, call in calls.items()]


REFUSED_T = [-1.0, -1e-30, float("nan"), float("inf"), float("-inf"), 1e-39, -1e-45, 1e39]


@pytest.mark.parametrize("T", REFUSED_T)
def test_a_temperature_outside_the_range_is_refused(T):
    from soillib_amd import _abi, soil
    assert not soil.valid_temperature(T)
    for name, rc, msg in _with_temperature(_abi.lib(), T):
        assert rc == _abi.SOIL_ERR_INVALID_ARGUMENT, (name, rc)
        assert msg == "%s: T must be 0 or a normal positive float" % name[len("soil_"):], msg
    with pytest.raises(ValueError, match=r"ErosionBatch\.flow: T must be|ErosionBatch\.flow: kind 'random_weighted' needs"):
        _batch_without_a_device().flow(kind="random_weighted", T=T)


@pytest.mark.parametrize("T", [0.0, -0.0, 2.0 ** -126, 10.0, 3.4028234663852886e38])
def test_a_temperature_inside_the_range_passes_the_check(T):
    from soillib_amd import _abi, soil
    assert soil.valid_temperature(T)
    for name, rc, msg in _with_temperature(_abi.lib(), T):
        assert rc in (_abi.SOIL_ERR_NO_DEVICE, _abi.SOIL_ERR_INVALID_ARGUMENT), (name, rc)     # no device, or the null tensors
        assert "T must be" not in msg, msg


def test_the_header_states_the_temperature_rule():
    text = _squash(re.sub(r"\n \* ?", "\n", _header()))
    for phrase in ("T must be 0 or a normal positive float", "-1 in every cell",
                   "with or without a device", "soil_random_weighted_batch and soil_multiflow alike"):
        assert phrase in text, phrase
