"""The fill of a batch (include/soil_hip.h: soil_fill_depressions_batch, soil_fill_depressions_info), what can be
checked without a GPU: the symbols and the surfaces, the refusals with the entry's name in the message, the Python
wrappers' refusals before any library call, the numpy restatement of the fill (tests/fill_ref.py) against the
priority-flood oracle, and that the DEMs of the GPU tests (tests/test_gpu_fill_batch.py) are worth filling."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fill_ref as ref
import flats_ref
from fill_ref import D4, D8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    "soil_fill_depressions_batch": "float* out, const float* height, int64_t B, int64_t H, int64_t W, int edge, "
                                   "void* stream",
    "soil_fill_depressions_info": "int64_t info[16]",
}


def _squash(s):
    return re.sub(r"\s+", " ", s).strip()


# ---- the header, the symbols, the surfaces ---------------------------------------------------------------------

def test_the_header_declares_both_entries():
    text = open(os.path.join(ROOT, "include", "soil_hip.h")).read()
    for name, args in ENTRIES.items():
        m = re.search(r"int %s\((.*?)\);" % name, text, re.S)
        assert m, name
        assert _squash(m.group(1)) == args
    assert "WS_CONDITIONING" in text, "the header says which workspace slot the batch uses"


def test_the_library_exports_them_and_the_table_holds_them():
    from soillib_amd import _abi, build
    lib = _abi.lib()
    i64, vp, cint = C.c_int64, C.c_void_p, C.c_int
    assert _abi.SIGNATURES["soil_fill_depressions_batch"] == (cint, [vp, vp, i64, i64, i64, cint, vp])
    assert _abi.SIGNATURES["soil_fill_depressions_info"] == (cint, [C.POINTER(i64)])
    for name in ENTRIES:
        assert hasattr(lib, name), name
    found = [s for s in build.SOURCES if "int soil_fill_depressions_batch(" in open(os.path.join(build.CSRC, s)).read()]
    assert found == ["conditioning.hip"]


def test_the_call_info_is_sixteen_zeros_before_a_call_and_needs_no_device():
    """The record is the calling host thread's: asked from a thread that has made no call yet, whatever other tests
    of this process did before."""
    import threading
    from soillib_amd import _abi, soil
    seen = {}

    def fresh_thread():
        info = (C.c_int64 * 16)(*([7] * 16))
        seen["rc"] = _abi.lib().soil_fill_depressions_info(info)
        seen["info"] = list(info)
        seen["dict"] = soil.fill_info()
    t = threading.Thread(target=fresh_thread)
    t.start()
    t.join()
    assert seen["rc"] == _abi.SOIL_OK and seen["info"] == [0] * 16
    assert seen["dict"] == dict(launches=0, levels=0, models=0, looks=0, per_level=[])
    assert _abi.lib().soil_fill_depressions_info(None) == _abi.SOIL_ERR_INVALID_ARGUMENT
    assert _abi.last_error().startswith("fill_depressions_info: ")


def test_the_surfaces():
    import soillib
    from soillib_amd import soil
    from soillib_amd.erosion import ErosionBatch
    for name in ("fill_depressions_batch", "fill_info", "condition", "condition_batch"):
        assert callable(getattr(soil, name)) and getattr(soillib, name) is getattr(soil, name), name
    text = open(os.path.join(ROOT, "include", "soil.hpp")).read()
    assert re.search(r"inline [^;{]*\bfill_depressions_batch\(", text) and "soil_fill_depressions_batch(" in text
    assert callable(ErosionBatch.filled) and callable(ErosionBatch.conditioned)
    for graph_user in ("drainage(graph=g)", "basins(graph=g)", "flow_length(graph=g)"):
        assert graph_user in ErosionBatch.conditioned.__doc__, graph_user


# ---- refusals, without a device --------------------------------------------------------------------------------

def _refused():
    p, q = C.c_void_p(4096), C.c_void_p(8192)
    big = 1 << 16
    return [("null out", (None, p, 3, 4, 4, D8)), ("null height", (p, None, 3, 4, 4, D8)), ("out == height", (p, p, 3, 4, 4, D8)),
            ("B = 0", (p, q, 0, 4, 4, D8)), ("B < 0", (p, q, -2, 4, 4, D8)), ("H = 0", (p, q, 3, 0, 4, D8)),
            ("H < 0", (p, q, 3, -1, 4, D4)), ("W = 0", (p, q, 3, 4, 0, D8)), ("W < 0", (p, q, 3, 4, -5, D4)),
            ("H W > INT32_MAX", (p, q, 1, big, big // 2, D8)), ("edge 2", (p, q, 3, 4, 4, 2)), ("edge -1", (p, q, 3, 4, 4, -1))]


def test_every_refusal_names_the_entry():
    from soillib_amd import _abi
    call = _abi.lib().soil_fill_depressions_batch
    for what, args in _refused():
        assert call(*args, None) == _abi.SOIL_ERR_INVALID_ARGUMENT, what
        assert _abi.last_error().startswith("fill_depressions_batch: "), (what, _abi.last_error())
    info = (C.c_int64 * 16)()
    assert _abi.lib().soil_fill_depressions_info(info) == _abi.SOIL_OK
    if _abi.lib().soil_device_count() == 0:
        assert list(info) == [0] * 16, "a refused call is no call"


def test_a_well_formed_call_fails_loudly_without_a_device():
    from soillib_amd import _abi
    lib = _abi.lib()
    if lib.soil_device_count() > 0:
        pytest.skip("a HIP device is present")
    p, q = C.c_void_p(4096), C.c_void_p(8192)
    assert lib.soil_fill_depressions_batch(p, q, 3, 4, 4, D8, None) == _abi.SOIL_ERR_NO_DEVICE
    assert lib.soil_fill_depressions_batch(p, q, 1, (1 << 16) - 1, 1 << 15, D4, None) == _abi.SOIL_ERR_NO_DEVICE


# ---- the Python wrappers refuse before any library call ---------------------------------------------------------

def _host(dtype, shape):
    from soillib_amd import silt
    return silt.tensor._wrap_numpy(np.zeros(shape, dtype))


@pytest.fixture
def no_library(monkeypatch):
    """Any call into the library from here on is a failure of the test."""
    from soillib_amd import _abi

    def refuse():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_abi, "lib", refuse)


def _module_refusals():
    from soillib_amd import soil
    h2, h3, g2, g3 = _host(np.float32, (4, 3)), _host(np.float32, (5, 4, 3)), _host(np.int32, (4, 3)), _host(np.int32, (5, 4, 3))
    return [
        (soil.fill_depressions_batch, (h2,), r"fill_depressions_batch: height: expected a \(B, H, W\)"),
        (soil.fill_depressions_batch, (g3,), "fill_depressions_batch: height: expected a float32"),
        (soil.fill_depressions_batch, (_host(np.float64, (5, 4, 3)), soil.d4), "fill_depressions_batch: height: expected a float32"),
        (soil.fill_depressions_batch, (h3, 2), "fill_depressions_batch: edge"),
        (soil.fill_depressions_batch, (np.zeros((5, 4, 3), np.float32),), "fill_depressions_batch: height"),
        (soil.condition, (h3,), r"condition: height: expected a \(H, W\)"),
        (soil.condition, (g2,), "condition: height: expected a float32"),
        (soil.condition, (h2, True), "condition: edge"),
        (soil.condition_batch, (h2,), r"condition_batch: height: expected a \(B, H, W\)"),
        (soil.condition_batch, (g3,), "condition_batch: height: expected a float32"),
        (soil.condition_batch, (h3, soil.d8, h3), "condition_batch: graph: expected an int32"),
        (soil.condition_batch, (h3, soil.d8, _host(np.int32, (5, 4, 4))), "condition_batch: graph"),
    ]


def test_the_module_functions_refuse(no_library):
    for fn, args, match in _module_refusals():
        with pytest.raises(ValueError, match=match):
            fn(*args)


def _stub():
    from soillib_amd.erosion import ErosionBatch
    bt = ErosionBatch.__new__(ErosionBatch)
    bt.B, bt.H, bt.W, bt.seeds = 3, 8, 8, [1, 2, 3]
    return bt


CONDITIONED = [(dict(kind="direction"), "not indices"), (dict(kind="flow"), "kind must be"), (dict(kind=None), "kind must be"),
               (dict(edge=2), "edge must be"), (dict(edge=True), "edge must be"),
               (dict(kind="random_weighted"), "needs a finite temperature"), (dict(kind="random_weighted", T=float("nan")), "finite"),
               (dict(kind="random_weighted", T=-1.0), "T must be 0 or a normal positive"),
               (dict(kind="random_weighted", T=1e-42), "T must be 0 or a normal positive"),
               (dict(kind="random_weighted", T=True), "finite temperature"),
               (dict(kind="random_weighted", T=0.5, offset=-1), "offset"), (dict(kind="random_weighted", T=0.5, offset=1.5), "offset")]


def test_the_batch_methods_refuse(no_library):
    """On a stub: an ErosionBatch cannot be made without a device, and the refusals touch none of its planes."""
    bt = _stub()
    for kwargs, match in CONDITIONED:
        with pytest.raises(ValueError, match="ErosionBatch.conditioned: .*%s" % match):
            bt.conditioned(**kwargs)
        if "kind" in kwargs and kwargs["kind"] == "random_weighted":       # exactly as flow() checks them
            with pytest.raises(ValueError, match="ErosionBatch.flow: .*%s" % match):
                bt.flow(**kwargs)
    with pytest.raises(ValueError, match="ErosionBatch.filled: edge"):
        bt.filled(edge=7)


# ---- the restatement against the oracle -------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", [(63, 65), (65, 129)])
@pytest.mark.parametrize("edge", [D4, D8])
def test_the_restatement_equals_the_oracle(oracle, H, W, edge):
    cases = flats_ref.constructions(H, W) + [("serpentine", flats_ref.serpentine(H, W)),
                                             ("all nan", np.full((H, W), np.nan, np.float32)),
                                             ("all inf", np.full((H, W), np.inf, np.float32))]
    cases += [("pitted %d" % s, ref.pitted(H, W, s)) for s in (0, 1, 2)]
    for name, dem in cases:
        assert ref.has_negative_zero(dem) == (name == "signed zeros"), name
        ref.compare(ref.fill(dem, edge), oracle.fill_depressions(dem, edge), dem, "%s at %dx%d edge %d" % (name, H, W, edge))


@pytest.mark.parametrize("edge", [D4, D8])
def test_the_restatement_on_two_levels_and_on_degenerate_shapes(oracle, edge):
    for dem in [ref.pitted(130, 130, 0)] + [ref.small(H, W, s) for H, W in ((1, 1), (1, 200), (3, 3)) for s in range(3)]:
        ref.compare(ref.fill(dem, edge), oracle.fill_depressions(dem, edge), dem, str(dem.shape))


def test_the_restatement_by_hand():
    z = np.float32([[5, 5, 5, 5], [5, 1, 2, 5], [5, 5, 3, 5], [5, 5, 4, 9]])
    want4 = np.float32([[5, 5, 5, 5], [5, 4, 4, 5], [5, 5, 4, 5], [5, 5, 4, 9]])       # out along 2, 3, 4: the lake stands at 4
    assert (ref.fill(z, D4) == want4).all() and (ref.fill(z, D8) == want4).all()
    z = np.float32([[9, 9, 9], [9, 1, 9], [2, 9, 9]])                    # the pit leaves through the corner under D8 only
    assert ref.fill(z, D4)[1, 1] == 9 and ref.fill(z, D8)[1, 1] == 2
    z[0, 1] = np.nan                                                   # a NaN cell is an outlet and stays NaN
    w = ref.fill(z, D4)
    assert w[1, 1] == 1 and np.isnan(w[0, 1])


# ---- the DEMs of the GPU tests are worth filling ----------------------------------------------------------------

@pytest.mark.parametrize("H,W,seed", ref.PITTED_USED)
def test_the_fill_raises_a_fair_share_of_every_pitted_model(oracle, H, W, seed):
    """A test on surfaces the fill leaves alone, or drowns whole, shows nothing."""
    dem = ref.used(H, W, seed)
    assert not ref.has_negative_zero(dem) and np.isfinite(dem).all()
    for edge in (D4, D8):
        share = ref.raised_share(dem, oracle.fill_depressions(dem, edge))
        print("%dx%d seed %d edge %d: %.3f raised" % (H, W, seed, edge, share))
        assert 0.2 < share < 0.6, (H, W, seed, edge, share)
