"""The C ABI of the order statistics (include/soil_hip.h, "erosion: summaries": soil_erode_batch_quantiles,
soil_erode_batch_exceedance) is declared, exported and bound, the contract is stated where the ABI is, and ErosionBatch
has `quantiles`, `order_statistics`, `median` and `exceedance`, which refuse bad arguments before any device work (no
compute call succeeds here: this runs without a GPU; what the entries compute and refuse is in
test_gpu_erosion_quantiles.py)."""
import ctypes as C
import inspect
import os
import re

import pytest

from test_abi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUANTILES, EXCEEDANCE = "soil_erode_batch_quantiles", "soil_erode_batch_exceedance"


def _header():
    return open(os.path.join(ROOT, "include", "soil_hip.h")).read()


def _declared_args(entry):
    """The argument list of `entry` as the header declares it, comments and line breaks removed."""
    m = re.search(r"int %s\((.*?)\);" % entry, _header(), re.S)
    assert m, "no declaration of " + entry
    text = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [" ".join(a.split()) for a in text.split(",")]


def test_header_declares_both_entry_points():
    assert QUANTILES in declared_symbols() and EXCEEDANCE in declared_symbols()
    assert _declared_args(QUANTILES) == ["const soil_erosion_planes* planes", "int64_t B", "int64_t H", "int64_t W",
                                         "const double* pos", "int nq", "float* out", "void* stream"]
    assert _declared_args(EXCEEDANCE) == ["const soil_erosion_planes* planes", "int64_t B", "int64_t H", "int64_t W",
                                          "const float thresholds[SOIL_ENSEMBLE_CHANNELS]", "float* out",
                                          "void* stream"]
    text = _header()
    assert re.search(r"#define SOIL_QUANTILES_MAX 16\b", text)
    # both live under the summaries' heading
    assert text.index("erosion: summaries") < text.index("int " + QUANTILES) < text.index("int " + EXCEEDANCE)


def test_header_states_the_order_and_the_interpolation():
    text = " ".join(_header().split())
    assert "0x7FC00000" in text
    assert "key = (u >> 31) ? ~u : u | 0x80000000" in text
    assert "compared unsigned" in text
    assert "-inf < ... < -denormal < -0 < +0 < +denormal < ... < +inf < NaN" in text
    assert "lo = floor(pos)" in text and "frac = pos - lo" in text
    assert "(float)((double)a + frac * ((double)b - (double)a))" in text
    assert "frac == 0 or a == b" in text
    assert "-inf next to a finite value" in text       # the two cases the arithmetic decides
    assert "spoils only" in text
    assert "(float)((double)c / (double)B)" in text    # the exceedance
    assert "SOIL_QUANTILE_PATH" in text


def test_library_exports_and_binds_the_entry_points():
    from soillib_amd import _abi
    lib = _abi.lib()
    for entry in (QUANTILES, EXCEEDANCE):
        assert hasattr(lib, entry)
        assert entry in _abi.SIGNATURES
        restype, args = _abi.SIGNATURES[entry]
        assert restype is C.c_int
        assert args[0] is C.POINTER(_abi.ErosionPlanes)
        assert all(a is C.c_int64 for a in args[1:4])
    assert _abi.SIGNATURES[QUANTILES][1][4:] == [C.POINTER(C.c_double), C.c_int, C.c_void_p, C.c_void_p]
    assert _abi.SIGNATURES[EXCEEDANCE][1][4:] == [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    assert set(declared_symbols()) == set(_abi.SIGNATURES)
    assert _abi.SOIL_QUANTILES_MAX == 16
    assert lib.soil_abi_version() == 1


def test_the_source_is_part_of_the_build():
    from soillib_amd import build
    assert "erosion_quantiles.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "erosion_quantiles.hip"))


@pytest.mark.parametrize("name,params,entry", [
    ("quantiles", ["self", "q"], QUANTILES),
    ("order_statistics", ["self", "ranks"], QUANTILES),
    ("median", ["self"], QUANTILES),
    ("exceedance", ["self", "thresholds"], EXCEEDANCE)])
def test_the_batch_has_the_methods(name, params, entry):
    from soillib_amd import erosion
    method = getattr(erosion.ErosionBatch, name)
    assert list(inspect.signature(method).parameters) == params
    assert entry in method.__doc__
    assert not hasattr(erosion.ErosionModel, name)   # on the batch only


def _batch_without_a_device(B=5):
    """An ErosionBatch with its sizes and no planes: the validation comes before any device work, so a refusal never
    reaches them."""
    from soillib_amd.erosion import ErosionBatch
    bt = ErosionBatch.__new__(ErosionBatch)
    bt.B, bt.H, bt.W = B, 4, 3
    return bt


@pytest.mark.parametrize("q", [[], (), float("nan"), [0.5, float("nan")], -0.01, 1.0000001, [0.0, 2], float("inf"),
                               "0.5", [None], None, [[0.5]], True])
def test_quantiles_refuses(q):
    with pytest.raises(ValueError, match="ErosionBatch.quantiles"):
        _batch_without_a_device().quantiles(q)


@pytest.mark.parametrize("ranks", [[], 1.0, [0, 1.5], [0.0], -1, 5, [0, 4, 5], float("nan"), "1", [None], None, True])
def test_order_statistics_refuses(ranks):
    with pytest.raises(ValueError, match="ErosionBatch.order_statistics"):
        _batch_without_a_device(5).order_statistics(ranks)


@pytest.mark.parametrize("thresholds", [[], [0.0] * 5, [0.0] * 7, 1.0, None, [0, 0, 0, 0, 0, "x"], [0, 0, 0, 0, 0, None]])
def test_exceedance_refuses(thresholds):
    with pytest.raises(ValueError, match="ErosionBatch.exceedance"):
        _batch_without_a_device().exceedance(thresholds)


def test_the_entry_points_fail_loudly_without_a_device():
    from soillib_amd import _abi
    lib = _abi.lib()
    if lib.soil_device_count() > 0:
        pytest.skip("a HIP device is present")
    planes = _abi.ErosionPlanes()
    pos = (C.c_double * 1)(0.0)
    thresholds = (C.c_float * 6)()
    assert lib.soil_erode_batch_quantiles(C.byref(planes), 2, 8, 8, pos, 1, None, None) == _abi.SOIL_ERR_NO_DEVICE
    assert lib.soil_erode_batch_exceedance(C.byref(planes), 2, 8, 8, thresholds, None, None) == _abi.SOIL_ERR_NO_DEVICE
