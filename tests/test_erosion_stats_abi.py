"""The C ABI of the summaries (include/soil_hip.h, "erosion: summaries": soil_erode_batch_stats,
soil_erode_batch_ensemble) is declared, exported and bound, the two record structs have their sizes, and
ErosionModel / ErosionBatch have their `stats` and `ensemble` methods (no compute call succeeds here: this runs
without a GPU; what the entries compute and refuse is in test_gpu_erosion_stats.py)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from test_abi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS, ENSEMBLE = "soil_erode_batch_stats", "soil_erode_batch_ensemble"


def _header():
    return open(os.path.join(ROOT, "include", "soil_hip.h")).read()


def _declared_args(entry):
    """The argument list of `entry` as the header declares it, comments and line breaks removed."""
    m = re.search(r"int %s\((.*?)\);" % entry, _header(), re.S)
    assert m, "no declaration of " + entry
    text = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [" ".join(a.split()) for a in text.split(",")]


def test_header_declares_both_entry_points():
    assert STATS in declared_symbols() and ENSEMBLE in declared_symbols()
    assert _declared_args(STATS) == ["const soil_erosion_planes* planes", "int64_t B", "int64_t H", "int64_t W",
                                     "soil_model_stats* out", "void* stream"]
    assert _declared_args(ENSEMBLE) == ["const soil_erosion_planes* planes", "int64_t B", "int64_t H", "int64_t W",
                                        "float* mean", "float* var", "void* stream"]
    text = _header()
    assert "erosion: summaries" in text   # a heading of its own
    assert re.search(r"#define SOIL_STAT_CHANNELS 10\b", text)
    assert re.search(r"#define SOIL_ENSEMBLE_CHANNELS 6\b", text)
    # the records, field by field in the declared order
    m = re.search(r"typedef struct soil_channel_stats \{(.*?)\} soil_channel_stats;", text, re.S)
    assert m, "no soil_channel_stats"
    fields = [" ".join(f.split()) for f in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";") if f.strip()]
    assert fields == ["double sum", "double sumsq", "int64_t nonfinite", "float min, max"], fields
    assert re.search(r"typedef struct soil_model_stats \{ soil_channel_stats ch\[SOIL_STAT_CHANNELS\]; \} "
                     r"soil_model_stats;", text)
    # the contract is stated where the ABI is: the finite test, the variance's cancellation limit
    assert "v - v == 0" in text and "2^-53" in text


def test_library_exports_and_binds_the_entry_points():
    from soillib_amd import _abi
    lib = _abi.lib()
    for entry, n_args in ((STATS, 6), (ENSEMBLE, 7)):
        assert hasattr(lib, entry)
        assert entry in _abi.SIGNATURES
        restype, args = _abi.SIGNATURES[entry]
        assert restype is C.c_int
        assert len(args) == n_args
        assert args[0] is C.POINTER(_abi.ErosionPlanes)
        assert all(a is C.c_int64 for a in args[1:4])
        assert all(a is C.c_void_p for a in args[4:])
    assert set(declared_symbols()) == set(_abi.SIGNATURES)
    assert lib.soil_abi_version() == 1


def test_struct_sizes_and_the_numpy_mirror():
    from soillib_amd import _abi, erosion
    assert C.sizeof(_abi.ChannelStats) == 32
    assert C.sizeof(_abi.ModelStats) == 320
    assert [f[0] for f in _abi.ChannelStats._fields_] == ["sum", "sumsq", "nonfinite", "min", "max"]
    assert [getattr(_abi.ChannelStats, f).offset for f in ("sum", "sumsq", "nonfinite", "min", "max")] == [
        0, 8, 16, 24, 28]
    dt = erosion.STATS_DTYPE
    assert dt.itemsize == 32 and dt.names == ("sum", "sumsq", "nonfinite", "min", "max")
    assert [dt.fields[f][1] for f in dt.names] == [0, 8, 16, 24, 28]
    assert [dt.fields[f][0] for f in dt.names] == [np.dtype("<f8"), np.dtype("<f8"), np.dtype("<i8"),
                                                   np.dtype("<f4"), np.dtype("<f4")]


def test_the_channel_lists():
    from soillib_amd import _abi, erosion
    assert erosion.STAT_CHANNELS == ("bedrock", "sediment", "height", "waterHeight", "mass", "debris", "velocity.x",
                                     "velocity.y", "debrisVelocity.x", "debrisVelocity.y")
    assert erosion.ENSEMBLE_CHANNELS == ("bedrock", "sediment", "height", "waterHeight", "mass", "debris")
    assert len(erosion.STAT_CHANNELS) == _abi.SOIL_STAT_CHANNELS == 10
    assert len(erosion.ENSEMBLE_CHANNELS) == _abi.SOIL_ENSEMBLE_CHANNELS == 6


def test_the_source_is_part_of_the_build():
    from soillib_amd import build
    assert "erosion_stats.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "erosion_stats.hip"))


@pytest.mark.parametrize("cls,name,params,entry", [
    ("ErosionBatch", "stats", ["self"], STATS),
    ("ErosionModel", "stats", ["self"], STATS),
    ("ErosionBatch", "ensemble", ["self", "var"], ENSEMBLE)])
def test_the_classes_have_the_methods(cls, name, params, entry):
    from soillib_amd import erosion
    method = getattr(getattr(erosion, cls), name)
    sig = inspect.signature(method)
    assert list(sig.parameters) == params
    if "var" in sig.parameters:
        assert sig.parameters["var"].default is True
    assert entry in method.__doc__


def test_the_entry_points_fail_loudly_without_a_device():
    from soillib_amd import _abi
    lib = _abi.lib()
    if lib.soil_device_count() > 0:
        pytest.skip("a HIP device is present")
    planes = _abi.ErosionPlanes()
    assert lib.soil_erode_batch_stats(C.byref(planes), 2, 8, 8, None, None) == _abi.SOIL_ERR_NO_DEVICE
    assert lib.soil_erode_batch_ensemble(C.byref(planes), 2, 8, 8, None, None, None) == _abi.SOIL_ERR_NO_DEVICE
