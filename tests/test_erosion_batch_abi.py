"""The C ABI of the twelve batch entry points (include/soil_hip.h: soil_erode_step_batch, soil_particles_batch and
soil_erode_cells_fused_batch, each plain, _colour, _params and _models) is declared, exported and bound, the
soil_batch_model record has the layout the header states, and ErosionBatch refuses wrong seeds and params before
any device work (no compute calls succeed here: this runs without a GPU).  What ErosionBatch and from_models refuse
of per-model inputs: test_erosion_batch_models_abi.py."""
import ctypes as C
import os
import re

import pytest

from test_abi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFFSETS = {"param": 0, "scale": 112, "N": 128, "seed": 136, "step_index": 144}
# (name, arguments, argument 1 is POINTER(ColourPlanes), takes POINTER(Param) or POINTER(BatchModel));
# (planes[, colour], B, H, W[, N, seeds, step_index], scale, param(s) | models[, flags], stream)
ENTRIES = [
    ("soil_erode_step_batch", 10, False, "Param"),
    ("soil_particles_batch", 10, False, "Param"),
    ("soil_erode_cells_fused_batch", 8, False, "Param"),
    ("soil_erode_step_batch_colour", 11, True, "Param"),
    ("soil_particles_batch_colour", 11, True, "Param"),
    ("soil_erode_cells_fused_batch_colour", 9, True, "Param"),
    ("soil_erode_step_batch_params", 11, True, "Param"),
    ("soil_particles_batch_params", 11, True, "Param"),
    ("soil_erode_cells_fused_batch_params", 9, True, "Param"),
    ("soil_erode_step_batch_models", 7, True, "BatchModel"),
    ("soil_particles_batch_models", 7, True, "BatchModel"),
    ("soil_erode_cells_fused_batch_models", 8, True, "BatchModel"),
]


def test_header_declares_the_twelve_batch_entry_points():
    syms = declared_symbols()
    for name, _, _, _ in ENTRIES:
        assert name in syms, name


def test_header_declares_the_record():
    text = open(os.path.join(ROOT, "include", "soil_hip.h")).read()
    m = re.search(r"typedef struct soil_batch_model \{(.*?)\} soil_batch_model;", text, re.S)
    assert m, "soil_batch_model is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"\b(\w+)(?:\[\d+\])?;", body)
    assert fields == list(OFFSETS), fields


def test_library_exports_and_binds_the_twelve_batch_entry_points():
    from soillib_amd import _abi
    lib = _abi.lib()
    assert lib.soil_abi_version() == 1
    for name, count, colour, record in ENTRIES:
        assert hasattr(lib, name), name
        assert name in _abi.SIGNATURES, name
        args = _abi.SIGNATURES[name][1]
        assert len(args) == count, name
        assert args[0] is C.POINTER(_abi.ErosionPlanes), name
        assert (args[1] is C.POINTER(_abi.ColourPlanes)) == colour, name
        assert (C.POINTER(_abi.Param) in args) == (record == "Param"), name
        assert (C.POINTER(_abi.BatchModel) in args) == (record == "BatchModel"), name
        if record == "BatchModel":
            assert args[5] is C.POINTER(_abi.BatchModel), name


def test_the_record_is_152_bytes_with_the_header_offsets():
    from soillib_amd import _abi
    assert C.sizeof(_abi.BatchModel) == 152
    assert C.alignment(_abi.BatchModel) == 8
    for name, offset in OFFSETS.items():
        assert getattr(_abi.BatchModel, name).offset == offset, name
    assert C.sizeof(_abi.Param) == 112
    # the library checks the same numbers at compile time
    src = open(os.path.join(ROOT, "soillib_amd", "csrc", "erosion_particles.hip")).read()
    assert re.search(r"static_assert\(sizeof\(soil_batch_model\) == 152", src)
    for name, offset in OFFSETS.items():
        assert re.search(r"offsetof\(soil_batch_model, %s\) == %d\b" % (name, offset), src), name


def _no_device():
    from soillib_amd import _abi
    if _abi.lib().soil_device_count() > 0:
        pytest.skip("a HIP device is present")


def _records(B, Ns=None):
    from soillib_amd import _abi, soil
    models = (_abi.BatchModel * B)()
    for b, m in enumerate(models):
        m.param = soil.param_t()._c
        m.scale[:] = [1.0, 1.0, 1.0 + b]
        m.N = 16 if Ns is None else Ns[b]
        m.seed = b + 1
        m.step_index = b
    return models


def test_the_twelve_batch_entry_points_fail_loudly_without_a_device():
    """SOIL_ERR_NO_DEVICE from every entry, with colour planes and, where the entry accepts it, with colour NULL."""
    _no_device()
    from soillib_amd import _abi, soil
    planes = _abi.ErosionPlanes()
    seeds = (C.c_uint64 * 2)(1, 2)
    scale = _abi.vec((1.0, 1.0, 1.0), 3)
    params = (_abi.Param * 2)(soil.param_t()._c, soil.param_t()._c)
    for name, count, colour, record in ENTRIES:
        fn = getattr(_abi.lib(), name)
        args = (2, 8, 8)
        if record == "BatchModel":
            args += (_records(2),)
        else:
            args += () if "cells" in name else (16, seeds, 0)
            args += (scale, params if name.endswith("_params") else soil.param_t()._ref())
        args += ((0,) if "cells" in name else ()) + (None,)
        assert len(args) + 1 + colour == count, name
        if not colour:
            assert fn(C.byref(planes), *args) == _abi.SOIL_ERR_NO_DEVICE, name
            continue
        for colour_planes in (C.byref(_abi.ColourPlanes()),) + (() if name.endswith("_colour") else (None,)):
            assert fn(C.byref(planes), colour_planes, *args) == _abi.SOIL_ERR_NO_DEVICE, name


def test_erosion_batch_fails_loudly_without_a_device():
    _no_device()
    from soillib_amd import _abi, soil
    from soillib_amd.erosion import ErosionBatch
    with pytest.raises(_abi.SoilError, match="no usable HIP device"):
        ErosionBatch(2, 16, 16, (1.0, 1.0, 1.0), soil.param_t(), 32, seeds=[1, 2])


def test_coloured_erosion_batch_fails_loudly_without_a_device():
    _no_device()
    from soillib_amd import _abi, soil
    from soillib_amd.erosion import ErosionBatch
    with pytest.raises(_abi.SoilError, match="no usable HIP device"):
        ErosionBatch(2, 16, 16, (1.0, 1.0, 1.0), soil.param_t(), 32, seeds=[1, 2], colour=True)


@pytest.mark.parametrize("seeds", [[], [7], [1, 2, 3, 4]])
def test_erosion_batch_refuses_a_wrong_number_of_seeds(seeds):
    from soillib_amd import soil
    from soillib_amd.erosion import ErosionBatch
    with pytest.raises(ValueError, match="seeds"):
        ErosionBatch(3, 16, 16, (1.0, 1.0, 1.0), soil.param_t(), 32, seeds=seeds)


@pytest.mark.parametrize("count", [2, 4])
def test_erosion_batch_refuses_a_wrong_number_of_params(count):
    from soillib_amd import soil
    from soillib_amd.erosion import ErosionBatch
    with pytest.raises(ValueError, match="%d params for 3 models" % count):
        ErosionBatch(3, 16, 16, (1.0, 1.0, 1.0), [soil.param_t() for _ in range(count)], 32, seeds=[1, 2, 3])


@pytest.mark.parametrize("bad", [None, 0.5, "param", {"maxage": 64}])
def test_erosion_batch_refuses_an_element_that_is_not_a_param(bad):
    from soillib_amd import soil
    from soillib_amd.erosion import ErosionBatch
    with pytest.raises(ValueError, match=r"params\[1\]"):
        ErosionBatch(3, 16, 16, (1.0, 1.0, 1.0), [soil.param_t(), bad, soil.param_t()], 32, seeds=[1, 2, 3])


def test_erosion_batch_refuses_a_param_that_is_no_sequence():
    from soillib_amd.erosion import ErosionBatch
    with pytest.raises(ValueError, match="sequence of 2 param_t"):
        ErosionBatch(2, 16, 16, (1.0, 1.0, 1.0), 7, 32, seeds=[1, 2])


def test_a_sweep_of_legacy_params_passes_the_checks():
    """legacy.param_t is a param_t: a sweep of them gets past the checks (and without a device, no further)."""
    _no_device()
    from soillib_amd import _abi, legacy
    from soillib_amd.erosion import ErosionBatch
    with pytest.raises(_abi.SoilError, match="no usable HIP device"):
        ErosionBatch(2, 16, 16, (1.0, 1.0, 1.0), [legacy.param_t(), legacy.param_t()], 32, seeds=[1, 2])
