"""The parameter sweep's C ABI (include/soil_hip.h: soil_erode_step_batch_params, soil_particles_batch_params,
soil_erode_cells_fused_batch_params) is declared, exported and bound, and ErosionBatch refuses a wrong sequence
of params before any device work (no compute calls succeed here: this runs without a GPU)."""
import ctypes as C

import pytest

from test_abi_symbols import declared_symbols

ENTRY_POINTS = ("soil_erode_step_batch_params", "soil_particles_batch_params", "soil_erode_cells_fused_batch_params")


def test_header_declares_the_sweep_entry_points():
    syms = declared_symbols()
    for name in ENTRY_POINTS:
        assert name in syms, name


def test_library_exports_and_binds_the_sweep_entry_points():
    from soillib_amd import _abi
    lib = _abi.lib()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in _abi.SIGNATURES, name
        args = _abi.SIGNATURES[name][1]
        assert args[1] is C.POINTER(_abi.ColourPlanes), name
        assert C.POINTER(_abi.Param) in args, name
    assert lib.soil_abi_version() == 1
    # (planes, colour, B, H, W[, N, seeds, step_index], scale, params[, flags], stream)
    assert len(_abi.SIGNATURES["soil_erode_step_batch_params"][1]) == 11
    assert len(_abi.SIGNATURES["soil_particles_batch_params"][1]) == 11
    assert len(_abi.SIGNATURES["soil_erode_cells_fused_batch_params"][1]) == 9


def _no_device():
    from soillib_amd import _abi
    if _abi.lib().soil_device_count() > 0:
        pytest.skip("a HIP device is present")


def test_sweep_entry_points_fail_loudly_without_a_device():
    _no_device()
    from soillib_amd import _abi, soil
    lib = _abi.lib()
    planes = _abi.ErosionPlanes()
    seeds = (C.c_uint64 * 2)(1, 2)
    scale = _abi.vec((1.0, 1.0, 1.0), 3)
    params = (_abi.Param * 2)(soil.param_t()._c, soil.param_t()._c)
    for colour in (None, C.byref(_abi.ColourPlanes())):
        assert lib.soil_erode_step_batch_params(C.byref(planes), colour, 2, 8, 8, 16, seeds, 0, scale, params,
                                                None) == _abi.SOIL_ERR_NO_DEVICE
        assert lib.soil_particles_batch_params(C.byref(planes), colour, 2, 8, 8, 16, seeds, 0, scale, params,
                                               None) == _abi.SOIL_ERR_NO_DEVICE
        assert lib.soil_erode_cells_fused_batch_params(C.byref(planes), colour, 2, 8, 8, scale, params, 0,
                                                       None) == _abi.SOIL_ERR_NO_DEVICE


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
