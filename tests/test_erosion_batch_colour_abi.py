"""The coloured batch step's C ABI (include/soil_hip.h: soil_erode_step_batch_colour, soil_particles_batch_colour,
soil_erode_cells_fused_batch_colour) is declared, exported and bound, and ErosionBatch(colour=True) fails loudly
before any device work (no compute calls succeed here: this runs without a GPU)."""
import ctypes as C

import pytest

from test_abi_symbols import declared_symbols

ENTRY_POINTS = ("soil_erode_step_batch_colour", "soil_particles_batch_colour", "soil_erode_cells_fused_batch_colour")


def test_header_declares_the_coloured_batch_entry_points():
    syms = declared_symbols()
    for name in ENTRY_POINTS:
        assert name in syms, name


def test_library_exports_and_binds_the_coloured_batch_entry_points():
    from soillib_amd import _abi
    lib = _abi.lib()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in _abi.SIGNATURES, name
        assert _abi.SIGNATURES[name][1][1] is C.POINTER(_abi.ColourPlanes), name
    assert lib.soil_abi_version() == 1
    # (planes, colour, B, H, W[, N, seeds, step_index], scale, param[, flags], stream)
    assert len(_abi.SIGNATURES["soil_erode_step_batch_colour"][1]) == 11
    assert len(_abi.SIGNATURES["soil_particles_batch_colour"][1]) == 11
    assert len(_abi.SIGNATURES["soil_erode_cells_fused_batch_colour"][1]) == 9


def _no_device():
    from soillib_amd import _abi
    if _abi.lib().soil_device_count() > 0:
        pytest.skip("a HIP device is present")


def test_coloured_batch_entry_points_fail_loudly_without_a_device():
    _no_device()
    from soillib_amd import _abi, soil
    lib = _abi.lib()
    planes, colour = _abi.ErosionPlanes(), _abi.ColourPlanes()
    seeds = (C.c_uint64 * 2)(1, 2)
    scale = _abi.vec((1.0, 1.0, 1.0), 3)
    p = soil.param_t()
    assert lib.soil_erode_step_batch_colour(C.byref(planes), C.byref(colour), 2, 8, 8, 16, seeds, 0, scale,
                                            p._ref(), None) == _abi.SOIL_ERR_NO_DEVICE
    assert lib.soil_particles_batch_colour(C.byref(planes), C.byref(colour), 2, 8, 8, 16, seeds, 0, scale,
                                           p._ref(), None) == _abi.SOIL_ERR_NO_DEVICE
    assert lib.soil_erode_cells_fused_batch_colour(C.byref(planes), C.byref(colour), 2, 8, 8, scale, p._ref(), 0,
                                                   None) == _abi.SOIL_ERR_NO_DEVICE


def test_coloured_erosion_batch_fails_loudly_without_a_device():
    _no_device()
    from soillib_amd import _abi, soil
    from soillib_amd.erosion import ErosionBatch
    with pytest.raises(_abi.SoilError, match="no usable HIP device"):
        ErosionBatch(2, 16, 16, (1.0, 1.0, 1.0), soil.param_t(), 32, seeds=[1, 2], colour=True)
