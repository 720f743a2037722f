"""The coloured erosion step's C ABI (include/soil_hip.h: soil_colour_planes and its three entry points) is
declared, exported and bound (no compute calls: this runs without a GPU)."""
import ctypes

from test_abi_symbols import declared_symbols

COLOUR_ENTRY_POINTS = ("soil_erode_cells_fused_colour", "soil_particles_pair_colour", "soil_erode_step_colour")


def test_header_declares_the_coloured_step():
    syms = declared_symbols()
    for name in COLOUR_ENTRY_POINTS:
        assert name in syms


def test_library_exports_the_coloured_step():
    from soillib_amd import _abi
    lib = _abi.lib()
    for name in COLOUR_ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in _abi.SIGNATURES, name
    assert lib.soil_abi_version() == 1


def test_colour_planes_layout():
    from soillib_amd import _abi
    assert ctypes.sizeof(_abi.ColourPlanes) == 32
    assert [f for f, _ in _abi.ColourPlanes._fields_] == ["albedo_bedrock", "albedo_surface", "albedo_fluvial",
                                                          "albedo_debris"]
