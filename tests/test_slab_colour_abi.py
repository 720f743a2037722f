"""The C-ABI surface of the sharded coloured step (include/soil_slab.h: soil_slab_colour_ops,
soil_slab_create_colour, soil_slab_colour_ops_hip_*; include/soil_hip.h: soil_particles_pair_colour_slab):
declared, exported and bound, struct sizes as the header says.  No GPU."""
import ctypes

from test_abi_symbols import declared_symbols

NEW_SLAB = ("soil_slab_create_colour", "soil_slab_colour_ops_hip_create", "soil_slab_colour_ops_hip_destroy")


def test_new_symbols_are_declared_exported_and_bound():
    from soillib_amd import _abi
    lib = _abi.lib()
    assert "soil_particles_pair_colour_slab" in declared_symbols()
    assert "soil_particles_pair_colour_slab" in _abi.SIGNATURES
    for name in NEW_SLAB:
        assert name in declared_symbols("soil_slab.h") and name in _abi.SLAB_SIGNATURES
    for name in NEW_SLAB + ("soil_particles_pair_colour_slab",):
        fn = getattr(lib, name)
        assert fn.argtypes is not None
    args = _abi.SIGNATURES["soil_particles_pair_colour_slab"][1]
    assert len(args) == 11 and args[1] is ctypes.POINTER(_abi.ColourPlanes)


def test_colour_ops_layout():
    from soillib_amd import _abi
    # ctx + particles_fluvial, particles_debris, particles_pair, cells, particles_pass (static_assert in
    # csrc/slab_runner.hip); soil_slab_ops stays 20 pointers
    assert ctypes.sizeof(_abi.SlabColourOps) == 6 * 8
    assert [n for n, _ in _abi.SlabColourOps._fields_] == ["ctx", "particles_fluvial", "particles_debris",
                                                           "particles_pair", "cells", "particles_pass"]
    assert ctypes.sizeof(_abi.SlabOps) == 20 * 8


def test_colour_ops_hip_create_refuses_a_foreign_table():
    """The HIP colour table shares the HIP physics table's state: any other table is refused (no device
    touched)."""
    from soillib_amd import _abi
    lib = _abi.lib()
    out = ctypes.POINTER(_abi.SlabColourOps)()
    foreign = _abi.SlabOps()
    assert lib.soil_slab_colour_ops_hip_create(ctypes.byref(out), ctypes.byref(foreign)) == _abi.SOIL_ERR_INVALID_ARGUMENT
    assert "soil_slab_ops_hip_create" in _abi.last_error()
