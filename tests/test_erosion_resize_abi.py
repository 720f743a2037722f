"""The C ABI of the whole-model resample (include/soil_hip.h: soil_erode_resize_batch) is declared, exported and
bound with its ten arguments, and ErosionModel / ErosionBatch have their `resized` method (no compute calls succeed
here: this runs without a GPU; the refusals of resized() itself need a model, so they are in
test_gpu_erosion_resize.py)."""
import ctypes as C
import inspect
import os
import re

import pytest

from test_abi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "soil_erode_resize_batch"


def test_header_declares_the_entry_point():
    assert ENTRY in declared_symbols()
    text = open(os.path.join(ROOT, "include", "soil_hip.h")).read()
    m = re.search(r"int soil_erode_resize_batch\((.*?)\);", text, re.S)
    assert m, "no declaration"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const soil_erosion_planes* dst", "const soil_erosion_planes* src",
                    "const soil_colour_planes* dst_colour", "const soil_colour_planes* src_colour", "int64_t B",
                    "int64_t Hn", "int64_t Wn", "int64_t Ho", "int64_t Wo", "void* stream"], args
    assert "erosion: changing resolution" in text   # a heading of its own


def test_library_exports_and_binds_the_entry_point():
    from soillib_amd import _abi
    lib = _abi.lib()
    assert hasattr(lib, ENTRY)
    assert ENTRY in _abi.SIGNATURES
    restype, args = _abi.SIGNATURES[ENTRY]
    assert restype is C.c_int
    assert len(args) == 10
    assert args[0] is C.POINTER(_abi.ErosionPlanes) and args[1] is C.POINTER(_abi.ErosionPlanes)
    assert args[2] is C.POINTER(_abi.ColourPlanes) and args[3] is C.POINTER(_abi.ColourPlanes)
    assert all(a is C.c_int64 for a in args[4:9])
    assert args[9] is C.c_void_p
    assert lib.soil_abi_version() == 1


def test_the_source_is_part_of_the_build():
    from soillib_amd import build
    assert "erosion_resize.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "erosion_resize.hip"))


@pytest.mark.parametrize("cls", ["ErosionModel", "ErosionBatch"])
def test_the_classes_have_a_resized_method(cls):
    from soillib_amd import erosion
    method = getattr(getattr(erosion, cls), "resized")
    sig = inspect.signature(method)
    assert list(sig.parameters) == ["self", "H", "W", "scale", "n_particles"]
    assert sig.parameters["scale"].default is None and sig.parameters["n_particles"].default is None
    assert "soil_erode_resize_batch" in method.__doc__


def test_the_entry_point_fails_loudly_without_a_device():
    from soillib_amd import _abi
    lib = _abi.lib()
    if lib.soil_device_count() > 0:
        pytest.skip("a HIP device is present")
    dst, src = _abi.ErosionPlanes(), _abi.ErosionPlanes()
    assert lib.soil_erode_resize_batch(C.byref(dst), C.byref(src), None, None, 2, 8, 8, 4, 4,
                                       None) == _abi.SOIL_ERR_NO_DEVICE
    dc, sc = _abi.ColourPlanes(), _abi.ColourPlanes()
    assert lib.soil_erode_resize_batch(C.byref(dst), C.byref(src), C.byref(dc), C.byref(sc), 1, 8, 8, 4, 4,
                                       None) == _abi.SOIL_ERR_NO_DEVICE
