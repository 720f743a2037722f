"""The C ABI of batches of different models (include/soil_hip.h: soil_batch_model, soil_erode_step_batch_models,
soil_particles_batch_models, soil_erode_cells_fused_batch_models) is declared, exported and bound, its record has
the layout the header states, and ErosionBatch / ErosionBatch.from_models refuse bad per-model inputs before any
device work (no compute calls succeed here: this runs without a GPU)."""
import ctypes as C
import os
import re

import pytest

from test_abi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("soil_erode_step_batch_models", "soil_particles_batch_models", "soil_erode_cells_fused_batch_models")
OFFSETS = {"param": 0, "scale": 112, "N": 128, "seed": 136, "step_index": 144}


def test_header_declares_the_entry_points_and_the_record():
    syms = declared_symbols()
    for name in ENTRY_POINTS:
        assert name in syms, name
    text = open(os.path.join(ROOT, "include", "soil_hip.h")).read()
    m = re.search(r"typedef struct soil_batch_model \{(.*?)\} soil_batch_model;", text, re.S)
    assert m, "soil_batch_model is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"\b(\w+)(?:\[\d+\])?;", body)
    assert fields == list(OFFSETS), fields


def test_library_exports_and_binds_the_entry_points():
    from soillib_amd import _abi
    lib = _abi.lib()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in _abi.SIGNATURES, name
        args = _abi.SIGNATURES[name][1]
        assert args[0] is C.POINTER(_abi.ErosionPlanes), name
        assert args[1] is C.POINTER(_abi.ColourPlanes), name
        assert args[5] is C.POINTER(_abi.BatchModel), name
    assert lib.soil_abi_version() == 1
    # (planes, colour, B, H, W, models[, flags], stream)
    assert len(_abi.SIGNATURES["soil_erode_step_batch_models"][1]) == 7
    assert len(_abi.SIGNATURES["soil_particles_batch_models"][1]) == 7
    assert len(_abi.SIGNATURES["soil_erode_cells_fused_batch_models"][1]) == 8


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


def test_entry_points_fail_loudly_without_a_device():
    _no_device()
    from soillib_amd import _abi
    lib = _abi.lib()
    planes = _abi.ErosionPlanes()
    models = _records(2)
    for colour in (None, C.byref(_abi.ColourPlanes())):
        assert lib.soil_erode_step_batch_models(C.byref(planes), colour, 2, 8, 8, models,
                                                None) == _abi.SOIL_ERR_NO_DEVICE
        assert lib.soil_particles_batch_models(C.byref(planes), colour, 2, 8, 8, models,
                                               None) == _abi.SOIL_ERR_NO_DEVICE
        assert lib.soil_erode_cells_fused_batch_models(C.byref(planes), colour, 2, 8, 8, models, 0,
                                                       None) == _abi.SOIL_ERR_NO_DEVICE


def _batch(**kw):
    from soillib_amd import soil
    from soillib_amd.erosion import ErosionBatch
    args = dict(B=3, H=16, W=16, scale=(1.0, 1.0, 1.0), param=soil.param_t(), n_particles=32, seeds=[1, 2, 3])
    args.update(kw)
    return ErosionBatch(**args)


@pytest.mark.parametrize("count", [2, 4])
def test_erosion_batch_refuses_a_wrong_number_of_scales(count):
    with pytest.raises(ValueError, match="%d scales for 3 models" % count):
        _batch(scale=[(1.0, 1.0, 1.0)] * count)


@pytest.mark.parametrize("bad", [(1.0, 1.0), (1.0, 1.0, 1.0, 1.0), 2.0, "abc", (1.0, "x", 1.0), None])
def test_erosion_batch_refuses_a_scale_that_is_not_three_numbers(bad):
    with pytest.raises(ValueError, match=r"scales\[1\]"):
        _batch(scale=[(1.0, 1.0, 1.0), bad, (2.0, 2.0, 2.0)])


@pytest.mark.parametrize("count", [1, 2, 4])
def test_erosion_batch_refuses_a_wrong_number_of_walker_counts(count):
    with pytest.raises(ValueError, match="%d walker counts for 3 models" % count):
        _batch(n_particles=[32] * count)


@pytest.mark.parametrize("bad", [-1, -1024, 2.5, "8", None])
def test_erosion_batch_refuses_a_walker_count_that_is_negative_or_no_int(bad):
    with pytest.raises(ValueError, match=r"Ns\[2\]"):
        _batch(n_particles=[32, 0, bad])


def test_from_models_refuses_an_empty_list():
    from soillib_amd.erosion import ErosionBatch
    with pytest.raises(ValueError, match="no models"):
        ErosionBatch.from_models([])


def _host_model(H=16, W=16, colour=False, dom=None, N=8):
    """An ErosionModel on host tensors: enough for from_models' checks, which come before any device work."""
    from soillib_amd import silt, soil
    from soillib_amd.erosion import ErosionModel
    alloc = lambda dtype, shape: silt.tensor(dtype, silt.shape(*shape), silt.cpu)  # noqa: E731
    return ErosionModel(H, W, (1.0, 1.0, 1.0), soil.param_t(), N, seed=1, dom=dom, alloc=alloc, colour=colour)


def test_from_models_refuses_mixed_shapes():
    from soillib_amd.erosion import ErosionBatch
    with pytest.raises(ValueError, match="16x24"):
        ErosionBatch.from_models([_host_model(), _host_model(W=24)])
    with pytest.raises(ValueError, match="20x16"):
        ErosionBatch.from_models([_host_model(), _host_model(), _host_model(H=20)])


def test_from_models_refuses_mixed_colour_settings():
    from soillib_amd.erosion import ErosionBatch
    with pytest.raises(ValueError, match="colour"):
        ErosionBatch.from_models([_host_model(colour=True), _host_model()])
    with pytest.raises(ValueError, match="colour"):
        ErosionBatch.from_models([_host_model(), _host_model(colour=True)])


def test_from_models_refuses_a_slab():
    from soillib_amd import _abi
    from soillib_amd.erosion import ErosionBatch
    slab = _host_model(dom=_abi.Domain(32, 16, 8, 16, 1, 15), H=32)
    with pytest.raises(ValueError, match="row slab"):
        ErosionBatch.from_models([slab])
    with pytest.raises(ValueError, match="row slab"):
        ErosionBatch.from_models([_host_model(H=32), slab])


def test_from_models_refuses_what_is_not_a_model():
    from soillib_amd.erosion import ErosionBatch
    with pytest.raises(ValueError, match=r"models\[1\]"):
        ErosionBatch.from_models([_host_model(), object()])
