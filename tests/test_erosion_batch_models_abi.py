"""ErosionBatch and ErosionBatch.from_models refuse bad per-model inputs (scales, walker counts, the models handed
to from_models) before any device work; this runs without a GPU.  The C ABI of the soil_*_batch_models entry points
and the soil_batch_model record: test_erosion_batch_abi.py."""
import pytest


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
