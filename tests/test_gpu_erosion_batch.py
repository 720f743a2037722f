"""A batch of independent models stepped together (include/soil_hip.h: soil_erode_step_batch,
soil_particles_batch, soil_erode_cells_fused_batch; soillib_amd.erosion.ErosionBatch) against the same models
stepped one at a time through ErosionModel with seed = seeds[b]:

  * whole steps, every physics plane of every model, in the direct, staged and (alone: tiled) shapes;
  * the cell phase bit for bit, with and without SOIL_CELLS_KEEP_FLUX;
  * the same trajectories: the particle step count equals the sum of the single models' exactly;
  * isolation: a model whose walkers go NaN spoils its own cell (0, 0) and nothing of the others;
  * plumbing: another stream, a smaller batch after a larger one, the phases one by one, refused arguments.
"""
import ctypes as C

import numpy as np
import pytest

from util import product_param, script_param, terrain, to_gpu, to_np

pytestmark = pytest.mark.gpu

OUT = ("layers", "height", "waterHeight", "mass", "velocity", "debris", "debrisVelocity")
FLUX = ("waterFlux", "massFlux", "velocityFlux", "debrisFlux", "debrisVelocityFlux")


def _param(oracle, maxage):
    p = product_param(script_param(oracle.default_param()))
    p.maxage = maxage
    return p


def _inputs(oracle, B, H, W):
    """Per model: its own terrain (noise of another seed, some sediment), rainfall and uplift."""
    r = np.random.default_rng(1000 * B + H + W)
    layers = np.stack([terrain(oracle, H, W, seed=3.0 + 5.0 * b, sediment=0.05, rng_seed=b) for b in range(B)])
    rain = (0.5 + r.random((B, H, W))).astype(np.float32)
    uplift = (0.5 * r.random((B, H, W))).astype(np.float32)
    return dict(layers=layers, rainfall=rain, uplift=uplift)


def _batch(B, H, W, scale, p, N, seeds, inp):
    from soillib_amd import silt
    from soillib_amd.erosion import ErosionBatch
    bt = ErosionBatch(B, H, W, scale, p, N, seeds)
    bt.set_layers(to_gpu(inp["layers"]))
    silt.set(bt.rainfall, to_gpu(inp["rainfall"]))
    silt.set(bt.uplift, to_gpu(inp["uplift"]))
    return bt


def _single(b, H, W, scale, p, N, seed, inp):
    from soillib_amd import silt
    from soillib_amd.erosion import ErosionModel
    m = ErosionModel(H, W, scale, p, N, seed=seed)
    m.set_layers(to_gpu(inp["layers"][b]))
    silt.set(m.rainfall, to_gpu(inp["rainfall"][b]))
    silt.set(m.uplift, to_gpu(inp["uplift"][b]))
    return m


def _close(got, want, what):
    """The slab runner's tolerance against the whole grid (test_gpu_slab_colour._compare)."""
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5 * (np.nanmax(np.abs(want)) + 1e-30), err_msg=what)


def _steps_equal_models(oracle, B, H, W, N, maxage, steps, seeds=None):
    p = _param(oracle, maxage)
    scale = (20.0 / H, 20.0 / W, 4.0)
    seeds = seeds or [11 + 7 * b for b in range(B)]
    inp = _inputs(oracle, B, H, W)
    bt = _batch(B, H, W, scale, p, N, seeds, inp)
    for _ in range(steps):
        bt.step()
    assert bt.step_index == steps
    for b in range(B):
        m = _single(b, H, W, scale, p, N, seeds[b], inp)
        for _ in range(steps):
            m.step()
        got = bt.model_planes(b)
        for name in OUT:
            _close(got[name], to_np(getattr(m, name)), "model %d: %s" % (b, name))
        for name in FLUX:   # zeroed on exit
            assert not got[name].any(), "model %d: %s not zeroed" % (b, name)
        assert np.isfinite(got["layers"]).all()
        assert (got["layers"] != inp["layers"][b]).any(), "model %d did not change" % b


@pytest.mark.parametrize("B,H,W,N,maxage,steps", [
    (1, 64, 64, 512, 64, 3),            # one model
    (3, 33, 47, 700, 64, 3),            # direct shape (N < 1024), odd H x W: the scalar cell kernel
    (4, 96, 80, 2048, 96, 3),           # staged shape
    (3, 48, 160, 1500, 64, 3),          # non-square, staged
])
def test_batch_equals_models(hip, oracle, B, H, W, N, maxage, steps):
    _steps_equal_models(oracle, B, H, W, N, maxage, steps)


def test_batch_equals_models_at_the_example_shape(hip, oracle):
    """example/erosion_gpu.py: 256^2, 8192 particles, maxage 256 — eight models, two steps."""
    _steps_equal_models(oracle, 8, 256, 256, 8192, 256, 2)


def test_batch_equals_models_tiled_alone(hip, oracle):
    """N = H*W/8 = 51200 at 640^2 gets the tiled shape alone; the batch runs it staged."""
    _steps_equal_models(oracle, 2, 640, 640, 640 * 640 // 8, 64, 2)


# ---------------------------------------------------------------- the cell phase

def _cell_batch_inputs(B, H, W, seed):
    r = np.random.default_rng(seed)
    f = lambda *s: (r.random((B, H, W) + s) * 2.0).astype(np.float32)
    g = dict(layers=f(2), uplift=f(), rainfall=f(), waterFlux=f(), massFlux=f() * 1e-3,
             velocityFlux=f(2) - 1.0, debrisFlux=f() * 1e-3, debrisVelocityFlux=f(2) - 1.0)
    g["layers"][..., 1] *= 0.1
    return g


@pytest.mark.parametrize("B,H,W", [(3, 33, 47), (4, 96, 80), (2, 256, 256), (5, 8, 4)])
@pytest.mark.parametrize("keep", [False, True])
def test_cell_phase_bit_exact(hip, oracle, B, H, W, keep):
    from util import assert_bit_equal
    from soillib_amd import silt
    from soillib_amd.erosion import ErosionModel
    p = _param(oracle, 64)
    scale = (20.0 / H, 20.0 / W, 4.0)
    g = _cell_batch_inputs(B, H, W, B * H + W)
    inp = dict(layers=g["layers"], rainfall=g["rainfall"], uplift=g["uplift"])
    bt = _batch(B, H, W, scale, p, 0, [0] * B, inp)
    for name in FLUX:
        silt.set(getattr(bt, name), to_gpu(g[name]))
    bt.cells_fused(keep_flux=keep)
    for b in range(B):
        m = ErosionModel(H, W, scale, p, 1, seed=0)
        m.set_layers(to_gpu(g["layers"][b]))
        for name in ("rainfall", "uplift") + FLUX:
            silt.set(getattr(m, name), to_gpu(g[name][b]))
        m.cells_fused(keep_flux=keep)
        got = bt.model_planes(b)
        for name in ("layers_next", "height", "waterHeight", "mass", "velocity", "debris", "debrisVelocity") + FLUX:
            assert_bit_equal(got[name], to_np(getattr(m, name)), "model %d: %s" % (b, name))
        if keep:
            assert_bit_equal(got["waterFlux"], g["waterFlux"][b], "kept flux")


# ---------------------------------------------------------------- trajectories

@pytest.fixture
def retire_off(hip):
    from soillib_amd import soil
    before = soil.debris_retire()
    soil.debris_retire(0)
    yield
    soil.debris_retire(before)


@pytest.mark.parametrize("B,H,W,N", [(3, 40, 52, 600), (4, 96, 80, 4096), (2, 640, 640, 51200)])
def test_same_trajectories(hip, oracle, retire_off, B, H, W, N):
    """After one particle phase from identical fields, the device step counter holds the sum of the single
    models' counts exactly (the tiled single model walks every debris walker to the end: retirement off)."""
    from soillib_amd import soil
    p = _param(oracle, 96)
    scale = (20.0 / H, 20.0 / W, 4.0)
    seeds = [5 + 3 * b for b in range(B)]
    inp = _inputs(oracle, B, H, W)
    bt = _batch(B, H, W, scale, p, N, seeds, inp)
    soil.particle_steps(reset=True)
    bt.step_index = 2
    bt.particles()
    got = soil.particle_steps(reset=True)
    want = 0
    for b in range(B):
        m = _single(b, H, W, scale, p, N, seeds[b], inp)
        m.step_index = 2
        m.seed_step()
        m.particles_pair()
        want += soil.particle_steps(reset=True)
        planes = bt.model_planes(b)
        for name in FLUX:
            _close(planes[name], to_np(getattr(m, name)), "model %d: %s" % (b, name))
    assert got == want > 0


# ---------------------------------------------------------------- isolation

def test_nan_walkers_stay_in_their_model(hip, oracle):
    from soillib_amd import silt
    B, H, W, N = 3, 64, 72, 2048
    p = _param(oracle, 64)
    scale = (20.0 / H, 20.0 / W, 4.0)
    seeds = [21, 22, 23]
    inp = _inputs(oracle, B, H, W)
    # a velocity everywhere: no walker starts at rest on a pit cell (speed 0 / sqrt(0) = NaN, the reference's own
    # NaN walkers, DESIGN.md "Reference quirks"), so that only model 1's NaN cells make NaN walkers
    vel = np.ones((B, H, W, 2), np.float32)
    vel[1, 20:36, 30:50] = np.nan        # model 1's walkers through these cells go NaN
    dvel = np.ones((B, H, W, 2), np.float32)
    bt = _batch(B, H, W, scale, p, N, seeds, inp)
    silt.set(bt.velocity, to_gpu(vel))
    silt.set(bt.debrisVelocity, to_gpu(dvel))
    bt.step()
    for b in range(B):
        m = _single(b, H, W, scale, p, N, seeds[b], inp)
        silt.set(m.velocity, to_gpu(vel[b]))
        silt.set(m.debrisVelocity, to_gpu(dvel[b]))
        m.step()
        got = bt.model_planes(b)
        for name in OUT:
            want = to_np(getattr(m, name))
            g = got[name]
            assert np.array_equal(np.isnan(g), np.isnan(want)), "model %d: %s NaN cells differ" % (b, name)
            if b != 1:
                assert np.isfinite(g).all(), "model %d: %s" % (b, name)
            fin = np.isfinite(want)
            _close(g[fin], want[fin], "model %d: %s" % (b, name))
        if b == 1:
            assert np.isnan(got["waterHeight"][0, 0]), "model 1's NaN walkers did not reach its cell (0, 0)"


# ---------------------------------------------------------------- plumbing

def _run_and_compare(oracle, B, H, W, N, steps):
    p = _param(oracle, 48)
    scale = (20.0 / H, 20.0 / W, 4.0)
    seeds = [101 + b for b in range(B)]
    inp = _inputs(oracle, B, H, W)
    bt = _batch(B, H, W, scale, p, N, seeds, inp)
    for _ in range(steps):
        bt.step()
    for b in range(B):
        m = _single(b, H, W, scale, p, N, seeds[b], inp)
        for _ in range(steps):
            m.step()
        got = bt.model_planes(b)
        for name in OUT:
            _close(got[name], to_np(getattr(m, name)), "model %d: %s" % (b, name))


def test_batch_on_another_stream(hip, oracle):
    import torch
    from soillib_amd import _abi
    s = torch.cuda.Stream()
    _abi.set_stream(s.cuda_stream)
    try:
        _run_and_compare(oracle, 3, 48, 64, 1200, 2)
        s.synchronize()
    finally:
        _abi.set_stream(0)


def test_small_batch_after_a_larger_one(hip, oracle):
    """The workspace and the seed staging are sized by the first, larger batch and reused by the second."""
    _run_and_compare(oracle, 6, 96, 96, 4096, 1)
    _run_and_compare(oracle, 2, 40, 36, 700, 2)
    _run_and_compare(oracle, 3, 64, 64, 2048, 1)


def test_phases_one_by_one_equal_step(hip, oracle):
    """particles(), cells_fused(), swap over several steps equals step() (step_index carried on)."""
    B, H, W, N = 3, 48, 56, 1500
    p = _param(oracle, 48)
    scale = (20.0 / H, 20.0 / W, 4.0)
    seeds = [7, 8, 9]
    inp = _inputs(oracle, B, H, W)
    a = _batch(B, H, W, scale, p, N, seeds, inp)
    c = _batch(B, H, W, scale, p, N, seeds, inp)
    for k in range(4):
        a.step()
        c.particles()
        c.cells_fused()
        c.swap_layers()
        c.step_index += 1
    assert a.step_index == c.step_index == 4
    for b in range(B):
        pa, pc = a.model_planes(b), c.model_planes(b)
        for name in OUT:
            _close(pc[name], pa[name], "model %d: %s" % (b, name))


def test_invalid_arguments_are_refused(hip, oracle):
    from soillib_amd import _abi
    from soillib_amd.erosion import ErosionBatch
    lib = _abi.lib()
    p = _param(oracle, 32)
    bt = _batch(2, 16, 16, (1.0, 1.0, 1.0), p, 64, [1, 2], _inputs(oracle, 2, 16, 16))
    planes = bt._planes()
    seeds = (C.c_uint64 * 2)(1, 2)
    scale = _abi.vec((1.0, 1.0, 1.0), 3)
    bad = [  # (B, H, W, N, seeds)
        (0, 16, 16, 64, seeds), (-1, 16, 16, 64, seeds), (2, 0, 16, 64, seeds), (2, 16, 0, 64, seeds),
        (2, 16, 16, -1, seeds), (2, 16, 16, 64, None), (1 << 40, 1 << 20, 16, 64, seeds),
        (2, 1 << 31, 1 << 31, 64, seeds), (1 << 32, 16, 16, 1 << 30, seeds)]
    for B, H, W, N, s in bad:
        for fn in (lib.soil_erode_step_batch, lib.soil_particles_batch):
            rc = fn(C.byref(planes), B, H, W, N, s, 0, scale, p._ref(), None)
            assert rc == _abi.SOIL_ERR_INVALID_ARGUMENT, (fn.__name__, B, H, W, N)
            assert _abi.last_error()
    for B, H, W in [(0, 16, 16), (2, 0, 16), (2, 16, -3), (1 << 40, 1 << 20, 16)]:
        rc = lib.soil_erode_cells_fused_batch(C.byref(planes), B, H, W, scale, p._ref(), 0, None)
        assert rc == _abi.SOIL_ERR_INVALID_ARGUMENT, (B, H, W)
    # N == 0 needs no seeds; a null plane is refused
    assert lib.soil_particles_batch(C.byref(planes), 2, 16, 16, 0, None, 0, scale, p._ref(), None) == _abi.SOIL_OK
    empty = _abi.ErosionPlanes()
    assert lib.soil_erode_step_batch(C.byref(empty), 2, 16, 16, 64, seeds, 0, scale, p._ref(),
                                     None) == _abi.SOIL_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        ErosionBatch(2, 16, 16, (1.0, 1.0, 1.0), p, 64, seeds=[1, 2, 3])
    with pytest.raises(ValueError):
        _abi.check(lib.soil_erode_step_batch(C.byref(planes), 0, 16, 16, 64, seeds, 0, scale, p._ref(), None))
    bt.step()   # the batch itself still steps
    _abi.check(lib.soil_stream_synchronize(None))
