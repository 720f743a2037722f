"""A coloured batch of independent models stepped together (include/soil_hip.h: soil_erode_step_batch_colour,
soil_particles_batch_colour, soil_erode_cells_fused_batch_colour; ErosionBatch(colour=True)) against the same
models stepped one at a time through ErosionModel(colour=True) with seed = seeds[b]:

  * whole steps, every physics plane and the three colour planes a step writes, in the direct, staged and
    (alone: tiled) shapes — every model with its own terrain, rainfall, uplift, bedrock and surface colours;
  * the coloured cell phase bit for bit, with and without SOIL_CELLS_KEEP_FLUX, W % 4 == 0 and not;
  * the same trajectories: the particle step count equals the single coloured models' sum and the physics
    batch's;
  * the colour flux planes are cleared before the launches;
  * isolation: NaN walkers and non-finite spawn colours spoil their own model only;
  * the physics planes are those of the physics batch;
  * plumbing: another stream, a smaller batch after a larger one, the phases one by one, refused arguments.
"""
import ctypes as C

import numpy as np
import pytest

from util import assert_bit_equal, product_param, script_param, terrain, to_gpu, to_np

pytestmark = pytest.mark.gpu

OUT = ("layers", "height", "waterHeight", "mass", "velocity", "debris", "debrisVelocity")
FLUX = ("waterFlux", "massFlux", "velocityFlux", "debrisFlux", "debrisVelocityFlux")
COLOUR_OUT = ("albedoSurface", "albedoFluvial", "albedoDebris")


def _param(oracle, maxage):
    p = product_param(script_param(oracle.default_param()))
    p.maxage = maxage
    return p


def _inputs(oracle, B, H, W):
    """Per model: its own terrain, rainfall, uplift, bedrock colour and surface colour."""
    r = np.random.default_rng(2000 * B + H + W)
    layers = np.stack([terrain(oracle, H, W, seed=3.0 + 5.0 * b, sediment=0.05, rng_seed=b) for b in range(B)])
    rain = (0.5 + r.random((B, H, W))).astype(np.float32)
    uplift = (0.5 * r.random((B, H, W))).astype(np.float32)
    # model b's colours lean towards channel b % 3: a colour read from another model shows
    tint = np.zeros((B, 1, 1, 3), np.float32)
    tint[np.arange(B), 0, 0, np.arange(B) % 3] = 1.0
    bed = (0.2 * r.random((B, H, W, 3)) + 0.6 * tint).astype(np.float32)
    surf = (0.3 * r.random((B, H, W, 3)) + 0.5 * np.roll(tint, 1, axis=-1)).astype(np.float32)
    return dict(layers=layers, rainfall=rain, uplift=uplift, albedoBedrock=bed, albedoSurface=surf)


def _batch(B, H, W, scale, p, N, seeds, inp, colour=True):
    from soillib_amd import silt
    from soillib_amd.erosion import ErosionBatch
    bt = ErosionBatch(B, H, W, scale, p, N, seeds, colour=colour)
    bt.set_layers(to_gpu(inp["layers"]))
    silt.set(bt.rainfall, to_gpu(inp["rainfall"]))
    silt.set(bt.uplift, to_gpu(inp["uplift"]))
    if colour:
        bt.set_colour("albedoBedrock", to_gpu(inp["albedoBedrock"]))
        bt.set_colour("albedoSurface", to_gpu(inp["albedoSurface"]))
    return bt


def _single(b, H, W, scale, p, N, seed, inp):
    from soillib_amd import silt
    from soillib_amd.erosion import ErosionModel
    m = ErosionModel(H, W, scale, p, N, seed=seed, colour=True)
    m.set_layers(to_gpu(inp["layers"][b]))
    for name in ("rainfall", "uplift", "albedoBedrock", "albedoSurface"):
        silt.set(getattr(m, name), to_gpu(inp[name][b]))
    return m


def _close(got, want, what):
    """The slab runner's tolerance against the whole grid (test_gpu_slab_colour._compare)."""
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5 * (np.nanmax(np.abs(want)) + 1e-30), err_msg=what)


def _compare_models(bt, models, what=""):
    for b, m in enumerate(models):
        got = bt.model_planes(b)
        for name in OUT + COLOUR_OUT:
            _close(got[name], to_np(getattr(m, name)), "%smodel %d: %s" % (what, b, name))


def _steps_equal_models(oracle, B, H, W, N, maxage, steps):
    p = _param(oracle, maxage)
    scale = (20.0 / H, 20.0 / W, 4.0)
    seeds = [13 + 7 * b for b in range(B)]
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
        for name in OUT + COLOUR_OUT:
            _close(got[name], to_np(getattr(m, name)), "model %d: %s" % (b, name))
        for name in FLUX:   # zeroed on exit
            assert not got[name].any(), "model %d: %s not zeroed" % (b, name)
        for name in ("layers",) + COLOUR_OUT:
            assert np.isfinite(got[name]).all(), "model %d: %s" % (b, name)
        assert (got["albedoSurface"] != inp["albedoSurface"][b]).any(), "model %d's colours did not change" % b
        assert got["albedoFluvial"].any() and got["albedoDebris"].any(), "model %d: no transport colour" % b


@pytest.mark.parametrize("B,H,W,N,maxage,steps", [
    (3, 33, 47, 700, 64, 3),            # direct shape (N < 1024), odd H x W: the scalar cell kernel
    (4, 96, 80, 2048, 96, 3),           # staged shape
    (3, 48, 160, 1500, 64, 2),          # non-square, staged
])
def test_coloured_batch_equals_models(hip, oracle, B, H, W, N, maxage, steps):
    _steps_equal_models(oracle, B, H, W, N, maxage, steps)


def test_coloured_batch_equals_models_at_the_example_shape(hip, oracle):
    """example/erosion_gpu.py: 256^2, 8192 particles, maxage 256 — eight models, two steps."""
    _steps_equal_models(oracle, 8, 256, 256, 8192, 256, 2)


def test_coloured_batch_equals_models_tiled_alone(hip, oracle):
    """N = H*W/8 = 51200 at 640^2 gets the tiled shape alone; the batch runs it staged."""
    _steps_equal_models(oracle, 2, 640, 640, 640 * 640 // 8, 64, 2)


# ---------------------------------------------------------------- the cell phase

def _cell_batch_inputs(B, H, W, seed):
    r = np.random.default_rng(seed)
    f = lambda *s: (r.random((B, H, W) + s) * 2.0).astype(np.float32)
    g = dict(layers=f(2), uplift=f(), rainfall=f(), waterFlux=f(), massFlux=f() * 1e-3,
             velocityFlux=f(2) - 1.0, debrisFlux=f() * 1e-3, debrisVelocityFlux=f(2) - 1.0,
             albedoBedrock=f(3) * 0.65, albedoSurface=f(3) * 0.65, albedoFluvial=f(3) * 2e-3,
             albedoDebris=f(3) * 1e-3)
    g["layers"][..., 1] *= 0.1
    for name in ("albedoFluvial", "albedoDebris"):   # cells without colour flux take the surface colour
        g[name][r.random((B, H, W)) < 0.2] = 0.0
    return g


@pytest.mark.parametrize("B,H,W", [(3, 33, 47), (4, 96, 80), (2, 256, 256), (5, 8, 4), (3, 20, 30)])
@pytest.mark.parametrize("keep", [False, True])
def test_coloured_cell_phase_bit_exact(hip, oracle, B, H, W, keep):
    from soillib_amd import silt
    from soillib_amd.erosion import ErosionModel
    p = _param(oracle, 64)
    scale = (20.0 / H, 20.0 / W, 4.0)
    g = _cell_batch_inputs(B, H, W, B * H + W)
    bt = _batch(B, H, W, scale, p, 0, [0] * B, g)
    for name in FLUX + ("albedoFluvial", "albedoDebris"):
        silt.set(getattr(bt, name), to_gpu(g[name]))
    bt.cells_fused(keep_flux=keep)
    for b in range(B):
        m = ErosionModel(H, W, scale, p, 1, seed=0, colour=True)
        m.set_layers(to_gpu(g["layers"][b]))
        for name in ("rainfall", "uplift", "albedoBedrock", "albedoSurface", "albedoFluvial", "albedoDebris") + FLUX:
            silt.set(getattr(m, name), to_gpu(g[name][b]))
        m.cells_fused(keep_flux=keep)
        got = bt.model_planes(b)
        for name in ("layers_next", "height", "waterHeight", "mass", "velocity", "debris", "debrisVelocity") + \
                FLUX + COLOUR_OUT:
            assert_bit_equal(got[name], to_np(getattr(m, name)), "model %d: %s" % (b, name))
        assert_bit_equal(got["albedoBedrock"], g["albedoBedrock"][b], "model %d: albedoBedrock is read only" % b)
        if keep:
            assert_bit_equal(got["massFlux"], g["massFlux"][b], "kept flux")


# ---------------------------------------------------------------- trajectories

@pytest.fixture
def retire_off(hip):
    from soillib_amd import soil
    before = soil.debris_retire()
    soil.debris_retire(0)
    yield
    soil.debris_retire(before)


@pytest.mark.parametrize("B,H,W,N", [(3, 40, 52, 600), (4, 96, 80, 4096), (2, 640, 640, 51200)])
def test_coloured_same_trajectories(hip, oracle, retire_off, B, H, W, N):
    """After one particle phase from identical fields the device step counter holds the sum of the single
    coloured models' counts exactly, and the physics batch's count (retirement off: the tiled single model
    walks every debris walker to the end)."""
    from soillib_amd import soil
    p = _param(oracle, 96)
    scale = (20.0 / H, 20.0 / W, 4.0)
    seeds = [5 + 3 * b for b in range(B)]
    inp = _inputs(oracle, B, H, W)
    bt = _batch(B, H, W, scale, p, N, seeds, inp)
    phys = _batch(B, H, W, scale, p, N, seeds, inp, colour=False)
    soil.particle_steps(reset=True)
    bt.step_index = phys.step_index = 2
    bt.particles()
    got = soil.particle_steps(reset=True)
    phys.particles()
    got_phys = soil.particle_steps(reset=True)
    want = 0
    for b in range(B):
        m = _single(b, H, W, scale, p, N, seeds[b], inp)
        m.step_index = 2
        m.seed_step()
        m.particles_pair()
        want += soil.particle_steps(reset=True)
        planes = bt.model_planes(b)
        for name in FLUX + ("albedoFluvial", "albedoDebris"):
            _close(planes[name], to_np(getattr(m, name)), "model %d: %s" % (b, name))
    assert got == want == got_phys > 0


# ---------------------------------------------------------------- the colour flux planes

def test_colour_flux_planes_are_cleared(hip, oracle):
    """Junk in albedoFluvial / albedoDebris before a step changes nothing."""
    from soillib_amd import silt
    B, H, W, N = 3, 64, 64, 2048
    p = _param(oracle, 64)
    scale = (20.0 / H, 20.0 / W, 4.0)
    seeds = [31, 32, 33]
    inp = _inputs(oracle, B, H, W)
    junk = np.random.default_rng(3).random((B, H, W, 3)).astype(np.float32) * 50.0
    # the particle phase alone leaves this step's colour flux only
    clean = _batch(B, H, W, scale, p, N, seeds, inp)
    dirty = _batch(B, H, W, scale, p, N, seeds, inp)
    silt.set(dirty.albedoFluvial, to_gpu(junk))
    silt.set(dirty.albedoDebris, to_gpu(junk[::-1].copy()))
    clean.particles()
    dirty.particles()
    for b in range(B):
        for name in ("albedoFluvial", "albedoDebris"):
            want = clean.model_plane(name, b)
            assert want.any(), "model %d: no %s" % (b, name)
            _close(dirty.model_plane(name, b), want, "model %d: %s" % (b, name))
    # whole steps
    clean = _batch(B, H, W, scale, p, N, seeds, inp)
    dirty = _batch(B, H, W, scale, p, N, seeds, inp)
    for k in range(2):
        silt.set(dirty.albedoFluvial, to_gpu(junk))
        silt.set(dirty.albedoDebris, to_gpu(junk[::-1].copy()))
        clean.step()
        dirty.step()
    for b in range(B):
        pc, pd = clean.model_planes(b), dirty.model_planes(b)
        for name in OUT + COLOUR_OUT:
            _close(pd[name], pc[name], "model %d: %s" % (b, name))


# ---------------------------------------------------------------- isolation

def test_non_finite_walkers_and_colours_stay_in_their_model(hip, oracle):
    from soillib_amd import silt
    B, H, W, N = 4, 64, 72, 2048
    p = _param(oracle, 64)
    scale = (20.0 / H, 20.0 / W, 4.0)
    seeds = [21, 22, 23, 24]
    inp = _inputs(oracle, B, H, W)
    # a velocity everywhere: no walker starts at rest on a pit cell (the reference's own NaN walkers), so that
    # only model 1's NaN cells make NaN walkers
    vel = np.ones((B, H, W, 2), np.float32)
    vel[1, 20:36, 30:50] = np.nan        # model 1's walkers through these cells go NaN
    dvel = np.ones((B, H, W, 2), np.float32)
    surf = inp["albedoSurface"]
    surf[2, 10:30, 10:40, 0] = np.nan    # model 2's walkers spawned here carry a non-finite colour
    surf[2, 40:50, 20:60, 2] = np.inf
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
        for name in OUT + COLOUR_OUT:
            want = to_np(getattr(m, name))
            g = got[name]
            assert np.array_equal(np.isfinite(g), np.isfinite(want)), "model %d: %s non-finite cells differ" % (b, name)
            if b in (0, 3):
                assert np.isfinite(g).all(), "model %d: %s" % (b, name)
            fin = np.isfinite(want)
            _close(g[fin], want[fin], "model %d: %s" % (b, name))
        if b == 1:
            assert np.isnan(got["waterHeight"][0, 0]), "model 1's NaN walkers did not reach its cell (0, 0)"
        if b == 2:
            assert np.isfinite(got["layers"]).all(), "model 2: colour reached the physics"
            assert not np.isfinite(got["albedoFluvial"]).all(), "model 2: no walker carried a non-finite colour"


# ---------------------------------------------------------------- physics

def test_physics_unaffected_by_colour(hip, oracle):
    B, H, W, N = 3, 96, 80, 2048
    p = _param(oracle, 96)
    scale = (20.0 / H, 20.0 / W, 4.0)
    seeds = [41, 42, 43]
    inp = _inputs(oracle, B, H, W)
    col = _batch(B, H, W, scale, p, N, seeds, inp)
    phys = _batch(B, H, W, scale, p, N, seeds, inp, colour=False)
    assert not hasattr(phys, "albedoSurface")
    for _ in range(3):
        col.step()
        phys.step()
    for b in range(B):
        pc, pp = col.model_planes(b), phys.model_planes(b)
        assert set(pc) == set(pp) | set(col.PLANES_3)
        for name in OUT:
            _close(pc[name], pp[name], "model %d: %s" % (b, name))


# ---------------------------------------------------------------- plumbing

def _run_and_compare(oracle, B, H, W, N, steps):
    p = _param(oracle, 48)
    scale = (20.0 / H, 20.0 / W, 4.0)
    seeds = [101 + b for b in range(B)]
    inp = _inputs(oracle, B, H, W)
    bt = _batch(B, H, W, scale, p, N, seeds, inp)
    for _ in range(steps):
        bt.step()
    models = []
    for b in range(B):
        m = _single(b, H, W, scale, p, N, seeds[b], inp)
        for _ in range(steps):
            m.step()
        models.append(m)
    _compare_models(bt, models)


def test_coloured_batch_on_another_stream(hip, oracle):
    import torch
    from soillib_amd import _abi
    s = torch.cuda.Stream()
    _abi.set_stream(s.cuda_stream)
    try:
        _run_and_compare(oracle, 3, 48, 64, 1200, 2)
        s.synchronize()
    finally:
        _abi.set_stream(0)


def test_small_coloured_batch_after_a_larger_one(hip, oracle):
    """The workspace and the seed staging are sized by the first, larger batch and reused by the second."""
    _run_and_compare(oracle, 6, 96, 96, 4096, 1)
    _run_and_compare(oracle, 2, 40, 36, 700, 2)
    _run_and_compare(oracle, 3, 64, 64, 2048, 1)


def test_coloured_phases_one_by_one_equal_step(hip, oracle):
    """particles(), cells_fused(), swap over several steps equals step() (step_index carried on)."""
    B, H, W, N = 3, 48, 56, 1500
    p = _param(oracle, 48)
    scale = (20.0 / H, 20.0 / W, 4.0)
    seeds = [7, 8, 9]
    inp = _inputs(oracle, B, H, W)
    a = _batch(B, H, W, scale, p, N, seeds, inp)
    c = _batch(B, H, W, scale, p, N, seeds, inp)
    for k in range(3):
        a.step()
        c.particles()
        c.cells_fused()
        c.swap_layers()
        c.step_index += 1
    assert a.step_index == c.step_index == 3
    for b in range(B):
        pa, pc = a.model_planes(b), c.model_planes(b)
        for name in OUT + COLOUR_OUT:
            _close(pc[name], pa[name], "model %d: %s" % (b, name))


def test_set_colour_checks_its_arguments(hip, oracle):
    from soillib_amd import silt
    p = _param(oracle, 32)
    inp = _inputs(oracle, 2, 16, 16)
    bt = _batch(2, 16, 16, (1.0, 1.0, 1.0), p, 64, [1, 2], inp)
    with pytest.raises(ValueError, match="16, 16, 3"):
        bt.set_colour("albedoSurface", to_gpu(inp["albedoSurface"][0]))
    with pytest.raises(ValueError, match="colour plane"):
        bt.set_colour("layers", to_gpu(inp["albedoSurface"]))
    phys = _batch(2, 16, 16, (1.0, 1.0, 1.0), p, 64, [1, 2], inp, colour=False)
    with pytest.raises(ValueError, match="colour=False"):
        phys.set_colour("albedoSurface", to_gpu(inp["albedoSurface"]))
    assert np.array_equal(bt.model_plane("albedoSurface", 1), inp["albedoSurface"][1])


def test_coloured_invalid_arguments_are_refused(hip, oracle):
    from soillib_amd import _abi
    lib = _abi.lib()
    p = _param(oracle, 32)
    bt = _batch(2, 16, 16, (1.0, 1.0, 1.0), p, 64, [1, 2], _inputs(oracle, 2, 16, 16))
    planes, colour = bt._planes(), bt._colour()
    seeds = (C.c_uint64 * 2)(1, 2)
    scale = _abi.vec((1.0, 1.0, 1.0), 3)
    step, parts, cells = (lib.soil_erode_step_batch_colour, lib.soil_particles_batch_colour,
                          lib.soil_erode_cells_fused_batch_colour)
    # a null colour struct, then each colour plane null in turn
    holes = [None]
    for field in _abi.COLOUR_PLANES:
        c = _abi.ColourPlanes()
        for f in _abi.COLOUR_PLANES:
            setattr(c, f, None if f == field else getattr(colour, f))
        holes.append(C.byref(c))
    for cp in holes:
        for fn in (step, parts):
            assert fn(C.byref(planes), cp, 2, 16, 16, 64, seeds, 0, scale, p._ref(),
                      None) == _abi.SOIL_ERR_INVALID_ARGUMENT, fn.__name__
            assert "colour plane" in _abi.last_error()
        assert cells(C.byref(planes), cp, 2, 16, 16, scale, p._ref(), 0, None) == _abi.SOIL_ERR_INVALID_ARGUMENT
        assert "colour plane" in _abi.last_error()
    # what the physics batch refuses: B < 1, empty grids, null seeds with N > 0, overflowing sizes
    bad = [(0, 16, 16, 64, seeds), (-1, 16, 16, 64, seeds), (2, 0, 16, 64, seeds), (2, 16, 16, -1, seeds),
           (2, 16, 16, 64, None), (1 << 40, 1 << 20, 16, 64, seeds)]
    for B, H, W, N, s in bad:
        for fn in (step, parts):
            rc = fn(C.byref(planes), C.byref(colour), B, H, W, N, s, 0, scale, p._ref(), None)
            assert rc == _abi.SOIL_ERR_INVALID_ARGUMENT, (fn.__name__, B, H, W, N)
            assert _abi.last_error()
    for B, H, W in [(0, 16, 16), (2, 0, 16), (1 << 40, 1 << 20, 16)]:
        assert cells(C.byref(planes), C.byref(colour), B, H, W, scale, p._ref(), 0,
                     None) == _abi.SOIL_ERR_INVALID_ARGUMENT, (B, H, W)
    empty = _abi.ErosionPlanes()
    assert step(C.byref(empty), C.byref(colour), 2, 16, 16, 64, seeds, 0, scale, p._ref(),
                None) == _abi.SOIL_ERR_INVALID_ARGUMENT
    # N == 0 needs no seeds
    assert parts(C.byref(planes), C.byref(colour), 2, 16, 16, 0, None, 0, scale, p._ref(), None) == _abi.SOIL_OK
    bt.step()   # the batch itself still steps
    _abi.check(lib.soil_stream_synchronize(None))
