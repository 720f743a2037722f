"""A parameter sweep: a batch of independent models stepped together, model b with a param_t of its own
(include/soil_hip.h: soil_erode_step_batch_params, soil_particles_batch_params, soil_erode_cells_fused_batch_params;
ErosionBatch(..., [params], ...)) against the same models stepped one at a time through ErosionModel with
param = params[b] and seed = seeds[b] (those paths are checked against the oracle elsewhere):

  * whole steps, every output plane of every model, in the direct, staged and (alone: tiled) shapes, physics
    and colour, under parameter sets drawn at random (maxage across 16..160, exitSlope, force on some models);
  * one terrain, rainfall, uplift and seed in every model: the models differ, and each equals its own model;
  * the same trajectories: the step counter equals the single models' sum exactly;
  * the cell phase bit for bit, with and without SOIL_CELLS_KEEP_FLUX, vector and scalar width, with colour;
  * B = 65537 (two launches per kernel);
  * B equal params: the uniform batch's cell phase bit for bit and its step counts;
  * an edited param takes effect at the next step, in its own model only;
  * refused arguments.
"""
import ctypes as C

import numpy as np
import pytest

from util import assert_bit_equal, copy_param, product_param, script_param, terrain, to_gpu, to_np

pytestmark = pytest.mark.gpu

OUT = ("layers", "height", "waterHeight", "mass", "velocity", "debris", "debrisVelocity")
FLUX = ("waterFlux", "massFlux", "velocityFlux", "debrisFlux", "debrisVelocityFlux")
COLOUR_OUT = ("albedoSurface", "albedoFluvial", "albedoDebris")
# drawn log-uniform around the script's values (test_gpu_parity.test_transport_random_parameter_sets)
JITTER = ("gravity", "evapRate", "viscosityWater", "bedShearWater", "frictionFactor", "suspensionRateFluvial",
          "depositionRateFluvial", "fluvialExponent", "exitSlope", "critSlopeBedrock", "critSlopeSediment",
          "landslideRateDebris", "suspensionRateDebris", "depositionRateDebris", "yieldStress", "viscosityDebris",
          "bedShearDebris", "uplift", "rainfall")


def _base(oracle):
    return product_param(script_param(oracle.default_param()))


def _sweep_params(oracle, B, seed):
    """B parameter sets: every JITTER field times a factor in [1/3, 3], maxage from 16 to 160 (both ends taken),
    a non-zero force on every other model."""
    from soillib_amd import soil
    r = np.random.default_rng(7000 + seed)
    base = _base(oracle)
    out = []
    for b in range(B):
        p = soil.param_t()
        copy_param(base._c, p._c)
        for name in JITTER:
            setattr(p, name, float(getattr(p, name) * np.exp(r.uniform(np.log(1 / 3), np.log(3)))))
        p.maxage = 16 if b == 0 else 160 if b == B - 1 else int(r.integers(16, 161))
        if b % 2:
            p.force = [float(r.normal(0, 0.3)), float(r.normal(0, 0.3))]
        out.append(p)
    return out


def _inputs(oracle, B, H, W, colour=False, same=False):
    """Per model its own terrain, rainfall and uplift (with colour: bedrock and surface colours), or with `same`
    model 0's in every model."""
    r = np.random.default_rng(3000 * B + H + W)
    n = 1 if same else B
    layers = np.stack([terrain(oracle, H, W, seed=3.0 + 5.0 * b, sediment=0.05, rng_seed=b) for b in range(n)])
    g = dict(layers=layers, rainfall=(0.5 + r.random((n, H, W))).astype(np.float32),
             uplift=(0.5 * r.random((n, H, W))).astype(np.float32))
    if colour:
        g["albedoBedrock"] = (0.2 + 0.6 * r.random((n, H, W, 3))).astype(np.float32)
        g["albedoSurface"] = (0.1 + 0.5 * r.random((n, H, W, 3))).astype(np.float32)
    if same:
        g = {k: np.ascontiguousarray(np.broadcast_to(v, (B,) + v.shape[1:])) for k, v in g.items()}
    return g


def _batch(B, H, W, scale, params, N, seeds, inp, colour=False):
    from soillib_amd import silt
    from soillib_amd.erosion import ErosionBatch
    bt = ErosionBatch(B, H, W, scale, params, N, seeds, colour=colour)
    bt.set_layers(to_gpu(inp["layers"]))
    silt.set(bt.rainfall, to_gpu(inp["rainfall"]))
    silt.set(bt.uplift, to_gpu(inp["uplift"]))
    if colour:
        bt.set_colour("albedoBedrock", to_gpu(inp["albedoBedrock"]))
        bt.set_colour("albedoSurface", to_gpu(inp["albedoSurface"]))
    return bt


def _single(b, H, W, scale, p, N, seed, inp, colour=False):
    from soillib_amd import silt
    from soillib_amd.erosion import ErosionModel
    m = ErosionModel(H, W, scale, p, N, seed=seed, colour=colour)
    m.set_layers(to_gpu(inp["layers"][b]))
    for name in ("rainfall", "uplift") + (("albedoBedrock", "albedoSurface") if colour else ()):
        silt.set(getattr(m, name), to_gpu(inp[name][b]))
    return m


def _close(got, want, what):
    """The batch tests' tolerance (test_gpu_erosion_batch_colour._close)."""
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5 * (np.nanmax(np.abs(want)) + 1e-30), err_msg=what)


def _steps_equal_models(oracle, B, H, W, N, steps, colour=False, seed=0):
    params = _sweep_params(oracle, B, seed)
    scale = (20.0 / H, 20.0 / W, 4.0)
    seeds = [13 + 7 * b for b in range(B)]
    inp = _inputs(oracle, B, H, W, colour)
    bt = _batch(B, H, W, scale, params, N, seeds, inp, colour)
    assert bt.params == params and bt.param is None
    for _ in range(steps):
        bt.step()
    assert bt.step_index == steps
    for b in range(B):
        m = _single(b, H, W, scale, params[b], N, seeds[b], inp, colour)
        for _ in range(steps):
            m.step()
        got = bt.model_planes(b)
        for name in OUT + (COLOUR_OUT if colour else ()):
            _close(got[name], to_np(getattr(m, name)), "model %d: %s" % (b, name))
        for name in FLUX:   # zeroed on exit
            assert not got[name].any(), "model %d: %s not zeroed" % (b, name)
        assert np.isfinite(got["layers"]).all(), "model %d" % b


@pytest.mark.parametrize("B,H,W,N,steps", [
    (3, 33, 47, 700, 3),            # direct shape (N < 1024), odd H x W: the scalar cell kernel
    (4, 96, 80, 2048, 3),           # staged shape
    (3, 48, 160, 1500, 2),          # non-square, staged
])
def test_sweep_equals_models(hip, oracle, B, H, W, N, steps):
    _steps_equal_models(oracle, B, H, W, N, steps, seed=B * H)


def test_sweep_equals_models_at_the_example_shape(hip, oracle):
    """example/erosion_gpu.py's 256^2 and 8192 particles: eight models, two steps."""
    _steps_equal_models(oracle, 8, 256, 256, 8192, 2, seed=1)


def test_sweep_equals_models_tiled_alone(hip, oracle):
    """N = H*W/8 = 51200 at 640^2 gets the tiled shape alone; the sweep runs it staged."""
    _steps_equal_models(oracle, 2, 640, 640, 640 * 640 // 8, 2, seed=2)


@pytest.mark.parametrize("B,H,W,N", [(3, 33, 47, 700), (4, 96, 80, 2048)])
def test_coloured_sweep_equals_models(hip, oracle, B, H, W, N):
    _steps_equal_models(oracle, B, H, W, N, 2, colour=True, seed=3 + B)


def test_one_terrain_and_seed_different_params(hip, oracle):
    """Every model starts from model 0's terrain, rainfall, uplift and seed: only the params tell them apart.
    A sweep that stepped every model with params[0] fails here."""
    B, H, W, N = 4, 64, 72, 2048
    params = _sweep_params(oracle, B, 11)
    scale = (20.0 / H, 20.0 / W, 4.0)
    seeds = [99] * B
    inp = _inputs(oracle, B, H, W, same=True)
    bt = _batch(B, H, W, scale, params, N, seeds, inp)
    for _ in range(2):
        bt.step()
    got = [bt.model_planes(b) for b in range(B)]
    for a in range(B):
        for b in range(a + 1, B):
            assert not np.array_equal(got[a]["layers"], got[b]["layers"]), "models %d and %d are equal" % (a, b)
    for b in range(B):
        m = _single(b, H, W, scale, params[b], N, seeds[b], inp)
        for _ in range(2):
            m.step()
        for name in OUT:
            _close(got[b][name], to_np(getattr(m, name)), "model %d: %s" % (b, name))


# ---------------------------------------------------------------- trajectories

@pytest.fixture
def retire_off(hip):
    from soillib_amd import soil
    before = soil.debris_retire()
    soil.debris_retire(0)
    yield
    soil.debris_retire(before)


@pytest.mark.parametrize("B,H,W,N", [(3, 40, 52, 600), (4, 96, 80, 4096)])
def test_sweep_same_trajectories(hip, oracle, retire_off, B, H, W, N):
    """After one particle phase from identical fields the device step counter holds the exact sum of the single
    models' counts, each with its own maxage."""
    from soillib_amd import soil
    params = _sweep_params(oracle, B, 20 + B)
    scale = (20.0 / H, 20.0 / W, 4.0)
    seeds = [5 + 3 * b for b in range(B)]
    inp = _inputs(oracle, B, H, W)
    bt = _batch(B, H, W, scale, params, N, seeds, inp)
    soil.particle_steps(reset=True)
    bt.step_index = 2
    bt.particles()
    got = soil.particle_steps(reset=True)
    want = []
    for b in range(B):
        m = _single(b, H, W, scale, params[b], N, seeds[b], inp)
        m.step_index = 2
        m.seed_step()
        m.particles_pair()
        want.append(soil.particle_steps(reset=True))
        planes = bt.model_planes(b)
        for name in FLUX:
            _close(planes[name], to_np(getattr(m, name)), "model %d: %s" % (b, name))
    assert got == sum(want) > 0, (got, want)
    assert len(set(want)) == B, want   # the maxages differ: so do the counts


# ---------------------------------------------------------------- the cell phase

def _cell_inputs(B, H, W, seed):
    r = np.random.default_rng(seed)
    f = lambda *s: (r.random((B, H, W) + s) * 2.0).astype(np.float32)
    g = dict(layers=f(2), uplift=f(), rainfall=f(), waterFlux=f(), massFlux=f() * 1e-3,
             velocityFlux=f(2) - 1.0, debrisFlux=f() * 1e-3, debrisVelocityFlux=f(2) - 1.0,
             albedoBedrock=f(3) * 0.65, albedoSurface=f(3) * 0.65, albedoFluvial=f(3) * 2e-3,
             albedoDebris=f(3) * 1e-3)
    g["layers"][..., 1] *= 0.1
    return g


def _cells_batch(B, H, W, scale, params, g, keep, colour):
    from soillib_amd import silt
    bt = _batch(B, H, W, scale, params, 0, [0] * B, g, colour)
    for name in FLUX + (("albedoFluvial", "albedoDebris") if colour else ()):
        silt.set(getattr(bt, name), to_gpu(g[name]))
    bt.cells_fused(keep_flux=keep)
    return bt


CELL_PLANES = ("layers_next", "height", "waterHeight", "mass", "velocity", "debris", "debrisVelocity") + FLUX


@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("B,H,W", [(3, 33, 47), (4, 96, 80), (2, 256, 256), (3, 20, 30)])
@pytest.mark.parametrize("keep", [False, True])
def test_sweep_cell_phase_bit_exact(hip, oracle, B, H, W, keep, colour):
    from soillib_amd import silt
    from soillib_amd.erosion import ErosionModel
    params = _sweep_params(oracle, B, 40 + B)
    scale = (20.0 / H, 20.0 / W, 4.0)
    g = _cell_inputs(B, H, W, B * H + W)
    bt = _cells_batch(B, H, W, scale, params, g, keep, colour)
    for b in range(B):
        m = ErosionModel(H, W, scale, params[b], 1, seed=0, colour=colour)
        m.set_layers(to_gpu(g["layers"][b]))
        names = ("rainfall", "uplift") + FLUX
        if colour:
            names += ("albedoBedrock", "albedoSurface", "albedoFluvial", "albedoDebris")
        for name in names:
            silt.set(getattr(m, name), to_gpu(g[name][b]))
        m.cells_fused(keep_flux=keep)
        got = bt.model_planes(b)
        for name in CELL_PLANES + (COLOUR_OUT if colour else ()):
            assert_bit_equal(got[name], to_np(getattr(m, name)), "model %d: %s" % (b, name))
        if keep:
            assert_bit_equal(got["massFlux"], g["massFlux"][b], "kept flux")


# ---------------------------------------------------------------- equal params

@pytest.mark.parametrize("B,H,W,N", [(3, 33, 47, 700), (4, 96, 80, 4096)])
def test_equal_params_equal_the_uniform_batch(hip, oracle, B, H, W, N):
    """A sweep of B equal params: the cell phase is the uniform batch's bit for bit, and one particle phase
    walks as many steps."""
    from soillib_amd import soil
    base = _base(oracle)
    base.maxage = 96
    params = [base] * B
    scale = (20.0 / H, 20.0 / W, 4.0)
    g = _cell_inputs(B, H, W, 5 + B)
    for keep in (False, True):
        sweep = _cells_batch(B, H, W, scale, params, g, keep, False)
        uniform = _cells_batch(B, H, W, scale, base, g, keep, False)
        assert sweep.params is not None and uniform.params is None
        for b in range(B):
            ps, pu = sweep.model_planes(b), uniform.model_planes(b)
            for name in CELL_PLANES:
                assert_bit_equal(ps[name], pu[name], "model %d: %s (keep_flux=%s)" % (b, name, keep))
    seeds = [61 + b for b in range(B)]
    inp = _inputs(oracle, B, H, W)
    counts = []
    for p in (params, base):
        bt = _batch(B, H, W, scale, p, N, seeds, inp)
        soil.particle_steps(reset=True)
        bt.particles()
        counts.append(soil.particle_steps(reset=True))
    assert counts[0] == counts[1] > 0, counts


# ---------------------------------------------------------------- many models

def test_65537_models(hip, oracle):
    """B = 65537 models of 4 x 4: two launches per kernel (grid.y <= 65535); models 0, 65534, 65535 and 65536
    (the second launch's first and second) each equal their single model."""
    from soillib_amd import soil
    B, H, W, N = 65537, 4, 4, 16
    base = _base(oracle)
    params = []
    for b in range(B):
        p = soil.param_t()
        copy_param(base._c, p._c)
        p.maxage = 16 + b % 145
        p.evapRate = base.evapRate * (1.0 + (b % 7) * 0.5)
        p.exitSlope = base.exitSlope * (0.5 + (b % 5) * 0.25)
        params.append(p)
    scale = (1.0, 1.0, 4.0)
    r = np.random.default_rng(65537)
    layers = np.zeros((B, H, W, 2), np.float32)
    layers[..., 0] = r.random((B, H, W)) * 2.0
    layers[..., 1] = r.random((B, H, W)) * 0.05
    inp = dict(layers=layers, rainfall=(0.5 + r.random((B, H, W))).astype(np.float32),
               uplift=(0.5 * r.random((B, H, W))).astype(np.float32))
    seeds = [3 * b + 1 for b in range(B)]
    bt = _batch(B, H, W, scale, params, N, seeds, inp)
    for _ in range(2):
        bt.step()
    for b in (0, 65534, 65535, 65536):
        m = _single(b, H, W, scale, params[b], N, seeds[b], inp)
        for _ in range(2):
            m.step()
        got = bt.model_planes(b)
        for name in OUT:
            _close(got[name], to_np(getattr(m, name)), "model %d: %s" % (b, name))


# ---------------------------------------------------------------- edits between steps

def test_an_edited_param_changes_its_own_model_from_the_next_step(hip, oracle):
    B, H, W, N = 3, 48, 56, 1500
    scale = (20.0 / H, 20.0 / W, 4.0)
    seeds = [7, 8, 9]
    inp = _inputs(oracle, B, H, W)
    params = _sweep_params(oracle, B, 50)
    ref = _sweep_params(oracle, B, 50)      # the same values, never edited
    edited = _batch(B, H, W, scale, params, N, seeds, inp)
    plain = _batch(B, H, W, scale, ref, N, seeds, inp)
    edited.step()
    plain.step()
    old = _sweep_params(oracle, B, 50)[1]
    params[1].evapRate = params[1].evapRate * 20.0
    params[1].suspensionRateFluvial = params[1].suspensionRateFluvial * 5.0
    params[1].maxage = 32
    for _ in range(2):
        edited.step()
        plain.step()
    for b in (0, 2):
        pe, pp = edited.model_planes(b), plain.model_planes(b)
        for name in OUT:
            _close(pe[name], pp[name], "model %d: %s" % (b, name))
    # model 1: one step with its old params, then two with the edited ones
    m = _single(1, H, W, scale, old, N, seeds[1], inp)
    m.step()
    m.param = params[1]
    m.step()
    m.step()
    got = edited.model_planes(1)
    for name in OUT:
        _close(got[name], to_np(getattr(m, name)), "model 1: %s" % name)
    assert not np.allclose(got["layers"], plain.model_plane("layers", 1), rtol=1e-4), "the edit changed nothing"


# ---------------------------------------------------------------- refusals

def test_sweep_invalid_arguments_are_refused(hip, oracle):
    from soillib_amd import _abi
    lib = _abi.lib()
    params = _sweep_params(oracle, 2, 60)
    bt = _batch(2, 16, 16, (1.0, 1.0, 1.0), params, 64, [1, 2], _inputs(oracle, 2, 16, 16, colour=True),
                colour=True)
    planes, colour = bt._planes(), bt._colour()
    pa = bt._params()
    seeds = (C.c_uint64 * 2)(1, 2)
    scale = _abi.vec((1.0, 1.0, 1.0), 3)
    step, parts, cells = (lib.soil_erode_step_batch_params, lib.soil_particles_batch_params,
                          lib.soil_erode_cells_fused_batch_params)
    # a NULL params
    for fn in (step, parts):
        assert fn(C.byref(planes), None, 2, 16, 16, 64, seeds, 0, scale, None, None) == _abi.SOIL_ERR_INVALID_ARGUMENT
        assert "null argument" in _abi.last_error()
    assert cells(C.byref(planes), None, 2, 16, 16, scale, None, 0, None) == _abi.SOIL_ERR_INVALID_ARGUMENT
    assert "null argument" in _abi.last_error()
    # a colour struct with one plane missing, each in turn
    for field in _abi.COLOUR_PLANES:
        c = _abi.ColourPlanes()
        for f in _abi.COLOUR_PLANES:
            setattr(c, f, None if f == field else getattr(colour, f))
        for fn in (step, parts):
            assert fn(C.byref(planes), C.byref(c), 2, 16, 16, 64, seeds, 0, scale, pa,
                      None) == _abi.SOIL_ERR_INVALID_ARGUMENT, fn.__name__
            assert "colour plane" in _abi.last_error()
        assert cells(C.byref(planes), C.byref(c), 2, 16, 16, scale, pa, 0, None) == _abi.SOIL_ERR_INVALID_ARGUMENT
        assert "colour plane" in _abi.last_error()
    # check_batch's sizes: B < 1, empty grids, N < 0, null seeds with N > 0, overflowing sizes
    bad = [(0, 16, 16, 64, seeds), (-1, 16, 16, 64, seeds), (2, 0, 16, 64, seeds), (2, 16, 16, -1, seeds),
           (2, 16, 16, 64, None), (1 << 40, 1 << 20, 16, 64, seeds)]
    for B, H, W, N, s in bad:
        for fn in (step, parts):
            for col in (None, C.byref(colour)):
                rc = fn(C.byref(planes), col, B, H, W, N, s, 0, scale, pa, None)
                assert rc == _abi.SOIL_ERR_INVALID_ARGUMENT, (fn.__name__, B, H, W, N)
                assert _abi.last_error()
    for B, H, W in [(0, 16, 16), (2, 0, 16), (1 << 40, 1 << 20, 16)]:
        assert cells(C.byref(planes), C.byref(colour), B, H, W, scale, pa, 0,
                     None) == _abi.SOIL_ERR_INVALID_ARGUMENT, (B, H, W)
    empty = _abi.ErosionPlanes()
    assert step(C.byref(empty), None, 2, 16, 16, 64, seeds, 0, scale, pa, None) == _abi.SOIL_ERR_INVALID_ARGUMENT
    # N == 0 needs no seeds
    assert parts(C.byref(planes), C.byref(colour), 2, 16, 16, 0, None, 0, scale, pa, None) == _abi.SOIL_OK
    assert parts(C.byref(planes), None, 2, 16, 16, 0, None, 0, scale, pa, None) == _abi.SOIL_OK
    bt.step()   # the sweep itself still steps
    _abi.check(lib.soil_stream_synchronize(None))
