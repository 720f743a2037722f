"""A batch of different models: B whole-grid models of one (H, W) stepped together, model b with its own param,
scale, walker count, seed and step index (include/soil_hip.h: soil_erode_step_batch_models,
soil_particles_batch_models, soil_erode_cells_fused_batch_models; ErosionBatch with per-model scales or walker
counts, ErosionBatch.from_models / to_models) against the same models stepped one at a time through ErosionModel
(those paths are checked against the oracle elsewhere):

  * three whole steps, every output plane of every model, direct and staged shapes, N_b across 1024 and N_b = 0
    (the cell phase alone), odd and non-square grids, physics and colour, under jittered params and scales;
  * the same trajectories: the step counter after the first step equals the single models' sum exactly;
  * models that took different numbers of steps, continued as a batch and handed back;
  * the cell phase bit for bit, with and without SOIL_CELLS_KEEP_FLUX, vector and scalar width, with colour;
  * B equal records: the sweep's and the uniform batch's cell phase bit for bit and their step counts;
  * B = 65537 (two launches per kernel);
  * refused arguments.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_erosion_batch_params import (CELL_PLANES, COLOUR_OUT, FLUX, OUT, _base, _batch, _cell_inputs, _close,
                                           _inputs, _single, _sweep_params)
from util import assert_bit_equal, copy_param, to_gpu, to_np

pytestmark = pytest.mark.gpu


@pytest.fixture
def retire_off(hip):
    """The single models walk every debris walker to the end, as a batch does: equal step counts."""
    from soillib_amd import soil
    before = soil.debris_retire()
    soil.debris_retire(0)
    yield
    soil.debris_retire(before)


def _scales(B, H, W, seed):
    """B scales: sx, sy and sz each times a factor in [1/2, 2] around (20/H, 20/W, 4)."""
    r = np.random.default_rng(9000 + seed)
    f = np.exp(r.uniform(np.log(0.5), np.log(2.0), (B, 3)))
    return [[float(20.0 / H * f[b, 0]), float(20.0 / W * f[b, 1]), float(4.0 * f[b, 2])] for b in range(B)]


def _cells_only(m, colour):
    """What a model with no walkers steps: the coloured step's cleared colour flux, then the cell phase."""
    from soillib_amd import silt
    if colour:
        silt.set(m.albedoFluvial, 0.0)
        silt.set(m.albedoDebris, 0.0)
    m.cells_fused()
    m.swap_layers()
    m.step_index += 1


def _mixed_equals_models(oracle, B, H, W, Ns, colour, seed, steps=3):
    from soillib_amd import soil
    params = _sweep_params(oracle, B, seed)
    scales = _scales(B, H, W, seed)
    seeds = [17 + 5 * b for b in range(B)]
    inp = _inputs(oracle, B, H, W, colour)
    bt = _batch(B, H, W, scales, params, Ns, seeds, inp, colour)
    assert bt.scales == scales and bt.scale is None and bt.Ns == list(Ns) and bt.N is None
    assert bt._per_model()
    soil.particle_steps(reset=True)
    bt.step()
    got_steps = soil.particle_steps(reset=True)
    for _ in range(steps - 1):
        bt.step()
    assert bt.step_index == steps
    want_steps = 0
    for b in range(B):
        m = _single(b, H, W, scales[b], params[b], max(Ns[b], 1), seeds[b], inp, colour)
        for k in range(steps):
            if k == 0:
                soil.particle_steps(reset=True)
            if Ns[b] == 0:
                _cells_only(m, colour)
            else:
                m.step()
            if k == 0:
                want_steps += soil.particle_steps(reset=True)
        got = bt.model_planes(b)
        for name in OUT + (COLOUR_OUT if colour else ()):
            _close(got[name], to_np(getattr(m, name)), "model %d (N %d): %s" % (b, Ns[b], name))
        for name in FLUX:   # zeroed on exit
            assert not got[name].any(), "model %d: %s not zeroed" % (b, name)
        assert np.isfinite(got["layers"]).all(), "model %d" % b
    assert got_steps == want_steps > 0, (got_steps, want_steps)


@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("B,H,W,Ns", [
    (3, 40, 52, [700, 300, 1000]),                  # direct shape (max N < 1024)
    (4, 64, 72, [2048, 0, 1023, 1024]),             # staged shape, N_b across 1024 and one model without walkers
    (3, 33, 47, [900, 1500, 64]),                   # odd H x W: the scalar cell kernel
    (3, 48, 160, [1500, 3000, 500]),                # non-square
])
def test_mixed_batch_equals_models(hip, oracle, retire_off, B, H, W, Ns, colour):
    _mixed_equals_models(oracle, B, H, W, Ns, colour, seed=B * H + W + colour)


def test_mixed_batch_equals_models_at_the_example_shape(hip, oracle, retire_off):
    """example/erosion_gpu.py's 256^2: eight models, N_b from 8192 down to 1024."""
    _mixed_equals_models(oracle, 8, 256, 256, [8192 - 1024 * b for b in range(8)], False, seed=1)


# ---------------------------------------------------------------- single models in and out

def _planes_of(m):
    names = ("layers", "layers_next") + m.PLANES_1 + m.PLANES_2 + (m.PLANES_3 if m.colour else ())
    return {name: to_np(getattr(m, name)) for name in names}


@pytest.mark.parametrize("colour", [False, True])
def test_models_round_trip(hip, oracle, retire_off, colour):
    """Three models that took 2, 0 and 1 steps alone: from_models, two batch steps, to_models equal the models
    stepped twice more alone, each at its own step index; with no step in between the copies are bit for bit.
    The first batch step starts from the models' own fields: it walks exactly their walks."""
    from soillib_amd import soil
    from soillib_amd.erosion import ErosionBatch
    B, H, W = 3, 48, 56
    Ns, taken = [1500, 600, 2500], [2, 0, 1]
    params = []
    for b in range(B):
        p = _base(oracle)
        p.maxage = (64, 128, 96)[b]
        params.append(p)
    scales = _scales(B, H, W, 70)
    seeds = [31, 32, 33]
    inp = _inputs(oracle, B, H, W, colour)
    ms = [_single(b, H, W, scales[b], params[b], Ns[b], seeds[b], inp, colour) for b in range(B)]
    for m, k in zip(ms, taken):
        for _ in range(k):
            m.step()
    bt = ErosionBatch.from_models(ms)
    assert bt.first_step == taken and bt.step_index == 0 and bt.Ns == Ns and bt.seeds == seeds
    assert bt.colour == colour and bt.params == params and bt._per_model()
    # no step: the planes come back as they went in, bit for bit
    for m, back in zip(ms, bt.to_models()):
        assert back.step_index == m.step_index and back.N == m.N and back.seed == m.seed
        assert back.scale == m.scale and back.param is m.param
        want, got = _planes_of(m), _planes_of(back)
        for name in want:
            assert_bit_equal(got[name], want[name], name)
    for k in range(2):
        soil.particle_steps(reset=True)
        bt.step()
        got_steps = soil.particle_steps(reset=True)
        want_steps = 0
        for m in ms:
            m.step()
            want_steps += soil.particle_steps(reset=True)
        if k == 0:
            assert got_steps == want_steps > 0, (got_steps, want_steps)
    out = bt.to_models()
    for b, (m, back) in enumerate(zip(ms, out)):
        assert back.step_index == m.step_index == taken[b] + 2
        for name in OUT + (COLOUR_OUT if colour else ()):
            _close(to_np(getattr(back, name)), to_np(getattr(m, name)), "model %d: %s" % (b, name))
    # a model handed back steps on by itself from where the batch left it
    out[1].step()
    ms[1].step()
    _close(to_np(out[1].layers), to_np(ms[1].layers), "model 1 stepped on alone")


# ---------------------------------------------------------------- the cell phase

def _cells_batch(B, H, W, scales, params, g, keep, colour, n=None):
    from soillib_amd import silt
    bt = _batch(B, H, W, scales, params, [0] * B if n is None else n, [0] * B, g, colour)
    for name in FLUX + (("albedoFluvial", "albedoDebris") if colour else ()):
        silt.set(getattr(bt, name), to_gpu(g[name]))
    bt.cells_fused(keep_flux=keep)
    return bt


@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("B,H,W", [(3, 33, 47), (4, 96, 80)])
@pytest.mark.parametrize("keep", [False, True])
def test_cell_phase_bit_exact(hip, oracle, B, H, W, keep, colour):
    """Model b's cell phase is soil_erode_cells_fused_ex / _colour with (scales[b], params[b]), bit for bit."""
    from soillib_amd import silt
    from soillib_amd.erosion import ErosionModel
    params = _sweep_params(oracle, B, 80 + B)
    scales = _scales(B, H, W, 80 + B)
    g = _cell_inputs(B, H, W, B * H + W + 1)
    bt = _cells_batch(B, H, W, scales, params, g, keep, colour)
    assert bt._per_model()
    for b in range(B):
        m = ErosionModel(H, W, scales[b], params[b], 1, seed=0, colour=colour)
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


# ---------------------------------------------------------------- equal records

@pytest.mark.parametrize("B,H,W,N", [(3, 33, 47, 700), (4, 96, 80, 4096)])
def test_equal_records_equal_the_sweep_and_the_uniform_batch(hip, oracle, retire_off, B, H, W, N):
    """B equal records: the cell phase is the sweep's and the uniform batch's bit for bit, and one particle phase
    walks as many steps as either."""
    from soillib_amd import soil
    base = _base(oracle)
    base.maxage = 96
    scale = [20.0 / H, 20.0 / W, 4.0]
    kinds = (([scale] * B, [base] * B, [N] * B), (scale, [base] * B, N), (scale, base, N))
    g = _cell_inputs(B, H, W, 15 + B)
    for keep in (False, True):
        runs = [_cells_batch(B, H, W, s, p, g, keep, False, n) for s, p, n in kinds]
        assert runs[0]._per_model() and not runs[1]._per_model() and runs[1].params is not None
        for b in range(B):
            want = runs[2].model_planes(b)
            for bt in runs[:2]:
                got = bt.model_planes(b)
                for name in CELL_PLANES:
                    assert_bit_equal(got[name], want[name], "model %d: %s (keep_flux=%s)" % (b, name, keep))
    seeds = [61 + b for b in range(B)]
    inp = _inputs(oracle, B, H, W)
    counts = []
    for s, p, n in kinds:
        bt = _batch(B, H, W, s, p, n, seeds, inp)
        bt.step_index = 3
        soil.particle_steps(reset=True)
        bt.particles()
        counts.append(soil.particle_steps(reset=True))
    assert counts[0] == counts[1] == counts[2] > 0, counts


# ---------------------------------------------------------------- many models

def test_65537_models(hip, oracle):
    """B = 65537 models of 4 x 4, each with its own param, scale and N: two launches per kernel (grid.y <= 65535);
    models 0, 65535 and 65536 (the second launch's first and last) each equal their single model."""
    from soillib_amd import soil
    B, H, W = 65537, 4, 4
    base = _base(oracle)
    params, scales, Ns = [], [], []
    for b in range(B):
        p = soil.param_t()
        copy_param(base._c, p._c)
        p.maxage = 16 + b % 145
        p.evapRate = base.evapRate * (1.0 + (b % 7) * 0.5)
        params.append(p)
        scales.append([1.0 + (b % 3) * 0.25, 1.0 + (b % 5) * 0.125, 4.0 * (1.0 + (b % 4) * 0.5)])
        Ns.append(8 + b % 11)
    r = np.random.default_rng(65537)
    layers = np.zeros((B, H, W, 2), np.float32)
    layers[..., 0] = r.random((B, H, W)) * 2.0
    layers[..., 1] = r.random((B, H, W)) * 0.05
    inp = dict(layers=layers, rainfall=(0.5 + r.random((B, H, W))).astype(np.float32),
               uplift=(0.5 * r.random((B, H, W))).astype(np.float32))
    seeds = [3 * b + 1 for b in range(B)]
    bt = _batch(B, H, W, scales, params, Ns, seeds, inp)
    for _ in range(2):
        bt.step()
    for b in (0, 65535, 65536):
        m = _single(b, H, W, scales[b], params[b], Ns[b], seeds[b], inp)
        for _ in range(2):
            m.step()
        got = bt.model_planes(b)
        for name in OUT:
            _close(got[name], to_np(getattr(m, name)), "model %d: %s" % (b, name))


# ---------------------------------------------------------------- refusals

def test_invalid_arguments_are_refused(hip, oracle):
    from soillib_amd import _abi
    lib = _abi.lib()
    B, H, W = 2, 16, 16
    bt = _batch(B, H, W, _scales(B, H, W, 90), _sweep_params(oracle, B, 90), [64, 32], [1, 2],
                _inputs(oracle, B, H, W, colour=True), colour=True)
    planes, colour = bt._planes(), bt._colour()
    step, parts, cells = (lib.soil_erode_step_batch_models, lib.soil_particles_batch_models,
                          lib.soil_erode_cells_fused_batch_models)
    calls = (lambda c, m: step(C.byref(planes), c, B, H, W, m, None),
             lambda c, m: parts(C.byref(planes), c, B, H, W, m, None),
             lambda c, m: cells(C.byref(planes), c, B, H, W, m, 0, None))
    for call in calls:
        for col in (None, C.byref(colour)):
            assert call(col, None) == _abi.SOIL_ERR_INVALID_ARGUMENT
            assert "null models" in _abi.last_error()
            for bad in (-1, -(1 << 40), 1 << 31, (1 << 31) + 5):
                models = bt._models()
                models[1].N = bad
                assert call(col, models) == _abi.SOIL_ERR_INVALID_ARGUMENT, bad
                assert "models[1].N" in _abi.last_error()
    # a colour struct with one plane missing, each in turn
    for field in _abi.COLOUR_PLANES:
        c = _abi.ColourPlanes()
        for f in _abi.COLOUR_PLANES:
            setattr(c, f, None if f == field else getattr(colour, f))
        for call in calls:
            assert call(C.byref(c), bt._models()) == _abi.SOIL_ERR_INVALID_ARGUMENT
            assert "colour plane" in _abi.last_error()
    # check_batch's sizes with N = max N_b
    models = bt._models()
    for b_, h_, w_ in [(0, 16, 16), (2, 0, 16)]:
        assert step(C.byref(planes), None, b_, h_, w_, models, None) == _abi.SOIL_ERR_INVALID_ARGUMENT
        assert cells(C.byref(planes), None, b_, h_, w_, models, 0, None) == _abi.SOIL_ERR_INVALID_ARGUMENT
    for fn in (step, parts):   # B x H x W x 16 bytes overflows
        assert fn(C.byref(planes), None, B, 1 << 40, 1 << 20, models, None) == _abi.SOIL_ERR_INVALID_ARGUMENT
        assert "overflow" in _abi.last_error()
    empty = _abi.ErosionPlanes()
    assert step(C.byref(empty), None, B, H, W, bt._models(), None) == _abi.SOIL_ERR_INVALID_ARGUMENT
    # every N_b == 0: nothing to walk, the colour flux planes still cleared
    zero = bt._models()
    for m in zero:
        m.N = 0
    assert parts(C.byref(planes), C.byref(colour), B, H, W, zero, None) == _abi.SOIL_OK
    assert not bt.model_plane("albedoFluvial", 1).any()
    assert step(C.byref(planes), C.byref(colour), B, H, W, zero, None) == _abi.SOIL_OK
    bt.swap_layers()
    bt.step()   # the batch itself still steps
    _abi.check(lib.soil_stream_synchronize(None))
