"""Batched erosion steps against the CPU oracle, model by model (include/soil_hip.h: soil_particles_batch[_colour],
soil_particles_batch_params, soil_particles_batch_models, soil_erode_cells_fused_batch[_colour|_params|_models];
ErosionBatch), not by way of the single model: since the two share the direct and staged particle kernels, a fault
in those shows on both sides of test_gpu_erosion_batch*.py.

Every step of every model starts from the batch's own state, so every step gets the tight bars: the oracle takes
model b's step from bt.model_planes(b) — the fluvial launch from streams (seed_b, n, (first_step_b + step_index) *
N_b), the debris launch from the same streams two draws on, every walker walked to the end as a batch walks them,
then the cell phase — and the GPU runs the phases one by one (particles, cells_fused, swap), three steps.  Bars,
every step:

  * the flux planes of every model, colour flux included: same trajectories, fp32 summation order
    (test_gpu_parity._flux_close; in a plane of deposits below 1e-6 its exemption of the deposits at the edge of the
    fp32 range taken at that edge, _flux_close_at_any_scale);
  * the step counter: the sum of the oracle's fluvial and debris steps over all models, exactly;
  * the cell phase of every model bit for bit against oracle.erode_cells (with colour: the coloured composition,
    test_gpu_colour_step._oracle_colour_cells) fed with the flux planes the GPU produced, every output plane,
    height and (with colour) albedoSurface, albedoFluvial and albedoDebris included; the flux planes zero after it;
  * the terrain of at least one model changed.

Cases: the uniform batch (with and without colour), the sweep, batches of different models (with and without
colour); the direct, staged and automatic launch shapes; odd, tiny and thin grids, B = 1 and B = 3..6; walker
counts mixed across 1024 and 0; parameter sets drawn log-uniform over decades (util.random_param) with maxage 0, 1,
2, 33 and 256 side by side; per-model scales, one strongly anisotropic; 64-bit seeds and Philox offsets that
straddle the 32-bit carry or sit near 2^42; a model whose walkers go NaN.

And the premise the batch tests lean on, for single models: the direct and staged launches under the random
parameter sets, and ErosionModel.step() at seed 2^64 - 1 and an offset past 2^32.
"""
import numpy as np
import pytest

from test_gpu_colour_step import _oracle_colour_cells
from test_gpu_erosion_batch_params import _batch, _inputs
from test_gpu_parity import _close_but_for_stray_walks, _flux_close, random_parameter_transport
from util import assert_bit_equal, log_uniform, product_param, random_param, script_param, terrain, to_gpu, to_np

pytestmark = pytest.mark.gpu

OUT = ("height", "waterHeight", "mass", "velocity", "debris", "debrisVelocity")
FLUX = ("waterFlux", "massFlux", "velocityFlux", "debrisFlux", "debrisVelocityFlux")
COLOUR_FLUX = ("albedoFluvial", "albedoDebris")
COLOUR_OUT = ("albedoSurface", "albedoFluvial", "albedoDebris")
SEEDS = (0, 2 ** 32 - 1, 2 ** 32 + 5, 2 ** 63 + 11, 2 ** 64 - 1)
CARRY = 2 ** 32 - 1


def _below(N, at=CARRY):
    """The step index whose offset step * N is the last at or below `at`: the next step's lies above.  N = 1, 255
    or 4369 (divisors of 2^32 - 1): exactly 2^32 - 1, the fluvial launch's two draws on both sides of the carry."""
    return at // max(N, 1)


class _shape:
    """`with _shape(hip, mode):` the launch shape (soil_set_particle_mode: 0 auto, 1 direct, 2 staged); auto after."""

    def __init__(self, hip, mode):
        self.hip, self.mode = hip, mode

    def __enter__(self):
        assert self.hip.soil_set_particle_mode(self.mode) == 0

    def __exit__(self, *exc):
        self.hip.soil_set_particle_mode(0)
        return False


def _flux_close_at_any_scale(got, want, what):
    """test_gpu_parity._flux_close.  Its visited-cell check exempts the deposits at the edge of the fp32 range — the
    attenuations' exponential flushes below 2^-126 on the device (soil_math.hpp: att_exp) and below e^-87 in the
    oracle, so a deposit of the order of 1e-38 times a walker's load sits on one side and not on the other — by a
    bound of 1e-30 of the plane's largest deposit.  A plane whose largest deposit is itself below 1e-6 (a random
    parameter set that hardly moves any debris) puts that bound under the edge: there the cells where one side is
    0 and the other below 1e-35 are those deposits, and are left out; every other cell takes the full bar."""
    if np.nanmax(np.abs(want), initial=0.0) >= 1e-6:
        return _flux_close(got, want, what)
    edge = ((want == 0) | (got == 0)) & (np.abs(got) <= 1e-35) & (np.abs(want) <= 1e-35)
    _flux_close(np.where(edge, 0.0, got).astype(np.float32), np.where(edge, 0.0, want).astype(np.float32), what)


# ---------------------------------------------------------------- the oracle's step of one model

def _oracle_particles(oracle, st, N, seed, offset, scale, op, colour):
    """Both launches of one model's step from state `st`: the flux planes (colour flux too) and the step count."""
    H, W = st["layers"].shape[:2]
    z = lambda *c: np.zeros((H, W) + c, np.float32)
    o = dict(waterFlux=z(), massFlux=z(), velocityFlux=z(2), debrisFlux=z(), debrisVelocityFlux=z(2))
    if colour:
        o.update(albedoFluvial=z(3), albedoDebris=z(3))
    if N == 0:
        return o, 0
    rng = oracle.rng_seed(N, seed, offset)
    surf = st["albedoSurface"].copy() if colour else None
    steps = oracle.particles_fluvial(o["waterFlux"], o["massFlux"], o["velocityFlux"], o.get("albedoFluvial"), rng,
                                     st["layers"], st["rainfall"], st["waterHeight"].copy(), st["velocity"].copy(),
                                     surf, scale, op)
    assert (rng["offset"] == offset + 2).all()   # what the batch's debris launch starts from (soil_hip.h)
    steps += oracle.particles_debris(o["debrisFlux"], o["debrisVelocityFlux"], o.get("albedoDebris"), rng,
                                     st["layers"], st["debrisVelocity"].copy(), surf, scale, op)
    return o, steps


def _oracle_cells(oracle, st, flux, scale, op, colour):
    """One model's cell phase from state `st` and the flux planes `flux` (the GPU's)."""
    args = [st["layers"], st["uplift"], st["rainfall"]] + [flux[k].copy() for k in FLUX]
    if colour:
        col = dict(albedoBedrock=st["albedoBedrock"], albedoSurface=st["albedoSurface"],
                   albedoFluvial=flux["albedoFluvial"], albedoDebris=flux["albedoDebris"])
        return _oracle_colour_cells(oracle, *args, col, scale, op)
    return oracle.erode_cells(*args, scale, op)


def _steps_against_the_oracle(oracle, bt, ops, scales, Ns, steps=3):
    """`steps` steps of batch `bt` phase by phase, each model's against the oracle's step from the batch's state;
    model b steps with oracle param ops[b], scale scales[b] and Ns[b] walkers.  Returns the first step's flux
    planes: the GPU's and the oracle's, per model."""
    from soillib_amd import soil
    B, colour = bt.B, bt.colour
    before = [bt.model_plane("layers", b) for b in range(B)]
    first = None
    for k in range(steps):
        states = [bt.model_planes(b) for b in range(B)]
        want, want_steps = [], 0
        for b in range(B):
            offset = ((bt.first_step[b] + bt.step_index) * Ns[b]) % 2 ** 64
            o, n = _oracle_particles(oracle, states[b], Ns[b], bt.seeds[b], offset, scales[b], ops[b], colour)
            want.append(o)
            want_steps += n
        soil.particle_steps(reset=True)
        bt.particles()
        got_steps = soil.particle_steps(reset=True)
        assert got_steps == want_steps, "step %d: %d particle steps, the oracle %d" % (k, got_steps, want_steps)
        flux = []
        for b in range(B):
            got = bt.model_planes(b)
            for name in FLUX + (COLOUR_FLUX if colour else ()):
                _flux_close_at_any_scale(got[name], want[b][name], "step %d, model %d (N %d): %s" % (k, b, Ns[b], name))
            flux.append({name: got[name] for name in FLUX + (COLOUR_FLUX if colour else ())})
        if first is None:
            first = (flux, want)
        bt.cells_fused()
        bt.swap_layers()
        bt.step_index += 1
        for b in range(B):
            cells = _oracle_cells(oracle, states[b], flux[b], scales[b], ops[b], colour)
            got = bt.model_planes(b)
            what = "step %d, model %d: " % (k, b)
            assert_bit_equal(got["layers"], cells["layers_next"], what + "layers")
            for name in OUT + (COLOUR_OUT if colour else ()):
                assert_bit_equal(got[name], cells[name], what + name)
            for name in FLUX:
                assert (got[name] == 0).all(), what + name + " not zeroed"
    assert any(not np.array_equal(bt.model_plane("layers", b), before[b], equal_nan=True) for b in range(B)), \
        "no model's terrain changed"
    return first


# ---------------------------------------------------------------- the draws of a case

def _scales(r, B, k):
    """B scales, log-uniform: 0.01..3 horizontal, 0.5..8 vertical; model k % B strongly anisotropic (a ratio of
    10..30 between the cell's sides, the long side along x or y as k is even or odd)."""
    out = []
    for b in range(B):
        s = [log_uniform(r, 0.01, 3.0), log_uniform(r, 0.01, 3.0), log_uniform(r, 0.5, 8.0)]
        if b == k % B:
            long = log_uniform(r, 0.3, 3.0)
            s[k % 2], s[1 - k % 2] = long, long / log_uniform(r, 10.0, 30.0)
        out.append(s)
    return out


def _params(oracle, r, B, k):
    """B oracle params (util.random_param, a force on every other model); maxage 256 on model k % B beside 0, 1,
    2 and 33 on the others."""
    ops = []
    for b in range(B):
        op = random_param(oracle, r, force=b % 2 == 1)
        op.maxage = 256 if b == k % B else (0, 1, 2, 33)[(b + k) % 4]
        ops.append(op)
    return ops


def _make(oracle, form, B, H, W, Ns, k, step_index=0, nan=None, min_age=0):
    """A batch of `form` with its oracle params, scales and walker counts; `nan`: (model, plane) made NaN over a
    patch (every model's velocity and debris velocity 1 elsewhere: no model spawns walkers at rest on a pit);
    `min_age`: every maxage at least that."""
    from soillib_amd import silt
    r = np.random.default_rng(4000 + k)
    colour = form.endswith("colour")
    ops = _params(oracle, r, B, k)
    for op in ops:
        op.maxage = max(op.maxage, min_age)
    scales = _scales(r, B, k)
    seeds = [SEEDS[(b + k) % len(SEEDS)] for b in range(B)]
    inp = _inputs(oracle, B, H, W, colour)
    if form.startswith("models"):
        bt = _batch(B, H, W, scales, [product_param(op) for op in ops], list(Ns), seeds, inp, colour)
        bt.first_step = [_below(n) for n in Ns]
        bt.first_step[(k + 1) % B] = 2 ** 42 // max(Ns[(k + 1) % B], 1)   # offsets near 2^42
        assert bt._per_model()
        Ns = list(Ns)
    else:
        if form.startswith("uniform"):
            ops[k % B].maxage = (256, 33, 2)[k % 3]
            ops = [ops[k % B]] * B
            param = product_param(ops[0])
        else:
            param = [product_param(op) for op in ops]
        scales = [scales[k % B]] * B
        bt = _batch(B, H, W, scales[0], param, Ns, seeds, inp, colour)
        bt.step_index = step_index
        assert not bt._per_model() and (bt.params is None) == form.startswith("uniform")
        Ns = [Ns] * B
    if nan is not None:
        one = np.ones((B, H, W, 2), np.float32)
        silt.set(bt.velocity, to_gpu(one))
        silt.set(bt.debrisVelocity, to_gpu(one))
        b, plane = nan
        patch = bt.model_plane(plane, b)
        patch[H // 4: H // 2 + 1, W // 4: W // 2 + 1] = np.nan
        full = to_np(getattr(bt, plane))
        full[b] = patch
        silt.set(getattr(bt, plane), to_gpu(full))
    return bt, ops, scales, Ns


# (form, launch shape, B, H, W, N or N_b, step_index of a uniform batch or a sweep)
CASES = [
    ("uniform", 1, 3, 33, 47, 255, _below(255)),
    ("uniform", 2, 4, 96, 80, 4369, _below(4369)),
    ("uniform", 0, 1, 8, 4, 64, 2 ** 42 // 64),
    ("uniform", 0, 3, 2, 37, 1025, _below(1025)),
    ("uniform-colour", 0, 3, 33, 47, 255, _below(255)),
    ("uniform-colour", 2, 5, 37, 2, 4369, _below(4369)),
    ("uniform-colour", 1, 1, 96, 80, 1023, 2 ** 42 // 1023),
    ("sweep", 1, 4, 33, 47, 255, _below(255)),
    ("sweep", 2, 3, 96, 80, 4369, _below(4369)),
    ("sweep", 0, 6, 2, 37, 1025, 2 ** 42 // 1025),
    ("sweep-colour", 0, 3, 8, 4, 64, _below(64)),
    ("models", 0, 5, 33, 47, [1023, 0, 255, 63, 1], None),        # max N_b < 1024: direct
    ("models", 0, 4, 96, 80, [4096, 1025, 0, 1024], None),        # max N_b >= 1024: staged
    ("models", 1, 6, 8, 4, [64, 65, 1, 0, 1023, 63], None),
    ("models", 2, 3, 2, 37, [1025, 1, 64], None),
    ("models", 0, 1, 33, 47, [4369], None),
    ("models-colour", 2, 4, 33, 47, [1024, 65, 0, 4096], None),
    ("models-colour", 1, 3, 96, 80, [1023, 63, 1], None),
    ("models-colour", 0, 4, 37, 2, [1, 1025, 64, 0], None),
]


def _case_id(k):
    form, mode, B, H, W, N, _ = CASES[k]
    return "%d-%s-%s-B%d-%dx%d" % (k, form, ("auto", "direct", "staged")[mode], B, H, W)


@pytest.mark.parametrize("k", range(len(CASES)), ids=_case_id)
def test_batch_steps_against_the_oracle(hip, oracle, k):
    form, mode, B, H, W, N, step_index = CASES[k]
    bt, ops, scales, Ns = _make(oracle, form, B, H, W, N, k, step_index or 0)
    with _shape(hip, mode):
        _steps_against_the_oracle(oracle, bt, ops, scales, Ns)


@pytest.mark.parametrize("form,mode,nan", [("models", 0, (1, "velocity")), ("uniform", 1, (2, "waterHeight")),
                                           ("models-colour", 2, (0, "velocity"))])
def test_nan_walkers_against_the_oracle(hip, oracle, form, mode, nan):
    """A model whose walkers go NaN through a patch of NaN velocity or water height: its planes against the oracle's
    (test_batch_steps_against_the_oracle's bars; NaN exactly where the oracle's are), with NaN velocity the NaN
    walkers' deposits in its own cell (0, 0); every other model's first-step flux planes finite."""
    B, H, W = 3, 48, 56
    Ns = [1500, 700, 1100] if form.startswith("models") else 900
    bt, ops, scales, Ns = _make(oracle, form, B, H, W, Ns, 20 + mode, _below(900), nan=nan, min_age=64)
    with _shape(hip, mode):
        flux, want = _steps_against_the_oracle(oracle, bt, ops, scales, Ns)
    for b in range(B):
        if b == nan[0]:
            assert np.isnan(want[b]["velocityFlux"]).any(), "no walker went NaN"
            if nan[1] == "velocity":
                assert np.isnan(want[b]["waterFlux"][0, 0]), "no NaN walker reached the oracle's (0, 0)"
                assert np.isnan(flux[b]["waterFlux"][0, 0]), "no NaN walker reached (0, 0)"
        else:
            for name, plane in flux[b].items():
                assert np.isfinite(plane).all(), "model %d: %s" % (b, name)


# ---------------------------------------------------------------- single models, the same two axes

@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("shape", [1, 2])
def test_small_shapes_random_parameter_sets(hip, oracle, shape, seed):
    """test_gpu_parity.test_transport_random_parameter_sets in the direct (1) and staged (2) launch shapes of a
    single model (soil_particles_fluvial_slab / _debris_slab on a seeded tensor): same walks step for step — the
    debris launch walks every walker to the end in these shapes — and flux within the summation-order tolerance."""
    random_parameter_transport(hip, oracle, seed, shape)


@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("N", [255, 4369])   # direct and staged; offsets exactly 2^32 - 1
def test_single_model_at_a_64_bit_seed_past_the_carry(hip, oracle, N, colour):
    """ErosionModel(..., seed=2^64 - 1).step() at the step index whose offset is 2^32 - 1 (the fluvial launch's draws
    on both sides of the carry, the debris launch's above it), forced from the oracle's state: the step count
    exactly, every plane (with colour the colour planes too) within test_three_coloured_steps_at_1024's bar."""
    from soillib_amd import silt, soil
    from soillib_amd.erosion import ErosionModel
    H, W, seed = 48, 56, 2 ** 64 - 1
    step_index = _below(N)
    assert step_index * N == CARRY
    op = script_param(oracle.default_param())
    op.maxage = 96
    scale = (20.0 / H, 20.0 / W, 4.0)
    r = np.random.default_rng(N + colour)
    st = dict(layers=terrain(oracle, H, W, sediment=0.02), rainfall=(0.5 + r.random((H, W))).astype(np.float32),
              uplift=(0.1 * r.random((H, W))).astype(np.float32),
              waterHeight=(0.1 * r.random((H, W))).astype(np.float32),
              velocity=r.standard_normal((H, W, 2)).astype(np.float32),
              debrisVelocity=(0.5 * r.standard_normal((H, W, 2))).astype(np.float32))
    if colour:
        st["albedoBedrock"] = r.random((H, W, 3)).astype(np.float32)
        st["albedoSurface"] = r.random((H, W, 3)).astype(np.float32)
    m = ErosionModel(H, W, scale, product_param(op), N, seed=seed, colour=colour)
    m.set_layers(to_gpu(st["layers"]))
    for name, v in st.items():
        if name != "layers":
            silt.set(getattr(m, name), to_gpu(v))
    m.step_index = step_index
    soil.particle_steps(reset=True)
    m.step()
    got_steps = soil.particle_steps(reset=True)
    assert m.step_index == step_index + 1
    o, steps = _oracle_particles(oracle, st, N, seed, CARRY, scale, op, colour)
    assert got_steps == steps > N, (got_steps, steps)
    want = _oracle_cells(oracle, st, o, scale, op, colour)
    got = dict(layers=to_np(m.layers), **{name: to_np(getattr(m, name)) for name in OUT + (COLOUR_OUT if colour else ())})
    want["layers"] = want["layers_next"]
    for name in got:
        tol = dict(rtol=1e-4, atol=1e-5 * (np.nanmax(np.abs(want[name])) + 1e-30))
        _close_but_for_stray_walks(got[name], want[name], tol["rtol"], tol["atol"], 2e-6, "seed 2^64 - 1: " + name)
    for name in FLUX:
        assert (to_np(getattr(m, name)) == 0).all(), name + " not zeroed"
