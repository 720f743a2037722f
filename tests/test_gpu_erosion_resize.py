"""A model or a whole batch resampled to a new resolution in one launch (include/soil_hip.h:
soil_erode_resize_batch; ErosionModel.resized, ErosionBatch.resized):

  1. every resampled plane of every model bit for bit against the CPU oracle's resize of that plane alone, `height`
     the fp32 sum of the new layers, the flux planes zero, the source unchanged;
  2. bit for bit equal to the single-plane route (legacy.resize) on the GPU;
  3. isolation: a model full of NaN and infinities spoils nothing of the others;
  4. seeds, params, step indices, walker counts and rescaled scales are carried over, and can be overridden;
  5. the resampled batch steps correctly against the oracle (test_gpu_erosion_batch_oracle's bars, unchanged);
  6. a multiscale schedule, the batch against its models taken one at a time;
  7. more models than one launch holds (65537);
  8. another stream; refused arguments, of the entry point and of resized().

No tolerance in 1-4, 7, 8: the operation is deterministic and the bar is bit equality.  5 and 6 take their bars
from the files they import.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_erosion_batch import OUT as STEP_OUT
from test_gpu_erosion_batch import _close, retire_off  # noqa: F401  (a fixture)
from test_gpu_erosion_batch_oracle import _make, _steps_against_the_oracle
from test_gpu_erosion_batch_params import _inputs
from util import assert_bit_equal, product_param, script_param, to_gpu, to_np

pytestmark = pytest.mark.gpu

RESAMPLED = ("layers", "uplift", "rainfall", "waterHeight", "mass", "debris", "velocity", "debrisVelocity")
COLOUR = ("albedoBedrock", "albedoSurface", "albedoFluvial", "albedoDebris")
FLUX = ("waterFlux", "massFlux", "velocityFlux", "debrisFlux", "debrisVelocityFlux")
# (Ho, Wo) -> (Hn, Wn): finer, odd and unequal ratios, coarser, a single row, the identity, 2x, one axis finer and
# the other coarser
SHAPES = [((16, 16), (32, 32)), ((17, 23), (40, 31)), ((32, 32), (16, 16)), ((1, 5), (3, 9)), ((8, 8), (8, 8)),
          ((64, 64), (128, 128)), ((48, 160), (100, 33))]


def _shape_id(pair):
    return "%dx%d-%dx%d" % (pair[0] + pair[1])


def _source(B, H, W, colour, seed, poison=None):
    """A batch whose every plane holds its own seeded random finite values (flux planes, height and layers_next
    too: junk the resample must not read), and those values on the host.  `poison`: a model whose persistent
    planes get NaN, +inf and -inf at scattered cells."""
    from soillib_amd import silt, soil
    from soillib_amd.erosion import ErosionBatch
    bt = ErosionBatch(B, H, W, (1.0, 1.0, 1.0), soil.param_t(), 16, list(range(1, B + 1)), colour=colour)
    r = np.random.default_rng(seed)
    host = {}
    for name in bt._names():
        a = (3.0 * r.standard_normal(tuple(getattr(bt, name).shape))).astype(np.float32)
        if name in ("mass", "debris"):
            a = np.abs(a)   # sediment-like planes: non-negative in, non-negative out
        host[name] = a
    if poison is not None:
        for name in RESAMPLED + (COLOUR if colour else ()):
            flat = host[name][poison].reshape(-1)
            at = r.choice(flat.size, size=max(3, flat.size // 7), replace=False)
            flat[at] = r.choice(np.array([np.nan, np.inf, -np.inf], np.float32), size=at.size)
    for name, a in host.items():
        silt.set(getattr(bt, name), to_gpu(a))
    return bt, host


def _assert_zero(a, what):
    assert not a.view(np.uint32).any(), what + " is not all +0.0"


def _against_the_oracle(oracle, new, host, models, what=""):
    """Models `models` of the resampled batch `new` against the oracle's resize of each source plane alone."""
    size = (new.H, new.W)
    for b in models:
        got = new.model_planes(b)
        w = "%smodel %d: " % (what, b)
        for name in RESAMPLED + (COLOUR if new.colour else ()):
            assert_bit_equal(got[name], oracle.resize(host[name][b], size), w + name)
        with np.errstate(invalid="ignore"):   # (inf + -inf in a poisoned model)
            merged = got["layers"][..., 0] + got["layers"][..., 1]
        assert_bit_equal(got["height"], merged, w + "height")
        for name in FLUX:
            _assert_zero(got[name], w + name)
        _assert_zero(got["layers_next"], w + "layers_next")


def _unchanged(bt, host, what="the source"):
    for name, a in host.items():
        assert_bit_equal(to_np(getattr(bt, name)), a, "%s: %s" % (what, name))


# ---------------------------------------------------------------- 1. against the oracle

@pytest.mark.parametrize("colour", [False, True], ids=["physics", "colour"])
@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("pair", SHAPES, ids=_shape_id)
def test_against_the_oracle_bit_for_bit(hip, oracle, pair, B, colour):
    (Ho, Wo), (Hn, Wn) = pair
    bt, host = _source(B, Ho, Wo, colour, seed=100 * Ho + Wn + B)
    new = bt.resized(Hn, Wn)
    assert (new.B, new.H, new.W, new.colour) == (B, Hn, Wn, colour)
    _against_the_oracle(oracle, new, host, range(B))
    _unchanged(bt, host)
    if (Ho, Wo) == (Hn, Wn):   # the identity
        for name in RESAMPLED + (COLOUR if colour else ()):
            assert_bit_equal(to_np(getattr(new, name)), host[name], "identity: " + name)
    for name in ("mass", "debris"):
        assert (to_np(getattr(new, name)) >= 0).all(), name + " went negative"
    for name in RESAMPLED:   # the four corner cells are kept
        a, g = host[name], to_np(getattr(new, name))
        for (i, j), (k, m) in zip([(0, 0), (0, Wo - 1), (Ho - 1, 0), (Ho - 1, Wo - 1)],
                                  [(0, 0), (0, Wn - 1), (Hn - 1, 0), (Hn - 1, Wn - 1)]):
            assert_bit_equal(g[:, k, m], a[:, i, j], "corner %s of %s" % ((k, m), name))


def test_a_single_model_against_the_oracle(hip, oracle):
    """ErosionModel.resized: the same entry point with B = 1, colour included."""
    from soillib_amd import silt, soil
    from soillib_amd.erosion import ErosionModel
    Ho, Wo, Hn, Wn = 24, 40, 61, 50
    m = ErosionModel(Ho, Wo, (0.5, 0.25, 4.0), soil.param_t(), 64, seed=9, colour=True)
    r = np.random.default_rng(5)
    host = {}
    for name in ("layers", "layers_next") + m.PLANES_1 + m.PLANES_2 + m.PLANES_3:
        host[name] = (3.0 * r.standard_normal(tuple(getattr(m, name).shape))).astype(np.float32)
        silt.set(getattr(m, name), to_gpu(host[name]))
    new = m.resized(Hn, Wn)
    for name in RESAMPLED + COLOUR:
        assert_bit_equal(to_np(getattr(new, name)), oracle.resize(host[name], (Hn, Wn)), name)
    layers = to_np(new.layers)
    assert_bit_equal(to_np(new.height), layers[..., 0] + layers[..., 1], "height")
    for name in FLUX + ("layers_next",):
        _assert_zero(to_np(getattr(new, name)), name)
    for name, a in host.items():
        assert_bit_equal(to_np(getattr(m, name)), a, "the source: " + name)


# ---------------------------------------------------------------- 2. the single-plane route

@pytest.mark.parametrize("pair,B,colour", [(SHAPES[1], 3, True), (SHAPES[6], 5, False)],
                         ids=["17x23-40x31-colour", "48x160-100x33"])
def test_equal_to_the_single_plane_route(hip, pair, B, colour):
    from soillib_amd import legacy, silt
    (Ho, Wo), (Hn, Wn) = pair
    bt, host = _source(B, Ho, Wo, colour, seed=77 + B)
    new = bt.resized(Hn, Wn)
    for name in RESAMPLED + (COLOUR if colour else ()):
        got = to_np(getattr(new, name))
        for b in range(B):
            src = to_gpu(host[name][b])
            dst = silt.tensor(silt.float32, silt.shape(*got.shape[1:]), silt.gpu)
            legacy.resize(dst, src, (Hn, Wn), (Ho, Wo))
            assert_bit_equal(got[b], to_np(dst), "model %d: %s" % (b, name))


# ---------------------------------------------------------------- 3. isolation

@pytest.mark.parametrize("colour", [False, True], ids=["physics", "colour"])
def test_a_model_of_nan_and_infinities_spoils_no_other(hip, oracle, colour):
    B, bad, (Ho, Wo), (Hn, Wn) = 4, 2, (17, 23), (40, 31)
    clean, _ = _source(B, Ho, Wo, colour, seed=31)
    dirty, host = _source(B, Ho, Wo, colour, seed=31, poison=bad)
    want, got = clean.resized(Hn, Wn), dirty.resized(Hn, Wn)
    for b in range(B):
        if b == bad:
            continue
        w, g = want.model_planes(b), got.model_planes(b)
        for name in w:
            assert np.isfinite(g[name]).all(), "model %d: %s" % (b, name)
            assert_bit_equal(g[name], w[name], "model %d: %s" % (b, name))
    assert np.isnan(got.model_plane("layers", bad)).any() and np.isinf(got.model_plane("layers", bad)).any()
    _against_the_oracle(oracle, got, host, [bad])   # NaN where the oracle's are, every other value bit for bit


# ---------------------------------------------------------------- 4. what is carried

def _different_models(oracle, B, H, W, colour, steps=(2, 0, 1, 3)):
    """B single models with their own param, scale, walker count and seed, model b `steps[b]` steps on."""
    from test_gpu_erosion_batch_params import _single
    inp = _inputs(oracle, B, H, W, colour)
    models = []
    for b in range(B):
        op = script_param(oracle.default_param())
        op.maxage = 24 + 8 * b
        scale = [20.0 / H * (1.0 + 0.25 * b), 20.0 / W * (1.0 + 0.125 * b), 4.0 + b]
        m = _single(b, H, W, scale, product_param(op), 300 + 100 * b, 5 + 3 * b, inp, colour)
        for _ in range(steps[b % len(steps)]):
            m.step()
        models.append(m)
    return models


@pytest.mark.parametrize("colour", [False, True], ids=["physics", "colour"])
def test_a_batch_carries_everything_over(hip, oracle, colour):
    from soillib_amd.erosion import ErosionBatch
    B, Ho, Wo, Hn, Wn = 4, 24, 32, 50, 41
    models = _different_models(oracle, B, Ho, Wo, colour)
    bt = ErosionBatch.from_models(models)
    bt.step()
    bt.step()
    assert bt.step_index == 2 and bt.first_step == [2, 0, 1, 3]
    before = {name: to_np(getattr(bt, name)) for name in bt._names()}
    new = bt.resized(Hn, Wn)
    assert (new.B, new.H, new.W, new.colour) == (B, Hn, Wn, colour)
    assert new.seeds == bt.seeds and new.first_step == bt.first_step and new.first_step is not bt.first_step
    assert new.step_index == 2
    assert new.param is None and len(new.params) == B and all(new.params[b] is bt.params[b] for b in range(B))
    assert new.N is None and new.Ns == bt.Ns == [300, 400, 500, 600]
    assert new.scale is None
    for b in range(B):
        sx, sy, sz = bt.scales[b]
        assert new.scales[b] == [sx * Ho / Hn, sy * Wo / Wn, sz]
    assert new._per_model()
    # explicit arguments: one triple and one count, then B of each
    one = bt.resized(Hn, Wn, scale=(0.5, 0.25, 3.0), n_particles=77)
    assert one.scale == [0.5, 0.25, 3.0] and one.scales is None and one.N == 77 and one.Ns is None
    assert one.first_step == bt.first_step and one._per_model()
    each = bt.resized(Hn, Wn, scale=[(1.0 + b, 2.0, 3.0) for b in range(B)], n_particles=[10, 0, 30, 40])
    assert each.scales == [(1.0 + b, 2.0, 3.0) for b in range(B)] and each.Ns == [10, 0, 30, 40]
    for other in (one, each):
        for name in RESAMPLED + (COLOUR if colour else ()):
            assert_bit_equal(to_np(getattr(other, name)), to_np(getattr(new, name)), name)
    # the original is unchanged and still steps
    _unchanged(bt, before, "the original")
    bt.step()
    assert bt.step_index == 3 and new.step_index == 2
    assert not np.array_equal(to_np(bt.layers), before["layers"])


def test_uniform_batches_and_sweeps_stay_what_they_are(hip, oracle):
    from soillib_amd.erosion import ErosionBatch
    B, Ho, Wo = 3, 16, 20
    p = product_param(script_param(oracle.default_param()))
    bt = ErosionBatch(B, Ho, Wo, (2.0, 3.0, 4.0), p, 128, [4, 5, 6])
    bt.step_index = 7
    new = bt.resized(32, 30)
    assert new.param is p and new.params is None and new.scale == [2.0 * 16 / 32, 3.0 * 20 / 30, 4.0]
    assert new.scales is None and new.N == 128 and new.Ns is None and new.step_index == 7
    assert new.first_step == [0] * B and not new._per_model() and new.seeds == [4, 5, 6]
    params = [product_param(script_param(oracle.default_param())) for _ in range(B)]
    sweep = ErosionBatch(B, Ho, Wo, (2.0, 3.0, 4.0), params, 128, [4, 5, 6], colour=True)
    new = sweep.resized(8, 8)
    assert new.param is None and all(a is b for a, b in zip(new.params, params)) and new.colour
    assert not new._per_model()


@pytest.mark.parametrize("colour", [False, True], ids=["physics", "colour"])
def test_a_model_carries_everything_over(hip, oracle, colour):
    m = _different_models(oracle, 2, 24, 32, colour)[0]
    assert m.step_index == 2
    before = {name: to_np(getattr(m, name)) for name in RESAMPLED + FLUX + ("height",)}
    new = m.resized(48, 48)
    assert (new.H, new.W, new.rows, new.colour) == (48, 48, 48, colour)
    assert new.param is m.param and new.seed == m.seed and new.step_index == 2 and new.N == m.N
    assert new.scale == [m.scale[0] * 24 / 48, m.scale[1] * 32 / 48, m.scale[2]]
    other = m.resized(48, 48, scale=(1.0, 2.0, 3.0), n_particles=55)
    assert other.scale == [1.0, 2.0, 3.0] and other.N == 55 and other.step_index == 2
    assert_bit_equal(to_np(other.layers), to_np(new.layers), "layers")
    _unchanged(m, before, "the original")
    m.step()
    new.step()
    assert m.step_index == 3 and new.step_index == 3
    assert np.isfinite(to_np(new.layers)).all()
    assert not np.array_equal(to_np(m.layers), before["layers"])


# ---------------------------------------------------------------- 5. the resampled batch steps correctly

@pytest.mark.parametrize("form,B,H,W,N,size", [("uniform", 3, 33, 47, 900, (50, 64)),
                                               ("models", 4, 40, 36, [1500, 0, 255, 1024], (64, 80)),
                                               ("models-colour", 3, 48, 40, [1100, 63, 700], (31, 57)),
                                               ("uniform-colour", 2, 24, 24, 2048, (48, 48))])
def test_the_resampled_batch_steps_against_the_oracle(hip, oracle, form, B, H, W, N, size):
    """Two steps, resized(), then three steps of the new batch phase by phase against the oracle, which starts
    from the new batch's own planes and each model's carried first_step + step_index, scale and walker count."""
    bt, ops, scales, Ns = _make(oracle, form, B, H, W, N, 40 + B, step_index=5, min_age=16)
    for _ in range(2):
        bt.step()
    new = bt.resized(*size)
    assert new._per_model() == bt._per_model() and (new.params is None) == (bt.params is None)
    assert new.step_index == bt.step_index and new.first_step == bt.first_step
    new_scales = [list(s) for s in new.scales] if new.scales is not None else [list(new.scale)] * B
    for b in range(B):
        assert new_scales[b] == [scales[b][0] * H / size[0], scales[b][1] * W / size[1], scales[b][2]]
    _steps_against_the_oracle(oracle, new, ops, new_scales, Ns)


# ---------------------------------------------------------------- 6. a multiscale schedule

def test_a_multiscale_schedule_batch_against_models(hip, oracle, retire_off):
    """48 x 48 -> 96 x 80 -> 33 x 47 with three steps at each (staged, staged, direct), the batch against the same
    four models one at a time: every output plane within the batch tests' bar, the particle steps exactly."""
    from soillib_amd import soil
    from soillib_amd.erosion import ErosionBatch
    from test_gpu_erosion_batch import _batch, _inputs as _inputs_physics, _param, _single
    B, H, W, N = 4, 48, 48, 1500
    p = _param(oracle, 48)
    scale = (20.0 / H, 20.0 / W, 4.0)
    seeds = [11 + 7 * b for b in range(B)]
    inp = _inputs_physics(oracle, B, H, W)
    schedule = [dict(H=96, W=80), dict(H=33, W=47, n_particles=700)]

    def run(x):
        for _ in range(3):
            x.step()
        for stage in schedule:
            x = x.resized(**stage)
            for _ in range(3):
                x.step()
        return x

    soil.particle_steps(reset=True)
    bt = run(_batch(B, H, W, scale, p, N, seeds, inp))
    batch_steps = soil.particle_steps(reset=True)
    assert isinstance(bt, ErosionBatch) and (bt.H, bt.W, bt.N, bt.step_index) == (33, 47, 700, 9)
    single_steps = 0
    for b in range(B):
        m = run(_single(b, H, W, scale, p, N, seeds[b], inp))
        single_steps += soil.particle_steps(reset=True)
        assert (m.H, m.W, m.N, m.step_index) == (33, 47, 700, 9) and m.scale == bt.scale
        got = bt.model_planes(b)
        for name in STEP_OUT:
            _close(got[name], to_np(getattr(m, name)), "model %d: %s" % (b, name))
        for name in FLUX:
            assert not got[name].any(), "model %d: %s" % (b, name)
    assert batch_steps == single_steps


# ---------------------------------------------------------------- 7. more models than one launch holds

def test_65537_models(hip, oracle):
    """B = 65537 models of 2 x 2 -> 3 x 3: two launches (grid.z <= 65535); the first launch's first, second and
    last two models and the second launch's two, each against the oracle."""
    bt, host = _source(65537, 2, 2, False, seed=65537)
    new = bt.resized(3, 3)
    _against_the_oracle(oracle, new, host, (0, 1, 65534, 65535, 65536))


# ---------------------------------------------------------------- 8. another stream, refusals

def test_on_another_stream(hip, oracle):
    import torch
    from soillib_amd import _abi
    want, _ = _source(3, 17, 23, True, seed=8)
    want = want.resized(40, 31)
    s = torch.cuda.Stream()
    _abi.set_stream(s.cuda_stream)
    try:
        bt, host = _source(3, 17, 23, True, seed=8)
        new = bt.resized(40, 31)
        s.synchronize()
        _against_the_oracle(oracle, new, host, range(3))
        for name in new._names():
            assert_bit_equal(to_np(getattr(new, name)), to_np(getattr(want, name)), name)
        s.synchronize()
    finally:
        _abi.set_stream(0)


def test_invalid_arguments_are_refused(hip):
    from soillib_amd import _abi
    lib = _abi.lib()
    B, (Ho, Wo), (Hn, Wn) = 2, (8, 12), (16, 10)
    src_bt, _ = _source(B, Ho, Wo, True, seed=1)
    dst_bt, sentinel = _source(B, Hn, Wn, True, seed=2)
    src, dst, src_c, dst_c = src_bt._planes(), dst_bt._planes(), src_bt._colour(), dst_bt._colour()

    def refused(naming, d=dst, s=src, dc=dst_c, sc=src_c, sizes=(B, Hn, Wn, Ho, Wo)):
        ref = lambda x: None if x is None else C.byref(x)  # noqa: E731
        rc = lib.soil_erode_resize_batch(ref(d), ref(s), ref(dc), ref(sc), *sizes, None)
        assert rc == _abi.SOIL_ERR_INVALID_ARGUMENT, naming
        assert naming in _abi.last_error(), (naming, _abi.last_error())

    def without(planes, field, cls):
        p = cls()
        for f, _ in cls._fields_:
            setattr(p, f, None if f == field else getattr(planes, f))
        return p

    refused("B >= 1", sizes=(0, Hn, Wn, Ho, Wo))
    refused("B >= 1", sizes=(-3, Hn, Wn, Ho, Wo))
    refused("new size", sizes=(B, 0, Wn, Ho, Wo))
    refused("new size", sizes=(B, Hn, -1, Ho, Wo))
    refused("old size", sizes=(B, Hn, Wn, 0, Wo))
    refused("old size", sizes=(B, Hn, Wn, Ho, 0))
    refused("overflow", sizes=(B, 1 << 40, 1 << 20, Ho, Wo))
    refused("overflow", sizes=(B, Hn, Wn, 1 << 31, 1 << 31))
    refused("null dst or src", d=None)
    refused("null dst or src", s=None)
    for field in RESAMPLED:
        refused("null plane in src", s=without(src, field, _abi.ErosionPlanes))
    for field in RESAMPLED + FLUX:
        refused("null plane in dst", d=without(dst, field, _abi.ErosionPlanes))
    refused("both be NULL or both be set", dc=None)
    refused("both be NULL or both be set", sc=None)
    for field in _abi.COLOUR_PLANES:
        refused("every colour plane", dc=without(dst_c, field, _abi.ColourPlanes))
        refused("every colour plane", sc=without(src_c, field, _abi.ColourPlanes))
    same = without(dst, None, _abi.ErosionPlanes)
    same.layers = src.layers
    refused("in place", d=same)
    _unchanged(dst_bt, sentinel, "dst after the refusals")
    # what may be NULL: dst's height and layers_next, src's flux planes, height and layers_next
    d = without(without(dst, "height", _abi.ErosionPlanes), "layers_next", _abi.ErosionPlanes)
    s = src
    for field in FLUX + ("height", "layers_next"):
        s = without(s, field, _abi.ErosionPlanes)
    assert lib.soil_erode_resize_batch(C.byref(d), C.byref(s), None, None, B, Hn, Wn, Ho, Wo, None) == _abi.SOIL_OK
    assert_bit_equal(to_np(dst_bt.height), sentinel["height"], "a NULL height")
    assert_bit_equal(to_np(dst_bt.albedoSurface), sentinel["albedoSurface"], "physics only: colour")
    assert not to_np(dst_bt.waterFlux).any()


def test_resized_refuses_bad_arguments_before_any_device_work(hip, oracle):
    from soillib_amd import _abi, soil
    from soillib_amd.erosion import ErosionModel
    B = 3
    bt, host = _source(B, 8, 12, True, seed=3)
    bad = [dict(H=0, W=8), dict(H=8, W=0), dict(H=-4, W=8), dict(H=8.5, W=8),
           dict(H=8, W=8, scale=[(1.0, 1.0, 1.0)] * 2), dict(H=8, W=8, scale=[(1.0, 1.0, 1.0)] * 4),
           dict(H=8, W=8, scale=[(1.0, 1.0, 1.0), (1.0, 1.0), (1.0, 1.0, 1.0)]), dict(H=8, W=8, scale=(1.0, 2.0)),
           dict(H=8, W=8, scale=(1.0, "x", 2.0)), dict(H=8, W=8, scale=2.0),
           dict(H=8, W=8, n_particles=[16, 16]), dict(H=8, W=8, n_particles=[16] * 4),
           dict(H=8, W=8, n_particles=[16, -1, 16]), dict(H=8, W=8, n_particles=-5),
           dict(H=8, W=8, n_particles=[16, 2.5, 16])]
    for kw in bad:
        with pytest.raises(ValueError):
            bt.resized(**kw)
    _unchanged(bt, host)
    m = ErosionModel(8, 12, (1.0, 1.0, 1.0), soil.param_t(), 16, seed=1)
    before = to_np(m.layers)
    for kw in [dict(H=0, W=8), dict(H=8, W=-1), dict(H=8, W=8, scale=(1.0, 2.0)), dict(H=8, W=8, scale=3.0),
               dict(H=8, W=8, scale=(1.0, None, 2.0)), dict(H=8, W=8, n_particles=-1),
               dict(H=8, W=8, n_particles=2.5)]:
        with pytest.raises(ValueError):
            m.resized(**kw)
    assert_bit_equal(to_np(m.layers), before, "the model")
    slab = ErosionModel(32, 12, (1.0, 1.0, 1.0), soil.param_t(), 16, seed=1, dom=_abi.Domain(32, 12, 8, 16, 1, 15))
    with pytest.raises(ValueError, match="row slab"):
        slab.resized(64, 24)
