"""A batch summarised on the device (include/soil_hip.h, "erosion: summaries": soil_erode_batch_stats,
soil_erode_batch_ensemble; ErosionBatch.stats, ErosionModel.stats, ErosionBatch.ensemble).  The expected values
are restated in numpy here; the oracle has no reductions.

  1. exact sums: planes whose every fp64 partial sum is exactly representable, bit for bit against numpy;
  2. random finite planes at ragged, square and full sizes: min, max and the non-finite count equal, sum and sumsq
     within the bound of an fp64 sum in any order;
  3. NaN and infinities: counted exactly, the finite statistics those of the remaining cells, no other model's
     record touched;
  4. a model's record in a batch byte for byte its record alone, in another batch, at another position, and from
     call to call;
  5. after real steps, against numpy over model_planes(b); the height channel is the `height` plane;
  6. the ensemble maps bit for bit against the numpy restatement of the contract;
  7. more models than one launch holds (65537);
  8. another stream; refused arguments; a row slab.

Every bar is derived, none is measured:
  - 1, 4 and 6 are bit equality.  In 1 it holds for ANY summation order because no partial sum rounds (the
    exponents are worked out at test_exact_sums); in 4 because the reduction tree is fixed by H*W alone; in 6 because
    the contract fixes every operation and its order.
  - 2, 3 and 5: a recursive fp64 sum of n terms in any order is within (n - 1) * 2^-53 * sum|x_i| of the exact sum
    (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4, to first order in 2^-53), and math.fsum
    returns the exact sum rounded once.  The squares are exact in fp64 (24-bit significands), so the same bound
    with x_i^2 for x_i holds for sumsq.  Where fsum is too slow (more than 2^20 cells) the reference is numpy's
    fp64 sum, which obeys the same bound, so the two are within twice the bound of each other.
  - min, max and the non-finite count involve no rounding: equality (min and max numerically, `==`: which of +0
    and -0 a tie returns is not specified).
"""
import ctypes as C
import math

import numpy as np
import pytest

from test_gpu_erosion_batch import _batch, _inputs, _param
from test_gpu_erosion_resize import _source
from util import assert_bit_equal, to_gpu, to_np

pytestmark = pytest.mark.gpu

READ = ("layers", "waterHeight", "mass", "debris", "velocity", "debrisVelocity")   # what the stats entry reads
ENSEMBLE_READ = ("layers", "waterHeight", "mass", "debris")
# channel -> (plane, component) of the nine stored channels; channel 2 (height) is computed
STORED = {0: ("layers", 0), 1: ("layers", 1), 3: ("waterHeight", None), 4: ("mass", None), 5: ("debris", None),
          6: ("velocity", 0), 7: ("velocity", 1), 8: ("debrisVelocity", 0), 9: ("debrisVelocity", 1)}
RAGGED = [(1, 1), (5, 1), (1, 8), (37, 53)]
SQUARE = [(256, 256), (1024, 1024)]
U = 2.0 ** -53
FSUM_MAX = 1 << 20   # cells up to which math.fsum is the reference


def _size_id(size):
    return "%dx%d" % size


def _channels(host, b):
    """The ten channels of model b of `host` (name -> (B, H, W[, C]) arrays), flattened, in the ABI's order."""
    with np.errstate(invalid="ignore"):   # inf + -inf
        height = host["layers"][b][..., 0] + host["layers"][b][..., 1]   # fp32, as layer_merge adds them
    out = []
    for c in range(10):
        if c == 2:
            a = height
        else:
            name, comp = STORED[c]
            a = host[name][b] if comp is None else host[name][b][..., comp]
        assert a.dtype == np.float32
        out.append(np.ascontiguousarray(a).reshape(-1))
    return out


def _check_channel(rec, x, what):
    """One soil_channel_stats record against the values `x` (fp32, flat) under the bars of the module docstring."""
    n = x.size
    finite = np.isfinite(x)
    f = x[finite].astype(np.float64)
    assert int(rec["nonfinite"]) == n - f.size, "%s: nonfinite %d, expected %d" % (what, rec["nonfinite"], n - f.size)
    if f.size == 0:
        assert rec["min"] == np.inf and rec["max"] == -np.inf, "%s: min/max of no finite value" % what
        assert rec["sum"] == 0.0 and rec["sumsq"] == 0.0, "%s: sums of no finite value" % what
        return
    assert rec["min"] == f.min() and rec["max"] == f.max(), "%s: min/max %r %r, expected %r %r" % (
        what, rec["min"], rec["max"], f.min(), f.max())
    sq = f * f   # exact
    if n <= FSUM_MAX:
        want, want_sq, k = math.fsum(f.tolist()), math.fsum(sq.tolist()), 1.0
        bound, bound_sq = (n - 1) * U * math.fsum(np.abs(f).tolist()), (n - 1) * U * want_sq
    else:
        want, want_sq, k = float(np.sum(f)), float(np.sum(sq)), 2.0
        bound, bound_sq = (n - 1) * U * float(np.sum(np.abs(f))), (n - 1) * U * want_sq
    err, err_sq = abs(float(rec["sum"]) - want), abs(float(rec["sumsq"]) - want_sq)
    assert err <= k * bound, "%s: sum %r, expected %r: off by %.3e, bound %.3e" % (what, rec["sum"], want, err, k * bound)
    assert err_sq <= k * bound_sq, "%s: sumsq %r, expected %r: off by %.3e, bound %.3e" % (
        what, rec["sumsq"], want_sq, err_sq, k * bound_sq)


def _check_model(rec, host, b, what=""):
    from soillib_amd.erosion import STAT_CHANNELS
    for c, x in enumerate(_channels(host, b)):
        _check_channel(rec[c], x, "%smodel %d: %s" % (what, b, STAT_CHANNELS[c]))


def _filled(host, B, H, W):
    """A batch whose planes named in `host` hold its (B, H, W[, C]) arrays; every other plane is zero."""
    from soillib_amd import silt, soil
    from soillib_amd.erosion import ErosionBatch
    bt = ErosionBatch(B, H, W, (1.0, 1.0, 1.0), soil.param_t(), 16, list(range(B)))
    for name, a in host.items():
        assert tuple(getattr(bt, name).shape) == a.shape
        silt.set(getattr(bt, name), to_gpu(a))
    return bt


def _single(host, b, H, W):
    """Model b of `host` alone, as an ErosionModel."""
    from soillib_amd import silt, soil
    from soillib_amd.erosion import ErosionModel
    m = ErosionModel(H, W, (1.0, 1.0, 1.0), soil.param_t(), 16, seed=b)
    for name, a in host.items():
        silt.set(getattr(m, name), to_gpu(a[b]))
    return m


def _random_read_planes(B, H, W, seed, names=READ):
    r = np.random.default_rng(seed)
    host = {}
    for name in names:
        shape = (B, H, W, 2) if name in ("layers", "velocity", "debrisVelocity") else (B, H, W)
        host[name] = (3.0 * r.standard_normal(shape, dtype=np.float32)).astype(np.float32)
    return host


def _assert_stats_shape(st, B):
    from soillib_amd.erosion import STATS_DTYPE
    assert isinstance(st, np.ndarray) and st.shape == (B, 10) and st.dtype == STATS_DTYPE
    assert st.dtype.names == ("sum", "sumsq", "nonfinite", "min", "max") and st.dtype.itemsize == 32


# ---------------------------------------------------------------- 1. exact sums

@pytest.mark.parametrize("cap_log2,both", [(8, False), (5, True)], ids=["below-2^8-sum", "below-2^5-sum-and-sumsq"])
@pytest.mark.parametrize("size", [(1024, 1024), (37, 53), (301, 211)], ids=_size_id)
def test_exact_sums(hip, size, cap_log2, both):
    """Every stored value is k * 2^-10 with an integer |k| < 2^(cap + 10), cap = 8 or 5, over n <= 2^20 cells.

    cap = 8 (the sums): |k| < 2^18 fits fp32's 24 bits.  The height channel is the sum of two such values: an
    integer multiple of 2^-10 below 2^9, 19 bits, so the fp32 addition is exact too.  Any partial sum of at most 2^20
    of them is a multiple of 2^-10 below 2^20 * 2^9 = 2^29, that is an integer below 2^39 in units of 2^-10: at most
    39 of fp64's 53 bits, so no addition rounds and `sum` equals numpy's fp64 sum in whatever order either adds.
    Their squares are multiples of 2^-20 below 2^18, partial sums below 2^38, integers below 2^58 in units of 2^-20:
    too many, so at this cap sumsq is only held to the bound of test 2.

    cap = 5 (the sums of squares too): values below 2^5, heights below 2^6, squares multiples of 2^-20 below 2^12,
    partial sums below 2^20 * 2^12 = 2^32, integers below 2^52 in units of 2^-20: at most 52 bits, nothing rounds,
    and `sumsq` is bit for bit numpy's as well (the sums need 10 + 20 + 6 = 36 bits).

    Any fp32 accumulation fails this: a 24-bit accumulator cannot hold these sums."""
    H, W = size
    B = 2
    assert H * W <= 1 << 20
    r = np.random.default_rng(H + W + cap_log2)
    k_max = 1 << (cap_log2 + 10)
    host = {}
    for name in READ:
        shape = (B, H, W, 2) if name in ("layers", "velocity", "debrisVelocity") else (B, H, W)
        k = r.integers(-k_max + 1, k_max, size=shape)
        host[name] = (k.astype(np.float64) * 2.0 ** -10).astype(np.float32)
        assert np.array_equal(host[name].astype(np.float64) * 1024.0, k)   # exact in fp32
    st = _filled(host, B, H, W).stats()
    _assert_stats_shape(st, B)
    for b in range(B):
        for c, x in enumerate(_channels(host, b)):
            f = x.astype(np.float64)
            what = "model %d channel %d" % (b, c)
            assert st[b, c]["sum"] == np.sum(f) == math.fsum(f.tolist()), what + ": sum"
            if both:
                assert st[b, c]["sumsq"] == np.sum(f * f) == math.fsum((f * f).tolist()), what + ": sumsq"
            assert st[b, c]["nonfinite"] == 0 and st[b, c]["min"] == x.min() and st[b, c]["max"] == x.max(), what
        _check_model(st[b], host, b)


# ---------------------------------------------------------------- 2. random finite planes

@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("size", RAGGED + SQUARE, ids=_size_id)
def test_random_finite_planes(hip, size, B):
    H, W = size
    bt, host = _source(B, H, W, False, seed=7 * H + W + B)
    st = bt.stats()
    _assert_stats_shape(st, B)
    for b in range(B):
        _check_model(st[b], host, b)
    for name, a in host.items():   # the batch is left as it is
        assert_bit_equal(to_np(getattr(bt, name)), a, "the source: " + name)


def test_one_full_size_model(hip):
    """One 8192 x 8192 model through ErosionModel.stats(): numpy's fp64 sums, twice the bound."""
    from soillib_amd import silt, soil
    from soillib_amd.erosion import ErosionModel
    H = W = 8192
    r = np.random.default_rng(8192)
    base = r.standard_normal((H, W, 2), dtype=np.float32)
    host = {}
    for k, name in enumerate(READ):   # every plane its own affine image of one draw (the draw is the slow part)
        a = (base if name in ("layers", "velocity", "debrisVelocity") else base[..., k % 2]) * np.float32(1.5 + k)
        host[name] = (a + np.float32(k - 2.5))[None]
    m = ErosionModel(H, W, (1.0, 1.0, 1.0), soil.param_t(), 16)
    for name, a in host.items():
        silt.set(getattr(m, name), to_gpu(a[0]))
    st = m.stats()
    assert st.shape == (10,)
    _check_model(st, host, 0)


# ---------------------------------------------------------------- 3. non-finite values

def _poison(a, r, b, comp):
    """NaN, +inf and -inf at scattered cells of model b of plane `a` (component `comp` of a 2-channel plane);
    returns how many of each."""
    view = a[b] if comp is None else a[b][..., comp]   # (H, W), a view
    at = r.choice(view.size, size=max(3, view.size // 9), replace=False)
    view[np.unravel_index(at, view.shape)] = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), at.size)
    return at.size


@pytest.mark.parametrize("channel", sorted(STORED), ids=lambda c: "ch%d" % c)
def test_nan_and_infinities_are_counted(hip, channel):
    B, bad, H, W = 3, 1, 37, 53
    clean = _random_read_planes(B, H, W, seed=300 + channel)
    dirty = {name: a.copy() for name, a in clean.items()}
    name, comp = STORED[channel]
    count = _poison(dirty[name], np.random.default_rng(channel), bad, comp)
    want, got = _filled(clean, B, H, W).stats(), _filled(dirty, B, H, W).stats()
    assert got[bad, channel]["nonfinite"] == count
    if channel < 2:   # a non-finite layer is a non-finite height
        assert got[bad, 2]["nonfinite"] == count
    for c in range(10):
        if c != channel and not (channel < 2 and c == 2):
            assert got[bad, c].tobytes() == want[bad, c].tobytes(), "channel %d of the poisoned model" % c
    _check_model(got[bad], dirty, bad, "poisoned ")   # the finite statistics: those of the remaining cells
    for b in range(B):
        if b != bad:
            assert got[b].tobytes() == want[b].tobytes(), "model %d" % b
            assert not got[b]["nonfinite"].any()


def test_a_model_with_no_finite_cell(hip):
    B, bad, H, W = 3, 2, 37, 53
    clean = _random_read_planes(B, H, W, seed=41)
    dirty = {name: a.copy() for name, a in clean.items()}
    r = np.random.default_rng(42)
    for name in READ:
        dirty[name][bad] = r.choice(np.array([np.nan, np.inf, -np.inf], np.float32), size=dirty[name][bad].shape)
    want, got = _filled(clean, B, H, W).stats(), _filled(dirty, B, H, W).stats()
    for c in range(10):
        rec = got[bad, c]
        assert rec["nonfinite"] == H * W and rec["min"] == np.inf and rec["max"] == -np.inf
        assert rec["sum"] == 0.0 and rec["sumsq"] == 0.0
    assert got[:bad].tobytes() == want[:bad].tobytes()


def test_opposite_infinities_are_one_nonfinite_height(hip):
    B, H, W = 2, 5, 8
    host = _random_read_planes(B, H, W, seed=43)
    host["layers"][1, 2, 3] = (np.inf, -np.inf)
    st = _filled(host, B, H, W).stats()
    assert [int(st[1, c]["nonfinite"]) for c in range(10)] == [1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
    assert not st[0]["nonfinite"].any()
    _check_model(st[1], host, 1)


# ---------------------------------------------------------------- 4. batch against single

@pytest.mark.parametrize("size", [(37, 53), (301, 211), (256, 256), (1, 1), (5, 1), (1, 8)], ids=_size_id)
def test_batch_against_single_byte_for_byte(hip, size):
    """37 x 53 and 301 x 211 have an odd cell count: models 1 and 3 of the batch start off a 16-byte boundary (the
    scalar loads) where the same model alone starts on one (the 16-byte loads)."""
    H, W = size
    B = 4
    host = _random_read_planes(B, H, W, seed=H * W)
    bt = _filled(host, B, H, W)
    st = bt.stats()
    assert bt.stats().tobytes() == st.tobytes(), "two calls differ"
    for b in range(B):
        alone = _single(host, b, H, W).stats()
        assert alone.shape == (10,) and alone.dtype == st.dtype
        assert alone.tobytes() == st[b].tobytes(), "model %d alone" % b
    order = [3, 1, 0]   # another B, other positions
    other = _filled({name: np.ascontiguousarray(a[order]) for name, a in host.items()}, len(order), H, W).stats()
    for k, b in enumerate(order):
        assert other[k].tobytes() == st[b].tobytes(), "model %d at position %d of a batch of %d" % (b, k, len(order))
    bigger = _filled({name: np.concatenate([a, a, a[:1]]) for name, a in host.items()}, 2 * B + 1, H, W).stats()
    for k in range(2 * B + 1):
        assert bigger[k].tobytes() == st[k % B].tobytes(), "position %d of a batch of %d" % (k, 2 * B + 1)


# ---------------------------------------------------------------- 5. after real steps

@pytest.mark.parametrize("B,H,W,N", [(3, 48, 40, 600), (2, 128, 128, 4096)])
def test_after_real_steps(hip, oracle, B, H, W, N):
    bt = _batch(B, H, W, (20.0 / H, 20.0 / W, 4.0), _param(oracle, 48), N, [5 + 3 * b for b in range(B)],
                _inputs(oracle, B, H, W))
    for _ in range(3):
        bt.step()
    st = bt.stats()
    planes = [bt.model_planes(b) for b in range(B)]
    host = {name: np.stack([p[name] for p in planes]) for name in READ}
    for b in range(B):
        _check_model(st[b], host, b)
        # the height channel is the `height` plane (layer_merge of the same layers)
        assert_bit_equal(_channels(host, b)[2], planes[b]["height"].reshape(-1), "height of model %d" % b)
        _check_channel(st[b, 2], planes[b]["height"].reshape(-1), "model %d: the height plane" % b)
        assert st[b, 3]["max"] > 0 and st[b, 0]["nonfinite"] == 0   # the steps left water and finite terrain


# ---------------------------------------------------------------- 6. the ensemble

def _ensemble_planes(host, b):
    """(H, W, 6): the six ensemble channels of model b, fp32."""
    l = host["layers"][b]
    with np.errstate(invalid="ignore"):
        height = l[..., 0] + l[..., 1]
    return np.stack([l[..., 0], l[..., 1], height, host["waterHeight"][b], host["mass"][b], host["debris"][b]], axis=-1)


def _ensemble_expected(host, B):
    """The contract restated: s and q are fp64 sums over b in order, then the expressions as written."""
    shape = host["waterHeight"].shape[1:] + (6,)
    s, q = np.zeros(shape, np.float64), np.zeros(shape, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            v = _ensemble_planes(host, b).astype(np.float64)
            s = s + v
            q = q + v * v
        m = s / np.float64(B)
        mean = m.astype(np.float32)
        v = q / np.float64(B) - m * m
        var = np.where(v < 0, 0.0, v).astype(np.float32)
    return mean, var


@pytest.mark.parametrize("B", [1, 2, 7, 64])
@pytest.mark.parametrize("size", RAGGED + SQUARE, ids=_size_id)
def test_ensemble_bit_for_bit(hip, size, B):
    H, W = size
    host = _random_read_planes(B, H, W, seed=H + 3 * W + B, names=ENSEMBLE_READ)
    bt = _filled(host, B, H, W)
    mean, var = bt.ensemble()
    for t in (mean, var):
        assert tuple(t.shape) == (H, W, 6) and t.host.name == "gpu"
    want_mean, want_var = _ensemble_expected(host, B)
    assert_bit_equal(to_np(mean), want_mean, "mean")
    assert_bit_equal(to_np(var), want_var, "var")
    assert (to_np(var) >= 0).all()
    if B == 1:
        assert_bit_equal(to_np(mean), _ensemble_planes(host, 0), "mean of one model")
        assert not to_np(var).view(np.uint32).any(), "var of one model is not all +0.0"
    only, none = bt.ensemble(var=False)
    assert none is None
    assert_bit_equal(to_np(only), want_mean, "mean alone")
    for name, a in host.items():
        assert_bit_equal(to_np(getattr(bt, name)), a, "the source: " + name)


def test_ensemble_of_identical_models(hip):
    """B copies of one model: the mean is the model; the variance is that of the one-pass formula (not forced to
    zero: q / B and m * m round separately), which the restatement gives bit for bit."""
    B, H, W = 7, 37, 53
    one = _random_read_planes(1, H, W, seed=5, names=ENSEMBLE_READ)
    host = {name: np.repeat(a, B, axis=0) for name, a in one.items()}
    mean, var = _filled(host, B, H, W).ensemble()
    want_mean, want_var = _ensemble_expected(host, B)
    assert_bit_equal(to_np(mean), want_mean, "mean")
    assert_bit_equal(to_np(var), want_var, "var")
    m = _ensemble_planes(one, 0).astype(np.float64)
    # the cancellation limit stated in the header: |var| <~ a few 2^-53 * m^2 where the true variance is 0
    assert (to_np(var).astype(np.float64) <= 8 * B * U * m * m).all()


def test_ensemble_a_poisoned_cell_spoils_only_itself(hip):
    B, H, W = 7, 37, 53
    clean = _random_read_planes(B, H, W, seed=66, names=ENSEMBLE_READ)
    dirty = {name: a.copy() for name, a in clean.items()}
    dirty["waterHeight"][3, 5, 7] = np.nan
    dirty["layers"][0, 10, 11, 0] = np.inf
    dirty["layers"][6, 36, 52] = (np.inf, -np.inf)
    dirty["debris"][2, 0, 0] = -np.inf
    cells = [(5, 7), (10, 11), (36, 52), (0, 0)]
    want = [to_np(t) for t in _filled(clean, B, H, W).ensemble()]
    got = [to_np(t) for t in _filled(dirty, B, H, W).ensemble()]
    expected = _ensemble_expected(dirty, B)
    spoiled = np.zeros((H, W), bool)
    for cell in cells:
        spoiled[cell] = True
    for g, w, e, what in zip(got, want, expected, ("mean", "var")):
        assert_bit_equal(g, e, what)
        assert_bit_equal(g[~spoiled], w[~spoiled], what + " of the other cells")
        assert np.isfinite(g[~spoiled]).all()
        for cell in cells:
            assert not np.isfinite(g[cell]).all(), "%s at %s" % (what, cell)
    assert np.isnan(got[0][5, 7, 3]) and np.isfinite(got[0][5, 7, [0, 1, 2, 4, 5]]).all()   # its channel only
    assert got[0][10, 11, 0] == np.inf and got[0][10, 11, 2] == np.inf
    assert np.isnan(got[0][36, 52, 2]) and got[0][0, 0, 5] == -np.inf


# ---------------------------------------------------------------- 7. more models than one launch holds

def test_65537_models(hip):
    """B = 65537 models of 2 x 2: two pairs of launches (grid.z <= 65535); the first pair's first, second and last two
    models and the second pair's two, each against numpy, and against the same model alone."""
    B = 65537
    bt, host = _source(B, 2, 2, False, seed=65537)
    st = bt.stats()
    _assert_stats_shape(st, B)
    for b in (0, 1, 65533, 65534, 65535, 65536):
        _check_model(st[b], host, b)
        assert _single({name: host[name] for name in READ}, b, 2, 2).stats().tobytes() == st[b].tobytes()
    # every record, cheaply: n = 4 finite cells each
    assert not st["nonfinite"].any()
    layers = host["layers"].reshape(B, 4, 2)
    assert np.array_equal(st[:, 0]["min"], layers[..., 0].min(axis=1))
    assert np.array_equal(st[:, 1]["max"], layers[..., 1].max(axis=1))
    assert np.array_equal(st[:, 4]["max"], host["mass"].reshape(B, 4).max(axis=1))


# ---------------------------------------------------------------- 8. another stream, refusals

def test_on_another_stream(hip):
    import torch
    from soillib_amd import _abi
    B, H, W = 3, 37, 53
    host = _random_read_planes(B, H, W, seed=8)
    want_st = _filled(host, B, H, W).stats()
    want_mean, want_var = _ensemble_expected(host, B)
    s = torch.cuda.Stream()
    _abi.set_stream(s.cuda_stream)
    try:
        bt = _filled(host, B, H, W)
        st = bt.stats()
        mean, var = bt.ensemble()
        s.synchronize()
        assert st.tobytes() == want_st.tobytes()
        assert_bit_equal(to_np(mean), want_mean, "mean")
        assert_bit_equal(to_np(var), want_var, "var")
        s.synchronize()
    finally:
        _abi.set_stream(0)


def test_invalid_arguments_are_refused(hip):
    from soillib_amd import _abi, silt
    lib = _abi.lib()
    B, H, W = 2, 8, 12
    bt = _filled(_random_read_planes(B, H, W, seed=1), B, H, W)
    planes = bt._planes()
    out = silt.tensor(silt.float32, silt.shape(B, 80), silt.gpu)
    mean = silt.tensor(silt.float32, silt.shape(H, W, 6), silt.gpu)
    var = silt.tensor(silt.float32, silt.shape(H, W, 6), silt.gpu)
    silt.set(out, 7.0)
    silt.set(mean, 7.0)
    silt.set(var, 7.0)

    def without(field):
        p = _abi.ErosionPlanes()
        for f, _ in _abi.ErosionPlanes._fields_:
            setattr(p, f, None if f == field else getattr(planes, f))
        return p

    def refused(rc, entry, naming):
        assert rc == _abi.SOIL_ERR_INVALID_ARGUMENT, (entry, naming, rc)
        assert entry in _abi.last_error() and naming in _abi.last_error(), (entry, naming, _abi.last_error())

    def stats(naming, p=planes, sizes=(B, H, W), o=out):
        ref = None if p is None else C.byref(p)
        refused(lib.soil_erode_batch_stats(ref, *sizes, None if o is None else o.c_ptr, None), "erode_batch_stats",
                naming)

    def ensemble(naming, p=planes, sizes=(B, H, W), m=mean, v=var):
        ref = None if p is None else C.byref(p)
        refused(lib.soil_erode_batch_ensemble(ref, *sizes, None if m is None else m.c_ptr,
                                              None if v is None else v.c_ptr, None), "erode_batch_ensemble", naming)

    for call in (stats, ensemble):
        call("B >= 1", sizes=(0, H, W))
        call("B >= 1", sizes=(-3, H, W))
        call("empty grid", sizes=(B, 0, W))
        call("empty grid", sizes=(B, H, -1))
        call("overflow", sizes=(B, 1 << 40, 1 << 20))
        call("overflow", sizes=(1 << 40, 1 << 12, 1 << 12))
        call("null planes", p=None)
    stats("null planes or out", o=None)
    ensemble("null mean", m=None)
    for field in READ:
        stats("null plane", p=without(field))
    for field in ENSEMBLE_READ:
        ensemble("null plane", p=without(field))
    # nothing was launched: the outputs still hold their fill
    for t in (out, mean, var):
        assert (to_np(t) == 7.0).all()
    # what is not read may be NULL
    p = _abi.ErosionPlanes()
    for f in READ:
        setattr(p, f, getattr(planes, f))
    assert lib.soil_erode_batch_stats(C.byref(p), B, H, W, out.c_ptr, None) == _abi.SOIL_OK
    assert lib.soil_erode_batch_ensemble(C.byref(p), B, H, W, mean.c_ptr, None, None) == _abi.SOIL_OK
    from soillib_amd.erosion import STATS_DTYPE
    assert to_np(out).view(STATS_DTYPE).reshape(B, 10).tobytes() == bt.stats().tobytes()
    assert_bit_equal(to_np(mean), to_np(bt.ensemble(var=False)[0]), "mean")
    assert (to_np(var) == 7.0).all()   # var = NULL writes no second plane


def test_stats_of_a_row_slab_is_refused(hip):
    from soillib_amd import _abi, soil
    from soillib_amd.erosion import ErosionModel
    m = ErosionModel(16, 8, (1.0, 1.0, 1.0), soil.param_t(), 16, dom=_abi.Domain(16, 8, 0, 8, 0, 8))
    with pytest.raises(ValueError, match="row slab"):
        m.stats()
