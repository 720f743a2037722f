"""A number is a number whatever its type: stream_power, stream_power_deposit, diffuse and their _batch forms given
numpy scalars (np.float32 / np.int64: what area.max(), np.float32(dt) and friends hand in) return word for word what
they return for float(x) / int(x) of the same values, out and out64 alike, and so does ErosionBatch.stream_power.  On
a (5, 7) grid and a batch of two models with a scale pair each; every comparison is of bit patterns."""
import numpy as np
import pytest

import flow_paths_ref as ref
from flow_paths_ref import D8
from util import to_gpu, to_np

pytestmark = pytest.mark.gpu

H, W, B = 5, 7, 2
PAIRS = [(0.3, 0.7), (2.5, 0.125)]
# values a float32 holds exactly, so that np.float32(x) and float(np.float32(x)) are the number x
DT, KAPPA, ITERS = 0.5, 0.25, 2


def _words(t):
    a = to_np(t)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _planes(batch):
    hs = np.stack([(ref.terrain(H, W, 2 + i) * 10).astype(np.float32) for i in range(B)])
    gs = np.stack([ref.descent(h, D8) for h in hs])
    r = np.random.default_rng(5)
    k = r.uniform(1e-3, 1e-1, hs.shape).astype(np.float32)
    d = r.uniform(0.0, 0.5, hs.shape).astype(np.float32)
    cut = (lambda p: p) if batch else (lambda p: p[0])
    return [to_gpu(cut(p)) for p in (hs, gs, k, d)]


@pytest.mark.parametrize("batch", [False, True])
def test_numpy_scalars_give_the_words_of_python_numbers(hip, batch):
    from soillib_amd import soil
    h, g, k, d = _planes(batch)
    scale = PAIRS if batch else PAIRS[0]
    power = soil.stream_power_batch if batch else soil.stream_power
    deposit = soil.stream_power_deposit_batch if batch else soil.stream_power_deposit
    diffuse = soil.diffuse_batch if batch else soil.diffuse
    for double in (False, True):
        want = _words(power(h, g, k, D8, scale, DT, double=double))
        for dt in (np.float32(DT), np.float64(DT)):
            assert (_words(power(h, g, k, D8, scale, dt, double=double)) == want).all(), (type(dt), double)
        want = _words(power(h, g, k, D8, scale, 1, double=double))
        assert (_words(power(h, g, k, D8, scale, np.int64(1), double=double)) == want).all(), double

        want = [_words(t) for t in deposit(h, g, k, d, D8, scale, DT, iters=ITERS, double=double, flux=True, residual=True)]
        got = deposit(h, g, k, d, D8, scale, np.float32(DT), iters=np.int64(ITERS), double=double, flux=True, residual=True)
        for w, t, name in zip(want, got, ("heights", "flux", "residual")):
            assert (_words(t) == w).all(), (name, double)
        assert soil.stream_power_deposit_info()["iters"] == ITERS

        want = _words(diffuse(h, scale, DT, kappa=KAPPA, double=double))
        assert (_words(diffuse(h, scale, np.float32(DT), kappa=np.float32(KAPPA), double=double)) == want).all(), double
        want = _words(diffuse(h, scale, 1, kappa=1, double=double))
        assert (_words(diffuse(h, scale, np.int64(1), kappa=np.int64(1), double=double)) == want).all(), double
    assert not (_words(power(h, g, k, D8, scale, DT)) == _words(power(h, g, k, D8, scale, 1))).all(), "dt is read"


def test_the_batch_method_takes_numpy_scalars(hip):
    from soillib_amd import silt, soil
    from soillib_amd.erosion import ErosionBatch
    bt = ErosionBatch(2, 8, 8, [(0.3, 0.7, 1.0), (2.5, 0.125, 1.0)], soil.param_t(), 16, [1, 2])
    silt.set(bt.height, to_gpu(np.stack([(ref.terrain(8, 8, 7 + i) * 10).astype(np.float32) for i in range(2)])))
    K = float(np.float32(1e-3))
    want = _words(bt.stream_power(dt=0.5, K=K))
    got = bt.stream_power(dt=np.float32(0.5), K=np.float32(1e-3))
    assert (_words(got) == want).all() and np.isfinite(to_np(got)).all()
