"""A numpy restatement of the depression fill (include/soil_hip.h: soil_fill_depressions and its _batch form; not a
test module), the lake-rich DEM the batch tests fill, and the models those tests share.

The restatement is the defining iteration itself, w <- max(z, min over the K neighbours of w), on whole planes from
+inf until no bit changes; a cell off the grid and a NaN cell count as -inf, and NaN is put back at the end.  Only min
and max are involved, so it meets the priority-flood oracle bit for bit wherever the DEM holds no -0 (min and max do
not order the two zeros: there the two are equal in value and every output is a zero, compare())."""
import functools

import numpy as np

import flats_ref
from flats_ref import D4, D8, DX, DY  # noqa: F401
from util import assert_bit_equal


def fill(z, edge):
    """The fixed point of w <- max(z, min over the K neighbours of w) below +inf."""
    z = np.asarray(z, np.float32)
    H, W = z.shape
    K = 4 if edge == D4 else 8
    nan = np.isnan(z)
    ninf = np.float32(-np.inf)
    lo = np.where(nan, ninf, z)
    w = np.where(nan, ninf, np.float32(np.inf)).astype(np.float32)
    while True:
        pad = np.full((H + 2, W + 2), ninf, np.float32)
        pad[1:-1, 1:-1] = w
        m = pad[1 + DX[0]:1 + DX[0] + H, 1 + DY[0]:1 + DY[0] + W]
        for k in range(1, K):
            m = np.minimum(m, pad[1 + DX[k]:1 + DX[k] + H, 1 + DY[k]:1 + DY[k] + W])
        new = np.where(nan, ninf, np.maximum(lo, m)).astype(np.float32)
        if (new.view(np.uint32) == w.view(np.uint32)).all():
            break
        w = new
    return np.where(nan, np.float32(np.nan), w).astype(np.float32)


def has_negative_zero(z):
    z = np.asarray(z, np.float32)
    return bool((np.signbit(z) & (z == 0)).any())


def compare(got, want, dem, what=""):
    """The rule of every comparison: bit for bit on a DEM without -0; on one of zeros of both signs (the "signed
    zeros" plane) equal in value, and every output a zero."""
    if not has_negative_zero(dem):
        assert_bit_equal(got, want, what)
    else:
        assert np.array_equal(got, want, equal_nan=True), what
        assert (np.asarray(dem)[~np.isnan(dem)] == 0).all() and (np.asarray(got) == 0).all(), what


def pitted(H, W, seed):
    """A lake-rich integer DEM without the noise generator: two crossed waves, a gentle tilt and 5 units of uniform
    noise, floored.  The fill raises a quarter to a half of its cells (asserted for every model the GPU tests use:
    tests/test_fill_batch_abi.py); it holds no -0."""
    x, y = np.mgrid[0:H, 0:W].astype(np.float64)
    h = np.floor(6 * np.sin(x / 9 + seed) + 6 * np.cos(y / 7 - seed) + 0.02 * (x + y)
                 + 5 * np.random.default_rng(seed).random((H, W)))
    return h.astype(np.float32)


def small(H, W, seed):
    """Integer heights 0 .. 4 for the degenerate shapes (nothing to assert about the raised share there)."""
    return np.random.default_rng(100 + seed).integers(0, 5, (H, W)).astype(np.float32)


# every pitted model of tests/test_gpu_fill_batch.py, (H, W, seed): the raised share of each is asserted on the CPU
PITTED_USED = ([(65, 129, s) for s in (0, 1, 2)] + [(130, 130, s) for s in (0, 1, 2)]
               + [(516, 516, s) for s in (0, 1)] + [(200, 200, s) for s in (0, 1, 2)])


def used(H, W, seed):
    assert (H, W, seed) in PITTED_USED, (H, W, seed)
    return pitted(H, W, seed)


@functools.lru_cache(maxsize=None)
def model(name, H, W):
    """A model of the batch tests by name; the array is shared: do not write into it."""
    if name.startswith("pitted"):
        a = used(H, W, int(name[6:]))
    elif name == "serpentine":
        a = flats_ref.serpentine(H, W)
    elif name == "nan":
        a = np.full((H, W), np.nan, np.float32)
    elif name == "inf":
        a = np.full((H, W), np.inf, np.float32)
    else:
        a = dict(flats_ref.constructions(H, W))[name]
    a.setflags(write=False)
    return a


# the models beside the serpentine corridor, in the order a batch takes them
OTHERS = ["nan", "inf", "pitted0", "pitted1", "closed", "nan blocks", "pitted2", "denormals"]


def batch_names(B, serpentine_at):
    """B model names with the serpentine corridor at `serpentine_at`."""
    names = OTHERS[:B - 1]
    names.insert(serpentine_at, "serpentine")
    return names


_WANT = {}


def want(oracle, name, H, W, edge):
    """The oracle's fill of model(name, H, W), computed once."""
    key = (name, H, W, edge)
    if key not in _WANT:
        _WANT[key] = oracle.fill_depressions(np.array(model(name, H, W)), edge)
        _WANT[key].setflags(write=False)
    return _WANT[key]


def raised_share(dem, filled):
    ok = ~np.isnan(dem)
    return float((filled[ok] > dem[ok]).mean())
