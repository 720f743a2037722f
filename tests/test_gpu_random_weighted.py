"""soil_random_weighted (csrc/graph.hip: rw_const, rw_cdf, rw_pick) on hostile inputs.

It is the one flow kernel whose arithmetic is not the oracle's: the weights are v_exp_f32(diff * c) with the division
by |shift| T folded into a host-made constant, and a draw picks by `u Z < CDF[k]`, not `u < CDF[k] / Z`.  So it is
held here to two statements.

  the restatement    The kernel's own order of operations in numpy, with the weights taken from rw_exp2 itself
                     (soil_selftest_math op 12, the inline function rw_cdf calls).  Everything else is plain fp32:
                     the kernel's graph must equal it on every cell, bit for bit, with no cell left out.  Steep
                     terrains, overflowing and exactly uniform weights, integer heights with ties, zeros of both
                     signs, NaN and inf cells, every launch path (one cell or four per thread, rows of one to
                     three work-groups, unaligned planes, 1 to 4 graphs per pass, batches, window shapes), seeds
                     and offsets above 2^32, the draws u = 1.0 and u = 2^-24, T at the ends of its range.
  the oracle         The reference's exact statement (expf_, IEEE divisions), with a per-cell tolerance derived from
                     the arithmetic (test_against_the_oracle_with_a_derived_tolerance) instead of fixed constants.

The restatement follows rw_cdf / rw_pick as written; it changes only if the kernel's written order of operations does.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from util import assert_bit_equal, terrain, to_gpu, to_np

pytestmark = pytest.mark.gpu

D4, D8 = 0, 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFT = ((-1, 0), (0, -1), (0, 1), (1, 0), (-1, -1), (-1, 1), (1, -1), (1, 1))    # graph.hpp:21-46
SQRT2 = np.float32(1.41421354)                                                     # soil_math.hpp: kSqrt2
LOG2E = 1.4426950408889634
FLT_MIN, FLT_MAX = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
BIG = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 5)


# ------------------------------------------------------------------ the restatement

def op12(hip, a, b):
    """rw_exp2(a, b) = v_exp_f32(fl(a * b)) on the device, element by element."""
    from soillib_amd import _abi
    a = np.ascontiguousarray(a, np.float32).ravel()
    b = np.ascontiguousarray(b, np.float32).ravel()
    ga, gb, out = to_gpu(a), to_gpu(b), to_gpu(np.zeros_like(a))
    _abi.check(hip.soil_selftest_math(out.c_ptr, ga.c_ptr, gb.c_ptr, a.size, 12, None))
    return to_np(out)


def rw_const(T):
    """rw_const: a double quotient, then a float, for the straight and the diagonal neighbours."""
    T = np.float64(np.float32(T))
    with np.errstate(all="ignore"):
        return np.float32(np.float64(LOG2E) / T), np.float32(np.float64(LOG2E) / (np.float64(SQRT2) * T))


def neighbours(h, K):
    """(K, H, W) planes: neighbour k's height (0 off the grid), whether it lies in the grid, its flat index."""
    H, W = h.shape
    pad = np.zeros((H + 2, W + 2), np.float32)
    pad[1:-1, 1:-1] = h
    idx = np.full((H + 2, W + 2), -1, np.int64)
    idx[1:-1, 1:-1] = np.arange(H * W).reshape(H, W)
    hn = np.stack([pad[1 + dx:1 + dx + H, 1 + dy:1 + dy + W] for dx, dy in SHIFT[:K]])
    to = np.stack([idx[1 + dx:1 + dx + H, 1 + dy:1 + dy + W] for dx, dy in SHIFT[:K]])
    return hn, to >= 0, to.astype(np.int32)


def restate_cdf(exp2, h, edge, T):
    """rw_cdf on every cell.  `exp2(a, b)`: the weights' primitive (op 12 on the device)."""
    K = 4 if edge == D4 else 8
    h = np.ascontiguousarray(h, np.float32)
    hn, ok, to = neighbours(h, K)
    straight, diagonal = rw_const(T)
    with np.errstate(all="ignore"):
        diff = h[None] - hn                                            # 1. fl(h - hn)
        c = np.empty_like(diff)                                        # 2. the two constants
        c[:4], c[4:] = straight, diagonal
        P = np.where(diff <= 0, np.float32(0), exp2(diff, c).reshape(diff.shape))   # (NaN <= 0 is false)
        P = np.where(ok, P, np.float32(0)).astype(np.float32)          # 3. no weight off the grid
        CDF = np.empty_like(P)
        Z = np.zeros(h.shape, np.float32)
        for k in range(K):                                             # 4. CDF[k] = fl(Z + P), in neighbour order
            CDF[k] = Z + P[k]
            Z = CDF[k]
    return CDF, Z, ok, to


def restate_pick(cdf, u):
    """rw_pick: the lowest in-grid k with fl(u Z) < CDF[k], else -1."""
    CDF, Z, ok, to = cdf
    with np.errstate(all="ignore"):
        uz = np.asarray(u, np.float32).reshape(Z.shape) * Z            # 5.
    nxt = np.full(Z.shape, -1, np.int32)
    for k in reversed(range(len(CDF))):                                # 6.
        nxt = np.where(ok[k] & (uz < CDF[k]), to[k], nxt)
    return nxt


_DRAWS = {}


def draws(oracle, seed, offset, n):
    key = (seed, offset, n)
    if key not in _DRAWS:
        _DRAWS[key] = oracle.rng_uniform_cell(seed, offset, range(n))
    return _DRAWS[key]


def restate(hip, oracle, h, edge, seed, offset, T):
    return restate_pick(restate_cdf(lambda a, b: op12(hip, a, b), h, edge, T), draws(oracle, seed, offset, h.size))


def assert_graph_properties(h, got, edge, what):
    """A receiver is -1 or an in-grid neighbour that is strictly lower or unordered with the cell (NaN); a cell
    without such a neighbour has -1."""
    K = 4 if edge == D4 else 8
    hn, ok, to = neighbours(h, K)
    with np.errstate(invalid="ignore"):
        may = ok & ~(h[None] <= hn)
    hit = ((got[None] == to) & may).any(0)
    assert ((got == -1) | hit).all(), "%s: a receiver that is no lower neighbour" % what
    assert (got[~may.any(0)] == -1).all(), "%s: a receiver in a cell without a lower neighbour" % what


def device_graph(h, edge, seed, offset, T):
    from soillib_amd import soil
    return to_np(soil.random_weighted(to_gpu(h), edge, seed, offset, T))


def check_kernel(hip, oracle, h, edge, seed, offset, T, what):
    """The kernel's graph for `h`: twice the same bits, the properties, and the restatement on every cell."""
    h = np.ascontiguousarray(h, np.float32)
    what = "%s %s %dx%d T=%g seed=%d offset=%d" % (what, "d4" if edge == D4 else "d8", h.shape[0], h.shape[1], T,
                                                  seed, offset)
    got = device_graph(h, edge, seed, offset, T)
    assert got.dtype == np.int32 and got.shape == h.shape
    assert_bit_equal(device_graph(h, edge, seed, offset, T), got, what + ": a second call")
    assert_graph_properties(h, got, edge, what)
    assert_bit_equal(got, restate(hip, oracle, h, edge, seed, offset, T), what + ": kernel vs restatement")
    return got


# ------------------------------------------------------------------ inputs

_BASE = {}


def base(oracle, H, W):
    """The noise terrain of the parity tests (heights in about [-1, 1]), read-only."""
    if (H, W) not in _BASE:
        b = terrain(oracle, H, W)[..., 0].copy()
        b.setflags(write=False)
        _BASE[(H, W)] = b
    return _BASE[(H, W)]


def slopes(h, edge, T):
    """x = dE / T in float64 on every (k, cell), -inf where neighbour k is not a lower in-grid neighbour."""
    K = 4 if edge == D4 else 8
    hn, ok, to = neighbours(h, K)
    with np.errstate(all="ignore"):
        d = (h[None] - hn).astype(np.float64)                         # the float difference both sides take
        s = np.array([1.0] * 4 + [float(SQRT2)] * 4)[:K, None, None]
        x = np.where(ok & (d > 0), d / (s * np.float64(np.float32(T))), -np.inf)
    return x, to


STEEP = [(scale, T) for scale in (1.0, 100.0, 1e4) for T in (1e-2, 1.0, 10.0, 1e4)]
STEEP_SHAPES = [(33, 50), (64, 64)]          # the one-cell kernel; the four-cell kernel


def with_specials(h):
    """NaN, +inf and -inf cells placed singly and in pairs, in the interior and on the border (grids >= 12 x 12)."""
    h = np.array(h, np.float32)
    H, W = h.shape
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    h[0, 0] = nan                                   # corner
    h[0, W // 2] = inf                              # border
    h[H - 1, 3] = -inf
    h[H // 2, 0], h[H // 2 + 1, 0] = nan, inf       # a pair on the border
    h[3, 3] = nan                                   # interior, single
    h[5, 7] = inf
    h[7, 5] = -inf
    h[9, 9], h[9, 10] = nan, nan                    # interior pairs
    h[H - 3, W - 4], h[H - 4, W - 3] = inf, -inf    # diagonal pair
    h[H - 6, W - 6], h[H - 6, W - 5] = inf, inf
    return h


def integer_inputs(oracle, H, W):
    """name -> heights: quantised terrain (ties, Z = 0 cells scattered everywhere), patterns with exactly one
    downhill neighbour, fields of zeros of both signs, NaN and inf cells."""
    b = base(oracle, H, W)
    x, y = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    r = np.random.default_rng(5)
    out = {
        "quantised": np.floor(b * 8.0),
        "quantised coarse": np.floor(b * 2.0),
        "checkerboard": ((x + y) % 2).astype(np.float32) * 3.0,
        "pits": np.where((x % 3 == 1) & (y % 3 == 1), 0.0, 2.0),                 # one lower neighbour: the pit
        "channels": np.where(x % 2 == 0, 1000.0, -1.0 * y),                      # walls; channels running east
        "zeros of both signs": np.where(r.random((H, W)) < 0.5, -0.0, 0.0),
        "constant": np.full((H, W), 7.0),
    }
    out = {k: v.astype(np.float32) for k, v in out.items()}
    out["quantised with NaN and inf"] = with_specials(out["quantised"])
    out["noise with NaN and inf"] = with_specials(b * 100.0)
    return out


def single_lower(h, edge, T):
    """Cells with exactly one lower in-grid neighbour, no unordered one and a weight that does not overflow
    (dE / T < 88), and that neighbour's index."""
    K = 4 if edge == D4 else 8
    hn, ok, to = neighbours(h, K)
    with np.errstate(invalid="ignore"):
        lower = ok & (hn < h[None])
        unordered = ok & (np.isnan(hn) | np.isnan(h[None]))
        infinite = ok & np.isinf(h[None] - hn)
    one = (lower.sum(0) == 1) & ~unordered.any(0) & ~infinite.any(0) & (slopes(h, edge, T)[0].max(0) < 88)
    return one, np.where(lower, to, 0).sum(0).astype(np.int32)


# ------------------------------------------------------------------ 1. the hook: op 12

def test_weight_primitive(hip):
    """op 12, v_exp_f32(fl(a b)), against 2^(a b) in float64 within the bound test_particle_step_primitives states
    for op 8: 1 ulp of the exponential (2^-22 covers it) plus the half-ulp of the rounded product carried through,
    |x| 1.5 2^-24 with x = a b ln 2 the natural argument.  Arguments a b across [-150, 130].

    Recorded on gfx950: results below 2^-126 are FLUSHED to +0, none comes out denormal (2^-126 itself is exact,
    2^-127 and below give 0) — the kernel's weights, with diff > 0 and T > 0, are all >= 1 and never get there;
    +inf -> +inf, -inf -> 0, NaN -> NaN, 0 * inf -> NaN; the product's own overflow gives +inf."""
    r = np.random.default_rng(12)
    n = 200000
    a = np.concatenate([r.uniform(-150, 130, n), r.uniform(-150, 130, n) / 3e4, np.linspace(-150, 130, 281)])
    b = np.concatenate([np.ones(n), np.full(n, 3e4), np.ones(281)])
    a, b = a.astype(np.float32), b.astype(np.float32)
    got = op12(hip, a, b).astype(np.float64)
    p = a.astype(np.float64) * b.astype(np.float64)
    want = np.exp2(p)
    normal = (p > -126) & (p < 127.99)
    err = np.abs(got[normal] / want[normal] - 1.0)
    bound = 2.0 ** -22 + np.abs(p[normal]) * np.log(2.0) * 1.5 * 2.0 ** -24
    print("op 12: largest error / bound %.3f over %d arguments" % ((err / bound).max(), normal.sum()))
    assert (err <= bound).all()
    # exact powers of two: what the uniform-weight and overflow cases rest on
    k = np.arange(-126, 128, dtype=np.float32)
    assert_bit_equal(op12(hip, k, np.ones_like(k)), np.exp2(k.astype(np.float64)).astype(np.float32), "2^k")
    # below 2^-126: flushed to +0 (just under -126 a result may still round up to 2^-126)
    low = p < -126.001
    assert low.sum() > 1000
    assert_bit_equal(got[low], np.zeros(low.sum()), "results below 2^-126")
    edge = (p <= -126) & ~low
    assert ((got[edge] == 0) | (np.abs(got[edge] / want[edge] - 1.0) <= 2.0 ** -21)).all()
    high = p > 128.001                                              # 2^128 and above: +inf
    assert high.sum() > 1000 and np.isposinf(got[high]).all()
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    a = np.array([inf, -inf, nan, 1.0, 0.0, inf, 1e30, -1e30, 128.0, 127.99999, -0.0, 0.0, 1e-30], np.float32)
    b = np.array([1.0, 1.0, 1.0, nan, inf, -1.0, 1e30, 1e30, 1.0, 1.0, 5.0, 5.0, 1e-30], np.float32)
    want = np.array([inf, 0.0, nan, nan, nan, 0.0, inf, 0.0, inf, 0.0, 1.0, 1.0, 1.0], np.float32)
    got = op12(hip, a, b)
    assert np.isfinite(got[9]) and got[9] > 3.4e38                  # just under the overflow
    got[9] = 0.0
    assert_bit_equal(got, want, "op 12 at the edges")


def test_unknown_ops_are_refused(hip):
    from soillib_amd import _abi
    t = to_gpu(np.zeros(4, np.float32))
    for op in (-1, 13):
        assert hip.soil_selftest_math(t.c_ptr, t.c_ptr, t.c_ptr, 4, op, None) == _abi.SOIL_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------ 2. the kernel against its restatement

@pytest.mark.parametrize("scale,T", STEEP)
def test_steep_terrains(hip, oracle, scale, T):
    for H, W in STEEP_SHAPES:
        for edge in (D4, D8):
            check_kernel(hip, oracle, base(oracle, H, W) * np.float32(scale), edge, 3, 1, T, "noise x %g" % scale)


def test_steep_terrains_are_steep(oracle):
    """|dE / T| reaches 1, 10 and 60 on many cells of the steep set, below the overflow (x < 88)."""
    H, W = STEEP_SHAPES[1]
    reach = {1: 0, 10: 0, 60: 0}
    for scale, T in STEEP:
        x = slopes(base(oracle, H, W) * np.float32(scale), D8, T)[0].max(0)
        for lo in reach:
            reach[lo] += int(((x >= lo) & (x < 88)).sum())
    print("cells of the steep set with lo <= max dE/T < 88:", reach)
    assert all(v >= 200 for v in reach.values()), reach


def _overflow_inputs(oracle, H, W):
    """(h, T above the overflow, T just below it): noise x 100; a tenth of the downhill differences overflow at the
    first T; at the second the steepest weight is e^86 = 2.2e37, so Z is finite (<= 8 e^86 = 1.8e38)."""
    h = base(oracle, H, W) * np.float32(100.0)
    x = slopes(h, D8, 1.0)[0]
    return h, float(np.float32(np.quantile(x[np.isfinite(x)], 0.9) / 88.0)), float(np.float32(x.max() / 86.0))


@pytest.mark.parametrize("H,W", STEEP_SHAPES)
def test_overflowing_weights(hip, oracle, H, W):
    """Cells with a weight of +inf: Z = inf, inf < inf is false, -1 — the oracle's inf / inf.  And just below the
    overflow, Z finite and about 1e38."""
    h, t_over, t_below = _overflow_inputs(oracle, H, W)
    for edge in (D4, D8):
        got = check_kernel(hip, oracle, h, edge, 3, 0, t_over, "overflow")
        CDF, Z, ok, to = restate_cdf(lambda a, b: op12(hip, a, b), h, edge, t_over)
        over = np.isinf(Z)
        assert over.sum() > h.size // 20 and (~over).sum() > h.size // 20, over.sum()
        want = oracle.random_weighted(h, edge, 3, 0, t_over)
        assert (got[over] == -1).all() and (want[over] == -1).all()
        check_kernel(hip, oracle, h, edge, 3, 0, t_below, "below overflow")
        Z = restate_cdf(lambda a, b: op12(hip, a, b), h, edge, t_below)[1]
        assert np.isfinite(Z).all() and Z.max() > 1e37, Z.max()


def test_uniform_weights(hip, oracle):
    """T = 1e30: every downhill weight is exactly 1.0f (confirmed through op 12), the CDF holds small integers and
    the pick is integer arithmetic on u: the kernel, the restatement and the oracle agree bit for bit.  That
    fl(u Z) < k and u < fl(k / Z) agree for every draw that occurs is asserted in numpy."""
    T = 1e30
    for H, W in STEEP_SHAPES:
        h = base(oracle, H, W) * np.float32(100.0)
        for edge in (D4, D8):
            hn, ok, to = neighbours(h, 4 if edge == D4 else 8)
            diff = (h[None] - hn)[ok & (h[None] - hn > 0)]
            for c in rw_const(T):
                assert (op12(hip, diff, np.full_like(diff, c)) == np.float32(1.0)).all()
            for seed, offset in ((0, 0), (7, 3)):
                got = check_kernel(hip, oracle, h, edge, seed, offset, T, "uniform weights")
                assert_bit_equal(got, oracle.random_weighted(h, edge, seed, offset, T), "uniform weights vs oracle")
        u = np.unique(np.concatenate([draws(oracle, s, o, H * W) for s, o in ((0, 0), (7, 3))]))
        for Z in range(1, 9):
            for k in range(1, Z + 1):
                a = u * np.float32(Z) < np.float32(k)
                b = u < np.float32(k) / np.float32(Z)
                assert (a == b).all(), (Z, k)


@pytest.mark.parametrize("H,W", STEEP_SHAPES)
def test_integer_heights(hip, oracle, H, W):
    """Ties, scattered Z = 0 cells, zeros of both signs, NaN and inf cells.  Where exactly one neighbour is lower
    the receiver is that neighbour whatever the draw (no draw of these seeds is 1.0)."""
    inputs = integer_inputs(oracle, H, W)
    q = inputs["quantised"]
    assert ((q[:, 1:] == q[:, :-1]).mean() > 0.2) and (slopes(q, D8, 10.0)[0].max(0) == -np.inf).sum() > 20
    for name, h in inputs.items():
        for edge in (D4, D8):
            one, only = single_lower(h, edge, 10.0)
            if name in ("pits", "channels"):
                assert one.sum() > h.size // 8, (name, one.sum())
            for seed, offset in ((0, 0), (11, 5)):
                assert draws(oracle, seed, offset, h.size).max() < 1.0
                got = check_kernel(hip, oracle, h, edge, seed, offset, 10.0, name)
                assert (got[one] == only[one]).all(), "%s: a single lower neighbour was not taken" % name
            if name in ("zeros of both signs", "constant"):
                assert (got == -1).all(), name
    nan_cells = np.isnan(inputs["noise with NaN and inf"])
    got = device_graph(inputs["noise with NaN and inf"], D8, 0, 0, 10.0)
    assert (got[nan_cells] == -1).all()


SHAPES = [(1, 1), (1, 4), (4, 1), (1, 7),      # 1-row and 1-column grids, border and corner cells
          (2, 4), (3, 8),                      # the smallest grids of the four-cell kernel
          (5, 7), (33, 50),                    # the one-cell kernel (W % 4 != 0)
          (65, 260),                           # one wave and a ragged second
          (33, 1024), (70, 2052),              # one full work-group per row; two and a ragged third
          (300, 4), (300, 8)]                  # one thread's / two threads' cells per row


@pytest.mark.parametrize("H,W", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_shapes(hip, oracle, H, W):
    h = base(oracle, H, W) * np.float32(100.0)
    for edge in (D4, D8):
        check_kernel(hip, oracle, h, edge, 5, 2, 2.0, "shape")
    if H == 1 or W == 1:                       # a monotone line: the one lower neighbour, whatever the draw
        line = -np.arange(H * W, dtype=np.float32).reshape(H, W)
        for edge in (D4, D8):
            got = check_kernel(hip, oracle, line, edge, 5, 2, 2.0, "line")
            want = np.arange(1, H * W + 1, dtype=np.int32).reshape(H, W)
            want[-1, -1] = -1
            assert_bit_equal(got, want, "line")


@pytest.mark.parametrize("H,W", [(3, 8), (33, 52), (70, 2052)])
def test_both_kernels_on_the_same_data(hip, oracle, H, W):
    """W % 4 == 0, the plane once on 16 bytes (four cells per thread) and once as a view starting 4 bytes into its
    allocation (one cell per thread) — the heights, then the graph: the same bits, and the restatement's."""
    from soillib_amd import _abi, silt, soil
    for name, h in (("noise x 100", base(oracle, H, W) * np.float32(100.0)),
                    ("quantised", np.floor(base(oracle, H, W) * 8.0).astype(np.float32))):
        flat = np.concatenate([np.zeros(1, np.float32), h.ravel()])
        block = to_gpu(flat)
        view = silt.tensor.from_device(block.ptr + 4, silt.float32, silt.shape(H, W), keepalive=block)
        assert block.ptr % 16 == 0
        for edge in (D4, D8):
            want = restate(hip, oracle, h, edge, 9, 4, 5.0)
            aligned = to_np(soil.random_weighted(to_gpu(h), edge, 9, 4, 5.0))
            assert_bit_equal(aligned, want, "%s: aligned plane vs restatement" % name)
            assert_bit_equal(to_np(soil.random_weighted(view, edge, 9, 4, 5.0)), aligned, "%s: heights off 16 bytes" % name)
            # an unaligned graph plane, aligned heights: through the ABI
            out = to_gpu(np.full(H * W + 1, -7, np.int32))
            _abi.check(hip.soil_random_weighted(out.ptr + 4, to_gpu(h).c_ptr, H, W, edge, 9, 4, 5.0, None))
            res = to_np(out)
            assert res[0] == -7
            assert_bit_equal(res[1:].reshape(H, W), aligned, "%s: graph off 16 bytes" % name)


@pytest.mark.parametrize("H,W", [(33, 50), (16, 64)])
def test_seeds_and_offsets_above_32_bits(hip, oracle, H, W):
    h = base(oracle, H, W) * np.float32(100.0)
    pairs = [(s, o) for s in BIG for o in BIG]
    for edge in (D4, D8):
        cdf = restate_cdf(lambda a, b: op12(hip, a, b), h, edge, 3.0)
        for seed, offset in pairs:
            got = device_graph(h, edge, seed, offset, 3.0)
            assert_bit_equal(got, restate_pick(cdf, draws(oracle, seed, offset, h.size)), "seed %d offset %d" % (seed, offset))
    # the upper words matter: no two pairs draw the same
    seen = {draws(oracle, s, o, h.size).tobytes() for s, o in pairs}
    assert len(seen) == len(pairs)


# The draws u = 1.0 and u = 2^-24 (one word in 2^24 each).  Found with find_draw_cells over seed 0, the cells below
# 4096 and the offsets from 0 up (the search was bounded by 2^16 offsets = 2^28 draws): the first hits, after 3e6
# and 2.9e7 draws, are the constants below.
UNIT_DRAW = (0, 743, 1010)        # (seed, offset, cell): u = 1.0
LEAST_DRAW = (0, 7096, 1549)      # u = 2^-24


def philox_cells(seed, offset, n):
    """The 32-bit words cells 0 .. n-1 (n a multiple of 4) draw from, numpy: Philox4x32-10, key `seed`, counter
    {offset, cell >> 2}, word cell & 3 (soil_oracle.c: orc_rng_uniform_cell)."""
    m32 = np.uint64(0xFFFFFFFF)
    sub = np.arange(n // 4, dtype=np.uint64)
    c = [np.full_like(sub, int(offset) & 0xFFFFFFFF), np.full_like(sub, int(offset) >> 32), sub & m32, sub >> np.uint64(32)]
    k0, k1 = int(seed) & 0xFFFFFFFF, int(seed) >> 32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c, 1).reshape(-1).astype(np.uint32)


def find_draw_cells(seed, offsets, n, top24):
    """[(offset, cell)] with cell < n whose word's upper 24 bits are `top24` (0xFFFFFF: u = 1.0, 0: u = 2^-24)."""
    found = []
    for offset in offsets:
        hit = np.flatnonzero((philox_cells(seed, offset, n) >> np.uint32(8)) == top24)
        found += [(offset, int(c)) for c in hit]
    return found


@pytest.mark.parametrize("edge", [D4, D8])
def test_the_draws_one_and_least(hip, oracle, edge):
    """u = 1.0 (the uniform is in (0, 1]) is below no edge, the last one, CDF = Z, included: -1 although the cell
    has lower neighbours, as in the reference.  u = 2^-24 takes the first lower neighbour."""
    H = W = 64
    x, y = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    h = (-(x + y)).astype(np.float32)                                      # every cell but the last drains east / south
    for (seed, offset, cell), u_want in ((UNIT_DRAW, 1.0), (LEAST_DRAW, 2.0 ** -24)):
        assert oracle.rng_uniform_cell(seed, offset, [cell])[0] == np.float32(u_want)
        xs = slopes(h, edge, 10.0)[0][:, cell // W, cell % W]
        assert (xs > 0).sum() >= 2
        got = check_kernel(hip, oracle, h, edge, seed, offset, 10.0, "u = %g" % u_want)
        want = oracle.random_weighted(h, edge, seed, offset, 10.0)
        first = slopes(h, edge, 10.0)[1][int(np.argmax(xs > 0)), cell // W, cell % W]
        assert got.ravel()[cell] == want.ravel()[cell] == (-1 if u_want == 1.0 else first)


def test_the_numpy_generator_is_the_oracles(oracle):
    """philox_cells, which found UNIT_DRAW and LEAST_DRAW, against orc_rng_uniform_cell."""
    for seed, offset in ((0, 743), (2 ** 63 + 5, 2 ** 32), (2 ** 32 - 1, 1)):
        w = philox_cells(seed, offset, 256)
        u = ((w >> np.uint32(8)).astype(np.float32) + np.float32(1)) * np.float32(2.0 ** -24)
        assert_bit_equal(u, oracle.rng_uniform_cell(seed, offset, range(256)), "philox_cells")


@pytest.mark.parametrize("T", [FLT_MIN, 1e-30, 1e30, FLT_MAX, 0.0, -0.0])
def test_temperature_at_the_ends_of_its_range(hip, oracle, T):
    """The smallest and the largest T the entry points take, and T = 0 of either sign (every downhill weight +inf,
    or 0 for -0: every receiver -1, on both sides)."""
    for H, W in STEEP_SHAPES:
        inputs = {"noise": base(oracle, H, W), "noise x 1e4 with NaN and inf": with_specials(base(oracle, H, W) * 1e4)}
        for name, h in inputs.items():
            for edge in (D4, D8):
                got = check_kernel(hip, oracle, h, edge, 1, 1, T, name)
                if T == 0.0:
                    assert (got == -1).all()
                    assert_bit_equal(got, oracle.random_weighted(h, edge, 1, 1, T), "T = 0 vs oracle")


# ------------------------------------------------------------------ 3. against the exact statement

def oracle_error_of_expf(oracle):
    """The largest relative error of the oracle's expf_ against float64 exp over the arguments the weights take."""
    x = np.concatenate([np.linspace(0, 88.7, 20001), np.random.default_rng(1).uniform(0, 88.7, 20000)]).astype(np.float32)
    return float(np.abs(oracle.expf(x).astype(np.float64) / np.exp(x.astype(np.float64)) - 1.0).max())


def edge_tolerance(h, edge, T, u):
    """The exact CDF edges of every cell in float64 and the tolerance of each; see the test below.  Returns
    (x, to, e, delta, live, border, within)."""
    K = 4 if edge == D4 else 8
    x, to = slopes(h, edge, T)
    down = x > -np.inf
    with np.errstate(all="ignore"):
        w = np.exp(x)                                                   # 0 where not downhill; inf above 709
        Cs = np.cumsum(w, 0)
        Zs = Cs[-1]
        xmax = np.where(down, x, 0.0).max(0)
        eps = 2.0 ** -22 + xmax * 2.5 * 2.0 ** -24                      # the kernel's (>= the oracle's 2^-22 + x 2^-23)
        rel = 1.01 * (2.0 * (eps + K * 2.0 ** -24) + 2.0 ** -24)
        e = Cs / Zs
        delta = rel * e
        over = 2.0 ** 128
        border = (Zs >= over * (1 - rel)) & (Zs <= over * (1 + rel))
        live = (Zs > 0) & (Zs <= over * (1 + rel))
        near = down & (np.abs(np.asarray(u, np.float64).reshape(Zs.shape) - e) <= delta)
    within = (near.any(0) & live) | border
    return x, to, e, delta, live, border, within


def compare_with_oracle(h, edge, T, u, got, want, what):
    """(cells that differ, largest |draw - edge| / delta among them, share of cells within delta of an edge)."""
    x, to, e, delta, live, border, within = edge_tolerance(h, edge, T, u)
    H, W = h.shape
    worst = 0.0
    bad = np.argwhere(got != want)
    for i, j in bad:
        g, w_ = int(got[i, j]), int(want[i, j])
        where = "%s: cell (%d, %d), receivers %d vs %d" % (what, i, j, g, w_)
        if border[i, j] and (g == -1) != (w_ == -1):
            continue                                                    # Z overflows on one side only
        assert live[i, j], where + ": no finite positive Z"
        order = [k for k in range(len(x)) if x[k, i, j] > -np.inf]      # the neighbours with an interval, in order
        recv = [int(to[k, i, j]) for k in order] + [-1]
        assert g in recv and w_ in recv, where
        a, b = sorted((recv.index(g), recv.index(w_)))
        assert b == a + 1, where + ": not neighbours in the cumulative order"     # (-1 only across the last edge)
        k = order[a]
        ratio = abs(float(u[i * W + j]) - e[k, i, j]) / delta[k, i, j]
        assert ratio <= 1.0, where + ": the draw is %.3g delta from the edge" % ratio
        worst = max(worst, ratio)
    return len(bad), worst, float(within.mean())


ORACLE_SHAPES = [(33, 50), (160, 160)]       # the one-cell kernel; the four-cell kernel, 25600 cells
ORACLE_CASES = [(scale, T) for scale, T in STEEP] + [(100.0, 2.0), (100.0, 0.5), (100.0, 5.0)]


@pytest.mark.parametrize("scale,T", ORACLE_CASES)
def test_against_the_oracle_with_a_derived_tolerance(hip, oracle, scale, T):
    """The kernel's graph against oracle.random_weighted on the steep and the mild terrains.  A cell may differ only
    if its draw lies within delta of the exact edge between its two receivers, which must be neighbours in the
    cumulative order (so -1 only across the last edge).

    Derivation of delta.  Both sides start from the same float d = fl(h - hn) > 0; write x = d / (|shift| T) for the
    exact argument and w = e^x for the exact weight.
      kernel  c = fl(log2(e) / (|shift| T)) is off by 2^-24 relative, which the exponential turns into x 2^-24
              relative in the weight; op 12 is within 2^-22 + x 1.5 2^-24 of 2^(d c) (test_weight_primitive: 1 ulp
              of v_exp_f32 and the half-ulp of the rounded product).  Weight error <= eps = 2^-22 + x 2.5 2^-24.
      oracle  fl(d / |shift|) and fl(. / T) are off by 2^-24 each: x 2^-23 in the weight; expf_ is within 2^-22 of
              exp (asserted below on the CPU).  Weight error <= 2^-22 + x 2^-23 <= eps.
      sums    CDF[k] and Z are sums of at most K positive floats: a further K 2^-24 relative on either.
      edge    with CDF[k] and Z each within eps + K 2^-24 of exact, CDF[k] / Z is within 2 (eps + K 2^-24) relative
              of the exact edge e_k; the division's rounding (oracle) or the product's in fl(u Z) (kernel) moves the
              comparison by another 2^-24 e_k.
    Two sides whose effective edges both lie within that of e_k can only differ on a draw between them, so
      delta_k = 1.01 e_k (2 (eps + K 2^-24) + 2^-24),  x the steepest of the cell,
    the 1 % for the second-order terms.  A cell whose exact Z lies within the same relative distance of 2^128 may
    overflow on one side only: it counts as within delta, and there one side may be -1.
    The share of cells that may differ is a condition computed here in float64 alone — the cells whose draw lies
    within delta of any of their edges, or whose Z is on the overflow — and must stay under 1e-3."""
    assert oracle_error_of_expf(oracle) <= 2.0 ** -22
    for H, W in ORACLE_SHAPES:
        h = base(oracle, H, W) * np.float32(scale)
        for edge in (D4, D8):
            for seed, offset in ((3, 1), (2 ** 32 + 1, 7)):
                u = draws(oracle, seed, offset, h.size)
                got = device_graph(h, edge, seed, offset, T)
                want = oracle.random_weighted(h, edge, seed, offset, T)
                what = "noise x %g, T = %g, %s %dx%d seed %d" % (scale, T, "d4" if edge == D4 else "d8", H, W, seed)
                n, worst, share = compare_with_oracle(h, edge, T, u, got, want, what)
                print("%s: %d of %d cells differ, largest |draw - edge| / delta %.3f, share within delta %.2e" % (
                    what, n, h.size, worst, share))
                assert share < 1e-3, what


def test_the_derived_tolerance_has_teeth(oracle):
    """The check above, on the CPU, with stand-ins for the kernel: the restatement with correctly rounded weights
    passes; with the diagonal weights off by 2^-10, or with the straight constant on the diagonals, it fails on the
    inputs of the test above.  (What 51200 draws can see: an edge moved by s catches a draw in about 51200 * 5 * s
    cells, so errors well under 1e-4 go unseen here at any tolerance — those are the restatement's to catch, bit
    for bit.)"""
    def exp2(a, b, skew=0.0, straight=False):
        with np.errstate(all="ignore"):
            if straight:
                b = np.full_like(b, b[0, 0, 0])
            w = np.exp2((a * b).astype(np.float32).astype(np.float64))
            w[4:] *= 1.0 + skew
            return w.astype(np.float32)

    def differing(scale, T, **kw):
        H, W = ORACLE_SHAPES[1]
        h = base(oracle, H, W) * np.float32(scale)
        total = 0
        for seed, offset in ((3, 1), (2 ** 32 + 1, 7)):
            u = draws(oracle, seed, offset, h.size)
            got = restate_pick(restate_cdf(lambda a, b: exp2(a, b, **kw), h, D8, T), u)
            total += compare_with_oracle(h, D8, T, u, got, oracle.random_weighted(h, D8, seed, offset, T), "stand-in")[0]
        return total
    for scale, T in ((100.0, 1.0), (100.0, 10.0), (1e4, 10.0)):
        differing(scale, T)
    for kw in (dict(skew=2.0 ** -10), dict(straight=True)):
        with pytest.raises(AssertionError, match="delta from the edge|not neighbours"):
            for scale, T in ((100.0, 1.0), (100.0, 10.0), (1e4, 10.0)):
                differing(scale, T, **kw)


# ------------------------------------------------------------------ 4. the callers

def _hostile(oracle, H, W):
    """name -> (heights, T): three of the hostile terrains at one shape."""
    b = base(oracle, H, W)
    return {"steep": (b * np.float32(100.0), 1.0),
            "quantised with NaN and inf": (with_specials(np.floor(b * 8.0)), 1.0),
            "overflow": (b * np.float32(1e4), 1.0)}


@pytest.mark.parametrize("H,W", [(33, 50), (64, 64)])
@pytest.mark.parametrize("edge", [D4, D8])
def test_multiflow_graphs_per_pass(hip, oracle, H, W, edge):
    """soil.multiflow with 1, 2, 3, 4, 5 and 9 realisations (passes of 1 to 4 graphs, tails of 1, 2 and 3), whole
    and in shards of stride 2 and 3: the float64 sum equals, bit for bit, the in-order sum of oracle.accumulate
    over the graphs the single call makes for the same offsets (the scheme of test_gpu_accumulate_oracle.py)."""
    from soillib_amd import soil
    src = (0.5 + np.random.default_rng(2).random((H, W))).astype(np.float32)
    gs = to_gpu(src)
    for name, (h, T) in _hostile(oracle, H, W).items():
        gh = to_gpu(h)
        graphs = [to_np(soil.random_weighted(gh, edge, 11, k, T)) for k in range(9)]
        for k in (0, 4, 8):
            assert_bit_equal(graphs[k], restate(hip, oracle, h, edge, 11, k, T), "%s: graph %d" % (name, k))
        terms = [oracle.accumulate(g, src, edge) for g in graphs]

        def mean(order, K):
            total = np.zeros((H, W), np.float64)
            for k in order:
                total += (terms[k] / np.float32(K)).astype(np.float64)
            return total
        for K in (1, 2, 3, 4, 5, 9):
            got = to_np(soil.multiflow(gh, gs, K, T, edge, seed=11))
            assert_bit_equal(got, mean(range(K), K), "%s: multiflow K = %d" % (name, K))
            for stride in (2, 3):
                out = soil.multiflow(gh, gs, K, T, edge, seed=11, first=0, stride=stride)
                for first in range(1, stride):
                    soil.multiflow(gh, gs, K, T, edge, seed=11, first=first, stride=stride, out=out)
                order = [k for first in range(stride) for k in range(first, K, stride)]
                assert_bit_equal(to_np(out), mean(order, K), "%s: multiflow K = %d, stride %d" % (name, K, stride))


@pytest.mark.parametrize("H,W", [(33, 50), (33, 52)])
@pytest.mark.parametrize("edge", [D4, D8])
def test_batch_of_hostile_terrains(hip, oracle, H, W, edge):
    """random_weighted_batch on three hostile terrains stacked, then with a model of NaN and inf between them: each
    slice is the restatement of its model alone, so nothing of the NaN / inf model reaches its neighbours."""
    from soillib_amd import soil
    models = [h for h, _ in _hostile(oracle, H, W).values()]
    wild = np.where(np.random.default_rng(3).random((H, W)) < 0.5, np.nan, np.inf).astype(np.float32)
    wild[0], wild[-1] = np.nan, -np.inf                              # the rows next to the neighbouring models
    for stack, seeds in ((models, [5, 2 ** 32, 7]), ([models[0], wild, models[2]], [5, 6, 7])):
        got = to_np(soil.random_weighted_batch(to_gpu(np.stack(stack)), edge, seeds, 3, 1.0))
        for b, (h, seed) in enumerate(zip(stack, seeds)):
            assert_bit_equal(got[b], restate(hip, oracle, h, edge, seed, 3, 1.0), "model %d" % b)
            assert_graph_properties(h, got[b], edge, "model %d" % b)
    assert (got[1] == -1).all()


@pytest.mark.parametrize("shape", [0, 1, 2, 3, 4, 5, 6, 7, 8])
def test_wide_rows_under_every_window_shape(hip, shape):
    """The (33, 1024) and (70, 2052) cases of test_shapes under each SOIL_WIN_SHAPE (read once per process: a child
    process each, one at a time, as in test_gpu_window_shapes.py)."""
    env = dict(os.environ, SOIL_WIN_SHAPE=str(shape))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu",
                        "-p", "no:cacheprovider", "-k", "test_shapes and (33x1024 or 70x2052)"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "SOIL_WIN_SHAPE=%d:\n%s\n%s" % (shape, r.stdout[-3000:], r.stderr[-1000:])
    assert "2 passed" in r.stdout and "failed" not in r.stdout


# ------------------------------------------------------------------ 5. T outside its range

REFUSED = [-1.0, -1e-30, float("nan"), float("inf"), float("-inf"), 1e-39, -1e-45, 1e39]


@pytest.mark.parametrize("T", REFUSED)
def test_a_temperature_outside_the_range_is_refused_everywhere(hip, oracle, T):
    """A negative, subnormal, NaN or infinite T (as a float32): ValueError from every wrapper, SOIL_ERR_INVALID_ARGUMENT
    from the three entry points, the outputs untouched."""
    from soillib_amd import _abi, soil
    from soillib_amd.erosion import ErosionBatch
    H, W = 8, 12
    assert not soil.valid_temperature(T)
    gh = to_gpu(np.array(base(oracle, H, W)))
    g3 = to_gpu(np.stack([base(oracle, H, W)] * 2))
    ones = to_gpu(np.ones((H, W), np.float32))
    graph = to_gpu(np.full((2, H, W), -7, np.int32))
    total = to_gpu(np.full((H, W), 3.0, np.float64))
    seeds = (C.c_uint64 * 2)(1, 2)
    bad = _abi.SOIL_ERR_INVALID_ARGUMENT
    assert hip.soil_random_weighted(graph.c_ptr, gh.c_ptr, H, W, D8, 0, 0, T, None) == bad
    assert b"random_weighted: T must be" in hip.soil_last_error()
    assert hip.soil_random_weighted_batch(graph.c_ptr, g3.c_ptr, 2, H, W, D8, seeds, 0, T, None) == bad
    assert b"random_weighted_batch: T must be" in hip.soil_last_error()
    assert hip.soil_multiflow(total.c_ptr, gh.c_ptr, ones.c_ptr, H, W, D8, 0, 0, 1, 2, 2, T, None) == bad
    assert b"multiflow: T must be" in hip.soil_last_error()
    assert (to_np(graph) == -7).all() and (to_np(total) == 3.0).all()
    for call in (lambda: soil.random_weighted(gh, D8, 0, 0, T), lambda: soil.random_weighted_batch(g3, D8, [1, 2], 0, T),
                 lambda: soil.multiflow(gh, ones, 2, T, D8)):
        with pytest.raises(ValueError, match="T must be"):
            call()
    bt = ErosionBatch.__new__(ErosionBatch)
    bt.B, bt.H, bt.W, bt.seeds, bt.height = 2, H, W, [1, 2], g3
    with pytest.raises(ValueError, match=r"ErosionBatch\.flow"):
        bt.flow(kind="random_weighted", T=T)


@pytest.mark.parametrize("T", [0.0, -0.0, FLT_MIN, FLT_MAX])
def test_the_entry_points_agree_at_the_ends_of_the_range(hip, oracle, T):
    """The batch entry, ErosionBatch.flow and multiflow take what soil.random_weighted takes, and make its graphs."""
    from soillib_amd import soil
    from soillib_amd.erosion import ErosionBatch
    H, W = 33, 52
    assert soil.valid_temperature(T)
    h = base(oracle, H, W) * np.float32(100.0)
    src = np.ones((H, W), np.float32)
    single = [device_graph(h, D8, 4, k, T) for k in range(2)]
    g3 = to_gpu(np.stack([h, h]))
    assert_bit_equal(to_np(soil.random_weighted_batch(g3, D8, [4, 4], 1, T)), np.stack([single[1]] * 2), "batch")
    bt = ErosionBatch.__new__(ErosionBatch)
    bt.B, bt.H, bt.W, bt.seeds, bt.height = 2, H, W, [4, 4], g3
    assert_bit_equal(to_np(bt.flow(kind="random_weighted", T=T, offset=1)), np.stack([single[1]] * 2), "flow")
    want = sum((oracle.accumulate(g, src, D8) / np.float32(2)).astype(np.float64) for g in single)
    assert_bit_equal(to_np(soil.multiflow(to_gpu(h), to_gpu(src), 2, T, D8, seed=4)), want, "multiflow")
