"""quot0(a, recip(b)) with ONE residual correction, and sqrt_rn, against the compiler's own `/` and
sqrtf on the device (soil_math.hpp; soil_selftest_math ops 6 / 5 and 10 / 11), bit for bit.

The whole proof is tools/microbench/quot_exhaust.hip (every pair of mantissas, the corners of the exponent
range, every bit pattern of the square root; profiles/quot_one_correction/exhaust.txt).  This file keeps
the slices of it that are cheap enough for every run of the suite: whole numerator sweeps over the
denominators at the ends and in the middle of the mantissa range, the exponent corners with both signs and
zeros, and the square root at the exponents where its domain begins and ends.  No tolerance, nothing
left out: one differing bit pattern fails."""
import numpy as np
import pytest

from util import assert_bit_equal, to_gpu, to_np

pytestmark = pytest.mark.gpu

ONE = np.uint32(0x3f800000)
K_NUM_LO, K_QUOT_HI = np.float32(2.0 ** -60), np.float32(2.0 ** 90)   # soil_math.hpp: kNumLo; quot_check.hip


def _selftest(hip, a, b, op):
    from soillib_amd import _abi
    ga, gb = to_gpu(a), to_gpu(b)
    out = to_gpu(np.zeros_like(a))
    _abi.check(hip.soil_selftest_math(out.c_ptr, ga.c_ptr, gb.c_ptr, a.size, op, None))
    return to_np(out)


def _f32(sign, exp, man):
    """sign in {0, 1}, UNBIASED exponent, 23-bit mantissa -> float32"""
    u = (np.asarray(sign, np.uint32) << np.uint32(31)) | ((np.asarray(exp, np.int64) + 127).astype(np.uint32) << np.uint32(23))
    return (u | np.asarray(man, np.uint32)).view(np.float32)


def test_one_correction_quotient_over_whole_numerator_sweeps(hip):
    """Every numerator mantissa (2^23, a in [1, 2)) over eight denominators in [1, 2): the mantissa's ends, its
    middle, and two seeded ones.  6.7e7 pairs, one call per operation."""
    r = np.random.default_rng(20)
    dens = np.concatenate([np.array([0, 1, 2, 0x400000, 0x7ffffe, 0x7fffff], np.uint32),
                           r.integers(0, 1 << 23, 2, dtype=np.uint32)])
    num = (ONE | np.arange(1 << 23, dtype=np.uint32))
    a = np.tile(num, dens.size).view(np.float32)
    b = np.repeat(ONE | dens, num.size).view(np.float32)
    want = _selftest(hip, a, b, 5)
    got = _selftest(hip, a, b, 6)
    assert_bit_equal(got, want, "quot0(a, recip(b)) vs a / b, numerator sweeps")
    # (the host agrees with the device's `/`: both are the correctly rounded quotient)
    assert_bit_equal(want, a / b, "device a / b vs numpy")


def test_one_correction_quotient_exponents_signs_and_zeros(hip):
    """2^22 seeded pairs built the way tools/microbench/quot_check.hip builds its own — |b| in [2^-40, 2^40),
    |a| in [2^-80, 2^50), random signs and mantissas; every 4th pair with a within 4 ulp of b; every 4th with a
    from all normal numbers and zeros of both signs, counted when the quotient comes out in [2^-60, 2^90] — and
    another 2^22 at the corners of the plain range: the smallest and largest exponents of b, of a and of the
    quotient, and the largest denominator 2^40 itself."""
    r = np.random.default_rng(21)
    n = 1 << 22
    man = lambda: r.integers(0, 1 << 23, n, dtype=np.uint32)
    sgn = lambda: r.integers(0, 2, n)
    j = np.arange(n) & 3

    # as quot_check.hip
    b = _f32(sgn(), r.integers(-40, 40, n), man())
    a = _f32(sgn(), r.integers(-80, 50, n), man())
    near = (b.view(np.uint32) + r.integers(-4, 5, n).astype(np.uint32)).view(np.float32)
    wide = _f32(sgn(), r.integers(-126, 128, n), man())
    zero = r.integers(0, 64, n) == 0
    wide[zero] = _f32(sgn(), np.full(n, -127), np.zeros(n, np.uint32))[zero]          # +0 and -0
    a = np.where(j == 3, near, np.where(j == 2, wide, a))
    by_size = j == 2

    # the corners
    eb = np.array([-40, 39, 40], np.int64)[r.integers(0, 3, n)]
    mb = np.where(eb == 40, np.uint32(0), man())                                      # kDenHi = 2^40 is the last one
    cb = _f32(sgn(), eb, mb)
    pick = r.integers(0, 6, n)
    ea = np.choose(pick, [np.full(n, -80), np.full(n, 49), eb - 60, eb - 61, eb + 89, eb + 90])
    ca = _f32(sgn(), np.minimum(ea, 127), man())
    ca[::16] = _f32(sgn(), np.full(n, -127), np.zeros(n, np.uint32))[::16]            # zeros of both signs

    a = np.concatenate([a, ca])
    b = np.concatenate([b, cb])
    want = _selftest(hip, a, b, 5)
    got = _selftest(hip, a, b, 6)
    # a numerator in [2^-80, 2^50] (or a zero) over a plain denominator always counts; any other by the size
    # of its quotient — the compiler's, not the sequence's under test
    fa = np.abs(a)
    plain_a = (a == 0) | ((fa >= np.float32(2.0 ** -80)) & (fa <= np.float32(2.0 ** 50)))
    plain_a[:n] &= ~by_size | (a[:n] == 0)
    sized = (np.abs(want) >= K_NUM_LO) & (np.abs(want) <= K_QUOT_HI)
    count = plain_a | sized
    assert count[:n].sum() > 0.8 * n and count[n:].sum() > 0.6 * n                    # the cases are there
    assert ((a == 0) & count).sum() > n // 32 and (np.signbit(a) & (a == 0)).any()
    assert_bit_equal(got[count], want[count], "quot0(a, recip(b)) vs a / b, exponents and signs")
    assert_bit_equal(want[count], (a[count].astype(np.float64) / b[count].astype(np.float64)).astype(np.float32),
                     "device a / b vs the host's")


def test_sqrt_rn_is_sqrtf_on_every_mantissa(hip):
    """All 2^24 mantissa x exponent-parity cases at exponents 0 / 1, the same next to 2^-96 (where sqrt_rn's
    contract begins) and next to 2^127, and +0, +inf, NaN."""
    m = np.arange(1 << 23, dtype=np.uint32)
    x = np.concatenate([_f32(0, np.full(m.size, e), m) for e in (0, 1, -96, -95, 126, 127)] +
                       [np.array([0.0, np.inf, np.nan], np.float32)])
    want = _selftest(hip, x, x, 11)
    got = _selftest(hip, x, x, 10)
    assert_bit_equal(got, want, "sqrt_rn vs sqrtf")
    assert np.isnan(got[-1]) and got[-2] == np.inf and got[-3:-2].view(np.uint32)[0] == 0
    assert_bit_equal(want, np.sqrt(x.astype(np.float64)).astype(np.float32), "device sqrtf vs the host's")
    # below 2^-96 the step only asks whether the norm is under eps = 1e-12: denormals and the smallest normals
    tiny = np.concatenate([np.array([1, 2, 0x7fffff, 0x800000, 0x800001], np.uint32),
                           np.random.default_rng(22).integers(1, (127 - 96) << 23, 1 << 16, dtype=np.uint32)]).view(np.float32)
    assert (_selftest(hip, tiny, tiny, 10) < np.float32(1e-12)).all()
