// soil_math.hpp — numerical contract of the hot path.
//
// The reference leans on two things no other platform can reproduce: CUDA's
// fast intrinsics __expf/__powf (erosion.cu:85,134-136,345-346,500,872;
// graph.cu:139,409-411; filter.cu:48; path.cu:134) and cuRAND XORWOW
// (erosion.cu:57-58, graph.cu:97-101,150).  This header fixes portable
// replacements, written for host and device alike so that host-side setup
// (blur weights, CPU twins) and the kernels agree to the bit:
//
//   soil::expf_  — range-reduced degree-6 polynomial, <= 1 ulp, flush below e^-87
//   soil::log2f_ — mantissa polynomial, positive normal inputs
//   soil::powf_  — exp2(y * log2 x), the definition of __powf
//   soil::Philox — Philox4x32-10, counter = {offset, subsequence}, key = seed
//
// Everything is plain IEEE fp32 evaluated in the written order; the library is
// compiled with -ffp-contract=off so no product-sum is fused behind our back.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cfloat>

#define SOIL_HD __host__ __device__ __forceinline__

namespace soil {

constexpr float kSqrt2 = 1.41421354f;  // CUDART_SQRT_TWO_F, erosion_map.cu:61
constexpr float kFltMin = 1.17549435e-38f;

SOIL_HD float bits2f(uint32_t u) { return __builtin_bit_cast(float, u); }
SOIL_HD uint32_t f2bits(float f) { return __builtin_bit_cast(uint32_t, f); }
SOIL_HD float pow2i(int n) { return bits2f(static_cast<uint32_t>(n + 127) << 23); }  // n in [-126,127]

// y * 2^n for y in [0.7, 1.42].  The contract spells this (y * 2^(n/2)) * 2^(n - n/2):
// the first product is exact, the second rounds the exact value once, which is what
// ldexp does in one instruction (v_ldexp_f32), overflow to +inf included.
SOIL_HD float scale2(float y, int n) { return __builtin_ldexpf(y, n); }

SOIL_HD float exp_poly(float r) {  // ~ exp(r) on |r| <= ln2/2
  float p = 1.9875691500E-4f;
  p = p * r + 1.3981999507E-3f;
  p = p * r + 8.3334519073E-3f;
  p = p * r + 4.1665795894E-2f;
  p = p * r + 1.6666665459E-1f;
  p = p * r + 5.0000001201E-1f;
  return (p * (r * r) + r) + 1.0f;
}

SOIL_HD float expf_(float x) {
  if (x != x) return x;
  if (x > 88.72283f) return __builtin_inff();
  if (x < -87.0f) return 0.0f;
  const float n = __builtin_rintf(x * 1.44269504f);
  float r = x - n * 0.693145752f;
  r = r - n * 1.42860677e-6f;
  const float y = exp_poly(r);
  return scale2(y, static_cast<int>(n));
}
// The same values in straight-line code: the three exits become two selects (a NaN
// runs through the arithmetic as a NaN; what the saturated cases compute is
// discarded).  For call sites where saturation is the exception — three of them per
// fluvial particle step — so the exits never skip anything for a whole wave and only
// cost exec-mask bookkeeping.
__device__ __forceinline__ float expf_flat(float x) {
  const float n = __builtin_rintf(x * 1.44269504f);
  float r = x - n * 0.693145752f;
  r = r - n * 1.42860677e-6f;
  const float y = scale2(exp_poly(r), static_cast<int>(n));
  return (x > 88.72283f) ? __builtin_inff() : ((x < -87.0f) ? 0.0f : y);
}

SOIL_HD float log2f_(float x) {
  if (x != x) return x;
  if (x < 0.0f) return __builtin_nanf("");
  if (x < kFltMin) return -__builtin_inff();
  if (x == __builtin_inff()) return x;
  const uint32_t b = f2bits(x);
  int e = static_cast<int>((b >> 23) & 0xffu) - 127;
  float m = bits2f((b & 0x007fffffu) | 0x3f800000u);
  if (m > kSqrt2) {
    m = m * 0.5f;
    e = e + 1;
  }
  const float f = m - 1.0f;
  const float z = f * f;
  float p = 7.0376836292E-2f;
  p = p * f - 1.1514610310E-1f;
  p = p * f + 1.1676998740E-1f;
  p = p * f - 1.2420140846E-1f;
  p = p * f + 1.4249322787E-1f;
  p = p * f - 1.6668057665E-1f;
  p = p * f + 2.0000714765E-1f;
  p = p * f - 2.4999993993E-1f;
  p = p * f + 3.3333331174E-1f;
  float y = (f * z) * p;
  y = y - 0.5f * z;
  const float ln_m = f + y;
  return ln_m * 1.44269504f + static_cast<float>(e);
}

SOIL_HD float powf_(float x, float y) {
  const float t = y * log2f_(x);
  if (t != t) return t;
  if (t > 128.0f) return __builtin_inff();
  if (t < -126.0f) return 0.0f;
  const float n = __builtin_rintf(t);
  const float r = (t - n) * 0.693147182f;
  const float v = exp_poly(r);
  return scale2(v, static_cast<int>(n));
}

// IEEE quotients that share a denominator (device only).
//
// A particle step (erosion_particles_tiled.hip) divides nine (debris: eleven) times,
// by four (five) different numbers.  recip()/quot() compute the reciprocal once per
// denominator and each quotient from it in three instructions:
//      r = rcp(b); r = fma(fma(-b, r, 1), r, r)          recip(): v_rcp_f32 (1 ulp), one Newton step
//      q = a * r;  q = fma(fma(-b, q, a), r, q)          quot():  one residual correction
// On the plain range below, q is the correctly rounded quotient RN(a / b), which is what
// the compiler's `/` gives as well — so the two agree to the bit.  (hipcc's own expansion
// of `/` is this sequence between v_div_scale and v_div_fixup with a SECOND residual
// correction; until the one-correction form was proved, quot() copied it.)
//
// Why the second correction does nothing.  Let q1 be the value above and suppose it is
// RN(a / b).  Then e1 = a - b q1 is exact in fp32; a / b lies no closer than 2^-25 ulp to a
// rounding midpoint (a - b mid is a non-zero multiple of 2^-47 for 24-bit operands in
// [1, 2)); so |e1 r| <= (1/2 - 2^-25)(1 + 2^-24) ulp < 1/2 ulp and fma(e1, r, q1) rounds
// back to q1.  That q1 always IS RN(a / b) with this device's v_rcp_f32 is established by
// exhaustion, not by argument: tools/microbench/quot_exhaust.hip compares quot0(a, recip(b)),
// the former two-correction sequence and `a / b` bit for bit on the device for every pair
// of mantissas (2^23 x 2^23, both operands in [1, 2)) and at the corners of the exponent
// range named below; its output is profiles/quot_one_correction/exhaust.txt, and
// tests/test_gpu_quot_one_correction.py keeps a slice of it in the suite.  All three
// operations are scale-invariant in the exponents as long as no intermediate leaves the
// normal range or, for the residual, stops being exact — which is what "plain" has to
// guarantee:
//   * b and r ~ 1/b normal: |b| in [2^-40, 2^40] (the particle step's directions: down
//     to 2^-60, numerators <= 1); 1 - b r is O(2^-23), never near the exponent limits;
//   * q = a r and a / b normal and finite: |a| in [2^-80, 2^50] over such a b, or any pair
//     whose quotient turns out in [2^-60, 2^90];
//   * the residual a - b q exact.  With b = Mb 2^(eb-23), q = Mq 2^(eq-23) it is a multiple
//     of u = 2^(eb+eq-46) >= 2^(ea-47) of fewer than 2^24 units (q is within an ulp of
//     a / b), so one fp32 number as long as u >= 2^-149, the smallest denormal: ea >= -102.
//     The smallest plain numerator is 2^-100 (a quotient of 2^-60 over 2^-40), its u
//     2^-147; from |a| >= 2^-79 the residual is a normal number or zero.  (The library is
//     built with fp32 denormals on — tests/test_gpu_parity.py::test_denormals_are_not_flushed —
//     and an fma takes a denormal operand at full precision.)  The product e r inside the
//     last fma is not rounded on its own; its size is that of an ulp of q.
//   * nothing overflows: |b q| is within an ulp of |a| and |e r| about an ulp of q, both
//     finite whenever a and q are; |r| <= 2^60.
// a == +0 runs through the chain to the correctly signed zero, -0 needs quot0().
// Anything else — denormals, infinities, zero or NaN denominators — has to take the
// written-out `/` (v_div_scale / v_div_fixup serve those).
struct Recip { float b, r; };
__device__ __forceinline__ Recip recip(float b) {
  float r = __builtin_amdgcn_rcpf(b);
  r = __builtin_fmaf(__builtin_fmaf(-b, r, 1.0f), r, r);
  return {b, r};
}
__device__ __forceinline__ float quot(float a, const Recip d) {
  const float q = a * d.r;
  return __builtin_fmaf(__builtin_fmaf(-d.b, q, a), d.r, q);
}
// 1 / b = quot(1, d): with q = 1 * r = r the correction is one more Newton step on the
// refined reciprocal.  Written out so that no product with 1 is left to the compiler.
__device__ __forceinline__ float recip_rn(const Recip d) {
  return __builtin_fmaf(__builtin_fmaf(-d.b, d.r, 1.0f), d.r, d.r);
}
// A zero numerator of either sign: the first product already is the IEEE answer (zero,
// sign of a times sign of b); the correction after it would turn -0 into +0.
__device__ __forceinline__ float quot0(float a, const Recip d) {
  const float q0 = a * d.r, q = quot(a, d);
  return (a == 0.0f) ? q0 : q;
}
constexpr float kDenLo = 0x1p-40f, kDenHi = 0x1p40f;  // denominators
constexpr float kNumLo = 0x1p-60f;                      // numerators (given a plain denominator)
__device__ __forceinline__ bool plain_den(float b) { return fabsf(b) >= kDenLo && fabsf(b) <= kDenHi; }
// +0 or of plain magnitude (the caller bounds it from above)
__device__ __forceinline__ bool plain_num(float a) { return f2bits(a) == 0u || fabsf(a) >= kNumLo; }


// Quotients of a stencil kernel over a denominator that is the same for every cell (a cell size,
// sqrt(2)): quot() with the reciprocal refined once per thread, and the check of the plain range
// made on the RESULTS of a whole group of cells at once — a quotient is beyond doubt when it is
// zero (from a +0 numerator: differences of equal heights; the denominators are positive) or lies
// in [2^-60, 2^90] (see above); Watch collects the extremes of the bit patterns, and a thread whose
// group has a quotient outside (a denormal difference, an infinity, a NaN that is not the
// kernels' own sentinel) redoes the group with the written-out divisions.
struct QuotWatch {
  uint32_t lo = 0xffffffffu, hi = 0u;
  bool neg_zero = false;
  __device__ __forceinline__ float operator()(float q) {
    const uint32_t u = f2bits(q) & 0x7fffffffu;
    lo = min(lo, u - 1u);  // a zero wraps to the top: never the minimum
    hi = max(hi, u);
    return q;
  }
  // For a quotient whose SIGN OF ZERO is seen by the caller (stored, not just compared): a
  // numerator -0 (the difference (-0) - (+0), half of it, ...) has the IEEE quotient -0 over these
  // positive denominators, the chain of quot() ends in +0.  Such a group is in doubt.
  __device__ __forceinline__ float operator()(float q, float numerator) {
    neg_zero = neg_zero || f2bits(numerator) == 0x80000000u;
    return (*this)(q);
  }
  __device__ __forceinline__ bool doubtful() const {
    constexpr uint32_t kLoBits = (127u - 60u) << 23, kHiBits = (127u + 90u) << 23;
    return lo < kLoBits - 1u || hi > kHiBits || neg_zero;
  }
};

// ---- device-only helpers of the particle step ----------------------------------------------

// The attenuation factors of a particle (att_m, att_w, att_v: erosion.cu:134-136; debris att_v :346)
// are __expf in the reference — the hardware's fast exponential, ex2.approx(x * log2e).  They only
// scale what a particle deposits and never feed back into where it goes, so they take gfx950's
// counterpart here: v_exp_f32(x * log2e), 1 ulp, two instructions instead of the ~22 of expf_.
// (Debris' att_d, :345, does feed back into the speed; it stays on expf_ so that trajectories remain
// bit-identical to the oracle's.)  Parity of the flux planes is a tolerance either way: fp32
// summation order (tests/test_gpu_parity.py, _flux_close).
__device__ __forceinline__ float att_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504f); }

// The Gibbs weight of random_weighted (graph.hip: rw_cdf): 2^(diff * c), the product rounded to fp32 and then
// v_exp_f32, with c = log2(e) / (|shift| T) made on the host.  soil_selftest_math op 12 is this function, so the
// tests' restatement of the kernel takes its weights from the very expression the kernel evaluates.
__device__ __forceinline__ float rw_exp2(float diff, float c) { return __builtin_amdgcn_exp2f(diff * c); }
// The constants of that weight, made on the host (graph.hip states which temperatures the entries take and why), and
// shared by random_weighted and the exact multiple-flow weights (mfd.hip): one definition, one set of bits.
struct RwConst {  // log2(e) / (|shift_k| T) for the straight and the diagonal neighbours
  float straight, diagonal;
};
inline bool rw_temperature_ok(float T) { return T == 0.0f || (T >= FLT_MIN && T <= FLT_MAX); }
inline RwConst rw_const(float T) {
  const double log2e = 1.4426950408889634;
  return RwConst{static_cast<float>(log2e / static_cast<double>(T)),
                 static_cast<float>(log2e / (static_cast<double>(kSqrt2) * static_cast<double>(T)))};
}

// The slope power of soil_stream_power_n (downstream.hip: pn_init_cell): S^e in fp64 through the device library's pow,
// which is deterministic but not correctly rounded.  soil_selftest_math64 op 0 is this function, so the tests'
// restatement of the kernel takes its powers from the very expression the kernel evaluates.  pow(+0, e > 0) is +0,
// pow(1, e) is 1 and a NaN S stays a NaN.
__device__ __forceinline__ double sp_pow(double S, double e) { return pow(S, e); }

// floor(f) as an integer in one instruction (v_cvt_flr_i32_f32), saturating at the int32 range
// — for a position inside the grid the same cell as the reference's float -> int truncation
// (erosion_map.cu:42-47), and for one outside of it an index an unsigned comparison against the grid
// size rejects (px in (-1, 0) floors to -1; -0.0 to 0, which `px < 0` lets pass as well).  A NaN
// comes out as INT_MAX (measured; CUDA's conversion, which the reference relies on, gives 0): the
// caller has to look at NaN positions itself, nan_cell() below.
__device__ __forceinline__ int floor_cell(float f) {
  int r;
  asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(f));
  return r;
}
__device__ __forceinline__ int nan_cell(float f, int cell) { return (f != f) ? 0 : cell; }

// Correctly rounded square root for x >= 2^-96 (and +0, +inf, NaN) in seven instructions: y = x rsq(x)
// (v_rsq_f32, 1 ulp) and one correction by the exact residual x - y*y times rsq(x) / 2.  That this is sqrtf
// to the bit on every such x holds for this device's v_rsq_f32 and by exhaustion only — all 2^32 bit
// patterns, tools/microbench/quot_exhaust.hip sqrt (profiles/quot_one_correction/exhaust.txt), and
// tests/test_gpu_quot_one_correction.py on every mantissa at the ends of the range; with a correctly
// rounded rsq or its neighbours the same sequence misses a few mantissas.  (Until then this was the
// compiler's expansion of sqrtf without its scaling: v_sqrt_f32 and the neighbours one ulp down and up
// tried against the residual, nine instructions.)  Zeros, denormals and +inf, whose rsq is infinite or
// zero, are handed through as they are.  Below 2^-96 the result is merely close, a denormal comes back
// unchanged; the particle step only asks whether it is under eps = 1e-12 there, and it is.
__device__ __forceinline__ float sqrt_rn(float x) {
  const float r = __builtin_amdgcn_rsqf(x), y = x * r, h = 0.5f * r;
  const float s = __builtin_fmaf(__builtin_fmaf(-y, y, x), h, y);
  return __builtin_amdgcn_classf(x, 0x200 | 0x80 | 0x40 | 0x20 | 0x10) ? x : s;  // +inf, +-denormal, +-0
}

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as
// easy as 1, 2, 3", SC'11).  Only word 0 of the block is consumed per draw.
SOIL_HD uint32_t philox4x32_10_w0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                  uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c0;
    const uint64_t p1 = static_cast<uint64_t>(0xCD9E8D57u) * c2;
    const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n1 = static_cast<uint32_t>(p1);
    const uint32_t n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
    const uint32_t n3 = static_cast<uint32_t>(p0);
    c0 = n0;
    c1 = n1;
    c2 = n2;
    c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}

// ... the whole block
SOIL_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                           uint32_t out[4]) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c0;
    const uint64_t p1 = static_cast<uint64_t>(0xCD9E8D57u) * c2;
    const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n1 = static_cast<uint32_t>(p1);
    const uint32_t n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
    const uint32_t n3 = static_cast<uint32_t>(p0);
    c0 = n0;
    c1 = n1;
    c2 = n2;
    c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}
SOIL_HD float uniform_of_word(uint32_t r) { return static_cast<float>((r >> 8) + 1u) * 5.9604644775390625e-08f; }  // (0, 1]
// The draws of the four cells 4 q .. 4 q + 3 of a flow graph (random_weighted): block (offset,
// subsequence q), cell n takes word n & 3.  The reference seeds a generator state per cell,
// curand_init(seed, n, offset), for ONE uniform (graph.cu:97-101, :150); Philox makes four words a
// block, so one block serves four cells — a quarter of what was half of the kernel's instructions
// (the generator is build-defined on both sides; oracle: orc_rng_uniform_cell).
SOIL_HD void rng_uniform_quad(uint64_t seed, uint64_t q, uint64_t offset, float u[4]) {
  uint32_t w[4];
  philox4x32_10(static_cast<uint32_t>(offset), static_cast<uint32_t>(offset >> 32), static_cast<uint32_t>(q),
                static_cast<uint32_t>(q >> 32), static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), w);
#pragma unroll
  for (int i = 0; i < 4; ++i) u[i] = uniform_of_word(w[i]);
}

// One draw in (0, 1] from stream (seed, subsequence) at position `offset` —
// the addressing of curand_init(seed, subsequence, offset) + curand_uniform.
SOIL_HD float rng_uniform_at(uint64_t seed, uint64_t subsequence, uint64_t offset) {
  const uint32_t r = philox4x32_10_w0(
      static_cast<uint32_t>(offset), static_cast<uint32_t>(offset >> 32),
      static_cast<uint32_t>(subsequence), static_cast<uint32_t>(subsequence >> 32),
      static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32));
  return static_cast<float>((r >> 8) + 1u) * 5.9604644775390625e-08f;  // 2^-24
}

}  // namespace soil
