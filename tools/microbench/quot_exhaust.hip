// quot_exhaust.hip — the proof by exhaustion behind the one-correction quotient of soil_math.hpp
// (recip/quot/quot0) and the sweep that holds sqrt_rn, sqrtf and shorter square roots against the
// nine-instruction sequence sqrt_rn used to be, on the device.
//
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -I soillib_amd/csrc \
//         tools/microbench/quot_exhaust.hip -o tools/microbench/quot_exhaust
//   quot_exhaust a [den_lo den_hi]   part A: every numerator mantissa (2^23, a in [1, 2)) over the
//                                    denominators with mantissas den_lo <= m < den_hi (default: all 2^23)
//   quot_exhaust b                   part B: the corners of the plain exponent range
//   quot_exhaust sqrt                every fp32 bit pattern through sqrt_rn, sqrtf and the candidates
//
// Three values are compared bit for bit per pair: NEW, quot0(a, recip(b)) as soil_math.hpp has it; OLD,
// the sequence with two residual corrections that quot() used to be (kept here as a local function, so
// that the comparison outlives the change); DIV, the compiler's `a / b`.  Per part it prints the pairs
// checked, the mismatches of each kind and the first offending pair (smallest bit pattern a:b).  The
// exit status is 1 when NEW differs from DIV or OLD anywhere (sqrt: when sqrtf or sqrt_rn leave the reference).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "soil_math.hpp"

using soil::bits2f;
using soil::f2bits;

#define HIP_OK(x)                                                                      \
  do {                                                                                 \
    const hipError_t e_ = (x);                                                         \
    if (e_ != hipSuccess) {                                                            \
      std::fprintf(stderr, "%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__); \
      std::exit(2);                                                                    \
    }                                                                                  \
  } while (0)

__device__ __forceinline__ uint64_t mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// quot0 with the former quot(): two residual corrections, hipcc's expansion of `/` on plain operands
__device__ __forceinline__ float quot0_old(float a, const soil::Recip d) {
  const float q0 = a * d.r;
  float q = __builtin_fmaf(__builtin_fmaf(-d.b, q0, a), d.r, q0);
  q = __builtin_fmaf(__builtin_fmaf(-d.b, q, a), d.r, q);
  return (a == 0.0f) ? q0 : q;
}

// counters: [0] NEW != DIV, [1] OLD != DIV, [2] NEW != OLD, [3] pairs checked (part B: some are
// accepted by the size of the quotient only); first[k]: the smallest (a << 32 | b) of kind k
struct Tally {
  unsigned long long n[4];
  unsigned long long first[3];
};

struct Mine {
  unsigned long long n[4] = {0, 0, 0, 0};
  __device__ __forceinline__ void pair(Tally* t, float a, float b) {
    const soil::Recip d = soil::recip(b);
    const uint32_t nw = f2bits(soil::quot0(a, d)), od = f2bits(quot0_old(a, d)), dv = f2bits(a / b);
    ++n[3];
    if (nw != dv || od != dv || nw != od) {  // (rare: the atomics are off the common path)
      const unsigned long long key = (static_cast<unsigned long long>(f2bits(a)) << 32) | f2bits(b);
      if (nw != dv) ++n[0], atomicMin(&t->first[0], key);
      if (od != dv) ++n[1], atomicMin(&t->first[1], key);
      if (nw != od) ++n[2], atomicMin(&t->first[2], key);
    }
  }
  __device__ __forceinline__ void flush(Tally* t) {
    for (int k = 0; k < 4; ++k)
      if (n[k]) atomicAdd(&t->n[k], n[k]);
  }
};

// ---- part A: a thread takes one denominator and 2^13 consecutive numerator mantissas ----
constexpr uint32_t kManBits = 23, kPerThreadLg = 13, kThreadsPerDen = 1u << (kManBits - kPerThreadLg);
__global__ void __launch_bounds__(256) k_part_a(Tally* t, uint32_t den_lo, uint32_t dens) {
  const uint64_t g = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const uint32_t di = static_cast<uint32_t>(g / kThreadsPerDen), chunk = static_cast<uint32_t>(g % kThreadsPerDen);
  if (di >= dens) return;
  const float b = bits2f(0x3f800000u | (den_lo + di));
  Mine m;
  const uint32_t a0 = 0x3f800000u | (chunk << kPerThreadLg);
  for (uint32_t j = 0; j < (1u << kPerThreadLg); ++j) m.pair(t, bits2f(a0 + j), b);
  m.flush(t);
}

// ---- part B: exponent corners ----
// One combination: exponents eb of b and ea of a (unbiased).  A pair whose numerator lies in the
// plain range proper, [2^-80, 2^50], always counts; any other counts when the quotient comes out in
// [2^-60, 2^90] (tools/microbench/quot_check.hip, the rule for debris' decay_d).
struct Corner {
  int eb, ea;
  uint32_t b_exact;  // 1: b is the power of two itself (kDenHi is the largest plain denominator)
};
__device__ __forceinline__ void corner_pair(Mine& m, Tally* t, uint32_t ua, uint32_t ub) {
  const float a = bits2f(ua), b = bits2f(ub);
  const float fa = fabsf(a);
  if (a != 0.0f && !(fa >= 0x1p-80f && fa <= 0x1p50f)) {
    const float q = fabsf(a / b);
    if (!(q >= soil::kNumLo && q <= 0x1p90f)) return;
  }
  m.pair(t, a, b);
}
__global__ void __launch_bounds__(256) k_part_b_random(Tally* t, Corner c, uint64_t per_thread, uint64_t salt) {
  const uint64_t g = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  Mine m;
  for (uint64_t j = 0; j < per_thread; ++j) {
    const uint64_t h = mix(salt + g * per_thread + j);
    uint32_t ub = (static_cast<uint32_t>(h) & 0x807fffffu) | (static_cast<uint32_t>(c.eb + 127) << 23);
    if (c.b_exact) ub &= 0xff800000u;
    const uint32_t ua = (static_cast<uint32_t>(h >> 32) & 0x807fffffu) | (static_cast<uint32_t>(c.ea + 127) << 23);
    corner_pair(m, t, ua, ub);
  }
  m.flush(t);
}
// every denominator mantissa, numerator mantissas within 4 ulp of it, the four sign combinations;
// and numerators +0 and -0 over every such denominator of either sign
__global__ void __launch_bounds__(256) k_part_b_near(Tally* t, Corner c) {
  const uint32_t mb = blockIdx.x * blockDim.x + threadIdx.x;
  if (mb >= (1u << 23)) return;
  Mine m;
  const uint32_t ub0 = (c.b_exact ? 0u : mb) | (static_cast<uint32_t>(c.eb + 127) << 23);
  for (int d = -4; d <= 4; ++d) {
    const int ma = static_cast<int>(mb) + d;
    if (ma < 0 || ma >= (1 << 23)) continue;
    const uint32_t ua0 = static_cast<uint32_t>(ma) | (static_cast<uint32_t>(c.ea + 127) << 23);
    for (uint32_t s = 0; s < 4; ++s) corner_pair(m, t, ua0 | ((s & 1u) << 31), ub0 | ((s >> 1) << 31));
  }
  for (uint32_t s = 0; s < 4; ++s) corner_pair(m, t, (s & 1u) << 31, ub0 | ((s >> 1) << 31));
  m.flush(t);
}

// ---- the square root ----
// The reference: the nine instructions sqrt_rn used to be (hipcc's expansion of sqrtf without its scaling
// and class test) — v_sqrt_f32 (1 ulp), then the neighbours one ulp down and up tried against the exact
// residual.  Kept here so that the comparison outlives a change of sqrt_rn.
__device__ __forceinline__ float sqrt_neighbours(float x) {
  const float y = __builtin_amdgcn_sqrtf(x);
  const float dn = bits2f(f2bits(y) - 1u), up = bits2f(f2bits(y) + 1u);
  const float r_dn = __builtin_fmaf(-dn, y, x), r_up = __builtin_fmaf(-up, y, x);
  float s = (r_dn <= 0.0f) ? dn : y;
  s = (r_up > 0.0f) ? up : s;
  return s;
}
// Candidates for a shorter correctly rounded square root, all from v_rsq_f32 (1 ulp):
//   c5  r = rsq(x); y = x r; h = r / 2; s = fma(fma(-y, y, x), h, y)                     5 instructions
//   c7  c5 with x handed through where it is a zero, a denormal or +inf (one class       7
//       test, one select: rsq of those is +inf or 0 and the products NaN)
//   c8  Markstein: y and h refined once (e = fma(-h, y, 1/2)) before the final residual  8
__device__ __forceinline__ float sqrt_c5(float x) {
  const float r = __builtin_amdgcn_rsqf(x), y = x * r, h = 0.5f * r;
  return __builtin_fmaf(__builtin_fmaf(-y, y, x), h, y);
}
__device__ __forceinline__ float sqrt_c7(float x) {
  const float s = sqrt_c5(x);
  return __builtin_amdgcn_classf(x, 0x200 | 0x80 | 0x40 | 0x20 | 0x10) ? x : s;  // +inf, +-denormal, +-0
}
__device__ __forceinline__ float sqrt_c8(float x) {
  const float r = __builtin_amdgcn_rsqf(x);
  float y = x * r, h = 0.5f * r;
  const float e = __builtin_fmaf(-h, y, 0.5f);
  y = __builtin_fmaf(y, e, y);
  h = __builtin_fmaf(h, e, h);
  return __builtin_fmaf(__builtin_fmaf(-y, y, x), h, y);
}
// Per function f in {sqrtf, soil::sqrt_rn, c5, c7, c8}, against sqrt_neighbours:
//   n[4 f + 0]  x >= 2^-96 finite: different bits            first[f]: the smallest such x
//   n[4 f + 1]  x in {+0, +inf}: different bits
//   n[4 f + 2]  x a NaN: the result is not a NaN
//   n[4 f + 3]  0 < x < 2^-96: a different answer to `< 1e-12`
constexpr int kSqrtFns = 5;
struct SqrtTally {
  unsigned long long n[4 * kSqrtFns];
  unsigned long long first[kSqrtFns];
};
__global__ void __launch_bounds__(256) k_sqrt(SqrtTally* t) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;  // 2^24 threads x 2^8 patterns
  unsigned long long n[4 * kSqrtFns] = {};
  for (uint32_t j = 0; j < 256u; ++j) {
    const uint32_t u = (g << 8) | j;
    const float x = bits2f(u);
    if ((u >> 31) && x == x) continue;  // negative numbers and -0: not the function's domain
    const float ref = sqrt_neighbours(x);
    const float got[kSqrtFns] = {sqrtf(x), soil::sqrt_rn(x), sqrt_c5(x), sqrt_c7(x), sqrt_c8(x)};
#pragma unroll
    for (int f = 0; f < kSqrtFns; ++f) {
      if (x != x) {
        n[4 * f + 2] += (got[f] == got[f]);
      } else if (u == 0u || u == 0x7f800000u) {
        n[4 * f + 1] += (f2bits(got[f]) != f2bits(ref));
      } else if (x >= 0x1p-96f) {
        if (f2bits(got[f]) != f2bits(ref)) ++n[4 * f], atomicMin(&t->first[f], static_cast<unsigned long long>(u));
      } else {
        n[4 * f + 3] += ((got[f] < 1e-12f) != (ref < 1e-12f));
      }
    }
  }
  for (int k = 0; k < 4 * kSqrtFns; ++k)
    if (n[k]) atomicAdd(&t->n[k], n[k]);
}

// ---- host ----
template <class T>
static T* device_tally() {
  T h;
  std::memset(&h, 0, sizeof h);
  for (auto& f : h.first) f = ~0ull;
  T* d;
  HIP_OK(hipMalloc(&d, sizeof h));
  HIP_OK(hipMemcpy(d, &h, sizeof h, hipMemcpyHostToDevice));
  return d;
}
static double now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static void print_kind(const char* name, unsigned long long n, unsigned long long first) {
  std::printf("  %-10s mismatches %llu", name, n);
  if (n) std::printf("  first a=%08x b=%08x", static_cast<unsigned>(first >> 32), static_cast<unsigned>(first));
  std::printf("\n");
}
static int report(const char* title, Tally* d, double seconds) {
  Tally h;
  HIP_OK(hipMemcpy(&h, d, sizeof h, hipMemcpyDeviceToHost));
  std::printf("%s: pairs %llu in %.2f s\n", title, h.n[3], seconds);
  print_kind("new != div", h.n[0], h.first[0]);
  print_kind("old != div", h.n[1], h.first[1]);
  print_kind("new != old", h.n[2], h.first[2]);
  std::fflush(stdout);
  return (h.n[0] || h.n[2]) ? 1 : 0;
}

static int part_a(uint32_t lo, uint32_t hi) {
  Tally* d = device_tally<Tally>();
  const double t0 = now();
  double t_line = t0;
  constexpr uint32_t kDensPerLaunch = 1u << 15;  // 2.7e11 pairs: a fraction of a second per launch
  for (uint32_t at = lo; at < hi; at += kDensPerLaunch) {
    const uint32_t dens = (hi - at < kDensPerLaunch) ? hi - at : kDensPerLaunch;
    const uint64_t threads = static_cast<uint64_t>(dens) * kThreadsPerDen;
    k_part_a<<<static_cast<uint32_t>((threads + 255) / 256), 256>>>(d, at, dens);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    if (now() - t_line > 20.0) {  // a sign of life for whoever watches a long slice
      std::printf("  ... denominators [%u, %u) done, %.1f s\n", lo, at + dens, now() - t0);
      std::fflush(stdout);
      t_line = now();
    }
  }
  char title[96];
  std::snprintf(title, sizeof title, "part A, denominator mantissas [%u, %u) x 2^23 numerators", lo, hi);
  return report(title, d, now() - t0);
}

static int part_b() {
  // smallest and largest plain exponents of b; of a by its own bounds (2^-80, 2^50) and by those of
  // the quotient (2^-60, 2^90); then the particle step's directions: denominators down to 2^-60
  // under numerators in [2^-60, 1]
  const int den[3][2] = {{-40, 0}, {39, 0}, {40, 1}};
  Corner corners[64];
  int n = 0;
  for (const auto& b : den) {
    const int eb = b[0];
    // (eb - 61 and eb + 90 straddle the quotient's bounds: its size decides pair by pair)
    const int ea[6] = {-80, 49, eb - 60, eb - 61, eb + 89, eb + 90};
    for (const int e : ea) corners[n++] = Corner{eb, e > 127 ? 127 : e, static_cast<uint32_t>(b[1])};
  }
  const int dir[4][2] = {{-60, -60}, {-60, -1}, {-60, 0}, {-1, -60}};
  for (const auto& c : dir) corners[n++] = Corner{c[0], c[1], 0u};
  int bad = 0;
  for (int i = 0; i < n; ++i) {
    Tally* d = device_tally<Tally>();
    const double t0 = now();
    const uint64_t threads = 256ull * 16384ull, per = (1ull << 30) / threads;
    k_part_b_random<<<16384, 256>>>(d, corners[i], per, static_cast<uint64_t>(i) << 40);
    HIP_OK(hipGetLastError());
    k_part_b_near<<<(1u << 23) / 256, 256>>>(d, corners[i]);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    char title[128];
    std::snprintf(title, sizeof title, "part B, |b| in 2^%d%s, |a| in 2^%d [1, 2): random, within 4 ulp, zeros",
                  corners[i].eb, corners[i].b_exact ? "" : " [1, 2)", corners[i].ea);
    bad |= report(title, d, now() - t0);
    HIP_OK(hipFree(d));
  }
  return bad;
}

static int part_sqrt() {
  SqrtTally* d = device_tally<SqrtTally>();
  const double t0 = now();
  k_sqrt<<<(1u << 24) / 256, 256>>>(d);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  SqrtTally h;
  HIP_OK(hipMemcpy(&h, d, sizeof h, hipMemcpyDeviceToHost));
  std::printf("square root, all 2^32 bit patterns against v_sqrt_f32 + neighbours in %.2f s\n", now() - t0);
  const char* names[kSqrtFns] = {"sqrtf", "sqrt_rn (soil_math.hpp)", "c5 (5 instr.)", "c7 (c5, 0/denormal/inf: x)",
                                 "c8 (Markstein)"};
  for (int f = 0; f < kSqrtFns; ++f) {
    std::printf("  %-30s x >= 2^-96: %llu", names[f], h.n[4 * f]);
    if (h.n[4 * f]) std::printf(" (first x=%08x)", static_cast<unsigned>(h.first[f]));
    std::printf("  +0/+inf: %llu  NaN lost: %llu  `< 1e-12` below 2^-96: %llu\n", h.n[4 * f + 1], h.n[4 * f + 2],
                h.n[4 * f + 3]);
  }
  // sqrtf and sqrt_rn have to agree with the reference wherever sqrt_rn is specified
  return (h.n[0] || h.n[1] || h.n[2] || h.n[4] || h.n[5] || h.n[6] || h.n[7]) ? 1 : 0;
}

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  if (!std::strcmp(mode, "a")) {
    const uint32_t lo = argc > 3 ? static_cast<uint32_t>(std::strtoul(argv[2], nullptr, 0)) : 0u;
    const uint32_t hi = argc > 3 ? static_cast<uint32_t>(std::strtoul(argv[3], nullptr, 0)) : 1u << 23;
    if (lo >= hi || hi > (1u << 23)) {
      std::fprintf(stderr, "denominator mantissas: 0 <= den_lo < den_hi <= %u\n", 1u << 23);
      return 2;
    }
    return part_a(lo, hi);
  }
  if (!std::strcmp(mode, "b")) return part_b();
  if (!std::strcmp(mode, "sqrt")) return part_sqrt();
  std::fprintf(stderr, "usage: quot_exhaust a [den_lo den_hi] | b | sqrt\n");
  return 2;
}
