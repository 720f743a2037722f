// erosion_quantiles.hip — order statistics across the models of a batch (include/soil_hip.h, "erosion: summaries";
// DESIGN.md 3.5 "Order statistics"): soil_erode_batch_quantiles (per cell and channel, the value at a fractional
// rank among the B models) and soil_erode_batch_exceedance (the share of the models above a threshold).
//
// The B values of a cell-channel are ordered by an integer key (key_of), never by a float compare, so the k-th
// order statistic is one definite bit pattern whatever path found it: three paths, the same bytes.
//   reg     B <= 64: a thread holds its cell-channel's keys in registers and sorts them with an unrolled
//           bitonic network (compile-time indices only: no scratch).
//   lds     B <= 256: a work-group sorts 64 cells, channel after channel; a thread holds 16 keys, the network's
//           steps of distance < 16 run in registers and those of distance >= 16 exchange through LDS.
//   bisect  any B: per rank, 32 walks over the models that halve the key space by counting keys <= mid.
// In all three a wave is 64 consecutive cells of one channel, so every load is coalesced along W.  Left to itself
// the entry takes reg up to B = 16, lds up to 256 and bisect above: from B = 32 on the LDS path measured faster
// than the register path at every grid, whose 64-key network leaves four waves to a SIMD.
#include <cstdlib>
#include <cstring>

#include "common.hpp"

namespace soil {
namespace {

constexpr int kE = SOIL_ENSEMBLE_CHANNELS;
constexpr int kWave = 64;
constexpr int kRegMaxB = 64;    // the register path's widest network
constexpr int kRegAutoB = 16;   // the widest it is given unforced
constexpr int kLdsMaxB = 256;   // the LDS path's widest network: 64 cells x 256 keys = 64 KiB a work-group
constexpr int kLdsKeys = 16;    // keys a thread of the LDS path holds
constexpr uint32_t kPadKey = 0xFFFFFFFFu;  // above every key of a value (a NaN's is 0xFFC00000)
static_assert(kE == 6, "soil_hip.h: the channel list");

struct QPlanes {  // the four planes read
  const float* layers;  // (B, n, 2)
  const float* waterHeight;
  const float* mass;
  const float* debris;
};
struct QArgs {  // pos[j] split on the host, by value in the launch arguments
  int64_t lo[SOIL_QUANTILES_MAX];
  double frac[SOIL_QUANTILES_MAX];
  int nq;
};
struct Thresholds {
  float t[kE];
};

// The order: every NaN becomes 0x7FC00000, then negative values have all their bits flipped and the others
// their sign bit set; keys compare unsigned.  -inf < ... < -denormal < -0 < +0 < +denormal < ... < +inf < NaN.
__device__ __forceinline__ uint32_t key_of(float v) {
  uint32_t u = __float_as_uint(v);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) u = 0x7FC00000u;
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint32_t bits_of(uint32_t key) { return (key >> 31) ? (key & 0x7FFFFFFFu) : ~key; }

// channel `ch` (uniform over the wave) of cell k = b * n + i; height is layers.x + layers.y in fp32
__device__ __forceinline__ float load_channel(const QPlanes& A, int ch, int64_t k) {
  switch (ch) {
    case 0: return A.layers[2 * k];
    case 1: return A.layers[2 * k + 1];
    case 2: {
      const float2 l = reinterpret_cast<const float2*>(A.layers)[k];
      return l.x + l.y;
    }
    case 3: return A.waterHeight[k];
    case 4: return A.mass[k];
    default: return A.debris[k];
  }
}

// The keys of models b0 .. b0 + N - 1 of one cell-channel of the tile whose first cell is `cell0` (uniform over
// the wave), pad keys from model B on.  No load sits under a branch: a model past the last reads the last one's
// cell, a lane past the grid its tile's last cell (`lane_cell`), and the pad is OR-ed in, so the N loads are in
// flight together where a branch per load would make each wait for the one before.  Every address is a uniform
// base (scalar arithmetic on b * n + cell0) plus the lane's small offset.  The channel is a base and a shift chosen
// by `ch`, and HEIGHT (ch == 2) is a template argument, so the caller branches once around all N loads.
template <bool HEIGHT, int N>
__device__ __forceinline__ void load_keys(uint32_t (&r)[N], const QPlanes& A, int ch, int64_t cell0, int lane_cell,
                                          int64_t n, int64_t b0, int64_t B) {
  const float* base = ch < 3 ? A.layers + (ch == 1 ? 1 : 0) : ch == 3 ? A.waterHeight : ch == 4 ? A.mass : A.debris;
  const int shift = ch < 3 ? 1 : 0;
#pragma unroll
  for (int e = 0; e < N; ++e) {
    const int64_t b = b0 + e < B ? b0 + e : B - 1;
    const int64_t k0 = b * n + cell0;
    float v;
    if constexpr (HEIGHT) {
      const float2 l = (reinterpret_cast<const float2*>(A.layers) + k0)[lane_cell];
      v = l.x + l.y;
    } else {
      v = (base + (k0 << shift))[lane_cell << shift];
    }
    r[e] = key_of(v) | (b0 + e < B ? 0u : kPadKey);
  }
}
// the tile's first cell and the lane's cell in it, for load_keys: a tile past the grid reads tile 0
__device__ __forceinline__ int64_t tile_cell0(int64_t tile, int64_t n) { return tile * kWave < n ? tile * kWave : 0; }
__device__ __forceinline__ int lane_in_tile(int64_t cell0, int64_t n, int lane) {
  const int64_t last = n - 1 - cell0;
  return last < lane ? static_cast<int>(last) : lane;
}

// The value at (lo, frac) from the order statistics at lo and min(lo + 1, B - 1), given as keys: a's bits when
// frac == 0 or a == b, otherwise three fp64 operations as written (-ffp-contract=off: none contracted).
__device__ __forceinline__ uint32_t interpolate(uint32_t key_a, uint32_t key_b, double frac) {
  const uint32_t ua = bits_of(key_a);
  const float a = __uint_as_float(ua), b = __uint_as_float(bits_of(key_b));
  if (frac == 0.0 || a == b) return ua;
  const double d = static_cast<double>(b) - static_cast<double>(a);
  const double p = frac * d;
  const double r = static_cast<double>(a) + p;
  return __float_as_uint(static_cast<float>(r));
}

constexpr int kTileFloats = kE * kWave;  // the six floats of a tile's 64 cells, contiguous in every out[q]

// A tile's results, staged in LDS as out holds them ([q][cell][channel]), written once and not read again here:
// thread t of the work-group takes float t, t + blockDim.x, ... of the tile's 384, so a wave's store is 256
// contiguous bytes where a wave writing its own channel would scatter 4 bytes every 24.
__device__ __forceinline__ void store_tile(float* __restrict__ out, const uint32_t* o, int nq, int64_t n,
                                           int64_t tile) {
  const int64_t first = tile * kTileFloats, total = n * kE;
  for (int q = 0; q < nq; ++q)
    for (int t = threadIdx.x; t < kTileFloats; t += blockDim.x)
      if (first + t < total)
        __builtin_nontemporal_store(__uint_as_float(o[q * kTileFloats + t]), out + q * total + first + t);
}

template <bool UP>
__device__ __forceinline__ void compare_exchange(uint32_t& x, uint32_t& y) {
  const uint32_t lo = x < y ? x : y, hi = x < y ? y : x;  // v_min_u32, v_max_u32: integers, nothing canonicalised
  x = UP ? lo : hi;
  y = UP ? hi : lo;
}

// ---- reg: one thread per cell-channel, a bitonic network over k[P] --------------------------------------------

constexpr int kRegBlock = kE * kWave;  // wave w of a work-group is channel w of the same 64 cells

// C: tiles a work-group takes at once, a thread holding C cell-channels of P keys.  A thread of a narrow network
// has only B loads to issue; C of them side by side keep enough bytes in flight to cover the memory latency.
template <int P, int C>
__global__ void __launch_bounds__(kRegBlock)
    k_quantiles_reg(QPlanes A, int64_t B, int64_t n, QArgs Q, float* __restrict__ out) {
  __shared__ uint32_t o[SOIL_QUANTILES_MAX * kTileFloats];
  const int ch = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int lane = threadIdx.x % kWave;
  const int64_t tiles = (n + kWave - 1) / kWave;
  for (int64_t first = static_cast<int64_t>(blockIdx.x) * C; first < tiles;
       first += static_cast<int64_t>(gridDim.x) * C) {  // uniform over the work-group
    uint32_t k[C][P];
    if (ch == 2) {  // one branch around all C * P loads
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int64_t cell0 = tile_cell0(first + c, n);
        load_keys<true>(k[c], A, ch, cell0, lane_in_tile(cell0, n, lane), n, 0, B);
      }
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int64_t cell0 = tile_cell0(first + c, n);
        load_keys<false>(k[c], A, ch, cell0, lane_in_tile(cell0, n, lane), n, 0, B);
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
#pragma unroll
      for (int kk = 2; kk <= P; kk <<= 1) {
#pragma unroll
        for (int j = kk >> 1; j > 0; j >>= 1) {
#pragma unroll
          for (int i = 0; i < P; ++i) {
            if ((i ^ j) > i) {
              if ((i & kk) == 0) compare_exchange<true>(k[c][i], k[c][i ^ j]);
              else compare_exchange<false>(k[c][i], k[c][i ^ j]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (first + c >= tiles) break;
      for (int q = 0; q < Q.nq; ++q) {
        const int lo = static_cast<int>(Q.lo[q]);  // < B <= P
        const int hi = lo + 1 < B ? lo + 1 : lo;
        uint32_t a = k[c][0], b = k[c][0];
#pragma unroll
        for (int i = 1; i < P; ++i) {  // a select per register: a runtime index would put k[] into scratch
          a = i == lo ? k[c][i] : a;
          b = i == hi ? k[c][i] : b;
        }
        o[q * kTileFloats + lane * kE + ch] = interpolate(a, b, Q.frac[q]);
      }
      __syncthreads();
      store_tile(out, o, Q.nq, n, first + c);
      __syncthreads();  // before the next tile's results overwrite o
    }
  }
}

// ---- lds: a work-group of P/16 waves per 64 cells, one channel at a time ----------------------------------------------
//
// Wave g holds keys 16g .. 16g+15 of the network's P positions for its lane's cell.  A step of distance j < 16
// pairs two registers of a thread; a step of distance j >= 16 pairs position 16g + e with 16(g ^ j/16) + e, the
// same register of another wave: every thread publishes its 16 keys in LDS, reads its partner's and keeps the
// smaller or the larger ones.  LDS is laid out [position][lane]: a wave's access is 64 consecutive words.

// the steps of distance 8 .. 1 inside a thread, all in one direction
template <bool UP>
__device__ __forceinline__ void merge16(uint32_t (&r)[kLdsKeys]) {
#pragma unroll
  for (int j = kLdsKeys >> 1; j > 0; j >>= 1) {
#pragma unroll
    for (int e = 0; e < kLdsKeys; ++e)
      if ((e ^ j) > e) compare_exchange<UP>(r[e], r[e ^ j]);
  }
}

// NQ: the requests the staged results hold room for (4 or SOIL_QUANTILES_MAX): at P = 256 the keys take 64 KiB,
// and 6 KiB of results beside them still let two work-groups share a CU's 160 KiB where 24 KiB would not.
template <int P, int NQ>
__global__ void __launch_bounds__(kWave * P / kLdsKeys)
    k_quantiles_lds(QPlanes A, int64_t B, int64_t n, QArgs Q, float* __restrict__ out) {
  constexpr int G = P / kLdsKeys;
  __shared__ uint32_t s[P * kWave];
  __shared__ uint32_t o[NQ * kTileFloats];
  const int g = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int lane = threadIdx.x % kWave;
  const int64_t tiles = (n + kWave - 1) / kWave;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // uniform over the work-group
    const int64_t cell0 = tile * kWave;
    const int lane_cell = lane_in_tile(cell0, n, lane);
    // the six channels of the tile one after the other: the three that come from `layers` find its lines cached
#pragma unroll 1
    for (int ch = 0; ch < kE; ++ch) {
      uint32_t r[kLdsKeys];
      if (ch == 2) load_keys<true>(r, A, ch, cell0, lane_cell, n, g * kLdsKeys, B);
      else load_keys<false>(r, A, ch, cell0, lane_cell, n, g * kLdsKeys, B);
      // the stages of length 2 .. 8: inside the thread, position 16g + e going up where its bit kk is clear
#pragma unroll
      for (int kk = 2; kk < kLdsKeys; kk <<= 1) {
#pragma unroll
        for (int j = kk >> 1; j > 0; j >>= 1) {
#pragma unroll
          for (int e = 0; e < kLdsKeys; ++e) {
            if ((e ^ j) > e) {
              if ((e & kk) == 0) compare_exchange<true>(r[e], r[e ^ j]);
              else compare_exchange<false>(r[e], r[e ^ j]);
            }
          }
        }
      }
      // the stages of length 16 .. P: in units of 16 positions, kb = kk / 16 and jb = j / 16.  The direction and
      // the side of a pair are uniform over the wave: branches, not selects.
#pragma unroll
      for (int kb = 1; kb <= G; kb <<= 1) {
        const bool up = (g & kb) == 0;  // (the last stage, kb == G: every wave up)
#pragma unroll
        for (int jb = kb >> 1; jb > 0; jb >>= 1) {
#pragma unroll
          for (int e = 0; e < kLdsKeys; ++e) s[(g * kLdsKeys + e) * kWave + lane] = r[e];
          __syncthreads();
          const uint32_t* partner = s + (g ^ jb) * kLdsKeys * kWave + lane;
          if (((g & jb) == 0) == up) {  // the lower position of a pair going up keeps the minimum
#pragma unroll
            for (int e = 0; e < kLdsKeys; ++e) {
              const uint32_t p = partner[e * kWave];
              r[e] = r[e] < p ? r[e] : p;
            }
          } else {
#pragma unroll
            for (int e = 0; e < kLdsKeys; ++e) {
              const uint32_t p = partner[e * kWave];
              r[e] = r[e] < p ? p : r[e];
            }
          }
          __syncthreads();  // before the next step overwrites what a partner may still be reading
        }
        if (up) merge16<true>(r);
        else merge16<false>(r);
      }
      // sorted: position i of the cell in s[i][lane]; wave g serves requests g, g + G, ...
#pragma unroll
      for (int e = 0; e < kLdsKeys; ++e) s[(g * kLdsKeys + e) * kWave + lane] = r[e];
      __syncthreads();
      for (int q = g; q < Q.nq; q += G) {
        const int64_t lo = Q.lo[q];
        const int64_t hi = lo + 1 < B ? lo + 1 : B - 1;
        o[q * kTileFloats + lane * kE + ch] = interpolate(s[lo * kWave + lane], s[hi * kWave + lane], Q.frac[q]);
      }
      __syncthreads();  // before the next channel's first step writes s; o complete after the last
    }
    store_tile(out, o, Q.nq, n, tile);
    __syncthreads();  // before the next tile's results overwrite o
  }
}

// ---- bisect: any B, neither registers nor LDS per model -------------------------------------------------------
//
// The order statistic of rank r is the least key x with |{b : key_b <= x}| >= r + 1: 32 halvings of [0, 2^32),
// each a coalesced walk over the models.  The statistic after it comes from one more walk: the least key above
// x, unless more than r + 1 keys are <= x (then it is x again).

__global__ void __launch_bounds__(kRegBlock)
    k_quantiles_bisect(QPlanes A, int64_t B, int64_t n, QArgs Q, float* __restrict__ out) {
  const int ch = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int lane = threadIdx.x % kWave;
  const int64_t tiles = (n + kWave - 1) / kWave;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t cell = tile * kWave + lane;
    if (cell >= n) continue;
    for (int q = 0; q < Q.nq; ++q) {
      const int64_t rank = Q.lo[q];
      uint32_t lo = 0u, hi = 0xFFFFFFFFu;
      for (int it = 0; it < 32; ++it) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        int64_t c = 0;
#pragma unroll 4
        for (int64_t b = 0; b < B; ++b) c += key_of(load_channel(A, ch, b * n + cell)) <= mid ? 1 : 0;
        if (c >= rank + 1) hi = mid;
        else lo = mid + 1u;
      }
      const uint32_t a = lo;
      uint32_t next = a;
      if (Q.frac[q] != 0.0 && rank + 1 < B) {
        int64_t c = 0;
        uint32_t above = kPadKey;
#pragma unroll 4
        for (int64_t b = 0; b < B; ++b) {
          const uint32_t k = key_of(load_channel(A, ch, b * n + cell));
          c += k <= a ? 1 : 0;
          above = (k > a && k < above) ? k : above;
        }
        next = c > rank + 1 ? a : above;
      }
      // (4 bytes every 24 from a wave: this path's time is its 33 walks)
      __builtin_nontemporal_store(__uint_as_float(interpolate(a, next, Q.frac[q])), out + (q * n + cell) * kE + ch);
    }
  }
}

// ---- exceedance: one thread per cell walks the models, k_ensemble's shape -------------------------------------

typedef float v2f __attribute__((ext_vector_type(2)));
constexpr int kXBlock = 256;

__global__ void __launch_bounds__(kXBlock)
    k_exceedance(QPlanes A, int64_t B, int64_t n, Thresholds T, float* __restrict__ out) {
  const float2* __restrict__ layers = reinterpret_cast<const float2*>(A.layers);
  const double count = static_cast<double>(B);
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kXBlock + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kXBlock) {
    int64_t c[kE];
#pragma unroll
    for (int e = 0; e < kE; ++e) c[e] = 0;
#pragma unroll 4
    for (int64_t b = 0; b < B; ++b) {
      const int64_t k = b * n + i;
      const float2 l = layers[k];
      const float v[kE] = {l.x, l.y, l.x + l.y, A.waterHeight[k], A.mass[k], A.debris[k]};
#pragma unroll
      for (int e = 0; e < kE; ++e) c[e] += v[e] > T.t[e] ? 1 : 0;  // a NaN on either side: false
    }
    float share[kE];
#pragma unroll
    for (int e = 0; e < kE; ++e) share[e] = static_cast<float>(static_cast<double>(c[e]) / count);
#pragma unroll
    for (int e = 0; e < kE; e += 2)
      __builtin_nontemporal_store(v2f{share[e], share[e + 1]}, reinterpret_cast<v2f*>(out + kE * i + e));
  }
}

enum QuantilePath { PATH_AUTO, PATH_REG, PATH_LDS, PATH_BISECT };

inline unsigned grid_for(int64_t groups) {
  constexpr int64_t cap = int64_t{1} << 22;
  return static_cast<unsigned>(groups < cap ? groups : cap);
}

template <int P, int C>
void launch_reg(int64_t tiles, hipStream_t st, const QPlanes& A, int64_t B, int64_t n, const QArgs& Q, float* out) {
  k_quantiles_reg<P, C><<<grid_for((tiles + C - 1) / C), kRegBlock, 0, st>>>(A, B, n, Q, out);
}
template <int P>
void launch_lds(unsigned grid, hipStream_t st, const QPlanes& A, int64_t B, int64_t n, const QArgs& Q, float* out) {
  if (Q.nq <= 4) k_quantiles_lds<P, 4><<<grid, kWave * P / kLdsKeys, 0, st>>>(A, B, n, Q, out);
  else k_quantiles_lds<P, SOIL_QUANTILES_MAX><<<grid, kWave * P / kLdsKeys, 0, st>>>(A, B, n, Q, out);
}

int common_checks(const soil_erosion_planes* planes, const void* out, const void* host, const char* host_name,
                  int64_t B, int64_t H, int64_t W, const char* what) {
  const std::string w(what);
  if (!planes) return fail(SOIL_ERR_INVALID_ARGUMENT, w + ": null planes");
  if (!out) return fail(SOIL_ERR_INVALID_ARGUMENT, w + ": null out");
  if (!host) return fail(SOIL_ERR_INVALID_ARGUMENT, w + ": null " + host_name);
  if (int rc = check_batch(B, H, W, 0, nullptr, what); rc != SOIL_OK) return rc;
  const soil_erosion_planes& S = *planes;
  if (!(S.layers && S.waterHeight && S.mass && S.debris))
    return fail(SOIL_ERR_INVALID_ARGUMENT, w + ": null plane (layers, waterHeight, mass and debris are read)");
  return SOIL_OK;
}

}  // namespace
}  // namespace soil

using namespace soil;

extern "C" {

int soil_erode_batch_quantiles(const soil_erosion_planes* planes, int64_t B, int64_t H, int64_t W, const double* pos,
                               int nq, float* out, void* stream) {
  SOIL_DEVICE();
  if (int rc = common_checks(planes, out, pos, "pos", B, H, W, "erode_batch_quantiles"); rc != SOIL_OK) return rc;
  SOIL_REQUIRE(nq >= 1 && nq <= SOIL_QUANTILES_MAX,
               "erode_batch_quantiles: nq must be in [1, SOIL_QUANTILES_MAX = 16]");
  QArgs Q;
  std::memset(&Q, 0, sizeof Q);
  Q.nq = nq;
  for (int j = 0; j < nq; ++j) {
    const double p = pos[j];
    SOIL_REQUIRE(std::isfinite(p) && p >= 0.0 && p <= static_cast<double>(B - 1),
                 "erode_batch_quantiles: pos must be finite and in [0, B - 1]");
    const double lo = std::floor(p);
    Q.lo[j] = static_cast<int64_t>(lo);
    Q.frac[j] = p - lo;
  }
  const int64_t n = H * W;
  SOIL_REQUIRE(n <= INT64_MAX / (int64_t{nq} * kE * static_cast<int64_t>(sizeof(float))),
               "erode_batch_quantiles: the output's byte size overflows int64");

  // read on every call (one getenv): the tests switch it between calls
  QuantilePath path = PATH_AUTO;
  if (const char* e = std::getenv("SOIL_QUANTILE_PATH")) {
    if (!std::strcmp(e, "reg")) path = PATH_REG;
    else if (!std::strcmp(e, "lds")) path = PATH_LDS;
    else if (!std::strcmp(e, "bisect")) path = PATH_BISECT;
    else SOIL_REQUIRE(!std::strcmp(e, "auto") || !e[0], "erode_batch_quantiles: SOIL_QUANTILE_PATH is not auto, reg, lds or bisect");
  }
  SOIL_REQUIRE(path != PATH_REG || B <= kRegMaxB, "erode_batch_quantiles: SOIL_QUANTILE_PATH=reg holds at most B = 64");
  SOIL_REQUIRE(path != PATH_LDS || B <= kLdsMaxB, "erode_batch_quantiles: SOIL_QUANTILE_PATH=lds holds at most B = 256");
  if (path == PATH_AUTO) path = B <= kRegAutoB ? PATH_REG : B <= kLdsMaxB ? PATH_LDS : PATH_BISECT;

  const hipStream_t st = as_stream(stream);
  const soil_erosion_planes& S = *planes;
  const QPlanes A{S.layers, S.waterHeight, S.mass, S.debris};
  const int64_t tiles = (n + kWave - 1) / kWave;
  if (path == PATH_REG) {
    if (B <= 4) launch_reg<4, 4>(tiles, st, A, B, n, Q, out);
    else if (B <= 8) launch_reg<8, 4>(tiles, st, A, B, n, Q, out);
    else if (B <= 16) launch_reg<16, 2>(tiles, st, A, B, n, Q, out);
    else if (B <= 32) launch_reg<32, 1>(tiles, st, A, B, n, Q, out);
    else launch_reg<64, 1>(tiles, st, A, B, n, Q, out);
  } else if (path == PATH_LDS) {
    const unsigned grid = grid_for(tiles);
    if (B <= 32) launch_lds<32>(grid, st, A, B, n, Q, out);
    else if (B <= 64) launch_lds<64>(grid, st, A, B, n, Q, out);
    else if (B <= 128) launch_lds<128>(grid, st, A, B, n, Q, out);
    else launch_lds<256>(grid, st, A, B, n, Q, out);
  } else {
    k_quantiles_bisect<<<grid_for(tiles), kRegBlock, 0, st>>>(A, B, n, Q, out);
  }
  SOIL_LAUNCH_CHECK();
  return SOIL_OK;
}

int soil_erode_batch_exceedance(const soil_erosion_planes* planes, int64_t B, int64_t H, int64_t W,
                                const float thresholds[SOIL_ENSEMBLE_CHANNELS], float* out, void* stream) {
  SOIL_DEVICE();
  if (int rc = common_checks(planes, out, thresholds, "thresholds", B, H, W, "erode_batch_exceedance");
      rc != SOIL_OK)
    return rc;
  const int64_t n = H * W;
  SOIL_REQUIRE(n <= INT64_MAX / (kE * static_cast<int64_t>(sizeof(float))),
               "erode_batch_exceedance: the output's byte size overflows int64");
  Thresholds T;
  for (int e = 0; e < kE; ++e) T.t[e] = thresholds[e];
  const soil_erosion_planes& S = *planes;
  const QPlanes A{S.layers, S.waterHeight, S.mass, S.debris};
  k_exceedance<<<grid_for((n + kXBlock - 1) / kXBlock), kXBlock, 0, as_stream(stream)>>>(A, B, n, T, out);
  SOIL_LAUNCH_CHECK();
  return SOIL_OK;
}

}  // extern "C"
