// erosion_stats.hip — the two reductions of a batch (include/soil_hip.h, "erosion: summaries"):
// soil_erode_batch_stats, over the cells of each model (one 320-byte record per model), and
// soil_erode_batch_ensemble, over the models of a batch (one mean and one variance map per quantity).
//
// Both accumulate in fp64 in an order that is a function of n = H*W alone: no floating-point atomics, no
// dependence on B, on the model's index or on the alignment of its first cell, so a model's record in a batch
// carries the bits of its record alone and two calls return the same bytes.
#include "common.hpp"

namespace soil {
namespace {

constexpr int kSBlock = 256;           // threads of a work-group, four waves
constexpr int kSWaves = kSBlock / 64;
constexpr int kLaneCells = 4;          // consecutive cells a lane takes per pass of its work-group: one 16-byte load
constexpr int64_t kPassCells = int64_t{kSBlock} * kLaneCells;  // cells a work-group takes per pass
constexpr int64_t kMinChunk = 4 * kPassCells;                  // the wave and LDS folds are paid once per 16 cells a lane
constexpr int64_t kMaxPartials = 4096;                         // of one model: what the second pass's one group folds
constexpr int64_t kMaxModels = 65535;                          // grid.z

constexpr int kCh = SOIL_STAT_CHANNELS;
static_assert(sizeof(soil_channel_stats) == 32 && sizeof(soil_model_stats) == 320, "soil_hip.h: the records' layout");
static_assert(kCh == 10 && SOIL_ENSEMBLE_CHANNELS == 6, "soil_hip.h: the channel lists");

// Cells of a model one work-group of the first pass reduces: a multiple of kPassCells, a function of n alone
// (never of B or b), at most kMaxPartials chunks to a model.
inline int64_t stats_chunk(int64_t n) {
  int64_t c = (n + kMaxPartials - 1) / kMaxPartials;
  c = (c + kPassCells - 1) / kPassCells * kPassCells;
  return c < kMinChunk ? kMinChunk : c;
}

// The running statistics of the ten channels, register-resident (every index a compile-time constant).
struct Acc {
  double sum[kCh], sumsq[kCh];
  long long nonfinite[kCh];
  float mn[kCh], mx[kCh];
};
__device__ __forceinline__ void acc_init(Acc& a) {
#pragma unroll
  for (int c = 0; c < kCh; ++c)
    a.sum[c] = 0.0, a.sumsq[c] = 0.0, a.nonfinite[c] = 0, a.mn[c] = __builtin_inff(), a.mx[c] = -__builtin_inff();
}
// one value into channel c.  Finite: v - v == 0.  A value that is not adds +0.0 to the sums, which changes no bit
// of them (they start at +0.0 and never become -0.0), and leaves min and max alone.
__device__ __forceinline__ void acc_value(Acc& a, int c, float v) {
  const bool finite = (v - v) == 0.0f;
  const double d = finite ? static_cast<double>(v) : 0.0;
  a.sum[c] += d;
  a.sumsq[c] += d * d;
  a.nonfinite[c] += finite ? 0 : 1;
  a.mn[c] = finite ? fminf(a.mn[c], v) : a.mn[c];
  a.mx[c] = finite ? fmaxf(a.mx[c], v) : a.mx[c];
}
// one cell: the channels in the order of soil_hip.h; height is layers.x + layers.y in fp32 (layer_merge)
__device__ __forceinline__ void acc_cell(Acc& a, float bedrock, float sediment, float waterHeight, float mass,
                                         float debris, float vx, float vy, float dvx, float dvy) {
  acc_value(a, 0, bedrock);
  acc_value(a, 1, sediment);
  acc_value(a, 2, bedrock + sediment);
  acc_value(a, 3, waterHeight);
  acc_value(a, 4, mass);
  acc_value(a, 5, debris);
  acc_value(a, 6, vx);
  acc_value(a, 7, vy);
  acc_value(a, 8, dvx);
  acc_value(a, 9, dvy);
}
__device__ __forceinline__ void acc_record(Acc& a, const soil_model_stats& r) {  // a += r
#pragma unroll
  for (int c = 0; c < kCh; ++c) {
    a.sum[c] += r.ch[c].sum;
    a.sumsq[c] += r.ch[c].sumsq;
    a.nonfinite[c] += r.ch[c].nonfinite;
    a.mn[c] = fminf(a.mn[c], r.ch[c].min);
    a.mx[c] = fmaxf(a.mx[c], r.ch[c].max);
  }
}

// The lanes' accumulators of a work-group folded into *out in a fixed order: across the wave by halving (lane i
// takes lane i + 32, then + 16, ... + 1), then the four waves' records through LDS, wave 0 first, one thread per
// channel.
__device__ __forceinline__ void block_fold(Acc& a, soil_model_stats* __restrict__ out) {
  __shared__ soil_model_stats s_wave[kSWaves];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
    for (int c = 0; c < kCh; ++c) {
      a.sum[c] += __shfl_down(a.sum[c], off);
      a.sumsq[c] += __shfl_down(a.sumsq[c], off);
      a.nonfinite[c] += __shfl_down(a.nonfinite[c], off);
      a.mn[c] = fminf(a.mn[c], __shfl_down(a.mn[c], off));
      a.mx[c] = fmaxf(a.mx[c], __shfl_down(a.mx[c], off));
    }
  }
  const int wave = threadIdx.x / 64;
  if (threadIdx.x % 64 == 0) {
#pragma unroll
    for (int c = 0; c < kCh; ++c)
      s_wave[wave].ch[c] = soil_channel_stats{a.sum[c], a.sumsq[c], a.nonfinite[c], a.mn[c], a.mx[c]};
  }
  __syncthreads();
  if (threadIdx.x < kCh) {
    soil_channel_stats r = s_wave[0].ch[threadIdx.x];
    for (int w = 1; w < kSWaves; ++w) {
      const soil_channel_stats& o = s_wave[w].ch[threadIdx.x];
      r.sum += o.sum;
      r.sumsq += o.sumsq;
      r.nonfinite += o.nonfinite;
      r.min = fminf(r.min, o.min);
      r.max = fmaxf(r.max, o.max);
    }
    out->ch[threadIdx.x] = r;
  }
}

struct StatsPlanes {  // the six planes read, from the launch's first model on
  const float* layers;  // (n, 2)
  const float* waterHeight;
  const float* mass;
  const float* debris;
  const float* velocity;        // (n, 2)
  const float* debrisVelocity;  // (n, 2)
};

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// First pass.  Work-group (x, z) reduces cells [x * chunk, (x + 1) * chunk) of model z into partials[z * P + x].
// In pass i lane t takes the four cells from x * chunk + (i * 256 + t) * 4 on, in their order: which cell goes to
// which lane at which turn does not depend on how it is loaded, so the 16-byte path (this model's six bases
// 16-byte aligned, all four cells inside the model) and the scalar one give the same bits.
__global__ void __launch_bounds__(kSBlock)
    k_stats_partial(StatsPlanes A, int64_t n, int64_t chunk, soil_model_stats* __restrict__ partials) {
  const int64_t first = static_cast<int64_t>(blockIdx.z) * n;  // this model's first cell
  const float* __restrict__ layers = A.layers + 2 * first;
  const float* __restrict__ waterHeight = A.waterHeight + first;
  const float* __restrict__ mass = A.mass + first;
  const float* __restrict__ debris = A.debris + first;
  const float* __restrict__ velocity = A.velocity + 2 * first;
  const float* __restrict__ debrisVelocity = A.debrisVelocity + 2 * first;
  const bool vec = aligned16(layers) && aligned16(waterHeight) && aligned16(mass) && aligned16(debris) &&
                   aligned16(velocity) && aligned16(debrisVelocity);  // uniform over the work-group

  const int64_t begin = static_cast<int64_t>(blockIdx.x) * chunk;
  const int64_t end = begin + chunk < n ? begin + chunk : n;
  Acc a;
  acc_init(a);
  for (int64_t c0 = begin + static_cast<int64_t>(threadIdx.x) * kLaneCells; c0 < end; c0 += kPassCells) {
    if (vec && c0 + kLaneCells <= end) {  // (c0 is a multiple of 4: the loads are 16-byte aligned)
      const float4 l0 = *reinterpret_cast<const float4*>(layers + 2 * c0);
      const float4 l1 = *reinterpret_cast<const float4*>(layers + 2 * c0 + 4);
      const float4 w = *reinterpret_cast<const float4*>(waterHeight + c0);
      const float4 m = *reinterpret_cast<const float4*>(mass + c0);
      const float4 d = *reinterpret_cast<const float4*>(debris + c0);
      const float4 v0 = *reinterpret_cast<const float4*>(velocity + 2 * c0);
      const float4 v1 = *reinterpret_cast<const float4*>(velocity + 2 * c0 + 4);
      const float4 u0 = *reinterpret_cast<const float4*>(debrisVelocity + 2 * c0);
      const float4 u1 = *reinterpret_cast<const float4*>(debrisVelocity + 2 * c0 + 4);
      acc_cell(a, l0.x, l0.y, w.x, m.x, d.x, v0.x, v0.y, u0.x, u0.y);
      acc_cell(a, l0.z, l0.w, w.y, m.y, d.y, v0.z, v0.w, u0.z, u0.w);
      acc_cell(a, l1.x, l1.y, w.z, m.z, d.z, v1.x, v1.y, u1.x, u1.y);
      acc_cell(a, l1.z, l1.w, w.w, m.w, d.w, v1.z, v1.w, u1.z, u1.w);
    } else {
      const int64_t c1 = c0 + kLaneCells < end ? c0 + kLaneCells : end;
      for (int64_t c = c0; c < c1; ++c)
        acc_cell(a, layers[2 * c], layers[2 * c + 1], waterHeight[c], mass[c], debris[c], velocity[2 * c],
                 velocity[2 * c + 1], debrisVelocity[2 * c], debrisVelocity[2 * c + 1]);
    }
  }
  block_fold(a, partials + static_cast<int64_t>(blockIdx.z) * gridDim.x + blockIdx.x);
}

// Second pass.  One work-group per model folds that model's P partial records: lane t takes records t, t + 256, ...
// in ascending order, then the first pass's fold of the lanes.
__global__ void __launch_bounds__(kSBlock)
    k_stats_final(const soil_model_stats* __restrict__ partials, int64_t P, soil_model_stats* __restrict__ out) {
  const soil_model_stats* __restrict__ mine = partials + static_cast<int64_t>(blockIdx.z) * P;
  Acc a;
  acc_init(a);
  for (int64_t p = threadIdx.x; p < P; p += kSBlock) acc_record(a, mine[p]);
  block_fold(a, out + blockIdx.z);
}

typedef float v2f __attribute__((ext_vector_type(2)));

// The ensemble: one thread per cell walks the models in their order, so every load is coalesced along W and the
// order of every sum is b = 0 ... B-1.  Every operation as written (-ffp-contract=off).
template <bool VAR>
__global__ void __launch_bounds__(kSBlock)
    k_ensemble(const float2* __restrict__ layers, const float* __restrict__ waterHeight,
               const float* __restrict__ mass, const float* __restrict__ debris, int64_t B, int64_t n,
               float* __restrict__ mean, float* __restrict__ var) {
  constexpr int kE = SOIL_ENSEMBLE_CHANNELS;
  const double count = static_cast<double>(B);
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kSBlock + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kSBlock) {
    double s[kE], q[kE];
#pragma unroll
    for (int c = 0; c < kE; ++c) s[c] = 0.0, q[c] = 0.0;
#pragma unroll 4
    for (int64_t b = 0; b < B; ++b) {
      const int64_t k = b * n + i;
      const float2 l = layers[k];
      const float v[kE] = {l.x, l.y, l.x + l.y, waterHeight[k], mass[k], debris[k]};
#pragma unroll
      for (int c = 0; c < kE; ++c) {
        const double d = static_cast<double>(v[c]);
        s[c] += d;
        q[c] += d * d;
      }
    }
    float m32[kE], v32[kE];
#pragma unroll
    for (int c = 0; c < kE; ++c) {
      const double m = s[c] / count;
      m32[c] = static_cast<float>(m);
      if constexpr (VAR) {
        const double v = q[c] / count - m * m;
        v32[c] = static_cast<float>(v < 0.0 ? 0.0 : v);
      }
    }
    // six floats per cell, 8-byte aligned: three 8-byte stores, written once and not read again here
#pragma unroll
    for (int c = 0; c < kE; c += 2) {
      __builtin_nontemporal_store(v2f{m32[c], m32[c + 1]}, reinterpret_cast<v2f*>(mean + kE * i + c));
      if constexpr (VAR)
        __builtin_nontemporal_store(v2f{v32[c], v32[c + 1]}, reinterpret_cast<v2f*>(var + kE * i + c));
    }
  }
}

}  // namespace
}  // namespace soil

using namespace soil;

extern "C" {

int soil_erode_batch_stats(const soil_erosion_planes* planes, int64_t B, int64_t H, int64_t W,
                           soil_model_stats* out, void* stream) {
  SOIL_DEVICE();
  SOIL_REQUIRE(planes && out, "erode_batch_stats: null planes or out");
  if (int rc = check_batch(B, H, W, 0, nullptr, "erode_batch_stats"); rc != SOIL_OK) return rc;
  const soil_erosion_planes& S = *planes;
  SOIL_REQUIRE(S.layers && S.waterHeight && S.mass && S.debris && S.velocity && S.debrisVelocity,
               "erode_batch_stats: null plane (layers, waterHeight, mass, debris, velocity and debrisVelocity are "
               "read; height, the flux planes, layers_next, uplift and rainfall are not)");
  const hipStream_t st = as_stream(stream);
  const int64_t n = H * W;
  const int64_t chunk = stats_chunk(n);
  const int64_t P = (n + chunk - 1) / chunk;  // <= kMaxPartials
  void* base = nullptr;
  if (int rc = workspace_get(WS_STATS, sizeof(soil_model_stats) * static_cast<size_t>(B) * static_cast<size_t>(P),
                             &base);
      rc != SOIL_OK)
    return rc;
  soil_model_stats* partials = static_cast<soil_model_stats*>(base);
  for (int64_t b0 = 0; b0 < B; b0 += kMaxModels) {
    const unsigned models = static_cast<unsigned>(B - b0 < kMaxModels ? B - b0 : kMaxModels);
    const int64_t c0 = b0 * n;
    const StatsPlanes A{S.layers + 2 * c0,   S.waterHeight + c0,    S.mass + c0,
                        S.debris + c0,       S.velocity + 2 * c0,   S.debrisVelocity + 2 * c0};
    k_stats_partial<<<dim3(static_cast<unsigned>(P), 1, models), kSBlock, 0, st>>>(A, n, chunk, partials + b0 * P);
    SOIL_LAUNCH_CHECK();
    k_stats_final<<<dim3(1, 1, models), kSBlock, 0, st>>>(partials + b0 * P, P, out + b0);
    SOIL_LAUNCH_CHECK();
  }
  return SOIL_OK;
}

int soil_erode_batch_ensemble(const soil_erosion_planes* planes, int64_t B, int64_t H, int64_t W, float* mean,
                              float* var, void* stream) {
  SOIL_DEVICE();
  SOIL_REQUIRE(planes, "erode_batch_ensemble: null planes");
  SOIL_REQUIRE(mean, "erode_batch_ensemble: null mean (var may be NULL)");
  if (int rc = check_batch(B, H, W, 0, nullptr, "erode_batch_ensemble"); rc != SOIL_OK) return rc;
  const soil_erosion_planes& S = *planes;
  SOIL_REQUIRE(S.layers && S.waterHeight && S.mass && S.debris,
               "erode_batch_ensemble: null plane (layers, waterHeight, mass and debris are read)");
  const hipStream_t st = as_stream(stream);
  const int64_t n = H * W;
  const int64_t blocks = (n + kSBlock - 1) / kSBlock;
  const unsigned grid = static_cast<unsigned>(blocks < (int64_t{1} << 22) ? blocks : (int64_t{1} << 22));
  const float2* layers = reinterpret_cast<const float2*>(S.layers);
  if (var)
    k_ensemble<true><<<grid, kSBlock, 0, st>>>(layers, S.waterHeight, S.mass, S.debris, B, n, mean, var);
  else
    k_ensemble<false><<<grid, kSBlock, 0, st>>>(layers, S.waterHeight, S.mass, S.debris, B, n, mean, nullptr);
  SOIL_LAUNCH_CHECK();
  return SOIL_OK;
}

}  // extern "C"
