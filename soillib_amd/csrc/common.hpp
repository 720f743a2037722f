// common.hpp — shared host/device plumbing of libsoil_hip.so.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <map>
#include <string>
#include <vector>

#include "../../include/soil_hip.h"
#include "soil_math.hpp"

namespace soil {

// ---- error channel ---------------------------------------------------------
void set_error(const std::string& msg);
int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* what, const char* file, int line);
// Makes sure a HIP device is usable; SOIL_ERR_NO_DEVICE otherwise.  There is no
// CPU fallback anywhere in this library.
int require_device();

#define SOIL_HIP(expr)                                                     \
  do {                                                                     \
    hipError_t soil_e_ = (expr);                                           \
    if (soil_e_ != hipSuccess) return ::soil::hip_fail(soil_e_, #expr, __FILE__, __LINE__); \
  } while (0)

#define SOIL_REQUIRE(cond, msg)                                            \
  do {                                                                     \
    if (!(cond)) return ::soil::fail(SOIL_ERR_INVALID_ARGUMENT, msg);      \
  } while (0)

#define SOIL_REQUIRE_IO(cond, msg)                            \
  do {                                                        \
    if (!(cond)) return ::soil::fail(SOIL_ERR_IO, msg);       \
  } while (0)

#define SOIL_DEVICE()                                  \
  do {                                                 \
    int soil_rc_ = ::soil::require_device();           \
    if (soil_rc_ != SOIL_OK) return soil_rc_;          \
  } while (0)

// Reports launch-configuration errors of the kernel launched just before.
#define SOIL_LAUNCH_CHECK() SOIL_HIP(hipGetLastError())

// Per-device scratch, grown on demand and reused across calls (the reference
// cudaMallocs its scratch on every call, graph.cu:539-550, 182-183).  One slot
// per user; calls that share a slot must be stream-ordered with respect to
// each other.
enum WorkspaceSlot {
  WS_ACCUMULATE_0 = 0,   // graph.hip: an accumulation, lane 0 (kAccSlot)
  WS_SMALL_LAUNCH = 1,   // erosion_particles.hip: a single model's staged particle launch
  WS_TILED_FLUVIAL = 2,  // erosion_particles_tiled.hip: the tiled fluvial launch
  WS_MULTIFLOW = 3,      // graph.hip: soil_multiflow
  WS_CONDITIONING = 4,   // conditioning.hip
  WS_TILED_DEBRIS = 5,   // erosion_particles_tiled.hip: the tiled debris launch
  WS_ERODE = 6,          // erosion_step.hip: soil_erode's layers and streams
  WS_STEP_RNG = 7,       // erosion_step.hip: the step's fluvial streams
  WS_PAIR_GATE = 9,      // erosion_particles_tiled.hip: the overlapped pair's gate
  WS_ACCUMULATE_1 = 10,  // graph.hip: an accumulation, lane 1 (kAccSlot)
  WS_BATCH = 11,         // erosion_particles.hip: a batch's seeds or records, then its staged scratch
  WS_STATS = 12,         // erosion_stats.hip: the partial records
  WS_FLOW_BATCH = 13,    // graph.hip: a batch entry's seeds or scale pairs
  WS_ACCUMULATE_BATCH = 14,  // graph.hip: soil_accumulate_batch (stream-ordered: not soil_accumulate's slot)
  WS_FLOW_PATHS = 15,    // flow_paths.hip: soil_flow_paths(_batch): scale records, the two record buffers, lists
  WS_FLATS = 16,         // flats.hip: soil_flat_distance(_batch): the tiles' marks, one mask byte per cell
  WS_DOWNSTREAM = 17,    // downstream.hip: soil_downstream / soil_stream_power (_batch): scale records, records, B, lists
  WS_DIFFUSE = 18,       // diffuse.hip: soil_diffuse(_batch): scale records, the e and g planes of a chunk
  WS_DEPOSIT = 19,       // downstream.hip: soil_stream_power_deposit(_batch): scale records, records, B, lists
  WS_DEPOSIT_RAKE = 20,  // graph.hip rake_accumulate for soil_stream_power_deposit(_batch): an accumulation's scratch
  WS_DEPOSIT_PLANES = 21,  // downstream.hip: soil_stream_power_deposit(_batch): the iterate, q and Qs of a chunk
  WS_POWER_N = 22,       // downstream.hip: soil_stream_power_n(_batch): scale records, records, B, lists
  WS_POWER_N_ITERATE = 23,  // downstream.hip: soil_stream_power_n(_batch): the fp64 iterate of a chunk, 8 bytes a cell
  WS_SLOPE_LIMIT = 24,   // slope_limit.hip: soil_slope_limit(_batch): scale records, the tiles' marks
  WS_UPSTREAM = 25,      // upstream.hip: soil_upstream_extreme(_batch): the two pointer buffers, the packed plane, lists
  WS_STREAM_ORDER = 26,  // stream_order.hip: soil_stream_order(_batch): the two pointer buffers, P, L, D, lists
  WS_MFD = 27,           // mfd.hip: soil_mfd_weights / soil_mfd_accumulate (_batch): scale records, marks, shares, iterate
};
int workspace_get(WorkspaceSlot slot, size_t bytes, void** out);
int workspace_release_all();

// ---- what a host thread owns besides its blocks -------------------------------------
// The streams, events and pinned words that a call keeps from one call of its host thread to the next live in a
// ThreadOwned<T>: device -> T, thread_local at its user.  When the thread ends, every T is released on its device,
// behind a hipDeviceSynchronize(): a pinned word is written by kernels on the caller's stream and a lane may hold
// queued work.  Nothing is released on the thread that loaded the library: its destructors run at process exit, next
// to the HIP runtime's own teardown.  No destructor takes a lock that a call holds while it waits for the device
// (WsThreadGuard synchronises under the workspace mutex; the counts below are atomics).
// Every creation and destruction goes through the helpers, which keep the process-wide counts of
// soil_host_objects_info (runtime.hip).
enum HostObject { HOST_STREAM = 0, HOST_EVENT = 1, HOST_PINNED = 2, HOST_BLOCK = 3 };
void host_object_count(HostObject what, int64_t delta);
bool on_loader_thread();
inline hipError_t owned_stream_create(hipStream_t* s) {
  const hipError_t e = hipStreamCreateWithFlags(s, hipStreamNonBlocking);
  if (e == hipSuccess) host_object_count(HOST_STREAM, 1);
  return e;
}
inline hipError_t owned_event_create(hipEvent_t* ev) {
  const hipError_t e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
  if (e == hipSuccess) host_object_count(HOST_EVENT, 1);
  return e;
}
inline hipError_t owned_pinned_alloc(void** p, size_t bytes, unsigned flags) {
  const hipError_t e = hipHostMalloc(p, bytes, flags);
  if (e == hipSuccess) host_object_count(HOST_PINNED, 1);
  return e;
}
inline hipError_t owned_pinned_free(void* p) {
  if (!p) return hipSuccess;
  host_object_count(HOST_PINNED, -1);
  return hipHostFree(p);
}
inline void owned_stream_destroy(hipStream_t& s) {
  if (!s) return;
  (void)hipStreamSynchronize(s);
  (void)hipStreamDestroy(s);
  host_object_count(HOST_STREAM, -1);
  s = nullptr;
}
inline void owned_event_destroy(hipEvent_t& ev) {
  if (!ev) return;
  (void)hipEventDestroy(ev);
  host_object_count(HOST_EVENT, -1);
  ev = nullptr;
}

template <class Fn>
inline void thread_end_on_device(int device, Fn&& release) {  // `release` on `device`, the thread's device kept
  if (on_loader_thread()) return;
  int before = 0;
  if (hipGetDevice(&before) != hipSuccess) {
    (void)hipGetLastError();
    return;
  }
  if (hipSetDevice(device) == hipSuccess) {
    (void)hipDeviceSynchronize();
    release();
  }
  (void)hipSetDevice(before);
  (void)hipGetLastError();
}

template <class T>  // T: default-constructible, with release()
struct ThreadOwned {
  std::map<int, T> of;  // device -> the thread's objects there
  T& operator[](int device) { return of[device]; }
  ~ThreadOwned() {
    for (auto& kv : of) thread_end_on_device(kv.first, [&] { kv.second.release(); });
  }
};

// "something changed in this launch": a pinned, device-mapped int the kernels write straight into
struct PinnedWord {
  int *host = nullptr, *dev = nullptr;
  hipError_t ensure() {
    if (host) return hipSuccess;
    void* p = nullptr;
    hipError_t e = owned_pinned_alloc(&p, sizeof(int), hipHostMallocMapped | hipHostMallocCoherent);
    if (e != hipSuccess) return e;
    host = static_cast<int*>(p);
    e = hipHostGetDevicePointer(reinterpret_cast<void**>(&dev), host, 0);
    if (e != hipSuccess) release();
    return e;
  }
  void release() {
    (void)owned_pinned_free(host);
    host = dev = nullptr;
  }
};

// Device counter of particle steps (iterations that pass the loop head and its
// slab check, i.e. what the oracle counts), accumulated by every particle launch
// on this device; read and reset through soil_particle_steps().
int step_counter(unsigned long long** out);

// The fused cell phase behind soil_erode_cells_fused_ex (`colour` null) and soil_erode_cells_fused_colour
// (erosion_cells.hip); the entries' own checks of `colour` are the caller's.
int erode_cells_fused(const soil_erosion_planes* pl, const soil_colour_planes* colour, const soil_domain* dom,
                      const float scale[3], const soil_param* param, int flags, void* stream);

// The batch entries' checks of their sizes (soil_hip.h, soil_*_batch): SOIL_ERR_INVALID_ARGUMENT with a message
// naming `what` for B < 1, an empty grid, N < 0, null seeds with N > 0, byte offsets that overflow
// (erosion_particles.hip).
int check_batch(int64_t B, int64_t H, int64_t W, int64_t N, const uint64_t* seeds, const char* what);
// The entries' null-plane checks (true: every plane of the set is there).  The particle launches read and add to
// ten physics planes; the step and the cell phase need all fourteen but `height`.  The colour entries need all
// four colour planes, the coloured slab pair every one but albedo_bedrock.
enum PlaneSet { PARTICLE_PLANES, STEP_PLANES };
inline bool has_planes(const soil_erosion_planes& P, PlaneSet set) {
  return P.layers && P.rainfall && P.waterHeight && P.waterFlux && P.massFlux && P.velocity && P.velocityFlux &&
         P.debrisFlux && P.debrisVelocity && P.debrisVelocityFlux &&
         (set == PARTICLE_PLANES || (P.layers_next && P.uplift && P.mass && P.debris));
}
inline bool has_colour(const soil_colour_planes* C, bool bedrock = true) {
  return C && (C->albedo_bedrock || !bedrock) && C->albedo_surface && C->albedo_fluvial && C->albedo_debris;
}
// B records (a host array) copied to the device in one copy through the batches' pinned staging, into workspace
// slot WS_BATCH (erosion_particles.hip); *models_dev valid in stream order until the slot's next use.
int batch_models_to_device(const soil_batch_model* models, int64_t B, hipStream_t st,
                           const soil_batch_model** models_dev);

// The accumulation of soil_accumulate_batch without decay (graph.hip: the rake-compress engine as it is, chunks of
// whole models, model b's slice the bits soil_accumulate gives for it alone), stream-ordered on `st` through workspace
// `slot` and without the entry's checks: B models of (H, W), `edge` SOIL_D4 or SOIL_D8.  `stats` (may be null): the
// launches are added, the bytes raised to the largest block asked for.
struct RakeStats {
  int64_t launches, bytes;
};
int rake_accumulate(float* out, const int32_t* graph, const float* source, int64_t B, int64_t H, int64_t W, int edge,
                    hipStream_t st, WorkspaceSlot slot, RakeStats* stats);

// `bytes` of a host array copied to `dst` (device) in one stream-ordered copy through the same pinned staging
// (erosion_particles.hip): the array may go as soon as the call returns.
int batch_upload(void* dst, const void* src, size_t bytes, hipStream_t st);

// One call of a batch entry point (soil_hip.h: soil_erode_step_batch, soil_particles_batch,
// soil_erode_cells_fused_batch and their _colour, _params and _models forms), as erosion_batch.hip fills and
// checks it and the two phases below read it: B whole-grid models of (H, W), one after the other in every plane.
struct BatchCall {
  const char* what;                        // the entry's name in its messages ("erode_step_batch_colour")
  const soil_erosion_planes* P;
  const soil_colour_planes* C = nullptr;   // null: physics only; otherwise the four colour planes of all B models
  int64_t B, H, W;
  int64_t N = 0;                           // walkers per model, or max N_b (a cells entry: 0)
  // a uniform batch: every model with *param and scale, model b's streams at (seeds[b], step_index * N), seeds a
  // host array of B ...
  const uint64_t* seeds = nullptr;
  uint64_t step_index = 0;
  const float* scale = nullptr;
  const soil_param* param = nullptr;       // (a sweep's entry: its B params, which become records)
  // ... or B host records (different models; a sweep's from its params): model b with the param, scale, N_b, seed
  // and step index of models[b], and the four above are not read
  const soil_batch_model* models = nullptr;
  int flags = 0;                           // the cell phase's (SOIL_CELLS_KEEP_FLUX)
  hipStream_t st;
};
// Both particle launches of a batch (erosion_particles.hip): direct or staged shape by the single model's rule, one
// launch after the other on c.st, the debris launch two draws on.  With c.C the two colour flux planes of all B
// models are cleared first, and the launches deposit colour from albedo_surface into them.  Records reach the
// device in place of the seeds; `records_dev` (the step's; may be null) receives that device copy for the cell
// phase, valid in stream order until WS_BATCH's next use — with N == 0 they are uploaded alone
// (batch_models_to_device), and only when asked for.
int particles_batch(const BatchCall& c, const soil_batch_model** records_dev = nullptr);
// The cell phase of a batch (erosion_cells.hip): a uniform batch's (`records_dev` null), or model b with the param
// and scale of records_dev[b], a device array of B records.
int erode_cells_fused_batch(const BatchCall& c, const soil_batch_model* records_dev);

// Launch shape of the per-cell kernels: threads along the contiguous axis, and a
// work-group walks a band of kRowBand consecutive rows (SOIL_ROW_LOOP).  A 64-bit
// n / W, n % W per cell costs more than most of these kernels' arithmetic, and with
// consecutive rows in one work-group the rows x-1, x of a 3x3 stencil come out of
// that CU's L1 instead of being fetched again by a work-group on another XCD.
constexpr int kRowBand = 16;
// grid.y is capped at 65535: a work-group of a taller grid (> 1 M rows) walks several bands
inline dim3 grid_rows(int64_t H, int64_t W, int threads) {
  const int64_t bands = (H + kRowBand - 1) / kRowBand;
  return dim3(static_cast<unsigned>((W + threads - 1) / threads),
              static_cast<unsigned>(bands < 65535 ? bands : 65535));
}
#define SOIL_ROW_LOOP(x, H)                                                          \
  for (int64_t x##_band = blockIdx.y; x##_band * ::soil::kRowBand < (H);             \
       x##_band += gridDim.y)                                                        \
    for (int64_t x = x##_band * ::soil::kRowBand,                                    \
                 x##_end = (x + ::soil::kRowBand < (H)) ? x + ::soil::kRowBand : (H); \
         x < x##_end; ++x)

inline hipStream_t as_stream(void* s) { return static_cast<hipStream_t>(s); }
inline unsigned blocks_for(int64_t n, int threads) {
  return static_cast<unsigned>((n + threads - 1) / threads);
}

// ---- kernel-side PODs ------------------------------------------------------

struct Dom {  // soil_domain by value
  int64_t H, W, x0, rows, r0, r1;
};
inline Dom full_domain(int64_t H, int64_t W) { return Dom{H, W, 0, H, 0, H}; }
inline Dom to_dom(const soil_domain* d) { return Dom{d->H, d->W, d->x0, d->rows, d->r0, d->r1}; }
int check_domain(const Dom& d);

struct Scale3 {
  float x, y, z;
};
struct Scale2 {
  float x, y;
};

// param_t travels to the kernels by value, like in the reference.
using Param = soil_param;

// Where a kernel's Param, scale and walker count come from, a compile-time choice (the batch kernels: grid.y is
// the model).  Every kernel takes its model's Param once at entry into a local copy (`model()`), and its scale and
// walker count through `scale(s)` and `walkers(N)`, which are handed the kernel's own arguments; blockIdx.y is
// uniform over the work-group, so a record's reads are scalar loads, and the walks and cells see
// register-resident constants either way.  `from_model(b0)`: the source of a launch whose model 0 is model b0 of
// the batch (grid.y <= 65535).
struct UniformParam {  // one param_t for every model: the kernel arguments themselves
  Param p;
  static constexpr bool kPerModel = false;
  UniformParam() = default;
  UniformParam(const Param& q) : p(q) {}  // (implicit: the single-model launches pass a Param)
  __device__ __forceinline__ Param model() const { return p; }
  __device__ __forceinline__ Scale3 scale(Scale3 s) const { return s; }
  __device__ __forceinline__ int64_t walkers(int64_t N) const { return N; }
  UniformParam from_model(int64_t) const { return *this; }
};
// a batch of different models (soil_*_batch_models, and the sweeps built on it): model b steps with models[b], a
// device array of B records; the kernel's scale and N arguments are not read
struct ModelParams {
  const soil_batch_model* __restrict__ models;
  static constexpr bool kPerModel = true;
  __device__ __forceinline__ const soil_batch_model& record() const { return models[blockIdx.y]; }
  __device__ __forceinline__ Param model() const { return record().param; }
  __device__ __forceinline__ Scale3 scale(Scale3) const {
    const soil_batch_model& m = record();
    return Scale3{m.scale[0], m.scale[1], m.scale[2]};
  }
  __device__ __forceinline__ int64_t walkers(int64_t) const { return record().N; }
  ModelParams from_model(int64_t b0) const { return ModelParams{models + b0}; }
};

// ---- device helpers shared by the erosion kernels --------------------------

// float -> cell coordinate with the semantics of the reference's device code
// (CUDA cvt.rzi: truncate toward zero, NaN -> 0).  The NaN case is live: a
// particle spawned on a pit cell with zero velocity has speed 0/sqrt(0) = NaN
// (erosion.cu:77-79), is never "out of bounds", and keeps depositing into cell
// (0,0) until maxage — restated as is.
__device__ __forceinline__ int64_t cell_of(float f) {
  return (f != f) ? 0 : static_cast<int64_t>(f);
}

__device__ __forceinline__ float length2(float x, float y) {  // erosion_map.cu:49-53
  return sqrtf(x * x + y * y);
}

// erosion_map.cu:56-78 (and its duplicate path.cu:27-49).  IEEE division by
// zero and fmaxf/fminf NaN handling are load-bearing here.
//
// The reference takes fmax of the times to both faces of the cell, (x_neg - px) / dx
// and (x_pos - px) / dx.  x_neg - px <= 0 <= x_pos - px for every finite px, and IEEE
// division is monotonic and sign-symmetric, so for dx > 0 the maximum IS the second
// quotient and for dx < 0 the first, bit for bit (signed zeros included; a NaN px or
// dx gives NaN either way): one division per axis instead of two.  A zero dx divides
// to infinities whose maximum depends on both numerators: that case keeps both — and so
// does a NaN in either component, whose product with the other one is NaN, not zero: a
// direction (NaN, 0) (a speed that has overflowed to (inf, finite), v_norm = inf) must
// keep the reference's fmaxf(-inf, +inf) = +inf on the zero axis, not take -inf from the
// single quotient (v_step = -inf and NaN attenuations, where the reference clamps to sqrt2).
__device__ __forceinline__ float stepsize_both(float neg, float pos, float d) {
  return fmaxf(neg / d, pos / d);
}
__device__ __forceinline__ float stepsize(float px, float py, float dx, float dy) {
  const float tmax = kSqrt2;
  const float x_neg = floorf(px);
  const float y_neg = floorf(py);
  const float x_pos = 1.0f + x_neg;
  const float y_pos = 1.0f + y_neg;
  float tx, ty;
  const float p = dx * dy;
  if (!(p < 0.0f || p > 0.0f)) {  // a zero (or underflowing) or NaN direction component: as written
    tx = stepsize_both(x_neg - px, x_pos - px, dx);
    ty = stepsize_both(y_neg - py, y_pos - py, dy);
  } else {
    tx = ((dx > 0.0f ? x_pos : x_neg) - px) / dx;
    ty = ((dy > 0.0f ? y_pos : y_neg) - py) / dy;
  }
  tx = fminf(tx, tmax);
  ty = fminf(ty, tmax);
  return 0.5f * (tx + ty);
}

// Downhill-clamped one-sided slopes from the five heights of a cell's
// neighbourhood, erosion_map.cu:131-157.  A NaN height marks a neighbour
// outside the GLOBAL grid (the reference's sentinel, :122-125).
__device__ __forceinline__ float2 glocal_from_heights(float h, float hn0, float hp0, float h0n,
                                                      float h0p, Scale3 s, float exitSlope) {
  float gxn = (h - hn0) * s.z / s.x;
  if (gxn != gxn) gxn = exitSlope;
  else gxn = fmaxf(gxn, 0.0f);
  float gyn = (h - h0n) * s.z / s.y;
  if (gyn != gyn) gyn = exitSlope;
  else gyn = fmaxf(gyn, 0.0f);
  float gxp = (hp0 - h) * s.z / s.x;
  if (gxp != gxp) gxp = -exitSlope;
  else gxp = fminf(gxp, 0.0f);
  float gyp = (h0p - h) * s.z / s.y;
  if (gyp != gyp) gyp = -exitSlope;
  else gyp = fminf(gyp, 0.0f);

  float gx = 0.0f;
  if (fabsf(gxn) > fabsf(gx)) gx = gxn;
  if (fabsf(gxp) > fabsf(gx)) gx = gxp;
  float gy = 0.0f;
  if (fabsf(gyn) > fabsf(gy)) gy = gyn;
  if (fabsf(gyp) > fabsf(gy)) gy = gyp;
  return make_float2(gx, gy);
}

// __glocal, erosion_map.cu:107-159, for global cell (gx, y) of a slab-local
// (rows, W, 2) layer plane.
__device__ __forceinline__ float2 glocal(const float2* __restrict__ layers, const Dom& d, Scale3 s,
                                         int64_t gx, int64_t y, float exitSlope) {
  const int64_t i = (gx - d.x0) * d.W + y;
  const float2 c = layers[i];
  const float h = c.x + c.y;
  const float nan = __builtin_nanf("");
  float hn0 = nan, hp0 = nan, h0n = nan, h0p = nan;
  if (gx - 1 >= 0) {
    const float2 v = layers[i - d.W];
    hn0 = v.x + v.y;
  }
  if (gx + 1 < d.H) {
    const float2 v = layers[i + d.W];
    hp0 = v.x + v.y;
  }
  if (y - 1 >= 0) {
    const float2 v = layers[i - 1];
    h0n = v.x + v.y;
  }
  if (y + 1 < d.W) {
    const float2 v = layers[i + 1];
    h0p = v.x + v.y;
  }
  return glocal_from_heights(h, hn0, hp0, h0n, h0p, s, exitSlope);
}

// soil.resize of the multiscale driver (example/erosion_gpu_multiscale.py:104-141).
// The reference snapshot holds no definition of it; defined here as
// bilinear resampling at corner-aligned positions: new cell (i, j) samples the old
// grid at (i*(Ho-1)/(Hn-1), j*(Wo-1)/(Wn-1)), with the weights written as in the
// reference's sampler, (1 - t)*a + t*b (sample.hpp:48-60) — exact at t = 0 and 1, so
// equal resolutions give the identity and the corners are kept.  (That sampler itself
// stops interpolating in the last cell of each axis, sample.hpp:172-173; a resize
// must not.)  Shared by k_resize (stencil.hip: one plane) and k_erode_resize
// (erosion_resize.hip: every plane of a model).
__device__ __forceinline__ float resize_pos(int64_t i, int64_t n_new, int64_t n_old) {
  if (n_new <= 1) return 0.0f;
  const float step = static_cast<float>(n_old - 1) / static_cast<float>(n_new - 1);
  return fminf(static_cast<float>(i) * step, static_cast<float>(n_old - 1));
}

}  // namespace soil
