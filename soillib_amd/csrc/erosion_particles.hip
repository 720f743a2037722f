// erosion_particles.hip — Monte-Carlo transport half of the erosion model:
//   __transport_fluvial erosion.cu:29-141, __transport_debris :245-351, and the
//   host wrappers soil::transport_fluvial :189-239 / soil::transport_debris :395-436.
//
// One lane integrates one streamline; the flux planes are accumulated with
// hardware fp32 atomics (global_atomic_add_f32; built with -munsafe-fp-atomics).
//
// The reference launches thread n on particle n and lets every step gather a
// 5-point float2 stencil at a random place: on MI355X that is one HBM sector
// per gather (measured, profiles/r01_first).  Two MI355X-side changes, neither
// of which alters a single trajectory or deposit:
//   * STAGED GATHERS — a streaming pre-pass evaluates __glocal once per cell and
//     packs {grad.x, grad.y, vel.x, vel.y} into one float4 plane, so a step
//     costs one 16-byte gather (+4 bytes of waterHeight for fluvial) instead of
//     seven scattered loads;
//   * SPATIAL ORDER — particles are bucketed by the 16x16-cell tile of their
//     spawn point (count / scan / scatter) and traced in tile order, and the
//     work-groups of one XCD walk a contiguous band of tiles, so the lanes of a
//     wave and the waves of an XCD share cache lines for most of their walk.
// The reference's launch shape (thread n = particle n, direct stencil gathers)
// is kept as `direct` mode for ablation (soil_set_particle_mode).
#include <cstddef>
#include <cstring>
#include <initializer_list>
#include <map>
#include <thread>

#include "particles_common.hpp"

namespace soil {

constexpr int kPBlock = 256;
constexpr int kTile = 16;  // spawn-order bucket edge, in cells

int launch_normalize_fluvial(const float* waterFlux, const float* massFlux,
                             const float* velocityFlux, float* albedoFlux, const float* layers,
                             const float* waterSource, float* waterHeight, float* mass,
                             float* velocity, const float* albedoSource, const Dom& d, Scale3 s,
                             const Param& p, hipStream_t st);
int launch_normalize_debris(const float* massFlux, const float* velocityFlux, float* albedoFlux,
                            const float* layers, float* mass, float* velocity,
                            const float* albedoSource, const Dom& d, Scale3 s, const Param& p,
                            hipStream_t st);

static int g_particle_mode = 0;  // 0 auto, 1 direct, 2 staged, 3 tiled
// Arithmetic of the particle step in the tiled shape: 0 exact (IEEE quotients and square root: the
// oracle's walks step for step), 1 fast (v_rcp_f32 / v_sqrt_f32, erosion_particles_tiled.hip:
// step_geom_fast; statistical parity).  SOIL_PARTICLE_DIV=fast in the environment sets the default.
static int g_particle_arith = [] {
  const char* e = std::getenv("SOIL_PARTICLE_DIV");
  return (e && (e[0] == 'f' || e[0] == 'F' || e[0] == '1')) ? 1 : 0;
}();
bool particle_arith_fast() { return g_particle_arith == 1; }
// Spent debris walkers (erosion_particles_tiled.hip: debris_spent): 1 (default) they end their walks, 0 every
// walker is walked to the end as in the reference, 2 they are marked, walked on and watched (tests).
// SOIL_DEBRIS_RETIRE in the environment sets the default of the process.
static int g_debris_retire = [] {
  const char* e = std::getenv("SOIL_DEBRIS_RETIRE");
  const int v = e ? std::atoi(e) : 1;
  return (v >= 0 && v <= 2) ? v : 1;
}();
int debris_retire_mode() { return g_debris_retire; }

// ---- where a step gets grad(cell) and velocity(cell) from -------------------

struct DirectFields {  // the reference's access pattern
  const float2* __restrict__ layers;
  const float2* __restrict__ velocity;
  Dom d;
  Scale3 s;
  float exitSlope;
  __device__ __forceinline__ void at(int64_t cx, int64_t cy, int64_t l, float2& grad,
                                     float2& vel) const {
    grad = glocal(layers, d, s, cx, cy, exitSlope);
    vel = velocity[l];
  }
};

struct PackedFields {  // one 16-byte gather per step
  const float4* __restrict__ p4;
  __device__ __forceinline__ void at(int64_t, int64_t, int64_t l, float2& grad,
                                     float2& vel) const {
    const float4 v = p4[l];
    grad = make_float2(v.x, v.y);
    vel = make_float2(v.z, v.w);
  }
};

struct FluvialPlanes {
  float* __restrict__ waterFlux;
  float* __restrict__ massFlux;
  float* __restrict__ velocityFlux;
  float* __restrict__ albedoFlux;
  const float* __restrict__ waterSource;
  const float* __restrict__ waterHeight;
  const float* __restrict__ albedoSource;
  float* __restrict__ remote0;
  unsigned long long* __restrict__ steps;  // step_counter() of the device
  float* __restrict__ remoteA = nullptr;   // float[6]: the NaN walkers' colour for (0,0), fluvial | debris (Remote0)
};

// __transport_fluvial, erosion.cu:49-139, from the spawn position on
template <class Fields>
__device__ __forceinline__ void trace_fluvial(const Fields& F, const FluvialPlanes& P, float px,
                                              float py, int64_t N, const Dom& d, Scale3 s,
                                              const Param& param) {
  const float A = s.x * s.y;                                   // :50
  const float Lx = s.x, Ly = s.y;                              // :51
  const float Pr = 1.0f / (A * static_cast<float>(d.H * d.W)); // :53
  const float Q = 1.0f / (Pr * static_cast<float>(N));         // :54
  const float eps = 1E-12f;                                    // :55
  const int64_t W = d.W;
  const int64_t base = d.x0 * W;
  int64_t ind = cell_of(px) * W + cell_of(py);  // :60

  const float rho_w = param.densityWater;                 // :63
  const float tau = param.bedShearWater;                  // :65
  const float nu = param.viscosityWater;                  // :66
  const float g = param.gravity;                          // :67
  const float ks = param.suspensionRateFluvial / 64.0f;   // :68
  const float kd = param.depositionRateFluvial * 1.33f;   // :69
  const float fD = param.frictionFactor / 8.0f;           // :70
  const float alpha = param.fluvialExponent;              // :71
  const float R = param.rainfall;                         // :72

  float2 vel, grad;
  F.at(cell_of(px), cell_of(py), ind - base, grad, vel);    // :75-76
  float spx = -(g * grad.x) + nu * vel.x + param.force[0];  // :77
  float spy = -(g * grad.y) + nu * vel.y + param.force[1];
  {
    const float den = sqrtf(length2(Lx * spx, Ly * spy));  // :78
    spx = spx / den;
    spy = spy / den;
  }
  if (length2(spx, spy) < eps) return;  // :79-80

  const float v = length2(vel.x, vel.y);                              // :83
  const float shear = 0.125f * fD * rho_w * v * v;                    // :84
  const float power = powf_(shear * length2(grad.x, grad.y), alpha);  // :85
  const float source_m = Q * ks * power;                              // :88
  const float source_w = Q * R * P.waterSource[ind - base];           // :89
  const float source_vx = Q * (-(g * grad.x) + nu * vel.x);           // :90
  const float source_vy = Q * (-(g * grad.y) + nu * vel.y);
  float source_a[3] = {0.0f, 0.0f, 0.0f};
  if (P.albedoSource)  // :91
    for (int c = 0; c < 3; ++c) source_a[c] = source_m * P.albedoSource[3 * (ind - base) + c];

  float att_w = 1.0f, att_m = 1.0f, att_v = 1.0f;  // :94-96
  const float lenL = length2(Lx, Ly);
  uint64_t iter = 0;
  uint32_t nsteps = 0;
  while (!oob(d, px, py) && ++iter < param.maxage) {  // :100
    const int64_t cx = cell_of(px), cy = cell_of(py);
    if (slab_escape(d, cx)) {
      // a NaN walker's single deposit belongs to global cell (0,0); when that
      // cell lives on another rank it is parked in `remote0` for its owner
      if (px != px && P.remote0 && ind != 0) {
        atomicAdd(&P.remote0[0], att_w * source_w);
        atomicAdd(&P.remote0[1], att_m * source_m);
        atomicAdd(&P.remote0[2], att_v * source_vx);
        atomicAdd(&P.remote0[3], att_v * source_vy);
      }
      if (px != px && P.remoteA && ind != 0)
        for (int c = 0; c < 3; ++c) atomicAdd(&P.remoteA[c], att_m * source_a[c]);
      break;
    }
    ++nsteps;
    const int64_t nind = cx * W + cy;  // :103
    if (nind != ind) {                 // :104-113
      ind = nind;
      const int64_t l = ind - base;
      atomicAdd(&P.waterFlux[l], att_w * source_w);
      atomicAdd(&P.massFlux[l], att_m * source_m);
      atomicAdd(&P.velocityFlux[2 * l], att_v * source_vx);
      atomicAdd(&P.velocityFlux[2 * l + 1], att_v * source_vy);
      if (P.albedoFlux)
        for (int c = 0; c < 3; ++c) atomicAdd(&P.albedoFlux[3 * l + c], att_m * source_a[c]);
    }
    const float v_norm = length2(spx, spy);            // :116
    const float ux = spx / v_norm, uy = spy / v_norm;  // :117
    const float v_step = stepsize(px, py, ux, uy);     // :118
    const float dL = v_step * lenL;                    // :119
    const float ds = dL / v_norm;                      // :120
    if (v_norm < eps) break;                           // :121-122

    const int64_t l = ind - base;
    float2 vc;
    F.at(cx, cy, l, grad, vc);                                    // :125
    const float ax = -(g * grad.x) + nu * vc.x + param.force[0];  // :126
    const float ay = -(g * grad.y) + nu * vc.y + param.force[1];
    const float w0 = 1.0f / (1.0f + dL * (tau + nu));  // :127
    const float w1 = dL / (1.0f + dL * (tau + nu));
    spx = w0 * spx + w1 * ax;
    spy = w0 * spy + w1 * ay;

    const float decay_m = kd;                                      // :130
    const float decay_w = param.evapRate;                          // :131
    const float decay_v = 0.125f * fD / (eps + P.waterHeight[l]);  // :132
    att_m = att_m * att_exp(-ds * decay_m);                          // :134
    att_w = att_w * att_exp(-ds * decay_w);                          // :135
    att_v = att_v * att_exp(-dL * decay_v);                        // :136
    px += v_step * ux;                                             // :137
    py += v_step * uy;
  }
  atomicAdd(P.steps, static_cast<unsigned long long>(nsteps));  // one atomic per wave
}

struct DebrisPlanes {
  float* __restrict__ massFlux;
  float* __restrict__ velocityFlux;
  float* __restrict__ albedoFlux;
  const float* __restrict__ albedoSource;
  float* __restrict__ remote0;
  unsigned long long* __restrict__ steps;  // step_counter() of the device
  float* __restrict__ remoteA = nullptr;   // as FluvialPlanes::remoteA
};

// __transport_debris, erosion.cu:262-349, from the spawn position on
template <class Fields>
__device__ __forceinline__ void trace_debris(const Fields& F, const DebrisPlanes& P, float px,
                                             float py, int64_t N, const Dom& d, Scale3 s,
                                             const Param& param) {
  const float A = s.x * s.y;                                    // :263
  const float Lx = s.x, Ly = s.y;                               // :264
  const float Pr = 1.0f / (A * static_cast<float>(d.H * d.W));  // :266
  const float Q = 1.0f / (Pr * static_cast<float>(N));          // :267
  const float eps = 1E-12f;                                     // :268
  const int64_t W = d.W;
  const int64_t base = d.x0 * W;
  int64_t ind = cell_of(px) * W + cell_of(py);  // :273

  const float theta = param.critSlopeBedrock;    // :276
  const float nu = param.viscosityDebris;        // :277
  const float tau = param.bedShearDebris;        // :278
  const float g = param.gravity;                 // :279
  const float kl = param.landslideRateDebris;    // :280
  const float kdd = param.depositionRateDebris;  // :281
  const float kds = param.suspensionRateDebris;  // :282
  const float tau_y = param.yieldStress;         // :283

  float2 vel, grad;
  F.at(cell_of(px), cell_of(py), ind - base, grad, vel);  // :286-287
  float spx = -(g * grad.x) + nu * vel.x;                 // :288
  float spy = -(g * grad.y) + nu * vel.y;
  {
    const float den = sqrtf(length2(Lx * spx, Ly * spy));  // :289
    spx = spx / den;
    spy = spy / den;
  }
  if (length2(spx, spy) < eps) return;  // :290-291

  const float excessSlope0 = length2(grad.x, grad.y) - theta;  // :294
  const float suspend = fmaxf(0.0f, kl * excessSlope0);        // :295
  const float source_d = Q * suspend;                          // :297
  const float source_vx = Q * (-g * grad.x + nu * vel.x);      // :298
  const float source_vy = Q * (-g * grad.y + nu * vel.y);
  float source_a[3] = {0.0f, 0.0f, 0.0f};
  if (P.albedoSource)  // :299
    for (int c = 0; c < 3; ++c) source_a[c] = source_d * P.albedoSource[3 * (ind - base) + c];

  float att_d = 1.0f, att_v = 1.0f;  // :301-302
  const float lenL = length2(Lx, Ly);
  uint64_t iter = 0;
  uint32_t nsteps = 0;
  while (!oob(d, px, py) && ++iter < param.maxage) {  // :306
    const int64_t cx = cell_of(px), cy = cell_of(py);
    if (slab_escape(d, cx)) {
      if (px != px && P.remote0 && ind != 0) {  // NaN walker: see trace_fluvial
        atomicAdd(&P.remote0[4], att_d * source_d);
        atomicAdd(&P.remote0[5], att_v * source_vx);
        atomicAdd(&P.remote0[6], att_v * source_vy);
      }
      if (px != px && P.remoteA && ind != 0)
        for (int c = 0; c < 3; ++c) atomicAdd(&P.remoteA[3 + c], att_d * source_a[c]);
      break;
    }
    ++nsteps;
    const int64_t nind = cx * W + cy;  // :309
    if (nind != ind) {                 // :310-318
      ind = nind;
      const int64_t l = ind - base;
      atomicAdd(&P.massFlux[l], att_d * source_d);
      atomicAdd(&P.velocityFlux[2 * l], att_v * source_vx);
      atomicAdd(&P.velocityFlux[2 * l + 1], att_v * source_vy);
      if (P.albedoFlux)
        for (int c = 0; c < 3; ++c) atomicAdd(&P.albedoFlux[3 * l + c], att_d * source_a[c]);
    }
    const float v_norm = length2(spx, spy);            // :321
    const float ux = spx / v_norm, uy = spy / v_norm;  // :322
    const float v_step = stepsize(px, py, ux, uy);     // :323
    const float dL = v_step * lenL;                    // :324
    const float ds = dL / v_norm;                      // :325
    if (v_norm < eps) break;                           // :326-327

    const int64_t l = ind - base;
    float2 vc;
    F.at(cx, cy, l, grad, vc);                          // :330
    const float debrisHeight = eps + att_d * source_d;  // :331
    const float ax = -(g * grad.x) + nu * vc.x;         // :332
    const float ay = -(g * grad.y) + nu * vc.y;
    const float decay = nu + tau / debrisHeight;        // :333
    const float w = 1.0f / (1.0f + dL * decay);         // :334
    spx = w * spx + w * dL * ax;                        // :335
    spy = w * spy + w * dL * ay;

    const float excessSlope = length2(grad.x, grad.y) - theta;            // :339
    const float excessStress = g * (excessSlope - tau_y / debrisHeight);  // :340
    const float shearRate = (excessStress < 0.0f) ? kdd : kds;            // :341
    const float decay_d = ds * shearRate * excessStress / v_norm;         // :342
    const float decay_v = nu + tau / debrisHeight;                        // :343
    att_d = att_d * expf_(decay_d);                                       // :345
    att_v = att_v * att_exp(-dL * decay_v);                               // :346
    px += v_step * ux;                                                    // :347
    py += v_step * uy;
  }
  atomicAdd(P.steps, static_cast<unsigned long long>(nsteps));
}

// ---- the small-N shapes: direct and staged -------------------------------------------
//
// One kernel per step of a shape, for a single model and for a batch of B independent models alike: grid.y is
// the model (a single model: gridDim.y == 1, model 0), and model b's planes start b * rows * W cells on (C
// channels: b * rows * W * C elements), its spawn and sorted arrays b * N walkers on, its tile counters, fills
// and starts b * (tiles + 1) on.  A batch is B whole-grid models (Dom{H, W, 0, H, 0, H}): every spawn is owned,
// the stencil covers every row, and no deposit leaves its model (remote0 / remoteA null).

constexpr int64_t kMaxGridY = 65535;  // models per launch

__device__ __forceinline__ int64_t model_base(int64_t per_model) {
  return static_cast<int64_t>(blockIdx.y) * per_model;
}

// Where a launch's walkers take their first two draws from, a compile-time choice.  (Streams, the tiled
// shape's runtime switch, stays as it is: its kernels take it by value.)
// `walkers(N)`: how many of a launch's N walkers per model model blockIdx.y draws (the others exit first).
struct TensorDraws {  // a single model's soil_rng tensor: every state read, drawn from and written back
  soil_rng* __restrict__ rng;
  __device__ __forceinline__ float2 spawn(int64_t n, const Dom& d) const { return spawn_position(rng, n, d); }
  __device__ __forceinline__ int64_t walkers(int64_t N) const { return N; }
  TensorDraws from_model(int64_t) const { return *this; }  // (B == 1)
};
struct SeedDraws {  // a batch's uniform streams: walker n of model b at (seeds[b], n, offset), nothing stored
  const uint64_t* __restrict__ seeds;
  uint64_t offset;
  __device__ __forceinline__ float2 spawn(int64_t n, const Dom& d) const {
    return spawn_position(Streams{nullptr, true, seeds[blockIdx.y], offset}, n, d);
  }
  __device__ __forceinline__ int64_t walkers(int64_t N) const { return N; }
  SeedDraws from_model(int64_t b0) const { return SeedDraws{seeds + b0, offset}; }
};
// a batch of different models' uniform streams (ModelParams): walker n < N_b of model b at
// (seed_b, n, step_index_b * N_b + extra), `extra` 2 for the debris launch; nothing stored
struct ModelDraws {
  ModelParams m;
  uint64_t extra;
  __device__ __forceinline__ float2 spawn(int64_t n, const Dom& d) const {
    const soil_batch_model& r = m.record();
    const uint64_t offset = r.step_index * static_cast<uint64_t>(r.N) + extra;
    return spawn_position(Streams{nullptr, true, r.seed, offset}, n, d);
  }
  __device__ __forceinline__ int64_t walkers(int64_t N) const { return m.walkers(N); }
  ModelDraws from_model(int64_t b0) const { return ModelDraws{m.from_model(b0), extra}; }
};

// the planes of model blockIdx.y.  ALB: a coloured batch (soil_particles_batch_colour) — the colour flux plane
// and the spawn colours (albedo_surface) are advanced too, where set; no other launch needs them advanced
template <bool ALB>
__device__ __forceinline__ FluvialPlanes model_of(FluvialPlanes P, int64_t cells) {
  const int64_t m = model_base(cells);
  P.waterFlux += m, P.massFlux += m, P.velocityFlux += 2 * m, P.waterSource += m, P.waterHeight += m;
  if constexpr (ALB) {
    if (P.albedoFlux) P.albedoFlux += 3 * m;
    if (P.albedoSource) P.albedoSource += 3 * m;
  }
  return P;
}
template <bool ALB>
__device__ __forceinline__ DebrisPlanes model_of(DebrisPlanes P, int64_t cells) {
  const int64_t m = model_base(cells);
  P.massFlux += m, P.velocityFlux += 2 * m;
  if constexpr (ALB) {
    if (P.albedoFlux) P.albedoFlux += 3 * m;
    if (P.albedoSource) P.albedoSource += 3 * m;
  }
  return P;
}
__device__ __forceinline__ DirectFields model_of(DirectFields F, int64_t cells) {
  const int64_t m = model_base(cells);
  F.layers += m, F.velocity += m;
  return F;
}

// direct: thread n = walker n of model blockIdx.y, of N_b = ps.walkers(N).  Params: UniformParam, or a batch's
// ModelParams (common.hpp), whose model's exitSlope and scale replace those F was made with
template <class Draws, bool ALB, class Params = UniformParam>
__global__ void __launch_bounds__(kPBlock)
    k_fluvial_direct(FluvialPlanes P, Draws draws, int64_t N, DirectFields F, Params ps) {
  const Param param = ps.model();
  if constexpr (Params::kPerModel) F.exitSlope = param.exitSlope, F.s = ps.scale(F.s);
  const int64_t n = static_cast<int64_t>(blockIdx.x) * kPBlock + threadIdx.x;
  const int64_t Nb = ps.walkers(N);
  if (n >= Nb) return;
  const float2 pos = draws.spawn(n, F.d);
  if (!owns_spawn(F.d, pos.x)) return;
  const int64_t cells = F.d.rows * F.d.W;
  trace_fluvial(model_of(F, cells), model_of<ALB>(P, cells), pos.x, pos.y, Nb, F.d, F.s, param);
}

template <class Draws, bool ALB, class Params = UniformParam>
__global__ void __launch_bounds__(kPBlock)
    k_debris_direct(DebrisPlanes P, Draws draws, int64_t N, DirectFields F, Params ps) {
  const Param param = ps.model();
  if constexpr (Params::kPerModel) F.exitSlope = param.exitSlope, F.s = ps.scale(F.s);
  const int64_t n = static_cast<int64_t>(blockIdx.x) * kPBlock + threadIdx.x;
  const int64_t Nb = ps.walkers(N);
  if (n >= Nb) return;
  const float2 pos = draws.spawn(n, F.d);
  if (!owns_spawn(F.d, pos.x)) return;
  const int64_t cells = F.d.rows * F.d.W;
  trace_debris(model_of(F, cells), model_of<ALB>(P, cells), pos.x, pos.y, Nb, F.d, F.s, param);
}

// The pack pass's exitSlope and scale: one for every model (the kernel arguments), or a batch's ModelParams
struct ExitSlope {
  float v;
};
__device__ __forceinline__ float exit_slope_of(const ExitSlope& e) { return e.v; }
__device__ __forceinline__ float exit_slope_of(const ModelParams& m) { return m.model().exitSlope; }
__device__ __forceinline__ Scale3 scale_of(const ExitSlope&, Scale3 s) { return s; }
__device__ __forceinline__ Scale3 scale_of(const ModelParams& m, Scale3 s) { return m.scale(s); }

// staged, pre-pass: p4[cell] = {__glocal(cell), velocity[cell]} for every row with a full stencil (`cells` of
// them per model from local row `row_lo`)
template <class Slope = ExitSlope>
__global__ void __launch_bounds__(kPBlock)
    k_pack_fields(float4* __restrict__ p4, const float2* __restrict__ layers,
                  const float2* __restrict__ velocity, Dom d, Scale3 s, Slope slope,
                  int64_t row_lo, int64_t cells) {
  const float exitSlope = exit_slope_of(slope);
  s = scale_of(slope, s);
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kPBlock + threadIdx.x;
  if (t >= cells) return;
  const int64_t m = model_base(d.rows * d.W);
  const int64_t lx = row_lo + t / d.W, y = t % d.W;
  const int64_t l = m + lx * d.W + y;
  const float2 g = glocal(layers + m, d, s, d.x0 + lx, y, exitSlope);
  const float2 v = velocity[l];
  p4[l] = make_float4(g.x, g.y, v.x, v.y);
}

__device__ __forceinline__ int64_t tile_of(const Dom& d, float px, float py, int64_t tiles_w) {
  const int64_t lx = cell_of(px) - d.x0, cy = cell_of(py);
  return (lx / kTile) * tiles_w + cy / kTile;
}

// pass 1: draw the spawn points (advancing every walker's stream) and count per tile; N walkers per model in
// the spawn array, of which model blockIdx.y draws draws.walkers(N)
template <class Draws>
__global__ void __launch_bounds__(kPBlock)
    k_spawn_count(float2* __restrict__ spawn, uint32_t* __restrict__ count, Draws draws, int64_t N, Dom d,
                  int64_t tiles_w, int64_t tiles) {
  const int64_t n = static_cast<int64_t>(blockIdx.x) * kPBlock + threadIdx.x;
  if (n >= draws.walkers(N)) return;
  const float2 pos = draws.spawn(n, d);
  spawn[model_base(N) + n] = pos;
  if (owns_spawn(d, pos.x)) atomicAdd(&count[model_base(tiles + 1) + tile_of(d, pos.x, pos.y, tiles_w)], 1u);
}

// pass 2: exclusive scan of the tile counts, start[tiles] = the number of owned walkers (one work-group per
// model: grid.x is the model here; tiles <= a few 1e5)
__global__ void __launch_bounds__(1024)
    k_tile_scan(uint32_t* start, const uint32_t* count, int64_t tiles) {
  const int64_t m = static_cast<int64_t>(blockIdx.x) * (tiles + 1);
  start += m, count += m;
  __shared__ uint32_t part[1024];
  const int tid = threadIdx.x;
  const int64_t chunk = (tiles + 1023) / 1024;
  const int64_t b = tid * chunk, e = (b + chunk < tiles) ? b + chunk : tiles;
  uint32_t sum = 0;
  for (int64_t i = b; i < e; ++i) sum += count[i];
  part[tid] = sum;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {  // Hillis-Steele inclusive scan
    const uint32_t v = (tid >= off) ? part[tid - off] : 0u;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  uint32_t run = part[tid] - sum;
  for (int64_t i = b; i < e; ++i) {
    start[i] = run;
    run += count[i];
  }
  if (tid == 1023) start[tiles] = part[1023];
}

// pass 3: drop every owned spawn point into its tile's range
__global__ void __launch_bounds__(kPBlock)
    k_spawn_scatter(float2* __restrict__ sorted, uint32_t* __restrict__ fill,
                    const uint32_t* __restrict__ start, const float2* __restrict__ spawn,
                    int64_t N, Dom d, int64_t tiles_w, int64_t tiles) {
  const int64_t n = static_cast<int64_t>(blockIdx.x) * kPBlock + threadIdx.x;
  if (n >= N) return;
  const float2 pos = spawn[model_base(N) + n];
  if (!owns_spawn(d, pos.x)) return;
  const int64_t tile = model_base(tiles + 1) + tile_of(d, pos.x, pos.y, tiles_w);
  sorted[model_base(N) + start[tile] + atomicAdd(&fill[tile], 1u)] = pos;
}
// the same for a batch of different models: of the N walkers per model, model blockIdx.y drew its record's N_b
__global__ void __launch_bounds__(kPBlock)
    k_spawn_scatter_models(float2* __restrict__ sorted, uint32_t* __restrict__ fill,
                           const uint32_t* __restrict__ start, const float2* __restrict__ spawn,
                           int64_t N, Dom d, int64_t tiles_w, int64_t tiles, ModelParams ps) {
  const int64_t n = static_cast<int64_t>(blockIdx.x) * kPBlock + threadIdx.x;
  if (n >= ps.walkers(N)) return;
  const float2 pos = spawn[model_base(N) + n];
  if (!owns_spawn(d, pos.x)) return;
  const int64_t tile = model_base(tiles + 1) + tile_of(d, pos.x, pos.y, tiles_w);
  sorted[model_base(N) + start[tile] + atomicAdd(&fill[tile], 1u)] = pos;
}

// work-group -> slot in the sorted order: block b runs on XCD b % 8; give every
// XCD one contiguous eighth of the tile sequence
__device__ __forceinline__ int64_t sorted_slot(const uint32_t* __restrict__ total_ptr) {
  const int64_t total = *total_ptr;
  const int64_t nb = (total + kPBlock - 1) / kPBlock;
  const int64_t per = (nb + 7) / 8;
  const int64_t b = blockIdx.x;
  const int64_t slot = b / 8;
  if (slot >= per) return -1;
  const int64_t blk = (b % 8) * per + slot;
  const int64_t t = blk * kPBlock + threadIdx.x;
  return (blk < nb && t < total) ? t : -1;
}

// pass 4: trace the owned walkers in tile order
template <bool ALB, class Params = UniformParam>
__global__ void __launch_bounds__(kPBlock)
    k_fluvial_sorted(FluvialPlanes P, const float2* __restrict__ sorted, const uint32_t* __restrict__ start,
                     int64_t tiles, int64_t N, PackedFields F, Dom d, Scale3 s, Params ps) {
  const Param param = ps.model();
  const int64_t t = sorted_slot(start + model_base(tiles + 1) + tiles);
  if (t < 0) return;
  const int64_t cells = d.rows * d.W;
  const float2 pos = sorted[model_base(N) + t];
  trace_fluvial(PackedFields{F.p4 + model_base(cells)}, model_of<ALB>(P, cells), pos.x, pos.y, ps.walkers(N), d,
                ps.scale(s), param);
}

template <bool ALB, class Params = UniformParam>
__global__ void __launch_bounds__(kPBlock)
    k_debris_sorted(DebrisPlanes P, const float2* __restrict__ sorted, const uint32_t* __restrict__ start,
                    int64_t tiles, int64_t N, PackedFields F, Dom d, Scale3 s, Params ps) {
  const Param param = ps.model();
  const int64_t t = sorted_slot(start + model_base(tiles + 1) + tiles);
  if (t < 0) return;
  const int64_t cells = d.rows * d.W;
  const float2 pos = sorted[model_base(N) + t];
  trace_debris(PackedFields{F.p4 + model_base(cells)}, model_of<ALB>(P, cells), pos.x, pos.y, ps.walkers(N), d,
               ps.scale(s), param);
}

static Scale3 s3p(const float* s) { return Scale3{s[0], s[1], s[2]}; }

static bool use_staged(int64_t N) {
  if (g_particle_mode == 1) return false;
  if (g_particle_mode == 2) return true;
  return N >= 1024;
}
// the tiled shape keeps the last cell index in 32 bits (and the slot indices of its
// queues): grids and launches beyond 2^31 stay on the staged shape
static bool use_tiled(int64_t N, const Dom& d) {
  if (d.H * d.W > 0x7fffffffll || N > 0x7fffffffll) return false;
  if (d.H >= (1 << 24) || d.W >= (1 << 24)) return false;  // its cell index is a 24-bit multiply-add
  if (g_particle_mode == 3) return true;
  // measured crossover against the staged shape: 512^2 (N = 32768) 2.15 vs 2.69 ms per step,
  // 640^2 (N = 51200) 2.90 vs 2.76
  return g_particle_mode == 0 && N >= 45000;
}

bool use_tiled_launch(int64_t N, const Dom& d) { return use_tiled(N, d); }

// The slab launches on explicit streams (particles_common.hpp, Streams): the tiled shape takes uniform
// streams as they are; the small-N shapes read a tensor, which is seeded here when the streams are
// uniform (the caller hands one over for that).
static int materialise(const Streams& st, int64_t N, hipStream_t s) {
  if (!st.uniform) return SOIL_OK;
  if (!st.rng) return fail(SOIL_ERR_INVALID_ARGUMENT, "uniform streams on a small launch need a tensor to seed");
  return soil_rng_seed(st.rng, N, st.seed, st.offset, s);
}

int check_batch(int64_t B, int64_t H, int64_t W, int64_t N, const uint64_t* seeds, const char* what) {
  const std::string w(what);
  SOIL_REQUIRE(B >= 1, w + ": a batch needs at least one model (B >= 1)");
  SOIL_REQUIRE(H >= 1 && W >= 1, w + ": empty grid (H and W must be >= 1)");
  SOIL_REQUIRE(N >= 0, w + ": negative particle count");
  SOIL_REQUIRE(N == 0 || seeds, w + ": null seeds with N > 0");
  // the largest arrays of a batch: B x H x W float4 (the staged shape's packed fields), B x N float2 twice;
  // per-model spawn counts are 32-bit
  int64_t cells = 0, t = 0;
  const bool overflow = __builtin_mul_overflow(H, W, &cells) || __builtin_mul_overflow(cells, B, &t) ||
                        __builtin_mul_overflow(t, int64_t{16}, &t) || __builtin_mul_overflow(N, B, &t) ||
                        __builtin_mul_overflow(t, int64_t{16}, &t) || N > 0x7fffffffll;
  SOIL_REQUIRE(!overflow, w + ": B, H, W, N too large (byte offsets overflow)");
  return SOIL_OK;
}

int clear_flux(const soil_erosion_planes* P, const soil_colour_planes* C, int kind, int64_t cells, hipStream_t st) {
  const size_t b = sizeof(float) * static_cast<size_t>(cells);
  std::pair<float*, size_t> planes[7] = {};  // (plane, floats per cell)
  if (P)
    planes[0] = {P->waterFlux, 1}, planes[1] = {P->massFlux, 1}, planes[2] = {P->velocityFlux, 2},
    planes[3] = {P->debrisFlux, 1}, planes[4] = {P->debrisVelocityFlux, 2};
  if (C && kind != DEBRIS) planes[5] = {C->albedo_fluvial, 3};
  if (C && kind != FLUVIAL) planes[6] = {C->albedo_debris, 3};
  for (const auto& [plane, n] : planes)
    if (n) SOIL_HIP(hipMemsetAsync(plane, 0, n * b, st));
  return SOIL_OK;
}

// The staged shape's scratch for B models in the workspace's `slot` (valid until the slot's next use), behind
// `lead` bytes the caller keeps for itself (a batch's device seeds).  Not staged: the lead alone.
struct Scratch {
  void* lead;
  float4* p4;
  float2 *spawn, *sorted;
  uint32_t *count, *fill, *start;  // three blocks of equal size, count and fill adjacent
  int64_t tiles_w, tiles;
};

static int scratch_get(WorkspaceSlot slot, size_t lead, int64_t B, int64_t N, const Dom& d, bool staged, Scratch* w) {
  w->tiles_w = (d.W + kTile - 1) / kTile;
  w->tiles = w->tiles_w * ((d.rows + kTile - 1) / kTile);
  auto align = [](size_t b) { return (b + 255) & ~static_cast<size_t>(255); };
  const size_t b_lead = align(lead);
  const size_t b_p4 = staged ? align(sizeof(float4) * static_cast<size_t>(B * d.rows * d.W)) : 0;
  const size_t b_pos = staged ? align(sizeof(float2) * static_cast<size_t>(B * N)) : 0;
  const size_t b_cnt = staged ? align(sizeof(uint32_t) * static_cast<size_t>(B * (w->tiles + 1))) : 0;
  void* base = nullptr;
  if (int rc = workspace_get(slot, b_lead + b_p4 + 2 * b_pos + 3 * b_cnt, &base); rc != SOIL_OK) return rc;
  char* c = static_cast<char*>(base);
  w->lead = c;                                   c += b_lead;
  w->p4 = reinterpret_cast<float4*>(c);          c += b_p4;
  w->spawn = reinterpret_cast<float2*>(c);       c += b_pos;
  w->sorted = reinterpret_cast<float2*>(c);      c += b_pos;
  w->count = reinterpret_cast<uint32_t*>(c);     c += b_cnt;
  w->fill = reinterpret_cast<uint32_t*>(c);      c += b_cnt;
  w->start = reinterpret_cast<uint32_t*>(c);
  return SOIL_OK;
}

// One launch of the small-N shapes: B models of domain d side by side (model b's planes b * rows * W cells on),
// N walkers each.  `albedoFlux` / `albedoSource`: the kind's colour flux plane and the spawn colours, or null.
// `s`, `p`: every model's scale and param; a batch of different models takes them, and each model's N_b <= N,
// from the ModelParams handed to launch_small instead.
struct SmallLaunch {
  const soil_erosion_planes* P;
  float* albedoFlux;
  const float* albedoSource;
  float* remote0;
  float* remoteA;
  int64_t B, N;
  Dom d;
  Scale3 s;
  Param p;
  hipStream_t st;
};

// the pack pass's exitSlope source for a launch's parameter source
static ExitSlope pack_slope(const UniformParam& u) { return ExitSlope{u.p.exitSlope}; }
static ModelParams pack_slope(const ModelParams& m) { return m; }

// The direct shape (`w` null) or the staged shape in `w`, at most kMaxGridY models per launch (every pointer
// advanced past the models launched before).  ALB: a coloured batch (model_of).  Params: UniformParam{L.p}, or
// a batch's ModelParams: the launch is sized by L.N = max N_b, and nothing else about it depends on the records
// (per-model maxage is a walker's bound, N_b a lane's).
template <bool ALB, class Draws, class Params = UniformParam>
static int launch_small(int kind, const SmallLaunch& L, Draws draws, const Scratch* w, Params params = {}) {
  if constexpr (!Params::kPerModel) params = UniformParam{L.p};
  const int64_t N = L.N, cells = L.d.rows * L.d.W;
  unsigned long long* steps = nullptr;
  if (int rc = step_counter(&steps); rc != SOIL_OK) return rc;
  const soil_erosion_planes& Q = *L.P;
  const bool fluvial = kind == FLUVIAL;
  const int64_t cnt = w ? w->tiles + 1 : 0;
  if (w) SOIL_HIP(hipMemsetAsync(w->count, 0, 2 * sizeof(uint32_t) * (w->fill - w->count), L.st));  // count, fill
  // the packed rows: every row whose stencil the slab holds
  const int64_t lo = stencil_lo(L.d), packed = (stencil_hi(L.d) - lo + 1) * L.d.W;
  for (int64_t b0 = 0; b0 < L.B; b0 += kMaxGridY) {
    const unsigned nb = static_cast<unsigned>(L.B - b0 < kMaxGridY ? L.B - b0 : kMaxGridY);
    const int64_t m = b0 * cells;
    const Draws dr = draws.from_model(b0);
    const Params ps = params.from_model(b0);
    const float2* layers = reinterpret_cast<const float2*>(Q.layers) + m;
    const float2* velocity = reinterpret_cast<const float2*>(fluvial ? Q.velocity : Q.debrisVelocity) + m;
    float* const albedoFlux = L.albedoFlux ? L.albedoFlux + 3 * m : nullptr;
    const float* const albedoSource = L.albedoSource ? L.albedoSource + 3 * m : nullptr;
    const FluvialPlanes PF{Q.waterFlux + m, Q.massFlux + m, Q.velocityFlux + 2 * m, albedoFlux, Q.rainfall + m,
                           Q.waterHeight + m, albedoSource, L.remote0, steps, L.remoteA};
    const DebrisPlanes PD{Q.debrisFlux + m, Q.debrisVelocityFlux + 2 * m, albedoFlux, albedoSource, L.remote0,
                          steps, L.remoteA};
    const dim3 walkers(blocks_for(N, kPBlock), nb);
    if (!w) {
      const DirectFields F{layers, velocity, L.d, L.s, L.p.exitSlope};  // (a sweep's kernels take the model's)
      if (fluvial)
        k_fluvial_direct<Draws, ALB, Params><<<walkers, kPBlock, 0, L.st>>>(PF, dr, N, F, ps);
      else
        k_debris_direct<Draws, ALB, Params><<<walkers, kPBlock, 0, L.st>>>(PD, dr, N, F, ps);
      SOIL_LAUNCH_CHECK();
      continue;
    }
    float4* p4 = w->p4 + m;
    float2 *spawn = w->spawn + b0 * N, *sorted = w->sorted + b0 * N;
    uint32_t *count = w->count + b0 * cnt, *fill = w->fill + b0 * cnt, *start = w->start + b0 * cnt;
    if (packed > 0)
      k_pack_fields<<<dim3(blocks_for(packed, kPBlock), nb), kPBlock, 0, L.st>>>(p4, layers, velocity, L.d, L.s,
                                                                                  pack_slope(ps), lo, packed);
    k_spawn_count<<<walkers, kPBlock, 0, L.st>>>(spawn, count, dr, N, L.d, w->tiles_w, w->tiles);
    k_tile_scan<<<nb, 1024, 0, L.st>>>(start, count, w->tiles);
    if constexpr (Params::kPerModel)
      k_spawn_scatter_models<<<walkers, kPBlock, 0, L.st>>>(sorted, fill, start, spawn, N, L.d, w->tiles_w,
                                                            w->tiles, ps);
    else
      k_spawn_scatter<<<walkers, kPBlock, 0, L.st>>>(sorted, fill, start, spawn, N, L.d, w->tiles_w, w->tiles);
    const dim3 traced(blocks_for(N, kPBlock) + 8, nb);
    if (fluvial)
      k_fluvial_sorted<ALB, Params><<<traced, kPBlock, 0, L.st>>>(PF, sorted, start, w->tiles, N,
                                                                  PackedFields{p4}, L.d, L.s, ps);
    else
      k_debris_sorted<ALB, Params><<<traced, kPBlock, 0, L.st>>>(PD, sorted, start, w->tiles, N,
                                                                 PackedFields{p4}, L.d, L.s, ps);
    SOIL_LAUNCH_CHECK();
  }
  return SOIL_OK;
}

// the colour flux plane of `kind` a launch adds to, or null (physics only)
static float* colour_flux(const Launch& L, int kind) {
  return L.C ? (kind == FLUVIAL ? L.C->albedo_fluvial : L.C->albedo_debris) : nullptr;
}

// One launch of a single model: the tiled shape, or the small-N shapes on the kind's tensor (workspace slot
// WS_SMALL_LAUNCH)
static int particles_single(int kind, const Launch& L) {
  const int64_t N = L.N;
  if (N <= 0) return SOIL_OK;
  if (use_tiled(N, L.d)) return launch_pass_tiled(kind, L);
  const Streams& streams = kind == FLUVIAL ? L.fluvial : L.debris;
  if (int rc = materialise(streams, N, L.st); rc != SOIL_OK) return rc;
  Scratch w{};
  const bool staged = use_staged(N);
  if (staged)
    if (int rc = scratch_get(WS_SMALL_LAUNCH, 0, 1, N, L.d, true, &w); rc != SOIL_OK) return rc;
  float* const albedoFlux = colour_flux(L, kind);
  const SmallLaunch S{L.P, albedoFlux, albedoFlux ? L.C->albedo_surface : nullptr, L.remote0,
                      albedoFlux ? L.remote_colour : nullptr, 1, N, L.d, L.s, L.p, L.st};
  return launch_small<false>(kind, S, TensorDraws{streams.rng}, staged ? &w : nullptr);
}

int particles_fluvial(const Launch& L) { return particles_single(FLUVIAL, L); }

// (with colour planes every walker is walked to the end: retirement makes no difference to the planes, and only
// the overlapped pair retires with colour)
int particles_debris(const Launch& L) { return particles_single(DEBRIS, L); }

// The seeds of a batch (or the records of a batch of different models) reach the device through a pinned buffer
// of the host thread (the caller's arrays may go as soon as the call returns): before it is written again, the
// copy queued from it the call before has been made — which lets the host queue one batch ahead of the device, and
// not further.
namespace {
struct SeedStaging {
  void* host = nullptr;
  size_t bytes = 0;
  hipEvent_t copied = nullptr;
  void release() {  // a thread's buffer goes with it (ThreadOwned, common.hpp)
    if (copied) (void)hipEventSynchronize(copied);
    owned_event_destroy(copied);
    (void)owned_pinned_free(host);
    host = nullptr, bytes = 0;
  }
};
}  // namespace

// One host-to-device copy: the host arrays of `parts` (pointer, bytes; null: left out) one after the other at dst.
static int upload_seeds(void* dst, std::initializer_list<std::pair<const void*, size_t>> parts, hipStream_t st) {
  static thread_local ThreadOwned<SeedStaging> staging;  // device -> staging
  int dev = 0;
  SOIL_HIP(hipGetDevice(&dev));
  SeedStaging& u = staging[dev];
  size_t bytes = 0;
  for (const auto& [src, n] : parts) bytes += src ? n : 0;
  if (u.copied) SOIL_HIP(hipEventSynchronize(u.copied));
  else SOIL_HIP(owned_event_create(&u.copied));
  if (u.bytes < bytes) {
    void* const old = u.host;
    u.host = nullptr;
    u.bytes = 0;
    SOIL_HIP(owned_pinned_free(old));
    SOIL_HIP(owned_pinned_alloc(&u.host, bytes, hipHostMallocDefault));
    u.bytes = bytes;
  }
  size_t at = 0;
  for (const auto& [src, n] : parts)
    if (src) std::memcpy(static_cast<char*>(u.host) + at, src, n), at += n;
  SOIL_HIP(hipMemcpyAsync(dst, u.host, bytes, hipMemcpyHostToDevice, st));
  SOIL_HIP(hipEventRecord(u.copied, st));
  return SOIL_OK;
}

int batch_upload(void* dst, const void* src, size_t bytes, hipStream_t st) {
  return upload_seeds(dst, {{src, bytes}}, st);
}

static_assert(sizeof(soil_batch_model) == 152 && alignof(soil_batch_model) == 8, "soil_batch_model: 152 bytes");
static_assert(offsetof(soil_batch_model, param) == 0 && offsetof(soil_batch_model, scale) == 112 &&
                  offsetof(soil_batch_model, N) == 128 && offsetof(soil_batch_model, seed) == 136 &&
                  offsetof(soil_batch_model, step_index) == 144,
              "soil_batch_model: field offsets as soil_hip.h");

// A batch's records on the device without walkers (the cell phase alone, or a step with every N_b == 0):
// workspace slot WS_BATCH.
int batch_models_to_device(const soil_batch_model* models, int64_t B, hipStream_t st,
                           const soil_batch_model** models_dev) {
  const size_t bytes = sizeof(soil_batch_model) * static_cast<size_t>(B);
  void* base = nullptr;
  if (int rc = workspace_get(WS_BATCH, bytes, &base); rc != SOIL_OK) return rc;
  if (int rc = upload_seeds(base, {{models, bytes}}, st); rc != SOIL_OK) return rc;
  *models_dev = static_cast<const soil_batch_model*>(base);
  return SOIL_OK;
}

// soil_particles_batch (soil_hip.h): walker n of model b draws from (seeds[b], n, offset), the state soil_erode_step
// seeds into its tensor for that model alone.  What a lane deposits stays in its model, a NaN walker's (0, 0)
// included.  Workspace slot WS_BATCH: the device seeds, then the staged scratch of all B models.  A batch of
// different models (c.models, soil_particles_batch_models): the slot starts with the B records in place of the
// seeds, in one copy.
int particles_batch(const BatchCall& c, const soil_batch_model** records_dev) {
  const soil_colour_planes* const C = c.C;
  const int64_t B = c.B, N = c.N;
  // the colour flux planes of all B models (consecutive): one memset each, also when N == 0, as the single
  // coloured pair does
  if (C)
    if (int rc = clear_flux(nullptr, C, BOTH_KINDS, B * c.H * c.W, c.st); rc != SOIL_OK) return rc;
  if (N == 0)
    return c.models && records_dev ? batch_models_to_device(c.models, B, c.st, records_dev) : SOIL_OK;
  const bool staged = use_staged(N);  // the single model's rule; what would be tiled alone runs staged
  const Dom d = full_domain(c.H, c.W);
  Scratch w{};
  // (152-byte records, 8-byte seeds: the scratch behind them is 256-aligned either way)
  const size_t lead = (c.models ? sizeof(soil_batch_model) : sizeof(uint64_t)) * static_cast<size_t>(B);
  if (int rc = scratch_get(WS_BATCH, lead, B, N, d, staged, &w); rc != SOIL_OK) return rc;
  if (int rc = upload_seeds(w.lead, {{c.models ? static_cast<const void*>(c.models) : c.seeds, lead}}, c.st);
      rc != SOIL_OK)
    return rc;
  const ModelParams records{static_cast<const soil_batch_model*>(w.lead)};
  if (c.models && records_dev) *records_dev = records.models;
  const uint64_t offset = c.step_index * static_cast<uint64_t>(N);
  for (int kind : {FLUVIAL, DEBRIS}) {
    // with colour: the kind's colour flux plane and the spawn colours (albedo_surface, also in the staged
    // shape: the packed fields hold none); a batch of different models: scale and param from the records
    const SmallLaunch S{c.P, C ? (kind == FLUVIAL ? C->albedo_fluvial : C->albedo_debris) : nullptr,
                        C ? C->albedo_surface : nullptr, nullptr, nullptr, B, N, d,
                        c.models ? Scale3{} : s3p(c.scale), c.models ? Param{} : *c.param, c.st};
    const uint64_t debris = kind == FLUVIAL ? 0 : 2;  // the debris launch: two draws on
    const Scratch* const ws = staged ? &w : nullptr;
    int rc;
    if (c.models) {
      const ModelDraws draws{records, debris};
      rc = C ? launch_small<true>(kind, S, draws, ws, records) : launch_small<false>(kind, S, draws, ws, records);
    } else {
      const SeedDraws draws{static_cast<const uint64_t*>(w.lead), offset + debris};
      rc = C ? launch_small<true>(kind, S, draws, ws) : launch_small<false>(kind, S, draws, ws);
    }
    if (rc != SOIL_OK) return rc;
  }
  return SOIL_OK;
}

int particles_pair(const Launch& L) {
  if (L.N > 0 && use_tiled(L.N, L.d)) return launch_pair_tiled(L);  // (clears the colour flux planes itself)
  // the small-N shapes: one launch after the other, every walker walked to the end; a launch that cannot store
  // its first round clears the planes it adds to
  if (int rc = clear_flux(L.overwrite ? L.P : nullptr, L.C, BOTH_KINDS, L.d.rows * L.d.W, L.st); rc != SOIL_OK)
    return rc;
  if (int rc = particles_fluvial(L); rc != SOIL_OK) return rc;
  return particles_debris(L);
}

}  // namespace soil

using namespace soil;

extern "C" {

int soil_set_particle_mode(int mode) {
  SOIL_REQUIRE(mode >= 0 && mode <= 3, "particle mode: 0 auto, 1 direct, 2 staged, 3 tiled");
  g_particle_mode = mode;
  return SOIL_OK;
}

int soil_set_particle_arith(int mode) {
  SOIL_REQUIRE(mode == 0 || mode == 1, "particle arithmetic: 0 exact, 1 fast");
  g_particle_arith = mode;
  return SOIL_OK;
}
int soil_get_particle_arith(void) { return g_particle_arith; }

int soil_set_debris_retire(int mode) {
  SOIL_REQUIRE(mode >= 0 && mode <= 2, "debris retirement: 0 off, 1 on, 2 watched");
  g_debris_retire = mode;
  return SOIL_OK;
}
int soil_get_debris_retire(void) { return g_debris_retire; }

int64_t soil_ghost_rows(const soil_param* param) {
  const double travel = 1.41421356237309515 * static_cast<double>(param ? param->maxage : 512);
  return static_cast<int64_t>(std::ceil(travel)) + 2;
}

int soil_transport_fluvial(const float* layers, const float* rainfall, float* waterHeight,
                           float* waterFlux, float* mass, float* massFlux, float* velocity,
                           float* velocityFlux, const float* albedo_bedrock, float* albedoFlux,
                           const float* albedoSource, soil_rng* rng, int64_t N, int64_t H,
                           int64_t W, const float scale[3], const soil_param* param,
                           void* stream) {
  (void)albedo_bedrock;  // accepted and unused, erosion.cu:198
  SOIL_DEVICE();
  SOIL_REQUIRE(layers && rainfall && waterHeight && waterFlux && mass && massFlux && velocity &&
                   velocityFlux && scale && param,
               "transport_fluvial: null tensor");
  SOIL_REQUIRE((albedoFlux == nullptr) == (albedoSource == nullptr),
               "transport_fluvial: pass both albedoFlux and albedoSource or neither");
  SOIL_REQUIRE(H > 0 && W > 0 && N >= 0 && (N == 0 || rng), "transport_fluvial: bad sizes");
  const Dom d = full_domain(H, W);
  const Scale3 s = s3p(scale);
  const soil_domain dom{H, W, 0, H, 0, H};
  int rc = soil_particles_fluvial_slab(waterFlux, massFlux, velocityFlux, albedoFlux, rng, N, layers, rainfall,
                                       waterHeight, velocity, albedoSource, nullptr, &dom, scale, param,
                                       stream);  // erosion.cu:209
  if (rc != SOIL_OK) return rc;
  return launch_normalize_fluvial(waterFlux, massFlux, velocityFlux, albedoFlux, layers, rainfall,
                                  waterHeight, mass, velocity, albedoSource, d, s, *param,
                                  as_stream(stream));  // erosion.cu:224
}

int soil_transport_debris(const float* layers, float* velocity, float* velocityFlux, float* mass,
                          float* massFlux, const float* albedo_bedrock, float* albedoFlux,
                          const float* albedoSource, soil_rng* rng, int64_t N, int64_t H,
                          int64_t W, const float scale[3], const soil_param* param,
                          void* stream) {
  (void)albedo_bedrock;  // accepted and unused, erosion.cu:401
  SOIL_DEVICE();
  SOIL_REQUIRE(layers && velocity && velocityFlux && mass && massFlux && scale && param,
               "transport_debris: null tensor");
  SOIL_REQUIRE((albedoFlux == nullptr) == (albedoSource == nullptr),
               "transport_debris: pass both albedoFlux and albedoSource or neither");
  SOIL_REQUIRE(H > 0 && W > 0 && N >= 0 && (N == 0 || rng), "transport_debris: bad sizes");
  const Dom d = full_domain(H, W);
  const Scale3 s = s3p(scale);
  const soil_domain dom{H, W, 0, H, 0, H};
  int rc = soil_particles_debris_slab(massFlux, velocityFlux, albedoFlux, rng, N, layers, velocity, albedoSource,
                                      nullptr, &dom, scale, param, stream);  // :412
  if (rc != SOIL_OK) return rc;
  return launch_normalize_debris(massFlux, velocityFlux, albedoFlux, layers, mass, velocity,
                                 albedoSource, d, s, *param, as_stream(stream));  // :424
}

// The per-op slab launches: the colour planes they get hold the colour source (only read) and their kind's
// flux plane, which they add to without clearing it; no colour reaches remote0.
int soil_particles_fluvial_slab(float* waterFlux, float* massFlux, float* velocityFlux,
                                float* albedoFlux, soil_rng* rng, int64_t N, const float* layers,
                                const float* rainfall, const float* waterHeight,
                                const float* velocity, const float* albedoSource, float* remote0,
                                const soil_domain* dom, const float scale[3],
                                const soil_param* param, void* stream) {
  SOIL_DEVICE();
  SOIL_REQUIRE(waterFlux && massFlux && velocityFlux && layers && rainfall && waterHeight &&
                   velocity && dom && scale && param,
               "particles_fluvial_slab: null argument");
  SOIL_REQUIRE((albedoFlux == nullptr) == (albedoSource == nullptr),
               "particles_fluvial_slab: pass both albedo planes or neither");
  SOIL_REQUIRE(N >= 0 && (N == 0 || rng), "particles_fluvial_slab: bad particle count");
  const Dom d = to_dom(dom);
  int rc = check_domain(d);
  if (rc != SOIL_OK) return rc;
  soil_erosion_planes P{};
  P.layers = layers, P.rainfall = rainfall;
  P.waterHeight = const_cast<float*>(waterHeight), P.velocity = const_cast<float*>(velocity);
  P.waterFlux = waterFlux, P.massFlux = massFlux, P.velocityFlux = velocityFlux;
  soil_colour_planes C{};
  C.albedo_surface = const_cast<float*>(albedoSource), C.albedo_fluvial = albedoFlux;
  return particles_fluvial(Launch{.P = &P, .C = albedoFlux ? &C : nullptr, .fluvial = streams_of(rng), .N = N,
                                  .remote0 = remote0, .d = d, .s = s3p(scale), .p = *param, .st = as_stream(stream)});
}

int soil_particles_debris_slab(float* massFlux, float* velocityFlux, float* albedoFlux,
                               soil_rng* rng, int64_t N, const float* layers,
                               const float* velocity, const float* albedoSource, float* remote0,
                               const soil_domain* dom, const float scale[3],
                               const soil_param* param, void* stream) {
  SOIL_DEVICE();
  SOIL_REQUIRE(massFlux && velocityFlux && layers && velocity && dom && scale && param,
               "particles_debris_slab: null argument");
  SOIL_REQUIRE((albedoFlux == nullptr) == (albedoSource == nullptr),
               "particles_debris_slab: pass both albedo planes or neither");
  SOIL_REQUIRE(N >= 0 && (N == 0 || rng), "particles_debris_slab: bad particle count");
  const Dom d = to_dom(dom);
  int rc = check_domain(d);
  if (rc != SOIL_OK) return rc;
  soil_erosion_planes P{};
  P.layers = layers, P.debrisVelocity = const_cast<float*>(velocity);
  P.debrisFlux = massFlux, P.debrisVelocityFlux = velocityFlux;
  soil_colour_planes C{};
  C.albedo_surface = const_cast<float*>(albedoSource), C.albedo_debris = albedoFlux;
  return particles_debris(Launch{.P = &P, .C = albedoFlux ? &C : nullptr, .debris = streams_of(rng), .N = N,
                                 .remote0 = remote0, .d = d, .s = s3p(scale), .p = *param, .st = as_stream(stream)});
}

int soil_particles_pair_slab(const soil_erosion_planes* planes, soil_rng* rng_fluvial,
                             soil_rng* rng_debris, int64_t N, float* remote0,
                             const soil_domain* dom, const float scale[3], const soil_param* param,
                             void* stream) {
  return soil_particles_pair_slab_ex(planes, rng_fluvial, rng_debris, N, remote0, dom, scale, param, 0, stream);
}

int soil_particles_pair_slab_ex(const soil_erosion_planes* planes, soil_rng* rng_fluvial,
                                soil_rng* rng_debris, int64_t N, float* remote0,
                                const soil_domain* dom, const float scale[3], const soil_param* param,
                                int flags, void* stream) {
  SOIL_DEVICE();
  SOIL_REQUIRE(planes && dom && scale && param, "particles_pair_slab: null argument");
  SOIL_REQUIRE(has_planes(*planes, PARTICLE_PLANES), "particles_pair_slab: null plane");
  SOIL_REQUIRE(N >= 0 && (N == 0 || (rng_fluvial && rng_debris && rng_fluvial != rng_debris)),
               "particles_pair_slab: needs two distinct rng tensors");
  const Dom d = to_dom(dom);
  if (int rc = check_domain(d); rc != SOIL_OK) return rc;
  return particles_pair(Launch{.P = planes, .fluvial = streams_of(rng_fluvial), .debris = streams_of(rng_debris),
                               .N = N, .remote0 = remote0, .d = d, .s = s3p(scale), .p = *param,
                               .st = as_stream(stream), .overwrite = (flags & SOIL_FLUX_OVERWRITE) != 0});
}

int soil_particles_pair_colour(const soil_erosion_planes* planes, const soil_colour_planes* colour,
                               soil_rng* rng_fluvial, soil_rng* rng_debris, int64_t N, int64_t H, int64_t W,
                               const float scale[3], const soil_param* param, int flags, void* stream) {
  SOIL_DEVICE();
  SOIL_REQUIRE(planes && colour && scale && param, "particles_pair_colour: null argument");
  SOIL_REQUIRE(has_planes(*planes, PARTICLE_PLANES), "particles_pair_colour: null plane");
  SOIL_REQUIRE(has_colour(colour), "particles_pair_colour: every colour plane is required");
  SOIL_REQUIRE(H > 0 && W > 0, "particles_pair_colour: empty grid");
  SOIL_REQUIRE(N >= 0 && (N == 0 || (rng_fluvial && rng_debris && rng_fluvial != rng_debris)),
               "particles_pair_colour: needs two distinct rng tensors");
  return particles_pair(Launch{.P = planes, .C = colour, .fluvial = streams_of(rng_fluvial),
                               .debris = streams_of(rng_debris), .N = N, .d = full_domain(H, W), .s = s3p(scale),
                               .p = *param, .st = as_stream(stream),
                               .overwrite = (flags & SOIL_FLUX_OVERWRITE) != 0});
}

// `remote0` (may be null) is float[16]: [0..7] as the physics slab launches, [8..10] / [11..13] the fluvial /
// debris colour deposits of NaN walkers for global (0, 0) (Remote0::colour = remote0 + 8)
int soil_particles_pair_colour_slab(const soil_erosion_planes* planes, const soil_colour_planes* colour,
                                    soil_rng* rng_fluvial, soil_rng* rng_debris, int64_t N, float* remote0,
                                    const soil_domain* dom, const float scale[3], const soil_param* param, int flags,
                                    void* stream) {
  SOIL_DEVICE();
  SOIL_REQUIRE(planes && colour && dom && scale && param, "particles_pair_colour_slab: null argument");
  SOIL_REQUIRE(has_planes(*planes, PARTICLE_PLANES), "particles_pair_colour_slab: null plane");
  SOIL_REQUIRE(has_colour(colour, false),
               "particles_pair_colour_slab: albedo_surface, albedo_fluvial and albedo_debris are required");
  SOIL_REQUIRE(N >= 0 && (N == 0 || (rng_fluvial && rng_debris && rng_fluvial != rng_debris)),
               "particles_pair_colour_slab: needs two distinct rng tensors");
  const Dom d = to_dom(dom);
  if (int rc = check_domain(d); rc != SOIL_OK) return rc;
  return particles_pair(Launch{.P = planes, .C = colour, .fluvial = streams_of(rng_fluvial),
                               .debris = streams_of(rng_debris), .N = N, .remote0 = remote0,
                               .remote_colour = remote0 ? remote0 + 8 : nullptr, .d = d, .s = s3p(scale),
                               .p = *param, .st = as_stream(stream),
                               .overwrite = (flags & SOIL_FLUX_OVERWRITE) != 0});
}

int soil_particle_steps(uint64_t* total, int reset, void* stream) {
  SOIL_REQUIRE(total != nullptr, "soil_particle_steps: null output");
  unsigned long long* counter = nullptr;
  if (int rc = step_counter(&counter); rc != SOIL_OK) return rc;
  unsigned long long v = 0;
  hipStream_t st = as_stream(stream);
  SOIL_HIP(hipMemcpyAsync(&v, counter, sizeof(v), hipMemcpyDeviceToHost, st));
  if (reset) SOIL_HIP(hipMemsetAsync(counter, 0, sizeof(v), st));
  SOIL_HIP(hipStreamSynchronize(st));
  *total = v;
  return SOIL_OK;
}

}  // extern "C"
