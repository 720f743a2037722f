/*
 * soil_hip.h — C ABI of the MI355X-native grid-erosion hot path.
 *
 * Every entry point below replaces one free function of the reference's
 * `namespace soil` operator API (the functions the nanobind module
 * python/source/model.cpp binds).  The reference file:line each one stands in
 * for is cited next to the declaration.  Paths are relative to the reference
 * repository root:
 *
 *   erosion.hpp / erosion.cu / erosion_map.cu = source/soillib/model/path/...
 *   graph.hpp / graph.cu                      = source/soillib/model/graph/...
 *   grad.hpp / grad.cu                        = source/soillib/model/grad/...
 *   filter.hpp / filter.cu                    = source/soillib/model/filter/...
 *   path.hpp / path.cu / sample.hpp           = source/soillib/model/path/...
 *   normal.hpp / noise.hpp                    = source/soillib/op/...
 *   model.cpp                                 = python/source/model.cpp
 *
 * Conventions
 *  - Plain pointers and sizes only.  All tensor pointers are DEVICE pointers
 *    (HBM) to dense row-major fp32 / int32 arrays unless the name ends in
 *    `_host`.  A grid has shape (H, W): axis 0 (x, H rows) is the slow axis,
 *    axis 1 (y, W columns) is contiguous; a trailing channel axis is fastest
 *    ((H,W,2) "vec2" planes are float pairs, (H,W,3) "vec3" planes triples).
 *  - `scale` = {sx, sy, sz}: cell size along axis 0 / axis 1 and metres per
 *    height unit (erosion.cu:50-51).  2-component scales are {sx, sy}.
 *  - `stream` is a hipStream_t passed as void*; NULL = the null stream.  All
 *    functions are asynchronous on that stream unless stated otherwise.
 *  - Return value: 0 (SOIL_OK) or a negative soil_status; the message of the
 *    last failure on the calling thread is available from soil_last_error().
 *  - No entry point has a CPU fallback.  Without a usable HIP device every
 *    compute call returns SOIL_ERR_NO_DEVICE.
 */
#ifndef SOIL_HIP_H
#define SOIL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SOIL_HIP_ABI_VERSION 1

/* ------------------------------------------------------------------ status */

typedef enum soil_status {
  SOIL_OK = 0,
  SOIL_ERR_INVALID_ARGUMENT = -1, /* std::invalid_argument in the reference (graph.cu:88) */
  SOIL_ERR_NO_DEVICE = -2,        /* no HIP device / runtime failure at init            */
  SOIL_ERR_HIP = -3,              /* a HIP runtime call failed (message has the detail) */
  SOIL_ERR_OUT_OF_MEMORY = -4,
  SOIL_ERR_IO = -5, /* silt::error::missing_file / an unreadable or unsupported file (tiff.hpp:73) */
  SOIL_ERR_COMM = -6 /* the wire between ranks failed or timed out (soil_slab.h); no reference counterpart */
} soil_status;

/* graph.hpp:11-14  enum edge_t { D4 = 0, D8 = 1 } */
typedef enum soil_edge { SOIL_D4 = 0, SOIL_D8 = 1 } soil_edge;

/* ------------------------------------------------------------------- types */

/* erosion.hpp:17-58  soil::param_t — same fields, same order, same defaults
 * (see soil_param_default).  112 bytes, passed by const pointer, copied into
 * kernel arguments. */
typedef struct soil_param {
  uint64_t maxage;              /* erosion.hpp:20 */
  float lrate;                  /* :21 (read by no kernel) */
  float timeStep;               /* :22 */
  float exitSlope;              /* :25 */
  float uplift;                 /* :26 */
  float rainfall;               /* :27 */
  float gravity;                /* :28 */
  float evapRate;               /* :29 */
  float frictionFactor;         /* :32 */
  float fluvialExponent;        /* :33 */
  float suspensionRateFluvial;  /* :35 */
  float depositionRateFluvial;  /* :36 */
  float suspensionRateDebris;   /* :38 */
  float depositionRateDebris;   /* :39 */
  float landslideRateDebris;    /* :40 */
  float critSlopeBedrock;       /* :43 */
  float critSlopeSediment;      /* :44 */
  float yieldStress;            /* :45 */
  float viscosityWater;         /* :47 */
  float bedShearWater;          /* :48 */
  float densityWater;           /* :49 */
  float viscosityDebris;        /* :51 */
  float bedShearDebris;         /* :52 */
  float densityDebris;          /* :53 */
  float force[2];               /* :56 */
  float _pad;
} soil_param;

/* One element of a `silt::rng` tensor (erosion.hpp:6 uses curandState).
 * The reference's generator is cuRAND XORWOW, closed source and not
 * reproducible off NVIDIA hardware; this ABI fixes a counter-based generator
 * instead: Philox4x32-10 with key = seed, counter =
 * {offset, subsequence}, subsequence = element index — i.e. the same
 * (seed, subsequence = n, offset) addressing as curand_init(seed, n, offset)
 * at graph.cu:100.  One draw advances `offset` by one. */
typedef struct soil_rng {
  uint64_t seed;
  uint64_t offset;
} soil_rng;

/* A row slab of a global (H, W) grid held by one GPU.  Every tensor handed to
 * a *_slab entry point covers local rows [0, rows) == global rows
 * [x0, x0+rows); the kernel writes only local rows [r0, r1) and evaluates
 * boundary conditions (exitSlope, clamp-to-self) against the GLOBAL border.
 * Single-GPU calls use {H, W, 0, H, 0, H}. */
typedef struct soil_domain {
  int64_t H, W;   /* global grid shape                              */
  int64_t x0;     /* global row index of local row 0                */
  int64_t rows;   /* local rows held by every buffer (owned+ghost)  */
  int64_t r0, r1; /* local row range this call computes / owns      */
} soil_domain;

/* ---------------------------------------------------------------- runtime */

int soil_abi_version(void);
const char* soil_last_error(void);
/* Number of visible HIP devices (0 if none); never fails. */
int soil_device_count(void);
int soil_set_device(int device);
/* Writes the gcnArchName of the current device ("gfx950...") into buf. */
int soil_device_name(char* buf, size_t len);
void soil_param_default(soil_param* p);

/* silt tensor storage (un-vendored silt: tensor_t(shape, GPU) allocations,
 * .cpu()/.gpu() copies — call sites graph.cu:80, example/dem_multiflow.py:25). */
int soil_malloc(void** ptr, size_t bytes);
int soil_free(void* ptr);
int soil_memcpy_h2d(void* dst, const void* src_host, size_t bytes, void* stream);
int soil_memcpy_d2h(void* dst_host, const void* src, size_t bytes, void* stream);
int soil_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream);
int soil_stream_synchronize(void* stream);
int soil_device_synchronize(void);

/* HIP-event timing on the stream kernels are launched on (bench.py). */
int soil_event_create(void** event);
int soil_event_destroy(void* event);
int soil_event_record(void* event, void* stream);
int soil_event_elapsed_ms(void* start, void* stop, float* ms); /* synchronises on stop */

/* silt element-wise ops used by the scripts (silt.set/add/multiply/seed:
 * example/erosion_gpu.py:19, example/dem_process.py:46-47,81; graph.cu:552-553). */
int soil_set_f32(float* t, float value, int64_t n, void* stream);
int soil_set_i32(int32_t* t, int32_t value, int64_t n, void* stream);
int soil_add_f32(float* t, const float* other, int64_t n, void* stream);       /* t += other */
int soil_multiply_f32(float* t, float value, int64_t n, void* stream);         /* t *= value */
int soil_rng_seed(soil_rng* rng, int64_t n, uint64_t seed, uint64_t offset, void* stream);

/* Evaluates the library's numerical primitives on device arrays so that tests
 * can compare them with the oracle bit for bit:
 *   op 0: out[i] = expf_(a[i])        stand-in for __expf
 *   op 1: out[i] = log2f_(a[i])
 *   op 2: out[i] = powf_(a[i], b[i])  stand-in for __powf
 *   op 3: out[i] = uniform in (0,1] of stream (seed = bits of a[i],
 *                  subsequence = i, offset = bits of b[i])  — Philox4x32-10
 *   op 4: out[i] = a[i] * b[i] (plain product; exposes denormal flushing)
 *   op 5: out[i] = a[i] / b[i] (the compiler's IEEE division)
 *   op 6: out[i] = quot0(a[i], recip(b[i])), the shared-reciprocal quotient of the
 *                  particle step (soil_math.hpp); equals op 5 on plain operands
 *   op 7: out[i] = expf_flat(a[i]), the branch-free twin of op 0
 *   op 8: out[i] = att_exp(a[i]) = v_exp_f32(a[i] * log2e), the particle attenuations'
 *                  exponential (the reference's __expf, erosion.cu:134-136,346)
 *   op 9: bits of out[i] = floor_cell(a[i]): floor as int32, saturating, NaN -> INT_MAX
 *   op 10: out[i] = sqrt_rn(a[i]), the particle step's square root; equals op 11 (sqrtf) for
 *                  a[i] >= 2^-96, +0, +inf and NaN
 *   op 12: out[i] = rw_exp2(a[i], b[i]) = v_exp_f32(a[i] * b[i]), the product rounded to fp32 first: the
 *                  Gibbs weight of soil_random_weighted for a height difference a[i] and the host-made
 *                  constant b[i] = log2(e) / (|shift| T); the kernel calls the same inline function */
int soil_selftest_math(float* out, const float* a, const float* b, int64_t n, int op,
                       void* stream);

/* --------------------------------------------------- erosion: particle ops */

/* soil::transport_fluvial — erosion.hpp:69-84, erosion.cu:189-239
 * (= __transport_fluvial :29-141 + __normalize_fluvial :143-187), bound at
 * model.cpp:237-268.  Argument names follow erosion.cu:189-204.
 *   layers (H,W,2)  rainfall (H,W)  waterHeight (H,W) out  waterFlux (H,W) inout
 *   mass (H,W) out  massFlux (H,W) inout  velocity (H,W,2) inout
 *   velocityFlux (H,W,2) inout  albedoFlux (H,W,3) inout  albedoSource (H,W,3)
 *   rng [N] inout.
 * The flux planes are only ever added to (atomics) and must be zeroed by the
 * caller.  `albedo_bedrock` is accepted and unused, as in the reference.
 * albedoFlux/albedoSource may both be NULL: the colour channels are then
 * skipped (physics planes are unaffected). */
int soil_transport_fluvial(const float* layers, const float* rainfall, float* waterHeight,
                           float* waterFlux, float* mass, float* massFlux, float* velocity,
                           float* velocityFlux, const float* albedo_bedrock, float* albedoFlux,
                           const float* albedoSource, soil_rng* rng, int64_t N, int64_t H,
                           int64_t W, const float scale[3], const soil_param* param,
                           void* stream);

/* soil::transport_debris — erosion.hpp:86-98, erosion.cu:395-436
 * (= __transport_debris :245-351 + __normalize_debris :353-393), model.cpp:270-295. */
int soil_transport_debris(const float* layers, float* velocity, float* velocityFlux, float* mass,
                          float* massFlux, const float* albedo_bedrock, float* albedoFlux,
                          const float* albedoSource, soil_rng* rng, int64_t N, int64_t H,
                          int64_t W, const float scale[3], const soil_param* param,
                          void* stream);

/* ------------------------------------------------------- erosion: cell ops */

/* soil::mass_transfer — erosion.hpp:104-119, erosion.cu:576-611 (__transfer
 * :453-574), model.cpp:297-328.  delta (H,W,2) inout, layers (H,W,2),
 * uplift/waterHeight/mass/debris (H,W), velocityFluvial/momentumDebris
 * (H,W,2); waterHeight and momentumDebris are accepted and unread, as in the
 * reference.  The four albedo planes (H,W,3) may all be NULL (colour mixing
 * skipped). */
int soil_mass_transfer(float* delta, const float* layers, const float* uplift,
                       const float* waterHeight, const float* mass, const float* velocityFluvial,
                       const float* debris, const float* momentumDebris,
                       const float* albedo_bedrock, const float* albedoFluxFluvial,
                       const float* albedoFluxDebris, float* albedo_surface, int64_t H, int64_t W,
                       const float scale[3], const soil_param* param, void* stream);

/* soil::mass_creep — erosion.hpp:121-126, erosion.cu:712-727 (__mass_creep
 * :633-710), model.cpp:330-341. */
int soil_mass_creep(float* delta, const float* layers, int64_t H, int64_t W,
                    const float scale[3], const soil_param* param, void* stream);

/* soil::layer_merge — erosion.hpp:130-133, erosion.cu:747-757 (__layer_merge
 * :733-745), model.cpp:343-351.  n = H*W cells. */
int soil_layer_merge(float* height, const float* layers, int64_t n, void* stream);

/* Interleave / split the (n,2) layer plane and its two (n) component planes:
 * the legacy map_t kept `height` (bedrock) and `sediment` apart
 * (model.cpp:67-97, commented out) while the live kernels take `layers`
 * (layer_t = vec2, erosion.hpp:60).  `sediment` == NULL reads as zeros in
 * from_planes and is skipped in to_planes. */
int soil_layers_from_planes(float* layers, const float* bedrock, const float* sediment, int64_t n,
                            void* stream);
int soil_layers_to_planes(float* bedrock, float* sediment, const float* layers, int64_t n,
                          void* stream);

/* soil::albedo_stratum / albedo_layer / albedo_discharge — erosion.hpp:139-166,
 * erosion.cu:828-854 / :877-898 / :900-919, model.cpp:353-407. */
int soil_albedo_stratum(float* albedoBedrock, const float* uplift, const float* layers,
                        int64_t n, const float scale[3], const soil_param* param,
                        const float colorA[3], const float colorB[3], float age, float freq,
                        void* stream);
int soil_albedo_layer(float* albedo, const float* albedoBedrock, const float* albedoSediment,
                      const float* layers, int64_t n, float scaleSediment,
                      const float shiftSediment[3], void* stream);
int soil_albedo_discharge(float* albedo, const float* discharge, int64_t n,
                          const float colorDischarge[3], float extinction, float scale,
                          void* stream);

/* ---------------------------------------------- erosion: fused step (slab) */

/* The planes of one erosion model, for the fused step.  All device pointers.
 * `layers`/`layers_next` are the double buffer of the (rows,W,2) layer plane:
 * the step reads `layers`, writes `layers_next`; the caller swaps them. */
typedef struct soil_erosion_planes {
  const float* layers;      /* (rows,W,2) in   bedrock, sediment                         */
  float* layers_next;       /* (rows,W,2) out  layers + delta                            */
  float* height;            /* (rows,W)   out  layer_merge of layers_next (may be NULL)  */
  const float* uplift;      /* (rows,W)   in                                             */
  const float* rainfall;    /* (rows,W)   in   waterSource                               */
  float* waterHeight;       /* (rows,W)   out  "discharge"                               */
  float* waterFlux;         /* (rows,W)   in → re-zeroed  "discharge_track"              */
  float* mass;              /* (rows,W)   out  fluvial suspended mass                    */
  float* massFlux;          /* (rows,W)   in → re-zeroed                                 */
  float* velocity;          /* (rows,W,2) out  fluvial "momentum"                        */
  float* velocityFlux;      /* (rows,W,2) in → re-zeroed                                 */
  float* debris;            /* (rows,W)   out  debris mass                               */
  float* debrisFlux;        /* (rows,W)   in → re-zeroed                                 */
  float* debrisVelocity;    /* (rows,W,2) out                                            */
  float* debrisVelocityFlux;/* (rows,W,2) in → re-zeroed                                 */
} soil_erosion_planes;

/* Fused cell phase of one erosion step: for every owned cell, in one pass,
 *   __normalize_fluvial (erosion.cu:143-187) + __normalize_debris (:353-393)
 *   + [delta = 0] + __transfer (:453-574) + __mass_creep (:633-710)
 *   + layers_next = layers + delta (silt.add, example/dem_process.py:47)
 *   + __layer_merge (:733-745) + re-zero of the five flux planes,
 * bit-identical to running those reference steps one after another (same
 * operation order per cell).  Physics planes only (no albedo; the coloured step
 * has soil_erode_cells_fused_colour below).  This is the HBM-roofline kernel:
 * 112 algorithmic bytes per cell. */
int soil_erode_cells_fused(const soil_erosion_planes* planes, const soil_domain* dom,
                           const float scale[3], const soil_param* param, void* stream);
/* The same with flags.  SOIL_CELLS_KEEP_FLUX: the five flux planes are read and left as they are
 * (84 bytes per cell instead of 112); whoever adds to them next must overwrite them first —
 * SOIL_FLUX_OVERWRITE of the particle launches does. */
#define SOIL_CELLS_KEEP_FLUX 1
int soil_erode_cells_fused_ex(const soil_erosion_planes* planes, const soil_domain* dom,
                              const float scale[3], const soil_param* param, int flags, void* stream);

/* Particle halves of transport_fluvial / transport_debris alone (no
 * normalise), on a slab: __transport_fluvial erosion.cu:29-141,
 * __transport_debris :245-351.  Thread n draws its spawn position in the
 * GLOBAL (dom->H, dom->W) grid from rng[n]; only particles whose spawn row
 * lies in global rows [x0+r0, x0+r1) are traced, the rest only advance their
 * rng state, so N ranks that each own one slab trace every particle exactly
 * once.  A trajectory that leaves local rows [0, rows) through an interior
 * (non-global) slab edge is a caller error (size the ghost zone with
 * soil_ghost_rows).
 * `remote0` (device float[8], may be NULL) collects what the reference's "NaN
 * walkers"  deposit into GLOBAL cell (0,0) when
 * that cell is not held by this slab: [0..3] = water, mass, velocity.x/.y flux
 * (fluvial), [4..6] = mass, velocity.x/.y flux (debris).  The owner of global
 * row 0 adds the all-reduced sums to its cell (0,0). */
int soil_particles_fluvial_slab(float* waterFlux, float* massFlux, float* velocityFlux,
                                float* albedoFlux, soil_rng* rng, int64_t N,
                                const float* layers, const float* rainfall,
                                const float* waterHeight, const float* velocity,
                                const float* albedoSource, float* remote0,
                                const soil_domain* dom, const float scale[3],
                                const soil_param* param, void* stream);
int soil_particles_debris_slab(float* massFlux, float* velocityFlux, float* albedoFlux,
                               soil_rng* rng, int64_t N, const float* layers,
                               const float* velocity, const float* albedoSource, float* remote0,
                               const soil_domain* dom, const float scale[3],
                               const soil_param* param, void* stream);
/* Both particle launches of one step (the two calls above) issued together so that
 * they overlap: the debris launch fills the SIMD slots the fluvial launch leaves idle
 * in its sparse late rounds (two internal streams forked from and joined into
 * `stream`).  The reference runs them back to back on ONE rng tensor, each launch
 * consuming two draws per particle; give the debris launch its own tensor seeded two
 * draws further — soil_rng_seed(rng_debris, N, seed, offset + 2) — and every
 * trajectory is the same as in the sequential order.  Planes as in
 * soil_erode_cells_fused (the cell-phase outputs are not touched). */
int soil_particles_pair_slab(const soil_erosion_planes* planes, soil_rng* rng_fluvial,
                             soil_rng* rng_debris, int64_t N, float* remote0,
                             const soil_domain* dom, const float scale[3], const soil_param* param,
                             void* stream);
/* The same with flags.  SOIL_FLUX_OVERWRITE: the flux planes hold stale values on entry (the cell
 * phase ran with SOIL_CELLS_KEEP_FLUX) and hold exactly this call's deposits on return.  The tiled
 * launch shape gets there without a clearing pass: the first round of each launch, whose tiles
 * partition the plane, flushes its LDS accumulators with plain stores — zeros included — instead
 * of read-modify-writes; where that cannot be done (an empty tile, a tile shared by several
 * work-groups, the small-N launch shapes) the planes are cleared first. */
#define SOIL_FLUX_OVERWRITE 1
int soil_particles_pair_slab_ex(const soil_erosion_planes* planes, soil_rng* rng_fluvial,
                                soil_rng* rng_debris, int64_t N, float* remote0,
                                const soil_domain* dom, const float scale[3],
                                const soil_param* param, int flags, void* stream);
/* ------------------------------------------------ erosion: whole steps */

/* One whole erosion step on one device: re-seed the particle streams at
 * (seed, subsequence n, offset step_index * N) — the `silt.seed(rng, seed, step * N)` of
 * example/dem_process.py:81 —, both particle launches, the fused cell phase.  Planes as in
 * soil_erode_cells_fused, single-device shapes (H, W[, 2]); `rng` holds N elements.  Reads
 * planes->layers, writes planes->layers_next: the caller swaps the two handles afterwards.
 * The two particle launches are issued overlapped (as soil_particles_pair_slab does: two
 * internal streams forked from `stream` and joined back into it; the fluvial launch draws
 * from a scratch tensor of the library's workspace, the debris launch from `rng` seeded two
 * draws on), with the results and the final state of `rng` of the sequential order;
 * SOIL_STEP_PAIR=0 in the environment issues them one after the other on `stream`.  The host
 * returns once the step is queued; it does wait, between the rounds of a particle launch, for
 * the word that tells it how many work-groups the next round needs. */
int soil_erode_step(const soil_erosion_planes* planes, soil_rng* rng, int64_t N, uint64_t seed,
                    uint64_t step_index, int64_t H, int64_t W, const float scale[3],
                    const soil_param* param, void* stream);
/* A step inside a chain of steps.  The reference zeroes its track planes between steps
 * (example/dem_process.py: silt.set(track.*, 0)) — 28 bytes of stores per cell that nobody reads.
 * SOIL_STEP_FLUX_OUT_DIRTY: this step leaves the five flux planes holding its accumulated flux
 * (SOIL_CELLS_KEEP_FLUX); SOIL_STEP_FLUX_IN_DIRTY: the previous step did so, this step's particle
 * launches overwrite them (SOIL_FLUX_OVERWRITE).  flags == 0 is soil_erode_step. */
#define SOIL_STEP_FLUX_IN_DIRTY 1
#define SOIL_STEP_FLUX_OUT_DIRTY 2
int soil_erode_step_ex(const soil_erosion_planes* planes, soil_rng* rng, int64_t N, uint64_t seed,
                       uint64_t step_index, int64_t H, int64_t W, const float scale[3],
                       const soil_param* param, int flags, void* stream);

/* ------------------------------------------ erosion: batches of models */

/* A batch: B independent whole-grid models of one shape (H, W), N walkers each, one `param`, one `scale`, one
 * step_index, one seed per model (models that differ in param, scale, N or step index: soil_erode_step_batch_models).  Every pointer of `planes` is model 0 of B consecutive models: model b of a
 * plane of C channels starts at element b * H * W * C (rainfall and uplift too: they are per model).  `seeds`
 * is a host array of B values, copied before the call returns.  A batch leaves model b holding what the
 * single-model entry leaves on that model alone with seed = seeds[b] (soil_erode_step; the streams of model b
 * at (seeds[b], n, step_index * N), the debris launch two draws on): the same trajectories, a NaN walker's
 * deposits in cell (0, 0) of its own model, nothing of one model in another, particle steps added to
 * soil_particle_steps' counter; the fp32 sums of a flux cell may be added up in another order.  The
 * particles are launched in the single model's direct or staged shape (soil_set_particle_mode: staged for
 * N >= 1024, direct below; an N that gets the tiled shape alone runs staged), exact arithmetic, every walker
 * walked to the end; each launch covers all B models (grid.y = model, at most 65535 per launch), one after
 * the other on `stream`.  SOIL_ERR_INVALID_ARGUMENT for B < 1, H or W < 1, N < 0, null seeds with N > 0, a
 * size whose byte offsets overflow (or N >= 2^31).
 *
 * One erosion step of every model: soil_particles_batch, then soil_erode_cells_fused_batch with flags 0.
 * The flux planes are zero on entry and on exit; reads `layers`, writes `layers_next` (the caller swaps).
 * Algorithmic bytes: the particle launches' (per walker step one 16-byte packed-field gather and, fluvial,
 * 4 bytes of waterHeight, plus 16 / 12 bytes of flux atomics per cell entered; the staged shape's pack pass
 * 28 bytes per cell and kind) and 112 bytes per cell of the cell phase. */
int soil_erode_step_batch(const soil_erosion_planes* planes, int64_t B, int64_t H, int64_t W, int64_t N,
                          const uint64_t* seeds, uint64_t step_index, const float scale[3],
                          const soil_param* param, void* stream);
/* Both particle launches of a batch step (fluvial, then debris), adding into the five flux planes of every
 * model as soil_particles_pair_slab adds into one model's; reads layers, rainfall, waterHeight, velocity and
 * debrisVelocity; the cell phase's output planes are not touched.  N == 0 launches nothing. */
int soil_particles_batch(const soil_erosion_planes* planes, int64_t B, int64_t H, int64_t W, int64_t N,
                         const uint64_t* seeds, uint64_t step_index, const float scale[3],
                         const soil_param* param, void* stream);
/* The fused cell phase of every model of a batch, bit-identical per model to soil_erode_cells_fused_ex on that
 * model's planes with the same flags (whole grid; every model has the grid's edges, no neighbour read crosses
 * into another model).  One launch per 65535 models.  112 algorithmic bytes per cell, 84 with
 * SOIL_CELLS_KEEP_FLUX. */
int soil_erode_cells_fused_batch(const soil_erosion_planes* planes, int64_t B, int64_t H, int64_t W,
                                 const float scale[3], const soil_param* param, int flags, void* stream);

/* ------------------------------------------ erosion: the coloured step */

/* The colour planes of one erosion model: (rows,W,3) float32, a vec3 per cell (AoS), the
 * albedo arguments the reference's live binding passes through erosion (model.cpp:237-328).
 * The reference has no composite step with colour; this build defines one:
 * the step of soil_erode_step with those arguments filled in —
 *   1. seed(rng, seed, step * N)
 *   2. albedo_fluvial = albedo_debris = 0
 *   3. transport_fluvial(..., albedo_bedrock, albedo_fluvial, albedo_surface, ...)
 *   4. transport_debris(..., albedo_bedrock, albedo_debris, albedo_surface, ...)
 *   5. delta = 0
 *   6. mass_transfer(..., albedo_bedrock, albedo_fluvial, albedo_debris, albedo_surface, ...)
 *   7. mass_creep   8. layers += delta   9. layer_merge
 *  10. the physics flux planes zeroed (or left dirty: SOIL_STEP_FLUX_*).
 * Step 2 keeps a step's colour flux from being added onto the previous step's colours. */
typedef struct soil_colour_planes {
  const float* albedo_bedrock; /* in     __transfer's colour where the cell has no sediment (erosion.cu:558-559) */
  float* albedo_surface;       /* inout  the particles' colour source at their spawn cells (:91, :299);
                                         mixed in place by __transfer (:558-572)                          */
  float* albedo_fluvial;       /* inout  stale on entry; this step's fluvial colour flux, normalised in
                                         place into the transport colour (:181-185), which it holds on exit */
  float* albedo_debris;        /* inout  the same for the debris launch (:387-391)                        */
} soil_colour_planes;

/* The fused cell phase of the coloured step: soil_erode_cells_fused_ex, plus per cell the colour
 * branches of both normalises (reading massFlux / debrisFlux for m; 3-component norm, SURVEY.md
 * Appendix A4), __transfer's colour mix and the in-place writes of albedo_fluvial, albedo_debris
 * and albedo_surface — bit-identical to normalize_fluvial, normalize_debris, mass_transfer,
 * mass_creep, add, layer_merge with the colour planes, one after another.  Flags and the row range
 * of `dom` as soil_erode_cells_fused_ex.  168 algorithmic bytes per cell with SOIL_CELLS_KEEP_FLUX
 * (84 physics + 48 colour read + 36 colour written; albedo_bedrock's read and albedo_surface's
 * write counted in full).  Every colour plane is required. */
int soil_erode_cells_fused_colour(const soil_erosion_planes* planes, const soil_colour_planes* colour,
                                  const soil_domain* dom, const float scale[3], const soil_param* param,
                                  int flags, void* stream);
/* Both particle launches of the coloured step, overlapped as soil_particles_pair_slab_ex (whole
 * (H, W) grid only): the fluvial launch adds its colour flux to albedo_fluvial, the debris launch to
 * albedo_debris, both reading the spawn cell's colour from albedo_surface.  The two colour planes are
 * cleared first and hold exactly this call's colour deposits on return; `flags` (SOIL_FLUX_OVERWRITE)
 * concerns the physics flux planes.  Spent debris walkers are retired as soil_set_debris_retire says,
 * a walker whose colour deposit can still be anything but zero excepted (debris_spent). */
int soil_particles_pair_colour(const soil_erosion_planes* planes, const soil_colour_planes* colour,
                               soil_rng* rng_fluvial, soil_rng* rng_debris, int64_t N, int64_t H, int64_t W,
                               const float scale[3], const soil_param* param, int flags, void* stream);
/* soil_particles_pair_colour on a row slab (the sharded coloured step, soil_slab.h): spawns, tracing and
 * ownership as soil_particles_pair_slab_ex, `flags` as there.  Before the launches the two colour flux planes
 * are cleared over local rows [0, dom->rows); spent debris walkers are retired as in soil_particles_pair_colour.
 * albedo_bedrock is not read (it may be NULL).  `remote0` (device float[16], may be NULL): [0..7] as
 * soil_particles_pair_slab's, [8..10] the fluvial and [11..13] the debris colour deposits (att * spawn colour)
 * of NaN walkers for GLOBAL cell (0,0) when this slab does not hold it; [14..15] unused. */
int soil_particles_pair_colour_slab(const soil_erosion_planes* planes, const soil_colour_planes* colour,
                                    soil_rng* rng_fluvial, soil_rng* rng_debris, int64_t N, float* remote0,
                                    const soil_domain* dom, const float scale[3], const soil_param* param, int flags,
                                    void* stream);
/* One whole coloured step on one device: soil_erode_step_ex with the colour planes (the contract
 * above): re-seed, soil_particles_pair_colour, soil_erode_cells_fused_colour.  Flags as
 * soil_erode_step_ex. */
int soil_erode_step_colour(const soil_erosion_planes* planes, const soil_colour_planes* colour,
                           soil_rng* rng, int64_t N, uint64_t seed, uint64_t step_index, int64_t H,
                           int64_t W, const float scale[3], const soil_param* param, int flags,
                           void* stream);

/* ------------------------------------------ erosion: coloured batches of models */

/* A coloured batch: the batch of soil_erode_step_batch (B whole-grid models of (H, W), N walkers each, one seed
 * per model, the same rules, refusals and launch shapes) carrying the four colour planes of the coloured step.
 * Every pointer of `colour` is model 0 of B consecutive (H, W, 3) models: model b starts at element
 * b * H * W * 3.  Model b ends each step holding what soil_erode_step_colour leaves on that model alone with
 * seed = seeds[b]: before the fluvial launch albedo_fluvial and albedo_debris of all B models are cleared, and
 * they then hold the step's normalised transport colour; a NaN walker's colour deposit lands in cell (0, 0) of
 * its own model; no colour of one model reaches another.  Exact arithmetic, every walker walked to the end; only
 * the fp32 order of the flux atomics may differ from the single model's.  A null `colour` or a null colour plane
 * is SOIL_ERR_INVALID_ARGUMENT ("colour plane"), as are the sizes soil_erode_step_batch refuses.
 *
 * One coloured step of every model: soil_particles_batch_colour, then soil_erode_cells_fused_batch_colour with
 * flags 0.  The physics flux planes are zero on entry and on exit. */
int soil_erode_step_batch_colour(const soil_erosion_planes* planes, const soil_colour_planes* colour, int64_t B,
                                 int64_t H, int64_t W, int64_t N, const uint64_t* seeds, uint64_t step_index,
                                 const float scale[3], const soil_param* param, void* stream);
/* soil_particles_batch with colour: the two colour flux planes of every model are cleared first (also when
 * N == 0), then the fluvial launch adds its colour flux to albedo_fluvial, the debris launch to albedo_debris,
 * both reading the spawn cell's colour from albedo_surface. */
int soil_particles_batch_colour(const soil_erosion_planes* planes, const soil_colour_planes* colour, int64_t B,
                                int64_t H, int64_t W, int64_t N, const uint64_t* seeds, uint64_t step_index,
                                const float scale[3], const soil_param* param, void* stream);
/* The coloured cell phase of every model of a batch, bit-identical per model to soil_erode_cells_fused_colour
 * on that model's planes with the same flags (SOIL_CELLS_KEEP_FLUX).  168 algorithmic bytes per cell with
 * SOIL_CELLS_KEEP_FLUX; without it one more pass re-zeroes the physics flux planes of all B models (28). */
int soil_erode_cells_fused_batch_colour(const soil_erosion_planes* planes, const soil_colour_planes* colour,
                                        int64_t B, int64_t H, int64_t W, const float scale[3],
                                        const soil_param* param, int flags, void* stream);

/* ------------------------------------------ erosion: parameter sweeps */

/* A sweep: a batch (soil_erode_step_batch, or with a non-NULL `colour` the coloured batch of
 * soil_erode_step_batch_colour) in which model b steps with params[b], a soil_param of its own.  `params` is a
 * host array of B values, copied before the call returns (as `seeds`); a change between calls takes effect at the
 * next call.  Model b ends each step holding what soil_erode_step (with colour: soil_erode_step_colour) leaves on
 * that model alone with seed = seeds[b] and param = params[b].  Every other rule of the batch holds: one (H, W),
 * N, scale and step_index, model-major planes, a NaN walker's deposits in cell (0, 0) of its own model, flux
 * planes zero on entry and exit, exact arithmetic, every walker walked to the end; only the fp32 order of the
 * flux atomics may differ.  SOIL_ERR_INVALID_ARGUMENT for a NULL `params`, the sizes soil_erode_step_batch
 * refuses, and a non-NULL `colour` with a NULL plane ("colour plane").
 *
 * Launch shapes: those of the (coloured) batch at the same B, N and (H, W), each model reading its params[b]
 * once per work-group (grid.y = model).  No launch shape depends on a value of `params`: a per-model maxage is
 * only each walker's loop bound.  A sweep is the batch of different models below with the shared scale, N and
 * step_index in every record: the records reach the device in the batch's one host-to-device copy, so a sweep
 * step issues as many dispatches as the batch step (14 physics, 17 coloured, in the staged shape).  Algorithmic
 * bytes: the batch's, plus one 152-byte record read per work-group of every launch and B x 152 bytes copied per
 * step.
 *
 * One step of every model: soil_particles_batch_params, then soil_erode_cells_fused_batch_params with flags 0,
 * the params uploaded once for both. */
int soil_erode_step_batch_params(const soil_erosion_planes* planes, const soil_colour_planes* colour, int64_t B,
                                 int64_t H, int64_t W, int64_t N, const uint64_t* seeds, uint64_t step_index,
                                 const float scale[3], const soil_param* params, void* stream);
/* Both particle launches of a sweep step (soil_particles_batch / soil_particles_batch_colour, model b with
 * params[b]).  With colour the two colour flux planes of all B models are cleared first, also when N == 0. */
int soil_particles_batch_params(const soil_erosion_planes* planes, const soil_colour_planes* colour, int64_t B,
                                int64_t H, int64_t W, int64_t N, const uint64_t* seeds, uint64_t step_index,
                                const float scale[3], const soil_param* params, void* stream);
/* The cell phase of a sweep (soil_erode_cells_fused_batch / _colour, model b with params[b]), bit-identical per
 * model to the single model's cell phase with params[b]; its own upload of `params` (one copy) before the
 * batch's launches.  Bytes as there. */
int soil_erode_cells_fused_batch_params(const soil_erosion_planes* planes, const soil_colour_planes* colour,
                                        int64_t B, int64_t H, int64_t W, const float scale[3],
                                        const soil_param* params, int flags, void* stream);

/* ------------------------------------------ erosion: batches of different models */

/* One model of a batch whose models differ in more than their param: everything the single model's step takes
 * beside its planes.  152 bytes (4 bytes of padding after `scale`), 8-aligned. */
typedef struct soil_batch_model {
  soil_param param;    /* 112 bytes, 8-aligned (maxage is uint64_t) */
  float scale[3];      /* {sx, sy, sz}, as every entry point's `scale` */
  int64_t N;           /* walkers of this model, 0 <= N < 2^31 */
  uint64_t seed;
  uint64_t step_index; /* this model's streams at (seed, n, step_index * N) */
} soil_batch_model;

/* A batch of B whole-grid models of one (H, W) in which model b steps with models[b]: its own param, scale, walker
 * count N_b, seed and step index (with a non-NULL `colour`, the coloured batch of soil_erode_step_batch_colour).
 * `models` is a host array of B records, copied before the call returns; the caller advances each step_index.
 * Model b ends a step holding what soil_erode_step (with colour: soil_erode_step_colour) leaves on that model alone
 * with param, scale, N, seed and step_index taken from models[b]; only the fp32 order of the flux atomics may
 * differ.  A model with N_b = 0 runs no walkers: its step is the cell phase alone.  Every other rule of the batch
 * holds: model-major planes, a NaN walker's deposits in cell (0, 0) of its own model, flux planes zero on entry
 * and exit, exact arithmetic, every walker walked to the end, at most 65535 models per launch, the particle step
 * counter adding every walker's steps.  SOIL_ERR_INVALID_ARGUMENT for a NULL `models`, any N_b < 0 or
 * N_b >= 2^31, what soil_erode_step_batch refuses with N = max N_b, and a non-NULL `colour` with a NULL plane
 * ("colour plane").  The soil_*_batch_params entries are this batch with the shared scale, N and step_index
 * filled into every record.
 *
 * Launch shapes: the batch's at N = max N_b (direct below 1024, staged at or above; what would be tiled alone runs
 * staged), grid.x sized by max N_b; lane n of model b exits before drawing when n >= N_b.  Spawn and sorted
 * arrays keep a stride of max N_b per model.  Every work-group reads its model's record once (grid.y = model).
 * The records reach the device in one host-to-device copy per step, and the step's cell phase reads that copy,
 * so a step issues as many dispatches as the batch step (14 physics, 17 coloured, in the staged shape).
 * Algorithmic bytes: the batch's at each model's own N_b, plus one 152-byte record read per work-group of every
 * launch and B x 152 bytes copied per step.
 *
 * One step of every model: soil_particles_batch_models, then soil_erode_cells_fused_batch_models with flags 0,
 * the records uploaded once for both. */
int soil_erode_step_batch_models(const soil_erosion_planes* planes, const soil_colour_planes* colour, int64_t B,
                                 int64_t H, int64_t W, const soil_batch_model* models, void* stream);
/* Both particle launches of such a step (model b: N_b walkers from (seed_b, n, step_index_b * N_b), the debris
 * launch two draws on).  With colour the two colour flux planes of all B models are cleared first, also when
 * every N_b is 0. */
int soil_particles_batch_models(const soil_erosion_planes* planes, const soil_colour_planes* colour, int64_t B,
                                int64_t H, int64_t W, const soil_batch_model* models, void* stream);
/* The cell phase of such a batch, bit-identical per model to soil_erode_cells_fused_ex (with colour:
 * soil_erode_cells_fused_colour) with models[b].param and models[b].scale and the same flags; N, seed and
 * step_index are not read.  Its own upload of the records (one copy) before the batch's launches. */
int soil_erode_cells_fused_batch_models(const soil_erosion_planes* planes, const soil_colour_planes* colour,
                                        int64_t B, int64_t H, int64_t W, const soil_batch_model* models,
                                        int flags, void* stream);

/* ------------------------------------------ erosion: changing resolution */

/* Every plane of every model of a batch resampled to a new resolution by one kernel: the step of the multiscale
 * schedule (erode coarse, resample, erode finer) for whole models.  `src` holds B whole-grid models of (Ho, Wo),
 * `dst` B models of (Hn, Wn), both model-major as in soil_erode_step_batch; B = 1 is a single model.  Any
 * Hn, Wn, Ho, Wo >= 1: finer, coarser, non-square, another ratio on each axis.  Per model b:
 *  - resampled (the persistent state): layers (2 channels), uplift, rainfall, waterHeight, mass, debris (1),
 *    velocity, debrisVelocity (2) and, with colour, the four planes of soil_colour_planes (3 channels each).  Every
 *    value is bit-identical to what soil_resize writes for that plane of that model alone: corner-aligned sample
 *    positions, clamped corner indices, weights written 1 + -1*w and 0 + 1*w, columns interpolated first, then
 *    rows, every fp32 operation as written.  So equal resolutions give the identity, the four corner cells are
 *    kept, planes that are non-negative stay so, and no value of one model reaches another.
 *  - dst->height (may be NULL) is layers'.x + layers'.y of the resampled layers, the layer_merge every step leaves
 *    behind, and NOT the resample of src->height, which differs from it in the last bit.
 *  - the five flux planes of dst are written zero (a step requires them zero on entry); the flux planes, height
 *    and layers_next of src are not read and may be NULL.  dst->layers_next is not touched.
 *  - dst->layers, dst->uplift and dst->rainfall are written, and with colour dst_colour->albedo_bedrock, although
 *    the structs declare them `const float*` for the step's sake.
 * `dst_colour` and `src_colour` are both NULL (physics only) or both set, then with every colour plane.
 * SOIL_ERR_INVALID_ARGUMENT before any launch for B < 1, a size < 1, a NULL required plane, one colour struct
 * without the other, dst->layers == src->layers (in place is not supported: the planes of dst and src must not
 * overlap), and sizes whose byte offsets overflow int64.
 *
 * One launch per 65535 models (grid.z is the model), on `stream`, no host synchronisation, no workspace.  One
 * thread per new column, a band of rows per work-group; the column index and weight are computed once per thread
 * and the row index and weight once per row for all 12 (24 with colour) floats of the cell.  Algorithmic bytes per
 * new cell, r = Hn*Wn / (Ho*Wo): written 48 state + 4 height + 28 zeros = 80 (128 with colour), read 44 / r
 * (92 / r with colour). */
int soil_erode_resize_batch(const soil_erosion_planes* dst, const soil_erosion_planes* src,
                            const soil_colour_planes* dst_colour, const soil_colour_planes* src_colour,
                            int64_t B, int64_t Hn, int64_t Wn, int64_t Ho, int64_t Wo, void* stream);

/* ------------------------------------------ erosion: summaries */

/* What a sweep or an ensemble asks of a batch, reduced on the device: one small record per model
 * (soil_erode_batch_stats) and one map per quantity across the models (soil_erode_batch_ensemble), where the
 * only other way to look at model b is to copy its planes to the host.  `planes` holds B whole-grid models of
 * (H, W), model-major as in soil_erode_step_batch; B = 1 is a single model.  Both are deterministic (no
 * floating-point atomics anywhere, every sum in an order fixed by H*W alone), leave the planes as they are, run on
 * `stream` without host synchronisation, and take a number of dispatches that does not depend on B. */

/* The statistics of one channel of one model over its H*W cells.  A value v is finite when v - v == 0; the
 * values that are not (NaN, +-inf) are counted in `nonfinite` and leave the other four fields alone.  `sum` adds
 * (double)v and `sumsq` (double)v * (double)v (exact: the product of two fp32 values fits fp64), both accumulated
 * in fp64 throughout; `min` and `max` are over the finite values (which of +0 and -0 a tie returns is not
 * specified). */
typedef struct soil_channel_stats { /* 32 bytes */
  double sum;        /* of the finite values */
  double sumsq;      /* of their squares */
  int64_t nonfinite; /* cells holding NaN or +-inf */
  float min, max;    /* over the finite values; +inf / -inf when there is none */
} soil_channel_stats;
/* The channels of a record, in this order: bedrock (layers.x), sediment (layers.y), height, waterHeight, mass,
 * debris, velocity.x, velocity.y, debrisVelocity.x, debrisVelocity.y.  "height" is layers.x + layers.y in fp32,
 * the value layer_merge leaves, computed from `layers` (so +inf bedrock under -inf sediment is one non-finite
 * height). */
#define SOIL_STAT_CHANNELS 10
typedef struct soil_model_stats { soil_channel_stats ch[SOIL_STAT_CHANNELS]; } soil_model_stats; /* 320 bytes */

/* out[b] (device, B records) = the statistics of model b.  Reads layers, waterHeight, mass, debris, velocity and
 * debrisVelocity: 36 algorithmic bytes per cell; `height`, the flux planes, layers_next, uplift and rainfall are
 * not read and may be NULL.
 * The reduction tree is fixed by n = H*W alone: a model's cells, flattened, are cut into chunks (a multiple of
 * 1024 cells, at least 4096, at most 4096 chunks to a model); a work-group reduces one chunk, lane-local first
 * (lane t of 256 takes cells 4t .. 4t+3 of every 1024), then across the wave, then across the four waves through
 * LDS, and writes one partial record to the library's workspace; a second launch folds each model's partials in
 * index order into out[b].  Neither B, nor b, nor the alignment of a model's first cell enters (loads are 16-byte
 * where the model's base allows and scalar otherwise, the same cells to the same lanes either way), so out[b] is
 * bit-identical to the record of model b alone, in a batch of another B or at another position, and from call to
 * call.  Two dispatches per 65535 models (grid.z is the model); the workspace is written in full before it is
 * read.
 * SOIL_ERR_INVALID_ARGUMENT before any launch for B < 1, a size < 1, sizes whose byte offsets overflow int64, a
 * NULL `planes` or `out`, or a NULL plane among the six read. */
int soil_erode_batch_stats(const soil_erosion_planes* planes, int64_t B, int64_t H, int64_t W,
                           soil_model_stats* out, void* stream);

/* Per cell, the mean and the population variance across the B models of bedrock, sediment, height (layers.x +
 * layers.y in fp32), waterHeight, mass and debris, in this order: `mean` and `var` are (H, W, 6) device planes;
 * `var` may be NULL (mean only).  Per cell and channel, every operation as written and none contracted:
 *   s = sum of (double)v_b, q = sum of (double)v_b * (double)v_b, for b = 0 ... B-1 in that order, in fp64;
 *   m = s / B;  mean = (float)m;  v = q / B - m * m;  var = (float)(v < 0 ? 0 : v).
 * The one-pass variance cancels: its relative error is about 2^-53 * m*m / v, so a variance below about
 * 2^-53 * m*m is noise (fp32 inputs one ulp apart have v / (m*m) of about 2^-46 / B, where the result keeps some
 * 7 - log2(B) bits; a spread of 2^-12 of the mean keeps full fp32 precision).  A NaN or an infinity in one
 * model's cell reaches the outputs of that cell and of no other cell.
 * Reads layers, waterHeight, mass and debris: 20 algorithmic bytes per cell and model, and writes 24 per cell (48
 * with `var`).  One dispatch whatever B is, no workspace: one thread per cell walks the models, every load
 * coalesced along W.
 * SOIL_ERR_INVALID_ARGUMENT before any launch for B < 1, a size < 1, sizes whose byte offsets overflow int64, a
 * NULL `planes` or `mean`, or a NULL plane among the four read. */
#define SOIL_ENSEMBLE_CHANNELS 6 /* bedrock, sediment, height, waterHeight, mass, debris */
int soil_erode_batch_ensemble(const soil_erosion_planes* planes, int64_t B, int64_t H, int64_t W,
                              float* mean /* (H, W, 6) */, float* var /* (H, W, 6) or NULL */, void* stream);

/* Order statistics across the models.  Per cell and channel (the six SOIL_ENSEMBLE_CHANNELS in their order, height
 * being layers.x + layers.y in fp32), the B values v_0 .. v_{B-1} are ordered by an integer key and never by a
 * float compare (which may canonicalise or flush).  From the value's bits u:
 *   every NaN first becomes 0x7FC00000;  key = (u >> 31) ? ~u : u | 0x80000000;  keys are compared unsigned.
 * That is -inf < ... < -denormal < -0 < +0 < +denormal < ... < +inf < NaN, so the k-th order statistic s_k is one
 * definite bit pattern, denormals kept, whatever the order of the models and whichever path computed it.
 *
 * out[j] (device, (nq, H, W, 6)) = the value at fractional rank pos[j] (host array, each in [0, B-1]; 0 the
 * minimum, B-1 the maximum, (B-1)/2 the median).  The host splits pos[j] in fp64 into lo = floor(pos) and
 * frac = pos - lo; with a = s_lo and b = s_min(lo+1, B-1) the result is
 *   a, bit for bit, when frac == 0 or a == b (float equality: -0 next to +0 gives -0);
 *   (float)((double)a + frac * ((double)b - (double)a)) otherwise: three fp64 operations as written, none
 *   contracted.
 * Infinities and NaN get what that arithmetic gives and no special case: -inf next to a finite value (or to +inf)
 * is NaN at a fractional position between them, +inf above a finite value is +inf; a model holding NaN in a cell
 * occupies the top ranks of that cell, so it spoils only positions above B - 1 - (number of NaN models) there, and
 * no other cell.  Which NaN an interpolation returns (sign, payload) is the fp64 unit's; an order statistic that
 * is a NaN is 0x7FC00000.
 * Reads layers, waterHeight, mass and debris (20 algorithmic bytes per cell and model), the other planes may be
 * NULL; writes 24 * nq bytes per cell, once.  The planes are left as they are.  One dispatch on `stream` whatever
 * B is, no host synchronisation, no workspace; the (lo, frac) pairs travel in the launch arguments, hence
 * SOIL_QUANTILES_MAX.  Three paths, the same bytes; a wave is 64 consecutive cells of one channel on each, so every
 * load is coalesced along W.  "reg" (B <= 64): a thread sorts its cell-channel's keys in registers, a bitonic
 * network padded to a power of two with key 0xFFFFFFFF.  "lds" (B <= 256): a work-group sorts 64 cells, a thread
 * holding 16 keys, the network's wide steps exchanged through LDS.  "bisect" (any B): each rank is found by
 * bisecting the key space, 32 walks over the models counting keys <= mid.  Left to itself the entry takes reg up to
 * B = 16, lds up to B = 256 and bisect above; SOIL_QUANTILE_PATH = auto | reg | lds | bisect forces one
 * (docs/KNOBS.md), and forcing one at a B it cannot hold is refused.
 * SOIL_ERR_INVALID_ARGUMENT before any launch for B < 1, a size < 1, sizes whose byte offsets overflow int64, a
 * NULL `planes`, `out` or `pos`, a NULL plane among the four read, nq < 1 or nq > SOIL_QUANTILES_MAX, a pos[j]
 * that is not finite or lies outside [0, B-1], and an output whose byte size overflows int64. */
#define SOIL_QUANTILES_MAX 16
int soil_erode_batch_quantiles(const soil_erosion_planes* planes, int64_t B, int64_t H, int64_t W,
                               const double* pos /* host, nq fractional ranks in [0, B-1] */, int nq,
                               float* out /* (nq, H, W, 6) device */, void* stream);

/* out (device, (H, W, 6)) = per cell and channel, the share of the models whose value exceeds thresholds[ch] (host
 * array, the six SOIL_ENSEMBLE_CHANNELS in their order): c = the number of b with v_b > thresholds[ch], a float
 * compare that is false with a NaN on either side, and out = (float)((double)c / (double)B).  Planes read, bytes,
 * stream and dispatch count as for soil_erode_batch_quantiles with nq = 1: one thread per cell walks the models.
 * SOIL_ERR_INVALID_ARGUMENT before any launch for what soil_erode_batch_quantiles refuses of B, H, W and the
 * planes, and a NULL `planes`, `out` or `thresholds`. */
int soil_erode_batch_exceedance(const soil_erosion_planes* planes, int64_t B, int64_t H, int64_t W,
                                const float thresholds[SOIL_ENSEMBLE_CHANNELS] /* host */,
                                float* out /* (H, W, 6) device */, void* stream);

/* The containers of the legacy API (example/erosion_gpu.py:44-71): model_t, the `data` and the
 * `track` buffers.  All float32 device planes of H*W cells ((H,W,2) for the momenta). */
typedef struct soil_erode_model {
  float* height;                /* inout  bedrock surface        (erosion_gpu.py:44-48)  */
  float* sediment;              /* inout  sediment on top of it                           */
  const float* uplift;          /* in                                                     */
  const float* rainfall;        /* in                                                     */
  float* discharge;             /* out    data.discharge = waterHeight (:59-63)           */
  float* mass;                  /* out    data.mass                                       */
  float* momentum;              /* out    data.momentum (H,W,2) = velocity                */
  float* debris;                /* out    data.debris                                     */
  float* debris_momentum;       /* out    data.debris_momentum (H,W,2)                    */
  float* discharge_track;       /* scratch track.* (:65-71): zeroed on entry and on exit  */
  float* mass_track;
  float* momentum_track;        /* (H,W,2) */
  float* debris_track;
  float* debris_momentum_track; /* (H,W,2) */
} soil_erode_model;

/* soil::erode(model, data, track, param[, steps]) — the legacy composite the acceptance script
 * calls (example/erosion_gpu.py:102-106; its binding survives only as a comment,
 * python/source/model.cpp:142): `steps` erosion steps numbered first_step, first_step + 1, ...
 * on the model's planes, in place.  The (H,W,2) layer double buffer and the N particle streams
 * live in the library's workspace for the duration of the call (and stay cached for the next). */
int soil_erode(const soil_erode_model* model, int64_t H, int64_t W, int64_t N, uint64_t seed,
               uint64_t first_step, int steps, const float scale[3], const soil_param* param,
               void* stream);

/* Launch shape of the particle kernels: 0 = auto, 1 = direct (the reference's:
 * thread n = particle n, 5-point stencil gathers), 2 = staged (packed field
 * plane + tile-ordered particles), 3 = tiled (per-tile particle queues, one
 * gather of pre-digested cell terms per step, flux tiles in LDS).  Auto picks
 * tiled for N >= 45000 (grids up to 2^31 cells), staged for N >= 1024, else direct.  All
 * shapes produce the same trajectories and deposits; only the order of the
 * fp32 additions into a cell differs.  For ablation and tests.
 * In the tiled shape the host follows the device: it reads one pinned word per round and queues the
 * next rounds, or the finishing launch, by what it finds.  A particle launch in that shape, alone or
 * inside a step, is ordered on `stream` like every other, but it synchronises with the stream's
 * progress: it returns when its last launch is queued, which is after the work queued ahead of it
 * has run.  The direct and the staged shape return with everything in flight. */
int soil_set_particle_mode(int mode);
/* Arithmetic of the particle step (the loops of erosion.cu:100-139 / :306-349) in the tiled shape:
 * 0 = exact (default): every `/` of the reference's step a correctly rounded IEEE quotient, sqrt
 *     correctly rounded — the walks of the oracle, step for step (the parity tests' contract);
 * 1 = fast: quotients as numerator x v_rcp_f32(denominator), v_sqrt_f32, debris' mass attenuation on the
 *     hardware exponential (what nvcc -use_fast_math makes of the same statements: __fdividef,
 *     sqrt.approx, __expf).  Walks are chaotic in the last bit, so results agree with the exact
 *     mode statistically: plane sums within 2e-3, visited cells within 0.5 %, step counts within
 *     0.5 % (tests/test_fast_particles.py).  9 % less time per 8192^2 step.
 * Launches that carry colour planes and the direct / staged shapes always run exact.
 * SOIL_PARTICLE_DIV=fast in the environment makes 1 the default of the process. */
int soil_set_particle_arith(int mode);
int soil_get_particle_arith(void);
/* Spent debris walkers (tiled shape; the loop of erosion.cu:306-349).  With the reference's example
 * parameters (example/erosion_gpu.py:75-100) a debris walker's two attenuations underflow to exact zeros
 * within two steps (decay_d ~ -1e18, decay_v ~ 1e10) and it walks the rest of its 256 steps adding +-0 to the
 * flux planes.  A walker for which that is certain — att_v == 0, att_d * source_d == 0, its state finite, and
 * every cell of the slab checked by the step's pack pass (excessStress finite and negative at debrisHeight =
 * eps, record finite), launch constants in range: csrc/erosion_particles_tiled.hip, debris_spent — is
 *   1 = retired (default): its walk ends there.  The flux planes hold the same bits as if it had been
 *       walked to the end (x + (+-0) = x); soil_particle_steps counts the steps actually walked.
 *   0 = walked to the end, as the reference does.
 *   2 = watched: marked, walked on, and every deposit of a marked walker that is not an exact zero (and every
 *       marked walker that stops qualifying) counted — soil_debris_retire_violations; the tests want 0.
 * Off in the slab runner's migrate mode (the walker's later cells lie on other ranks) and in the launches with
 * colour planes of soil_transport_debris / soil_particles_debris_slab (walked to the end); on in the coloured
 * step's launches (soil_particles_pair_colour, soil_erode_step_colour), where a spent walker's colour deposit
 * att_d * source_d * albedo must be an exact zero too.
 * SOIL_DEBRIS_RETIRE in the environment sets the default of the process. */
int soil_set_debris_retire(int mode);
int soil_get_debris_retire(void);
int soil_debris_retire_violations(uint64_t* total, int reset, void* stream);
/* Ghost rows a slab needs on each interior side so that no trajectory can
 * leave it: ceil(sqrt(2) * maxage) + 2 (one __stepsize step moves a particle
 * by at most sqrt(2) cells, erosion_map.cu:61-76). */
int64_t soil_ghost_rows(const soil_param* param);
/* What of a slab's ghost zone this step's deposits reached: depth[0] = number of rows above the
 * owned local rows [r0, r1) — counted from the boundary — down to the farthest one holding a
 * value other than zero in `plane` ((rows, row_floats) floats), depth[1] = likewise below.
 * Accumulates with max (clear `depth`, two device int32, first; call once per flux plane).  A
 * slab only has to ship that many rows of flux to its neighbour, and next step's particles
 * need the fields refreshed about that deep (soillib_amd/parallel.py).  No counterpart in the
 * single-GPU reference. */
int soil_ghost_extent(int32_t* depth, const float* plane, int64_t rows, int64_t row_floats,
                      int64_t r0, int64_t r1, void* stream);
/* Particle steps (loop iterations of erosion.cu:100 / :306 that pass the loop
 * head) executed by all particle launches on the current device since the last
 * reset; synchronises `stream`.  The reference has no counterpart: it is the
 * numerator of the Mparticle-steps/s that SURVEY.md 8d asks to report, and an
 * exact integer the parity tests compare with the oracle's count. */
int soil_particle_steps(uint64_t* total, int reset, void* stream);

/* ------------------------------------------------------------- flow graphs */

/* soil::direction — graph.hpp:49, graph.cu:246-264 (__direction :201-243), model.cpp:157-159. */
int soil_direction(int32_t* direction, const float* height, int64_t H, int64_t W, int edge,
                   void* stream);
/* soil::steepest — graph.hpp:52, graph.cu:73-91 (__steepest :27-70), model.cpp:169-171. */
int soil_steepest(int32_t* graph, const float* height, int64_t H, int64_t W, int edge,
                  void* stream);
/* soil::random_weighted — graph.hpp:54, graph.cu:175-195 (__seed :97-101,
 * __random_weighted :103-173), model.cpp:173-175.  Stateless: cell n draws its one uniform in (0, 1]
 * from the Philox4x32-10 block (key seed; counter {offset, n >> 2}), word n & 3 — the reference's
 * curand_init(seed, n, offset) + one curand_uniform per cell, with one block serving four cells.
 * Temperature: T must be 0 or a normal positive float (FLT_MIN .. FLT_MAX).  T = 0, of either sign, gives the
 * reference's graph for it, -1 in every cell (each downhill weight is +inf, or 0 for -0).  A subnormal, negative,
 * NaN or infinite T is refused with SOIL_ERR_INVALID_ARGUMENT before anything else, with or without a device — by
 * soil_random_weighted_batch and soil_multiflow alike. */
int soil_random_weighted(int32_t* graph, const float* height, int64_t H, int64_t W, int edge,
                         uint64_t seed, uint64_t offset, float T, void* stream);
/* soil::slope — graph.hpp:63, graph.cu:297-311 (__slope :270-295), model.cpp:161-163. */
int soil_slope(float* slope, const float* tensor, const int32_t* flow, int64_t H, int64_t W,
               const float scale[2], void* stream);
/* soil::accumulate / accumulate_decay — graph.hpp:57-60, graph.cu:578-593
 * (__accumulate :526-576: __donor :321-348, __count :350-380, my_decay
 * :382-420, __rake_compress :429-522), model.cpp:181-187.  `decay` == NULL
 * selects accumulate (scalar decay 1).  Scratch comes from a cached
 * per-device workspace, not from per-call allocations.  Synchronises the
 * stream before returning, like the reference (graph.cu:564). */
int soil_accumulate(float* out, const int32_t* graph, const float* source, const float* decay,
                    int64_t H, int64_t W, int edge, void* stream);
/* The realisation loop of example/dem_multiflow.py:43-49 as one call, without the
 * per-realisation trip through host memory: for k = k_first, k_first+k_stride, ... < k_end
 *   sum += double(float(accumulate(random_weighted(height, edge, seed, k, T), source) / K))
 * `sum` (H*W doubles) is accumulated into — zero it first.  A rank of an N-GPU run
 * passes k_first = rank, k_stride = N and all-reduces `sum` afterwards: accumulation
 * does not shard (pointer jumps span the grid), the realisations do.
 * Synchronises the stream before returning, like soil_accumulate: the realisations run on private
 * lanes that wait for `stream` and are joined back into it first. */
int soil_multiflow(double* sum, const float* height, const float* source, int64_t H, int64_t W,
                   int edge, uint64_t seed, uint64_t k_first, uint64_t k_stride, uint64_t k_end,
                   uint64_t K, float T, void* stream);
/* Depression filling before flow routing (BASELINE config 3).  The reference has
 * none — example/dem_condition.py:35-41 calls the third-party pysheds — so this is
 * build-defined, parity unpinned: out(c) = the lowest level at which
 * cell c can drain to an outlet (a step off the grid or onto a NaN cell) along `edge`
 * connectivity, i.e. the priority-flood surface; NaN cells stay NaN.  Exact in fp32
 * (only min/max): tile relaxation in LDS, started from the recursively filled 4x coarser
 * level (csrc/conditioning.hip); synchronises the stream. */
int soil_fill_depressions(float* out, const float* height, int64_t H, int64_t W, int edge,
                          void* stream);
/* The fill of B models of one (H, W) in one call.  `height` and `out` are model-major (B, H, W) float32; model b's
 * slice of `out` is, bit for bit, what soil_fill_depressions gives for model b's slice alone.  All models are on the
 * same level of the pyramid at the same time: the launch grid is tiles x models (whole models per launch, at most
 * 65535 of them; a larger batch goes in several launches side by side), one "changed" word serves the batch, and a
 * level ends at the first look that finds no tile of any model moved — a settled model costs its tiles an early
 * return.  The relaxation passes of a call are those of the model that needs most and do not grow with B.  Scratch:
 * the slot of soil_fill_depressions (WS_CONDITIONING in csrc/common.hpp; both calls synchronise the stream before
 * they return, so neither finds the other's data in use).  Refused with SOIL_ERR_INVALID_ARGUMENT before any device
 * work, with or without a device: a null pointer, out == height, B, H or W < 1, H * W > INT32_MAX, an invalid edge. */
int soil_fill_depressions_batch(float* out, const float* height, int64_t B, int64_t H, int64_t W, int edge,
                                void* stream);
/* What the calling host thread's last call of soil_fill_depressions or soil_fill_depressions_batch that got as far as
 * its first launch did (a call that was refused, found no device or failed to get its scratch leaves the record of the
 * call before it; one that fails later leaves what it did up to there): info[0] relaxation passes in all (one pass = every tile of every model once), info[1] levels of the
 * pyramid, info[2] models, info[3] looks at the "changed" word, info[4 + l] passes on level l (0: the DEM itself;
 * levels beyond the eleventh are added into info[15]).  All zero before the first call; needs no device. */
int soil_fill_depressions_info(int64_t info[16]);
/* Scratch memory.  The reference allocates its scratch per call (graph.cu:539-550, :182-183;
 * path.cu:195; filter.cu:77); this library keeps one cached block per host thread, device and
 * purpose (accumulate, the particle launches of either kind, fill_depressions, soil_erode) and
 * grows it on demand.  Several host threads may drive one device at the same time, each on its
 * own stream: they share no scratch (nor streams, events or pinned words of the launches, which
 * are per thread too).  Calls of ONE thread that use the same block must not overlap in time —
 * they do not, since a thread's calls are ordered on the streams it passes.  A call that finds its
 * block too small synchronises the device before replacing it.
 * soil_workspace_release frees all cached blocks of the current device, of every thread: call it
 * while no other thread is inside the library. */
int soil_workspace_release(void);
/* What the library holds for its host threads, process-wide and on every device: info[0] streams, info[1] events,
 * info[2] pinned host allocations, info[3] cached scratch blocks.  Counted where each is made and freed.  A host thread
 * owns its blocks, the pinned "changed" words of the relaxations, the pinned staging of the batch uploads, the lanes of
 * soil_multiflow and the forked streams and the pinned record of the tiled particle launches; all of them go when the
 * thread ends (behind a hipDeviceSynchronize()), except on the thread that loaded the library, which keeps them until
 * the process exits.  Not counted: what the caller owns (soil_event_create, the handles of soil_slab.h).  All zero
 * before the first call that needs one; needs no device.  SOIL_ERR_INVALID_ARGUMENT for a null `info`. */
int soil_host_objects_info(int64_t info[4]);

/* ------------------------------------------ flow graphs: batches of models */

/* The five calls above for B models of one (H, W) in one call, in a number of launches that does not grow with B.
 * Every tensor is model-major, as in soil_erode_step_batch: model b of a plane starts at element b * H * W.
 *
 * Per-model contract.  Model b's slice of every output is, bit for bit, what the single-grid call writes for
 * model b's slices of the inputs alone — with seed = seeds[b], and with the pair scales[b] (or the one pair).
 * A graph entry is an index WITHIN its own model (0 .. H*W-1, or -1): model b's slice of a batch graph can be
 * handed to soil_accumulate, and a single grid's graph can be a slice of a batch.  Nothing a model holds can
 * reach another model: a neighbour off a model's edge does not exist, and a graph entry that is not one of the
 * cell's K neighbours inside its model is no edge (as in the single grid's donor pass).
 *
 * Round count.  soil_accumulate_batch runs the rounds a single model of (H, W) runs,
 * 2 * (ceil(log2(H*W) / 2) + 1), not those of the stacked size: a graph that does not converge (a cycle) gets
 * the values of that round count, the single grid's.
 *
 * The batch entries are stream-ordered and do not synchronise (soil_accumulate keeps its synchronisation); a
 * call that finds its cached scratch too small synchronises the device before replacing it, as everywhere.
 * Because they return with their work in flight, a host thread's calls of soil_accumulate_batch on one device share
 * one cached scratch block (its own, not soil_accumulate's), and so do its calls of soil_random_weighted_batch and
 * soil_slope_batch (the device copy of seeds / scales): issue such calls on ONE stream, or order the streams yourself
 * (an event) so that the earlier call has finished before the later one starts.  Other threads have their own blocks.
 * `seeds` (B words) and `scales` (n_scales pairs (sx, sy), n_scales == 1 or B) are HOST arrays, read before the
 * call returns; they reach the device in at most one small stream-ordered copy.  Launches: each graph or slope
 * entry ceil(B / 65535) kernels; soil_accumulate_batch runs in chunks of whole models — as many as keep the
 * rounds' 32-bit offsets (K * cells * 4 < 2^32) and one donor pass (65535), SOIL_FLOW_BATCH_CELLS lowers the
 * cells of a chunk — and per chunk one donor pass, one control kernel and the rounds, whatever B is.  Results do
 * not depend on the chunking.
 *
 * Refused with SOIL_ERR_INVALID_ARGUMENT before any device work, the entry's name in soil_last_error(): a null
 * tensor, null `seeds` or `scales`, B, H or W < 1, H * W > INT32_MAX, n_scales not 1 or B, an invalid `edge`.
 * Without a device: SOIL_ERR_NO_DEVICE (a temperature soil_random_weighted refuses is refused first). */
/* soil_direction for B models. */
int soil_direction_batch(int32_t* direction, const float* height, int64_t B, int64_t H, int64_t W, int edge,
                         void* stream);
/* soil_steepest for B models. */
int soil_steepest_batch(int32_t* graph, const float* height, int64_t B, int64_t H, int64_t W, int edge,
                        void* stream);
/* soil_random_weighted for B models: cell n of model b (n within the model) draws from the Philox block (key
 * seeds[b]; counter {offset, n >> 2}), word n & 3. */
int soil_random_weighted_batch(int32_t* graph, const float* height, int64_t B, int64_t H, int64_t W, int edge,
                               const uint64_t* seeds, uint64_t offset, float T, void* stream);
/* soil_slope for B models, model b with scales[b] or with the one pair. */
int soil_slope_batch(float* slope, const float* tensor, const int32_t* flow, int64_t B, int64_t H, int64_t W,
                     const float* scales, int64_t n_scales, void* stream);
/* soil_accumulate for B models; `decay` may be NULL. */
int soil_accumulate_batch(float* out, const int32_t* graph, const float* source, const float* decay,
                          int64_t B, int64_t H, int64_t W, int edge, void* stream);

/* ------------------------------------------------- flow graphs: downstream */

/* Where every cell of a receiver graph drains to, how many edges away that is, and how long the way is: basin
 * labels, flow length to the outlet, and (with a stop plane) the catchment of a pour point.  The reference's binding
 * names `upstream(tensor, index, target)` and `distance(tensor, index, target)`, commented out and without an
 * implementation (model.cpp); the definition below is this library's.
 *
 * Grid (H, W), cell n = x * W + y, `edge` D4 or D8, `graph` as the calls above make it (any int32 is taken).
 *
 * Edge rule — the edges the donor pass of soil_accumulate accepts.  Cell n has an edge to r = graph[n] iff
 * 0 <= r < H * W and, with (qx, qy) = (r / W, r % W): |qx - x| <= 1 and |qy - y| <= 1, not both differences zero,
 * and for D4 not both nonzero.  Anything else is no edge and makes the cell a terminal: -1, the cell itself, a
 * non-neighbour, a diagonal under D4, any other int32 (INT32_MIN, INT32_MAX).  A cell with stop[n] != 0 is a terminal
 * whatever its graph entry; `stop` is an optional int32 plane of pour points.
 *
 * Walk.  The walk of n follows edges from n until it stands on a terminal.  terminal[n] is that cell (n itself for
 * a terminal), steps[n] the number of edges walked = n_row (only the row changed) + n_col (only the column) + n_diag,
 * and, in fp64 with one rounding per operation and no contraction, then one round-to-nearest conversion,
 *     length[n] = (float)(((double)n_row * sx + (double)n_col * sy) + (double)n_diag * dd)
 * sx, sy the floats of `scale` widened (sx belongs to a row step, as in soil_slope; the values are used as they are)
 * and dd = sqrt(sx * sx + sy * sy), computed once on the host in double.  A cell whose walk never ends — it is on a
 * cycle or drains into one — gets terminal = -1, steps = -1, length = NaN (quiet, 0x7fc00000).  Every cell of an
 * acyclic graph is resolved whatever its path length, up to H * W - 1 edges: ceil(log2(H * W)) pointer-doubling
 * rounds over 16-byte records (csrc/flow_paths.hip).
 *
 * Any of the three outputs may be NULL, `stop` may be NULL; `scale` / `scales` (n_scales pairs, 1 or B) are HOST
 * arrays read before the call returns, needed only when `length` is asked for (n_scales is checked either way).
 * Both entries are stream-ordered and do not synchronise (a call that finds its cached scratch too small
 * synchronises the device before replacing it, as everywhere); a host thread's calls on one device share one cached
 * scratch block of their own: issue them on ONE stream, or order the streams yourself.
 *
 * Batch form: model-major planes; graph, stop and terminal entries are indices WITHIN their model; model b's slice
 * of every output is bit for bit what soil_flow_paths gives for model b's slices alone, with scales[b] or the one
 * pair; nothing reaches another model (an entry in another model's numbering is no edge).  Chunks of whole models —
 * as many as keep 32-bit offsets (16 bytes a cell under 4 GiB) and one init launch (65535), SOIL_FLOW_BATCH_CELLS
 * lowers the cells of a chunk; a single model above that is a chunk of its own on 64-bit offsets — and per chunk
 * one init launch, ceil(log2(H * W)) rounds (ONE model's count) and one final launch, whatever B is.  Results do not
 * depend on the chunking.
 *
 * Refused with SOIL_ERR_INVALID_ARGUMENT before any device work, with or without a device, the entry's name in
 * soil_last_error(): null `graph`, all three outputs null, `length` without `scale`, B, H or W < 1,
 * H * W > INT32_MAX, n_scales not 1 or B, an invalid `edge`.  Otherwise, without a device: SOIL_ERR_NO_DEVICE. */
int soil_flow_paths(int32_t* terminal, int32_t* steps, float* length, const int32_t* graph, const int32_t* stop,
                    int64_t H, int64_t W, int edge, const float scale[2], void* stream);
int soil_flow_paths_batch(int32_t* terminal, int32_t* steps, float* length, const int32_t* graph,
                          const int32_t* stop, int64_t B, int64_t H, int64_t W, int edge, const float* scales,
                          int64_t n_scales, void* stream);
/* What the calling host thread's last call of soil_flow_paths or soil_flow_paths_batch did, for tests and tuning:
 * info[0] chunks, info[1] chunks whose init pass took the 16-byte form, info[2] chunks on 64-bit offsets
 * (SOIL_PATHS_IDX64=1 forces them), info[3] rounds per chunk.  All zero before the first call; needs no device. */
int soil_flow_paths_info(int64_t info[4]);

/* --------------------------------------------- flow graphs: downstream sums */

/* A value carried DOWN a receiver graph: the linear recurrence
 *     x[n] = t[n]                             n a terminal
 *     x[n] = a[n] * L(n) + b[n] * x[r(n)]     n has an edge to r(n), of length L(n)
 * chi and travel time to the outlet (sums of a per-cell weight along the way), the height of a cell's outlet (height
 * above nearest drainage), the share of a cell's output that survives a per-cell decay on the way down, and, with
 * coefficients made from the planes, the implicit stream-power incision step (Braun & Willett's O(N) solver, the
 * "fastflow" of the reference's example/dem_process.py).  The reference has no such call; the definition is this
 * library's.
 *
 * Grid, edge rule, `stop` and terminals are word for word those of soil_flow_paths above: cell n has an edge to
 * r = graph[n] iff r is the index of one of its K neighbours inside the model, anything else (INT32_MIN included)
 * makes it a terminal, and a cell with stop[n] != 0 is a terminal whatever its graph entry.
 *
 * soil_downstream.  `a`, `b`, `t`, `stop` and `scale` may each be NULL: a == 1, b == 1, t == 0, L == 1.  At least one
 * of `out` (float) and `out64` (double) is non-NULL.  A cell with an edge of kind row / column / diagonal has
 * L = sx / sy / dd, soil_flow_paths' scale: the floats of `scale` widened, dd = sqrt(sx * sx + sy * sy) made once on
 * the host in double (the values are used as they are).  Its coefficients, in fp64:
 *     A0 = (double)a[n] * L      one rounding; without a scale A0 = (double)a[n]
 *     B0 = (double)b[n]
 * A terminal has A0 = (double)t[n], B0 = 0, and is final.  Then ceil(log2(H * W)) rounds, the count for ONE model;
 * in each a cell that is not final, with pointer p (its receiver at the start), does
 *     A <- A + (B * A_p)         the product rounded first, then the sum
 *     B <- B * B_p
 *     ptr <- ptr_p
 * every operand from the records of the round before, in fp64 with no contraction (__dmul_rn, __dadd_rn); the cell
 * becomes final when the record it read was final, and a final record never changes again.  Result: out64[n] = A,
 * out[n] = (float)A rounded to nearest; any NaN is written as 0x7fc00000 / 0x7ff8000000000000, and a cell that is
 * not final after the last round — it is on a cycle or drains into one — gets that NaN too.  An acyclic graph
 * resolves whatever its path lengths, up to H * W - 1 edges.
 *
 * The result is therefore one definite bit pattern, fixed by the graph and the planes alone: lists, dense rounds,
 * offset widths, chunking and batching do not show, and b == NULL gives the bits of b == 1.0 everywhere (the kernels
 * then keep no B: csrc/downstream.hip).  It is the value of the recurrence up to fp64 rounding in another order of
 * association, not the serial sum's bits.
 *
 * soil_stream_power: the implicit step h' = (h + dt u + F h'[r]) / (1 + F), F = k dt / L, slope exponent n = 1 only
 * (n != 1 is not an affine map, so not associative: soil_stream_power_n below iterates on this solve).  The same rounds, the coefficients made in the
 * init pass from the planes, nothing materialised in between.  For a cell with an edge of length L, each operation
 * rounded once:
 *     F = ((double)erosivity[n] * dt) / L
 *     d = 1.0 + F
 *     A0 = ((double)height[n] + dt * (double)uplift[n]) / d      (double)height[n] / d with uplift == NULL
 *     B0 = F / d
 * A terminal keeps (double)height[n]: it is the base level, neither lifted nor eroded.  `erosivity` is K A^m, made by
 * the caller: the power is kept out of the kernel so that every operation in it is correctly rounded and can be
 * restated bit for bit.  `uplift` and `stop` may be NULL.
 *
 * `scale` / `scales` (n_scales pairs, 1 or B) are HOST arrays read before the call returns (per-model pairs travel in
 * one small stream-ordered copy).  The entries are stream-ordered and do not synchronise (a call that finds its cached
 * scratch too small synchronises the device before replacing it, as everywhere); a host thread's calls on one device
 * share one cached scratch block of their own: issue them on ONE stream, or order the streams yourself.
 *
 * Batch form: the conventions of soil_flow_paths_batch.  Model-major planes; graph entries are indices WITHIN their
 * model; model b's slice of each output is bit for bit what the single call gives for model b's slices alone, with
 * scales[b] or the one pair; nothing reaches another model.  Chunks of whole models, as many as keep 32-bit offsets
 * and one init launch (65535), SOIL_FLOW_BATCH_CELLS lowers the cells of a chunk; a single model above that is a
 * chunk of its own on 64-bit offsets.  Per chunk one init launch, the rounds of one model and one final launch,
 * whatever B is.
 *
 * Refused with SOIL_ERR_INVALID_ARGUMENT before any device work, with or without a device, the entry's name in
 * soil_last_error(): null `graph`, both outputs null, an output that aliases an input plane (or the other output),
 * B, H or W < 1, H * W > INT32_MAX, n_scales not 1 or B, an invalid `edge`; for the stream-power entries in addition
 * a null `height`, `erosivity` or `scale`, a scale entry that is not a positive finite float, a `dt` that is negative
 * or not finite.  Otherwise, without a device: SOIL_ERR_NO_DEVICE. */
int soil_downstream(float* out, double* out64, const int32_t* graph, const float* a, const float* b, const float* t,
                    const int32_t* stop, int64_t H, int64_t W, int edge, const float scale[2], void* stream);
int soil_downstream_batch(float* out, double* out64, const int32_t* graph, const float* a, const float* b,
                          const float* t, const int32_t* stop, int64_t B, int64_t H, int64_t W, int edge,
                          const float* scales, int64_t n_scales, void* stream);
int soil_stream_power(float* out, double* out64, const float* height, const int32_t* graph, const float* erosivity,
                      const float* uplift, const int32_t* stop, int64_t H, int64_t W, int edge, const float scale[2],
                      double dt, void* stream);
int soil_stream_power_batch(float* out, double* out64, const float* height, const int32_t* graph,
                            const float* erosivity, const float* uplift, const int32_t* stop, int64_t B, int64_t H,
                            int64_t W, int edge, const float* scales, int64_t n_scales, double dt, void* stream);
/* What the calling host thread's last call of one of the four entries above did, as soil_flow_paths_info: info[0]
 * chunks, info[1] chunks whose init pass took the 16-byte form, info[2] chunks on 64-bit offsets (SOIL_PATHS_IDX64=1
 * forces them), info[3] rounds per chunk.  All zero before the first call; needs no device. */
int soil_downstream_info(int64_t info[4]);

/* --------------------------------------------- flow graphs: upstream extrema */

/* A minimum or a maximum carried UP a receiver graph: for every cell the least (the greatest) of `value` over all the
 * cells that drain through it, and which cell holds it.  With the heights as `value` and the graph that depression
 * filling and flat routing give, the minimum is the breached (carved) surface — every cell lowered to the lowest
 * height of anything that drains through it, never above the DEM and never rising along the graph (`carve` in
 * fastscape, Cordonnier et al. 2019; "breach" in Lindsay's tools) —; the maximum of soil_flow_paths' length is the
 * longest flow path into a cell, the maximum of the heights the catchment's highest point.  The reference has no such
 * call; the definition is this library's.
 *
 * Grid (H, W), cell n = x * W + y, `edge` D4 or D8, `graph` any int32 plane.  Edge rule, `stop` and terminals are
 * word for word those of soil_flow_paths above: cell n has an edge to r = graph[n] iff r is the index of one of its K
 * neighbours inside the model, anything else (INT32_MIN included) is no edge, and a cell with stop[n] != 0 has no
 * outgoing edge whatever its graph entry: it collects its catchment and passes nothing on.  `stop` may be NULL.
 *
 * Reach.  u reaches n iff n is u or lies on the walk from u along edges.  Cycles are allowed: a cell on a cycle is
 * reached by every cell of the cycle and by everything that drains into it.  No cell is special-cased, and nothing is
 * -1 or NaN because of a cycle.
 *
 * Order.  Values are compared by the integer key of csrc/erosion_quantiles.hip key_of, never as floats:
 *     -inf < ... < -0 < +0 < ... < +inf < NaN
 * with denormals kept as they are and every NaN, whatever its sign and payload, one key.
 *
 * op 0, min.  out[n] = the least value[u] over all u that reach n, its own bits.  A NaN is ignored wherever a number
 * reaches the cell; out[n] is NaN — the quiet NaN 0x7fc00000 whatever the payloads were — only where every value
 * that reaches n is NaN.
 * op 1, max.  out = -min(-value) under the same rule, negation being the exact flip of the sign bit: a NaN is again
 * ignored (and written as 0x7fc00000 where nothing else reaches the cell), and +0 wins over -0.
 * `arg` (int32): the index within the model of the cell that attains out[n]; among cells of equal key the smallest
 * index, for min and for max alike; -1 where out[n] is NaN.
 * Either of `out` and `arg` may be NULL, not both.
 *
 * The result is one definite bit pattern, fixed by the graph and the planes alone: min is idempotent and order-free,
 * so path, chunking, launch shape and run do not show.  ceil(log2(H * W)) pointer-doubling rounds over 4-byte
 * pointers and one plane of packed (key << 32 | index) words lowered by 64-bit atomic minima (csrc/upstream.hip, with
 * the proof of the round rule).
 *
 * Both entries are stream-ordered and do not synchronise (a call that finds its cached scratch too small
 * synchronises the device before replacing it, as everywhere); a host thread's calls on one device share one cached
 * scratch block of their own: issue them on ONE stream, or order the streams yourself.
 *
 * Batch form: the conventions of soil_flow_paths_batch.  Model-major planes; graph and `arg` entries are indices
 * WITHIN their model; nothing reaches another model; model b's slice of each output is bit for bit what the single
 * call gives for model b's slices alone.  Chunks of whole models by soil_flow_paths_batch's rule (as many as would
 * keep 16-byte records on 32-bit offsets, at most 65535, SOIL_FLOW_BATCH_CELLS lowers the cells of a chunk; a single
 * model above that is a chunk of its own on 64-bit offsets), and per chunk one init launch, the rounds of ONE model
 * and one final launch, whatever B is.
 *
 * Refused with SOIL_ERR_INVALID_ARGUMENT before any device work, with or without a device, the entry's name in
 * soil_last_error(): null `graph` or `value`, both outputs null, an output that aliases an input plane (or the other
 * output), B, H or W < 1, H * W > INT32_MAX, an invalid `edge`, `op` not 0 or 1.  Otherwise, without a device:
 * SOIL_ERR_NO_DEVICE. */
int soil_upstream_extreme(float* out, int32_t* arg, const int32_t* graph, const float* value, const int32_t* stop,
                          int64_t H, int64_t W, int edge, int op, void* stream);
int soil_upstream_extreme_batch(float* out, int32_t* arg, const int32_t* graph, const float* value,
                                const int32_t* stop, int64_t B, int64_t H, int64_t W, int edge, int op, void* stream);
/* What the calling host thread's last call of one of the two entries above did, as soil_flow_paths_info: info[0]
 * chunks, info[1] chunks whose init pass took the 16-byte form, info[2] chunks on 64-bit offsets (SOIL_PATHS_IDX64=1
 * forces them), info[3] rounds per chunk.  All zero before the first call; needs no device. */
int soil_upstream_extreme_info(int64_t info[4]);

/* ------------------------------------------------ flow graphs: stream order */

/* The channel network of a receiver graph: which cells are channels, the Strahler order of each, how many channel
 * cells drain straight into it, where the links (junction to junction) and the Strahler streams (order change to order
 * change) end, and the graph restricted to the channels.  Per-segment steepness, Horton ratios, order-based channel
 * masks and the `stop` planes of soil_flow_paths start from these.  The reference has no such call; the definition is
 * this library's.
 *
 * Grid (H, W), cell n = x * W + y, `edge` D4 or D8, `graph` any int32 plane.  The edge rule and `stop` are word for
 * word those of soil_flow_paths above: cell n has an edge to r = graph[n] iff r is the index of one of its K
 * neighbours inside the model, anything else (INT32_MIN included) is no edge, with D4 a diagonal entry is no edge, and
 * a cell with stop[n] != 0 has no outgoing edge whatever its graph entry.  `stop` may be NULL.
 *
 * Channel cells.  Cell n is a channel cell iff  (channel == NULL || channel[n] != 0)  and
 * (area == NULL || area[n] >= threshold),  a float32 comparison: a NaN area fails, +inf passes any threshold, -inf
 * only threshold -inf.  Both planes are optional; with neither every cell is a channel cell.  `threshold` is not read
 * without `area`.
 *
 * The channel graph.  The edge n -> r exists iff the edge rule gives it, stop[n] == 0, and n and r are BOTH channel
 * cells.  A non-channel cell is isolated; a stream that leaves the channels and enters them again is cut in two.
 * donors[n] is the number of channel-graph edges into n: 0 .. K, and 0 off the channels.
 *
 * Order, by levels.  Cycles are allowed and no cell is special-cased.
 *     M_1     = the channel cells
 *     J_k     = the cells of M_1 with at least two donors in M_k
 *     M_{k+1} = every cell that some cell of J_k reaches along the channel graph, that cell included
 *     order[n] = the largest k with n in M_k, and 0 off the channels.
 * (M_1 contains M_2 contains ...: by induction J_{k+1} lies in J_k.)  On a forest this is the Strahler number S: a
 * head (no donor) has S = 1; a cell has the greatest S among its donors, plus one where two or more donors share it.
 * Proof, by induction on k along the forest from the heads down, of  n in M_k iff S(n) >= k:  S(u) >= k + 1 iff two
 * donors have S >= k (they share the maximum k, or the maximum is above k anyway — then one donor has S >= k + 1) or
 * one donor has S >= k + 1; that is, iff two donors are in M_k (u in J_k) or one donor is in M_{k+1} (u is reached
 * from J_k through it) — the definition of M_{k+1}.  On a cycle the value is whatever the levels give: an isolated
 * cycle has order 1, and a cycle that a tree of order k drains into has order k + 1 at least all round — the cell where
 * the tree enters has two donors in M_k, the tree's foot and its own predecessor on the cycle.
 *
 * Foot planes (int32, 0 / 1), both 0 off the channels:
 *     link_foot[n]  = 1 iff n is a channel cell and has no channel-graph edge, or its receiver has donors >= 2:
 *                     a link ends just above a junction, or at an outlet of the channel graph.
 *     order_foot[n] = 1 iff n is a channel cell and has no channel-graph edge, or order[receiver] > order[n].
 * channel_graph[n] = graph[n] where the channel-graph edge n -> graph[n] exists, -1 elsewhere: the graph that
 * soil_accumulate, soil_flow_paths and the other calls take to stay inside the network.  soil_flow_paths on it with
 * a foot plane as `stop` gives every channel cell the foot of its link (its Strahler stream) and the way there; a
 * non-channel cell is its own terminal at distance 0.
 *
 * Every output may be NULL, not all of them.  The results are integers fixed by the definition: one bit pattern
 * under any schedule, chunking and launch shape.
 *
 * How (csrc/stream_order.hip, with the invariant and its proof): per level one gather pass that raises the cells of
 * J_k and one max-closure of ceil(log2(H * W)) pointer-doubling rounds with 32-bit atomic maxima, until a gather pass
 * raises nothing; the host looks at one pinned word per level, so BOTH ENTRIES SYNCHRONISE THE STREAM, once per
 * level (the fill does the same).  The levels are at most floor(log2(H * W)) + 1.  A host thread's calls on one
 * device share one cached scratch block of their own.
 *
 * Batch form: the conventions of soil_flow_paths_batch.  Model-major planes; graph and channel_graph entries are
 * indices WITHIN their model; `threshold` is one number for the batch; model b's slice of each output is bit for bit
 * what the single call gives for model b's slices alone.  Chunks of whole models by soil_flow_paths_batch's rule;
 * the models of a chunk iterate together, as many levels as the model that needs most.
 *
 * Refused with SOIL_ERR_INVALID_ARGUMENT before any device work, with or without a device, the entry's name in
 * soil_last_error(): null `graph`, no output asked for, an output that aliases an input plane or another output, B, H
 * or W < 1, H * W > INT32_MAX, an invalid `edge`, a NaN `threshold` with `area` given.  Otherwise, without a device:
 * SOIL_ERR_NO_DEVICE. */
int soil_stream_order(int32_t* order, int32_t* donors, int32_t* link_foot, int32_t* order_foot, int32_t* channel_graph,
                      const int32_t* graph, const int32_t* channel, const float* area, float threshold,
                      const int32_t* stop, int64_t H, int64_t W, int edge, void* stream);
int soil_stream_order_batch(int32_t* order, int32_t* donors, int32_t* link_foot, int32_t* order_foot,
                            int32_t* channel_graph, const int32_t* graph, const int32_t* channel, const float* area,
                            float threshold, const int32_t* stop, int64_t B, int64_t H, int64_t W, int edge,
                            void* stream);
/* What the calling host thread's last call of one of the two entries above did: info[0 .. 3] as
 * soil_upstream_extreme_info (chunks, chunks whose init pass took the 16-byte form, chunks on 64-bit offsets, rounds
 * per closure), info[4] the levels run: the gather passes, which is the greatest order found (1 where there is no
 * channel cell), the most over the models of the call; the closures run per chunk are one fewer, the last gather pass
 * having raised nothing.  All zero before the first call; needs no device. */
int soil_stream_order_info(int64_t info[5]);

/* ----------------------------------------- flow graphs: erosion-deposition */

/* The stream-power step with sediment deposition: the erosion-deposition (xi-q) model of Davy & Lague in the implicit
 * form of Yuan et al. (2019),
 *     dh/dt = u - K A^m S + (G / A) * Qs
 * where Qs is the net material removed from everything upstream.  It is soil_stream_power plus a deposition term fed
 * by an upstream sum: the first call that needs both soil_accumulate (up the graph) and soil_downstream (down it).
 * The reference has no such call (its example/dem_process.py names the steps in its comments); the definition is this
 * library's.
 *
 * Grid, edge rule, terminals, `scale`, L(n) and the rounds of the records are word for word those of
 * soil_stream_power.  There is no `stop` plane: soil_accumulate has none, and the two passes must see the same graph.
 *
 * All arithmetic is fp64 with one rounding per operation, in this order, with no contraction.  Per cell n that has an
 * edge of length L:
 *     F   = ((double)erosivity[n] * dt) / L
 *     g   = (double)deposition[n]
 *     d   = (1.0 + F) + g
 *     b   = (double)height[n] + dt * (double)uplift[n]      (double)height[n] with uplift == NULL
 *     B0  = F / d
 * A terminal keeps (double)height[n], as in soil_stream_power.  `deposition[n]` is G * (cell area) / A[n], made by the
 * caller as `erosivity` is, so that every operation in the kernels is correctly rounded and can be restated.
 *
 * The iterate starts at x^0 = b on the cells with an edge ((double)height[n] on a terminal).  For k = 1 .. iters:
 *     q[n]  = (float)(b - x^(k-1)[n])   rounded to nearest; +0 on a terminal and wherever that float is not finite
 *     Qs    = the bits soil_accumulate(graph, q, no decay) gives   (float32: the upstream sum, the cell itself included)
 *     Qup   = (double)Qs[n] - (double)q[n]
 *     A0    = (((1.0 + g) * b) + (g * Qup)) / d
 *     x^k   = the solve x[n] = A0 + B0 * x[r(n)] down the graph, with soil_downstream's rounds, bit for bit, a NaN and
 *             a cell that is not final after the last round kept as 0x7ff8000000000000
 * (in iteration 1 q is +0 everywhere, and zeros accumulate to +0).  The self-implicit term: the cell's own share of Qs
 * is taken at the new iterate, which is what (1 + g) and the + g in d are.  The plain fixed point with all of Qs from
 * the iterate before diverges for G >= 1 at a small dt; this form contracted in every case tried.
 * `iters` >= 1 is the caller's: a fixed count keeps the result one definite bit pattern, fixed by the graph, the
 * planes and the arguments alone; chunking, batching, lists, offsets and alignment do not show.
 *
 * With `deposition` all zeros the result is the bits of soil_stream_power (stop == NULL) at any `iters`: d is 1 + F,
 * (1.0 + 0.0) * b is b and b + 0 * Qup is b — for a finite Qup, and but for b == -0.0, which comes out as +0.0.
 *
 * Outputs.  At least one of `out` (float) and `out64` (double) is non-NULL: x^iters, with the NaN words of
 * soil_downstream.  `flux` (float32, may be NULL): soil_accumulate's bits for the q made from the returned iterate,
 * one more q pass and accumulation; at a terminal it is the sediment delivered to that base level.  `residual` (may
 * be NULL): a device array of B doubles (one for the single call); entry b is the maximum over the cells of model b of
 * |x^iters - x^(iters-1)|, one fp64 subtraction a cell, the cells where that is a NaN left out, 0 for a model without
 * any other.  The maximum is taken over the words of the non-negative doubles as integers: it is exact and has one
 * value.  Nothing synchronises; the caller reads the residual when it wants to judge convergence.  Qs is a float32
 * sum, so the iteration has a floor: the residual stops falling at about 2^-24 of the largest Qs times g / d.
 *
 * The entries are stream-ordered on the caller's stream from the first launch to the last.  A host thread's calls on
 * one device share cached scratch of their own (the records and lists of soil_stream_power, an accumulation's scratch
 * and 16 bytes a cell for the iterate, q and Qs): issue them on ONE stream, or order the streams yourself.  That
 * scratch is shared with soil_stream_power_deposit_n and its _batch form (below): the rule holds across both families.
 *
 * Batch form: the conventions of soil_stream_power_batch.  Model-major planes, 1 or B scale pairs, model b's slices
 * bit for bit what the single call gives, chunks of whole models (SOIL_FLOW_BATCH_CELLS lowers the cells of a chunk,
 * SOIL_PATHS_IDX64=1 forces 64-bit offsets), every iteration of a chunk before the next chunk.
 *
 * Refused with SOIL_ERR_INVALID_ARGUMENT before any device work, with or without a device, the entry's name in
 * soil_last_error(): what soil_stream_power refuses, a null `deposition`, iters < 1, `flux` or `residual` aliasing an
 * input plane, an output or each other.  Otherwise, without a device: SOIL_ERR_NO_DEVICE. */
int soil_stream_power_deposit(float* out, double* out64, float* flux, double* residual, const float* height,
                              const int32_t* graph, const float* erosivity, const float* deposition,
                              const float* uplift, int64_t H, int64_t W, int edge, const float scale[2], double dt,
                              int iters, void* stream);
int soil_stream_power_deposit_batch(float* out, double* out64, float* flux, double* residual, const float* height,
                                    const int32_t* graph, const float* erosivity, const float* deposition,
                                    const float* uplift, int64_t B, int64_t H, int64_t W, int edge,
                                    const float* scales, int64_t n_scales, double dt, int iters, void* stream);
/* What the calling host thread's last soil_stream_power_deposit or _batch call did: info[0] kernel launches, info[1]
 * chunks, info[2] iterations run, info[3] bytes of scratch the call asked for.  All zero before the first call; needs
 * no device. */
int soil_stream_power_deposit_info(int64_t info[4]);

/* ------------------------------------- flow graphs: slope exponents above 1 */

/* The implicit stream-power step with a slope exponent n >= 1,
 *     dh/dt = u - K A^m S^n
 * the general case of Braun & Willett's solver.  For n != 1 the implicit equation of a cell is not linear in the new
 * heights, so it is no affine map and the rounds of soil_stream_power cannot compose it.  Its Newton linearisation
 * about a given iterate is affine again,
 *     S^n ~ (1 - n) S_j^n + n S_j^(n-1) S
 *     h'[i] = (b + c) / (1 + F) + F / (1 + F) * h'[r],   F = n k dt S_j^(n-1) / L,   c = (n - 1) k dt S_j^n
 * so a Newton step on the whole triangular system is one solve of soil_stream_power's rounds with other coefficients.
 * The reference has no such call; the definition is this library's.
 *
 * Grid, edge rule, terminals, `stop`, `scale`, L(n), chunking, NaN words and the rounds of the records are word for
 * word those of soil_stream_power.  `erosivity` is K A^m, made by the caller; `uplift` and `stop` may be NULL.
 *
 * All arithmetic is fp64 with one rounding per operation, in this order, with no contraction.
 *     x^0 = the solve of soil_stream_power on the same arguments, in fp64: a NaN and a cell that is not final after the
 *           last round kept as 0x7ff8000000000000
 * For j = 1 .. iters, per cell i that has an edge to r of length L and is not stopped:
 *     d  = x[i] - x[r]                      (x = x^(j-1), the receiver's value a gather of 8 bytes)
 *     S  = d <= 0 ? 0.0 : d / L             (a NaN d falls through to d / L and stays NaN)
 *     P  = n == 2 ? S : pow(S, n - 1)       (n - 1 made once on the host; pow: see below)
 *     kd = (double)erosivity[i] * dt
 *     F  = ((n * kd) / L) * P
 *     c  = (kd * (n - 1)) * (P * S)
 *     b  = (double)height[i] + dt * (double)uplift[i]      (double)height[i] with uplift == NULL
 *     D  = 1.0 + F ;  A = (b + c) / D ;  B = F / D
 * A terminal or stopped cell has A = (double)height[i], B = 0, and is final.  Then
 *     x^j = the solve x[i] = A + B * x[r] down the graph, with soil_downstream's rounds, bit for bit
 * A cell whose receiver is not below it in the iterate takes no erosion in that step: S = 0 gives F = c = 0, so
 * x = b.  A NaN height reaches everything upstream of it, as it does at n = 1.
 *
 * The start is the n = 1 solve, not the old heights: the tangent of S^n at S = 0 is flat, so across a run of level
 * cells (a filled lake) information enters one cell per iteration, and from the old heights the iteration stalls
 * there.  From the n = 1 solve it converges in 8 to 16 iterations for K dt / L up to order 1; under a K dt / L of
 * order 100 with n >= 2 it can still stall across a long flat, and the residual says so.  `iters`
 * >= 1 is the caller's: a fixed count keeps the result one definite bit pattern, fixed by the graph, the planes and
 * the arguments alone; chunking, batching, lists, offsets and alignment do not show.
 *
 * pow is the device library's fp64 pow behind one inline device function: deterministic, not correctly rounded.
 * soil_selftest_math64 op 0 evaluates that very function, so a restatement that takes its powers from it is bit-exact
 * on every path.  n == 2 needs no power: P = S.
 *
 * n == 1.0 runs soil_stream_power's single solve and nothing else and gives its bits; the residual is 0 and the
 * info's iterations are 0.  n < 1 is out of scope on purpose: the per-cell function is then concave, a tangent step
 * from above overshoots to negative slopes, where the derivative is infinite, and that needs a safeguarded solve per
 * cell, which no affine map expresses.
 *
 * Outputs.  At least one of `out` (float) and `out64` (double) is non-NULL: x^iters, with the NaN words of
 * soil_downstream.  `residual` (may be NULL): a device array of B doubles (one for the single call); entry b is the
 * maximum over the cells of model b of |x^iters - x^(iters-1)|, one fp64 subtraction a cell, the cells where that is a
 * NaN left out, 0 for a model without any other; taken over the words of the non-negative doubles as integers, as
 * soil_stream_power_deposit takes it.  In every stalled case tried the residual was within a factor of about two of
 * the true error.  Nothing synchronises.
 *
 * The entries are stream-ordered on the caller's stream from the first launch to the last.  A host thread's calls on
 * one device share cached scratch of their own (the records, B planes and lists of soil_stream_power and 8 bytes a
 * cell for the iterate): issue them on ONE stream, or order the streams yourself.
 *
 * Batch form: the conventions of soil_stream_power_batch.  Model-major planes, 1 or B scale pairs, model b's slices
 * bit for bit what the single call gives, chunks of whole models (SOIL_FLOW_BATCH_CELLS lowers the cells of a chunk,
 * SOIL_PATHS_IDX64=1 forces 64-bit offsets), every iteration of a chunk before the next chunk.
 *
 * Refused with SOIL_ERR_INVALID_ARGUMENT before any device work, with or without a device, the entry's name in
 * soil_last_error(): what soil_stream_power refuses, an n that is not finite, n < 1 or n > 16, iters < 1, `residual`
 * aliasing an input plane or an output.  Otherwise, without a device: SOIL_ERR_NO_DEVICE. */
int soil_stream_power_n(float* out, double* out64, double* residual, const float* height, const int32_t* graph,
                        const float* erosivity, const float* uplift, const int32_t* stop, int64_t H, int64_t W,
                        int edge, const float scale[2], double dt, double n, int iters, void* stream);
int soil_stream_power_n_batch(float* out, double* out64, double* residual, const float* height, const int32_t* graph,
                              const float* erosivity, const float* uplift, const int32_t* stop, int64_t B, int64_t H,
                              int64_t W, int edge, const float* scales, int64_t n_scales, double dt, double n,
                              int iters, void* stream);
/* What the calling host thread's last soil_stream_power_n or _batch call did: info[0] kernel launches, info[1]
 * chunks, info[2] iterations run (0 for n == 1), info[3] bytes of scratch the call asked for.  All zero before the
 * first call; needs no device. */
int soil_stream_power_n_info(int64_t info[4]);
/* out[i] = op(a[i], b[i]) of the fp64 device functions the kernels share with the tests' restatements, on device
 * arrays of n doubles.  op 0: the slope power of soil_stream_power_n, pow(a, b) as its init pass evaluates it.  Any
 * other op, or a null array, is refused with SOIL_ERR_INVALID_ARGUMENT before any device work. */
int soil_selftest_math64(double* out, const double* a, const double* b, int64_t n, int op, void* stream);

/* ------------- flow graphs: erosion-deposition at slope exponents above 1 */

/* The stream-power step with sediment deposition and a slope exponent n >= 1,
 *     dh/dt = u - K A^m S^n + (G / A) * Qs
 * soil_stream_power_deposit and soil_stream_power_n in one step.  It is the Newton linearisation of the latter,
 *     S^n ~ (1 - n) S_j^n + n S_j^(n-1) S
 * put into the self-implicit equation of the former, x - b = -k dt S^n + g (Qup + b - x): one iteration renews the
 * tangent and the upstream sum together.  The reference has no such call; the definition is this library's.
 *
 * Grid, edge rule, terminals, `scale`, L(n), NaN words, chunking, the q pass, the accumulation and the rounds of the
 * records are word for word those of soil_stream_power_deposit.  There is no `stop` plane, as there.  The slope and
 * the power are soil_stream_power_n's, the n == 2 shortcut and the one inline pow that soil_selftest_math64 op 0
 * returns included.
 *
 * All arithmetic is fp64 with one rounding per operation, in this order, with no contraction.
 *     x^0 = the solve of soil_stream_power on the same arguments with stop == NULL, in fp64: soil_stream_power_n's
 *           start, for its reason (a filled lake)
 * For j = 1 .. iters, with x = x^(j-1), per cell i that has an edge to r of length L:
 *     q[i] = (float)(b - x[i])               rounded to nearest; +0 on a terminal and wherever that float is not finite
 *     Qs   = the bits soil_accumulate(graph, q, no decay) gives      (float32)
 *     Qup  = (double)Qs[i] - (double)q[i]
 *     d    = x[i] - x[r]                     (the receiver's value a gather of 8 bytes)
 *     S    = d <= 0 ? 0.0 : d / L            (a NaN d falls through to d / L and stays NaN)
 *     P    = n == 2 ? S : pow(S, n - 1)      (n - 1 made once on the host)
 *     kd   = (double)erosivity[i] * dt
 *     F    = ((n * kd) / L) * P
 *     c    = (kd * (n - 1)) * (P * S)
 *     g    = (double)deposition[i]
 *     b    = (double)height[i] + dt * (double)uplift[i]      (double)height[i] with uplift == NULL
 *     D    = (1.0 + F) + g
 *     A    = ((((1.0 + g) * b) + (g * Qup)) + c) / D ;   B = F / D
 *     x^j  = the solve x[i] = A + B * x[r] down the graph, with soil_downstream's rounds, bit for bit
 * A terminal has A = (double)height[i], B = 0, and is final.  Unlike the deposit step's first iteration, iteration 1
 * here has its q pass and accumulation: x^0 is not b.
 *
 * With `deposition` all zeros the result is the bits of soil_stream_power_n with stop == NULL at the same `iters`: D
 * is 1 + F, (1.0 + 0.0) * b is b and b + 0 * Qup is b — for a finite Qup, and but for b == -0.0, which comes out as
 * +0.0.  n == 1.0 runs soil_stream_power_deposit's iterations and nothing else and gives its bits: its start is
 * x^0 = b, not the solve.
 *
 * THE ITERATION HAS A DOMAIN.  No damping is added; the arithmetic above is the definition.  Measured on conditioned
 * noise terrains of 256^2 to 4096^2 cells with a deposition plane G (cell area) / A (DESIGN.md 3.5 has the map): with
 * K A^m dt / L up to order 1 and G <= 1 it contracts for n up to 3 and stops at the float32 floor of Qs (about 1e-9 of
 * the height range) after 12 to 35 iterations; with G = 2 it is slow at n = 1.5 and on some terrains diverges for
 * n >= 2.  With K A^m dt / L of order 100 it still contracts for G <= 1, but for n >= 2 it stalls across level runs as
 * soil_stream_power_n does, and it diverges for G = 2 at every n: the changes grow from iteration to iteration while
 * every value stays finite.  Outside the domain the residual grows with `iters` instead of falling, nothing else says
 * so, and the caller must read it.
 *
 * Outputs: `out`, `out64`, `flux` and `residual` are soil_stream_power_deposit's, word for word: x^iters; one more q
 * pass and accumulation from the returned iterate; the integer maximum of |x^iters - x^(iters-1)| per model.
 *
 * Stream order, cached scratch (shared with soil_stream_power_deposit: one stream for both, or order them yourself)
 * and the batch form are soil_stream_power_deposit's.
 *
 * Refused with SOIL_ERR_INVALID_ARGUMENT before any device work, with or without a device, the entry's name in
 * soil_last_error(): what soil_stream_power_deposit refuses (a null `deposition`, iters < 1 and its aliasing rules
 * among them) and an n that is not finite, n < 1 or n > 16.  Otherwise, without a device: SOIL_ERR_NO_DEVICE. */
int soil_stream_power_deposit_n(float* out, double* out64, float* flux, double* residual, const float* height,
                                const int32_t* graph, const float* erosivity, const float* deposition,
                                const float* uplift, int64_t H, int64_t W, int edge, const float scale[2], double dt,
                                double n, int iters, void* stream);
int soil_stream_power_deposit_n_batch(float* out, double* out64, float* flux, double* residual, const float* height,
                                      const int32_t* graph, const float* erosivity, const float* deposition,
                                      const float* uplift, int64_t B, int64_t H, int64_t W, int edge,
                                      const float* scales, int64_t n_scales, double dt, double n, int iters,
                                      void* stream);
/* What the calling host thread's last soil_stream_power_deposit_n or _batch call did: info[0] kernel launches, info[1]
 * chunks, info[2] iterations run, info[3] bytes of scratch the call asked for.  All zero before the first call; needs
 * no device. */
int soil_stream_power_deposit_n_info(int64_t info[4]);

/* ------------------------------------------------------ hillslope diffusion */

/* One implicit step of dh/dt = div(kappa grad h) + u on a grid: the hillslope half of a landscape-evolution step, beside
 * soil_stream_power's channel half.  The reference has no such call (its example/dem_process.py carries a commented-out
 * explicit diffuse() of laplacian + multiply + add, stable only for kappa dt / s^2 <= 1/4); the definition is this
 * library's.
 *
 * The step is locally one-dimensional backward Euler: one implicit sweep along `first_axis` (0 or 1), then one along
 * the other axis.  It is unconditionally stable and first order in time; each sweep is an M-matrix solve, so the step
 * obeys the maximum principle (without uplift no free cell leaves the range of the non-void heights).  It is NOT
 * Peaceman-Rachford: that scheme's explicit half steps give up positivity for second order, and at the large dt this
 * is used with (the dt of a stream-power step) positivity is worth more than second order.
 *
 * Grid (H, W), cell n = x * W + y.  `scale` = (sx, sy), the spacings along axis 0 and axis 1 as in soil_flow_paths:
 * the floats widened to double, ss = s * s made once on the host in double (ss = sx * sx for the sweep along axis 0).
 *
 * Cell kinds.  A cell is void if height[n] is NaN.  It is fixed if fixed[n] != 0 (`fixed` may be NULL), or if it
 * lies on the outermost row or column and border == 1.  Any other cell is free.
 *
 * One sweep, for one line of cells 0 .. n-1 (a column for axis 0, a row for axis 1) with right-hand side d, in fp64:
 * cells i and i+1 are linked iff neither is void.  The weight of the face between them is
 *     w = (kf * dt) / ss            the product rounded, then the quotient
 * with kf = kappa where `diffusivity` is NULL, else kf = 0.5 * ((double)k[i] + (double)k[i+1]).  Then
 *     p_i = w_{i-1/2} if i is free and linked to i-1, else +0.0
 *     q_i = w_{i+1/2} if i is free and linked to i+1, else +0.0
 *     b_i = (1.0 + p_i) + q_i
 * Forward, i ascending: if i is free and linked to i-1
 *     den = b_i - p_i * g_{i-1},  e_i = (d_i + p_i * e_{i-1}) / den
 * otherwise den = b_i, e_i = d_i / den; in both cases g_i = q_i / den.  Backward, i descending:
 *     x_i = e_i + g_i * x_{i+1} if i is free and linked to i+1, else x_i = e_i
 * Every operation is fp64, rounded once, with no contraction (__dmul_rn, __dadd_rn, __dsub_rn, __ddiv_rn; a product
 * is rounded before the sum or difference it enters).  The selects are by predicate: a void neighbour's NaN is never
 * multiplied by zero.
 *
 * The first sweep's d is (double)height[n]; on a free cell with an `uplift` plane it is
 * (double)height[n] + dt * (double)uplift[n], soil_stream_power's expression.  The second sweep's d is the first
 * sweep's x, unrounded.  A fixed cell therefore comes out as exactly (double)height[n] and a void cell as NaN.
 * out64[n] = x, out[n] = (float)x rounded to nearest (at least one of the two is non-NULL); any NaN is written as
 * 0x7fc00000 / 0x7ff8000000000000, the words soil_downstream writes.  +-inf heights and negative, zero or NaN
 * diffusivities are used as they are and give what the arithmetic gives (dt == 0 or kappa == 0 gives the heights
 * back, except that a free, linked cell holding -0.0 comes out as +0.0: -0.0 + 0.0 * e, and that an infinite
 * neighbour makes 0 * inf).
 *
 * The result is one definite bit pattern, fixed by the planes and the arguments alone: tiling, chunking, batching,
 * offset width and alignment do not show.
 *
 * `scale` / `scales` (n_scales pairs, 1 or B) are HOST arrays read before the call returns.  The entries are
 * stream-ordered and do not synchronise (a call that finds its cached scratch too small synchronises the device
 * before replacing it, as everywhere); a host thread's calls on one device share one cached scratch block of their
 * own, 40 bytes a cell of a chunk (16 bytes a cell of e and g, x replacing e in place, and the transposed planes of the
 * sweep along axis 1): issue them on ONE stream, or order the streams yourself.
 *
 * Batch form: the conventions of soil_stream_power_batch.  Model-major planes; model b's slice of each output is bit
 * for bit what the single call gives for model b's slices alone, with scales[b] or the one pair; nothing reaches
 * another model.  Chunks of whole models, at most 65535 and at most 2^28 - 1 cells, SOIL_FLOW_BATCH_CELLS lowers the
 * cells of a chunk; a model of 2^29 cells or more runs on 64-bit offsets (SOIL_PATHS_IDX64=1 forces them).  Per chunk
 * five launches (first_axis == 0) or four, whatever B is.
 *
 * Refused with SOIL_ERR_INVALID_ARGUMENT before any device work, with or without a device, the entry's name in
 * soil_last_error(): null `height`, both outputs null, an output that aliases an input plane (or the other output),
 * null `scale`, B, H or W < 1, H * W > INT32_MAX, n_scales not 1 or B, a scale entry that is not a positive finite
 * float, a `dt` that is negative or not finite, a `kappa` that is negative or not finite while `diffusivity` is NULL
 * (with a plane kappa is not read), `border` not 0 / 1, `first_axis` not 0 / 1.  Otherwise, without a device:
 * SOIL_ERR_NO_DEVICE. */
int soil_diffuse(float* out, double* out64, const float* height, const float* diffusivity, const float* uplift,
                 const int32_t* fixed, int64_t H, int64_t W, const float scale[2], double kappa, double dt,
                 int border, int first_axis, void* stream);
int soil_diffuse_batch(float* out, double* out64, const float* height, const float* diffusivity, const float* uplift,
                       const int32_t* fixed, int64_t B, int64_t H, int64_t W, const float* scales, int64_t n_scales,
                       double kappa, double dt, int border, int first_axis, void* stream);
/* What the calling host thread's last soil_diffuse or soil_diffuse_batch call did: info[0] kernel launches, info[1]
 * chunks, info[2] chunks on 64-bit offsets, info[3] bytes of scratch the call asked for.  All zero before the first
 * call; needs no device. */
int soil_diffuse_info(int64_t info[4]);

/* ------------------------------------------------ flow graphs: conditioning */

/* Routing across flats and filled lakes.  soil_fill_depressions returns a surface on which every lake is level, and
 * on a level surface soil_steepest and soil_random_weighted give no receiver (-1 unless a slope is positive): every
 * cell of a filled lake is a terminal.  The two calls below give such cells receivers, as int32 indices — nothing is
 * added to the heights.  The reference leaves this step to pysheds too (example/dem_condition.py:35-41,
 * resolve_flats); the definition is this library's.
 *
 * Grid (H, W), cell n = x * W + y, `edge` D4 or D8, the neighbours in the order of the graph calls' tables
 * (dx, dy) = (-1,0) (0,-1) (0,1) (1,0) (-1,-1) (-1,1) (1,-1) (1,1), the first four for D4.  Heights are compared as
 * floats: -0 == +0, inf == inf, NaN equals nothing.
 *
 * Seed.  A non-NaN cell c is a seed if some neighbour position lies off the grid, or a neighbour is NaN (the two
 * are the fill's outlet rule), or a neighbour in the grid is strictly lower, h[nb] < h[c].
 *
 * Flat distance.  dist[c] = 0 for a seed; otherwise dist[c] = 1 + min dist[nb] over the neighbours in the grid with
 * h[nb] == h[c] and dist[nb] >= 0; dist[c] = -1 where no such chain reaches a seed (a closed depression, a single
 * pit) and for NaN cells.  This is the shortest-path distance inside the flat.  It is the only fixed point that can
 * be reached from "seeds 0, everything else unknown" by updates d(c) <- min(d(c), 1 + d(nb)) that only lower a value:
 * a value is always the length of a walk from a seed, so it never falls below the distance, and where no update
 * lowers anything any more every shortest path has been followed.  An iteration in any order therefore ends on the
 * same integers (csrc/flats.hip: 64 x 64 tiles relaxed in LDS, launches repeated until no tile moved;
 * SOIL_FLATS_PER_CHECK launches per look at the "changed" word).
 *
 * Flat receivers.  out[n] = in[n], except where in[n] < 0 and dist[n] > 0: there out[n] is the index of the first
 * neighbour k in table order that lies in the grid, has h[nb] == h[n] and dist[nb] == dist[n] - 1.  If no neighbour
 * qualifies (a dist that does not belong to this height), out[n] stays in[n].  out == in is allowed: a cell reads
 * only its own graph entry.  Guarantee: if every edge of `in` goes strictly downhill (every graph soil_steepest and
 * soil_random_weighted make), `out` is acyclic — along an edge the height never rises, and where it stays, dist
 * falls by one.  On a surface soil_fill_depressions made, every terminal of `out` is a cell on the grid's border or
 * beside a NaN cell.
 *
 * soil_flat_distance and soil_flat_distance_batch synchronise the stream before they return, as
 * soil_fill_depressions does (the host decides after every few launches whether another is needed).
 * soil_flat_receivers and soil_flat_receivers_batch are stream-ordered and do not synchronise.
 *
 * Batch form: model-major planes; entries of `in`, `out` are indices WITHIN their model; model b's slice is bit for
 * bit what the single-grid call gives for model b's slices alone (a model's first cell is addressed in int64).  The
 * models of a batch relax side by side: the launches of a batch are those of the model that needs most, not the sum.
 *
 * Refused with SOIL_ERR_INVALID_ARGUMENT before any device work, with or without a device, the entry's name in
 * soil_last_error(): a null pointer, B, H or W < 1, H * W > INT32_MAX, an invalid `edge`.  Otherwise, without a
 * device: SOIL_ERR_NO_DEVICE. */
int soil_flat_distance(int32_t* dist, const float* height, int64_t H, int64_t W, int edge, void* stream);
int soil_flat_distance_batch(int32_t* dist, const float* height, int64_t B, int64_t H, int64_t W, int edge,
                             void* stream);
int soil_flat_receivers(int32_t* out, const int32_t* in, const float* height, const int32_t* dist, int64_t H,
                        int64_t W, int edge, void* stream);
int soil_flat_receivers_batch(int32_t* out, const int32_t* in, const float* height, const int32_t* dist, int64_t B,
                              int64_t H, int64_t W, int edge, void* stream);
/* What the calling host thread's last call of soil_flat_distance or soil_flat_distance_batch did: info[0] relaxation
 * launches, info[1] tiles of a model, info[2] models, info[3] looks at the "changed" word.  All zero before the
 * first call; needs no device. */
int soil_flat_distance_info(int64_t info[4]);

/* Threshold hillslopes: the slope-limited surface of a DEM.  No cell may stand higher above a neighbour than a
 * critical slope times the distance allows; what stands above that surface is the excess topography, the unstable
 * mass above a threshold angle.  Not in the reference (its particle model has one explicit creep step per erosion
 * step, critSlopeBedrock); the definition is this library's.
 *
 * Grid (H, W), cell n = x * W + y, `edge` D4 or D8 with the neighbour table above.  The step length L_k toward
 * neighbour k is the fp64 length soil_flow_paths uses for that kind of edge: sx = (double)scale[0] for a row step
 * (dx != 0, dy == 0), sy = (double)scale[1] for a column step, sqrt(sx sx + sy sy) for a diagonal one.
 *
 * out = the greatest surface w <= height with
 *        w[n] <= w[k] (+) c_k[n]    for every neighbour k of n in the grid,
 * where c_k[n] = (float)((double)slope[n] * L_k), one fp64 product rounded once to fp32, and (+) is one fp32 addition,
 * round to nearest, denormals kept.  slope[n] is `slope_plane[n]` if a plane is given (lithology), the scalar `slope`
 * otherwise; the slope that binds an edge is the slope of the cell being lowered.  It is the fixed point that
 *        w[n] <- cand   if cand < w[n],   cand = w[k] (+) c_k[n]
 * reaches from w = height in any order of updates: the operator is monotone (round to nearest is), it only lowers
 * values, so every chaotic iteration stays on or above the greatest fixed point below height and ends on a fixed
 * point, that one; it ends because the floats between the least height and the heights are a finite set and c >= 0
 * (csrc/slope_limit.hip: 64 x 64 tiles relaxed in LDS, launches repeated until no tile moved;
 * SOIL_SLOPE_LIMIT_PER_CHECK launches per look at the "changed" word).  The rules that make it one bit pattern:
 *   - strict <: a tie keeps the bits the cell has (a -0 that is not lowered stays -0);
 *   - c is never -0: a product that is zero counts as +0, a scalar slope of -0 as 0;
 *   - a NaN height is a void: never lowered, lowering nobody, NaN in the result; a position off the grid binds nothing;
 *   - a slope_plane entry that is not >= 0 (NaN, negative) means "no limit at this cell": the cell keeps its height
 *     and still binds its neighbours; an entry of +inf does the same by arithmetic alone (c = +inf);
 *   - +-inf heights go through the arithmetic as they are: a -inf cell pulls every cell connected to it by finite
 *     steps to -inf, a +inf cell comes down to its lowest neighbour plus a step;
 *   - a slope of 0 levels every connected component to its minimum.
 * `excess` (may be NULL): height (-) out, one fp32 subtraction, +0 where the cell was not lowered, the height's NaN
 * on voids.
 *
 * Both calls synchronise the stream before they return, as soil_fill_depressions does.  Batch form: model-major
 * planes, `scales` one pair or B pairs (host), model b's slice bit for bit what the single call gives for it alone (a
 * model's first cell is addressed in int64).  The models relax side by side under one "changed" word: the launches of
 * a batch are those of the model that needs most.  The batch is never cut into chunks.  The launches of a call never
 * exceed tiles * 272 + 2 plus the launches of one look (csrc/slope_limit.hip derives it).
 *
 * Refused with SOIL_ERR_INVALID_ARGUMENT before any device work, with or without a device, the entry's name in
 * soil_last_error(): null `out` or `height`; a null scale; B, H or W < 1; H * W > INT32_MAX; n_scales not 1 or B; an
 * invalid `edge`; an output that shares a byte with `height`, `slope_plane` or the other output; a scale that is not
 * positive and finite; with a NULL slope_plane a `slope` that is negative or not finite (with a plane the scalar is
 * not read).  Otherwise, without a device: SOIL_ERR_NO_DEVICE. */
int soil_slope_limit(float* out, float* excess, const float* height, const float* slope_plane, double slope,
                     int64_t H, int64_t W, const float scale[2], int edge, void* stream);
int soil_slope_limit_batch(float* out, float* excess, const float* height, const float* slope_plane, double slope,
                           int64_t B, int64_t H, int64_t W, const float* scales, int64_t n_scales, int edge,
                           void* stream);
/* What the calling host thread's last call of soil_slope_limit or soil_slope_limit_batch did: info[0] relaxation
 * launches, info[1] tiles of a model, info[2] models, info[3] looks at the "changed" word.  All zero before the
 * first call; needs no device. */
int soil_slope_limit_info(int64_t info[4]);

/* ---- flow graphs: exact multiple-flow accumulation (not in the reference, whose multiple-flow product is the
 * Monte-Carlo mean of example/dem_multiflow.py: K random_weighted graphs, accumulated and averaged; soil_multiflow) ----
 *
 * Every cell of a random_weighted graph draws its receiver independently and every edge goes strictly downhill, so the
 * expectation of the accumulation is the solution of the sparse triangular system
 *        a[n] = source[n] + sum over donors d of w(d -> n) a[d],
 * w(d -> n) the Gibbs share random_weighted gives neighbour n of d.  soil_mfd_weights writes the shares,
 * soil_mfd_accumulate solves the system (csrc/mfd.hip: 64 x 64 tiles of doubles relaxed in LDS, launches repeated
 * until no tile moved; SOIL_MFD_PER_CHECK launches per look at the "changed" word).  With kind power the same system
 * is the deterministic multiple-flow (MFD) accumulation of Freeman, Quinn and Holmgren.
 *
 * Grid (H, W), cell n = x * W + y, `edge` D4 or D8 (K = 4 or 8) with the neighbour table above, as in the graph calls.
 *
 * Raw weight of cell n towards neighbour k.  diff = h[n] (-) h[k], one fp32 subtraction.  P_k = 0 where the neighbour
 * is off the grid or diff <= 0.  A NaN diff is not <= 0: the weight is NaN, for both kinds.  Otherwise
 *   - kind SOIL_MFD_GIBBS, param the temperature T: P_k = rw_exp2(diff, c_k) with the constants rw_const((float)T)
 *     (csrc/soil_math.hpp) — the weight function and the constants of soil_random_weighted, the same inline functions;
 *     soil_selftest_math op 12.  T obeys the rule of soil_random_weighted: as a float it is 0 or a normal positive
 *     number.  T = 0 makes every cell a terminal, as random_weighted does.  No scale is read.
 *   - kind SOIL_MFD_POWER, param the exponent p, finite, 0 <= p <= 16: P_k = (float) sp_pow((double)diff / L_k, p), one
 *     fp64 division, the inline pow of csrc/soil_math.hpp (soil_selftest_math64 op 0), one rounding to fp32.  L_k is
 *     the fp64 step length of soil_flow_paths: sx = (double)scale[0] for a row step (dx != 0, dy == 0), sy =
 *     (double)scale[1] for a column step, sqrt(sx sx + sy sy) for a diagonal one.  (pow(NaN, 0) is 1; the NaN diff is
 *     tested for itself, or two NaN cells would feed each other.)
 * Partition sum.  Z = ((P_0 + P_1) + ...) in fp32, in table order, as random_weighted sums it.
 * Sending.  A cell sends iff Z is finite and > 0 — exactly the cells where random_weighted can pick a receiver.  Its
 * share towards k is w_k = P_k / Z, one IEEE fp32 division.  Every other cell is a terminal with all shares 0.
 * Flats (`dist`, may be NULL: int32, as soil_flat_distance makes it).  A cell that does not send, with Z == 0 and
 * dist[n] > 0, sends share 1.0 to the first neighbour in table order that lies in the grid, has h[k] == h[n] and
 * dist[k] == dist[n] - 1: the rule of soil_flat_receivers.  Every edge strictly lowers the pair (height, dist), so the
 * graph of the non-zero shares is acyclic for any content of `dist`.
 *
 * soil_mfd_weights: weights[k * H * W + n] = w_k of cell n, planar (K, H, W) float32; batch (B, K, H, W).
 * Stream-ordered, nothing synchronises.
 *
 * Accumulation, in fp64.  s = (double)source[n] (`source` NULL: 1).  For k in table order: where neighbour k is in the
 * grid and its share w towards n is non-zero, s = s + a[k] * (double)w — one rounded product and one rounded sum, no
 * contraction.  A zero share is skipped, so an infinite a[k] never makes inf * 0.  a[n] = s, a NaN stored as the
 * canonical quiet NaN.  On a DAG this is one fixed expression of the donors' final values a cell: the result does not
 * depend on the schedule.  out64 (may be NULL) = a; out (may be NULL) = a rounded once to float; at least one is given.
 * Terminals keep what arrived: with a unit source their values sum to H * W, up to rounding.
 *
 * soil_mfd_accumulate(_batch) synchronise the stream before they return, as soil_slope_limit does.  Batch form:
 * model-major planes, `scales` one pair or B pairs (host; read by kind power only), model b's slice bit for bit what the
 * single call gives for it alone (a model's first cell is addressed in int64).  The models relax side by side under
 * one "changed" word; the batch is never cut into chunks, B above 65535 included.  The launches of a call never exceed
 * tiles * 272 + 2 plus the launches of one look (csrc/mfd.hip derives it from the longest chain of donors); reaching
 * that is an internal error (SOIL_ERR_HIP), never a property of the input.
 *
 * Refused with SOIL_ERR_INVALID_ARGUMENT before any device work, with or without a device, the entry's name in
 * soil_last_error(): a null `height` (or `weights`); both outputs null; B, H or W < 1; H * W > INT32_MAX; n_scales not 1
 * or B; an invalid `edge` or `kind`; a T that soil_random_weighted refuses, a p that is not in 0 .. 16; kind power with
 * a null scale or one that is not positive and finite; an output that shares a byte with `height`, `source`, `dist`
 * or the other output.  Otherwise, without a device: SOIL_ERR_NO_DEVICE. */
typedef enum soil_mfd_kind { SOIL_MFD_GIBBS = 0, SOIL_MFD_POWER = 1 } soil_mfd_kind;
int soil_mfd_weights(float* weights, const float* height, const int32_t* dist, int kind, double param, int64_t H,
                     int64_t W, const float scale[2], int edge, void* stream);
int soil_mfd_weights_batch(float* weights, const float* height, const int32_t* dist, int kind, double param, int64_t B,
                           int64_t H, int64_t W, const float* scales, int64_t n_scales, int edge, void* stream);
int soil_mfd_accumulate(float* out, double* out64, const float* height, const float* source, const int32_t* dist,
                        int kind, double param, int64_t H, int64_t W, const float scale[2], int edge, void* stream);
int soil_mfd_accumulate_batch(float* out, double* out64, const float* height, const float* source, const int32_t* dist,
                              int kind, double param, int64_t B, int64_t H, int64_t W, const float* scales,
                              int64_t n_scales, int edge, void* stream);
/* What the calling host thread's last call of soil_mfd_accumulate or soil_mfd_accumulate_batch did: info[0] relaxation
 * launches, info[1] tiles of a model, info[2] models, info[3] looks at the "changed" word.  All zero before the first
 * call; needs no device. */
int soil_mfd_info(int64_t info[4]);

/* ---------------------------------------------------------------- stencils */

/* soil::gradient — grad.hpp:11, grad.cu:89-97 (__gradient :22-87), model.cpp:193-195.  out (H,W,2). */
int soil_gradient(float* out, const float* in, int64_t H, int64_t W, const float scale[2],
                  void* stream);
/* soil::negslope — grad.hpp:17, grad.cu:133-141 (__negslope :101-131), model.cpp:201-203. */
int soil_negslope(float* out, const float* in, int64_t H, int64_t W, const float scale[2],
                  void* stream);
/* soil::laplacian — grad.hpp:14, grad.cu:186-206 (__laplacian<D> :147-183), model.cpp:197-199.
 * in/out (H,W,D), D in {1,2}. */
int soil_laplacian(float* out, const float* in, int64_t H, int64_t W, int D,
                   const float scale[2], void* stream);
/* soil::gaussian_blur — filter.hpp:11, filter.cu:72-91 (__blur :59-70,
 * __gaussian_blur :24-56), model.cpp:189-191.  tensor (H,W,C), C in {1,2}, is
 * blurred IN PLACE (the reference returns its input handle, filter.cu:90);
 * scratch (H,W,C) is the intermediate of the axis-0 pass. */
int soil_gaussian_blur(float* tensor, float* scratch, int64_t H, int64_t W, int C, float sigma,
                       void* stream);
/* soil::op::normal — normal.hpp:19-39 (CPU loop in the reference; unbound in
 * its module, used by example/tiff_normal.py:14).  out (H,W,3). */
int soil_normal(float* out, const float* in, int64_t H, int64_t W, const float scale[3],
                void* stream);
/* Host twin of soil_normal for CPU tensors (the reference's only placement). */
int soil_normal_host(float* out_host, const float* in_host, int64_t H, int64_t W,
                     const float scale[3]);

/* -------------------------------------------------------- path-integral MC */

/* soil::solve_uniform — path.hpp:30-37, path.cu:180-219 (__solve_uniform<K>
 * :52-139, __normalize<K> :142-170; bilinear gather sample.hpp:154-186),
 * model.cpp:209-227.  flow (H,W,2), source/flux (H,W,K), K in {1,2}, decay
 * (H,W), rng [N].  flux is zeroed, filled and normalised; synchronises. */
int soil_solve_uniform(float* flux, const float* flow, const float* source, const float* decay,
                       soil_rng* rng, int64_t N, int64_t H, int64_t W, int K,
                       const float scale[2], uint64_t count, void* stream);

/* ------------------------------------------------------------------- noise */

/* soil::noise_param_t / soil::noise — noise.hpp:14-56, model.cpp:413-421:
 * OpenSimplex2 FBm, 3-D sample at (x/ext0, y/ext1, seed). */
typedef struct soil_noise_param {
  float frequency;  /* noise.hpp:29, default 1    */
  int32_t octaves;  /* :30, default 8             */
  float gain;       /* :31, default 0.6           */
  float lacunarity; /* :32, default 2             */
  float seed;       /* :33, default 0 (z coord)   */
  float ext[2];     /* :34, default {512, 512}    */
} soil_noise_param;
void soil_noise_param_default(soil_noise_param* p);
/* Device generator (bench inputs at 8192^2+) and host twin (the reference's
 * placement, noise.hpp:49-52); both produce identical bits. */
int soil_noise(float* out, int64_t H, int64_t W, const soil_noise_param* p, void* stream);
int soil_noise_host(float* out_host, int64_t H, int64_t W, const soil_noise_param* p);
/* Rows [x0, x0+rows) of the same heightmap (the slab a rank owns). */
int soil_noise_window(float* out, int64_t rows, int64_t W, int64_t x0, const soil_noise_param* p,
                      void* stream);

/* ------------------------------------------------------ multiscale driver */
/* soil.resize(dst, src, newres, oldres) of example/erosion_gpu_multiscale.py:104-141
 * (SURVEY.md 8f row 4).  The reference snapshot has no definition of it; this
 * one is bilinear resampling at corner-aligned positions (equal resolutions give
 * the identity, corners are kept), for planes of D = 1..3 interleaved channels.
 * Parity unpinned. */
int soil_resize(float* dst, const float* src, int64_t Hn, int64_t Wn, int64_t Ho, int64_t Wo, int D,
                void* stream);

/* ------------------------------------------------------- TIFF / GeoTIFF IO */
/* Host-side file IO of the callers either side of the path:
 * soil::io::tiff (io/tiff.hpp:20-241) and soil::io::geotiff (io/geotiff.hpp:63-318),
 * bound in python/source/io.cpp:20-100.  The reference delegates the format to
 * libtiff (third party, not in its tree); this is a codec of its own for
 * single-band rasters: classic + BigTIFF, either byte order, strips or tiles,
 * compression none / LZW / Deflate / PackBits, predictors 1-3.  No GPU needed. */
#define SOIL_TIFFTAG_GEOPIXELSCALE 33550   /* geotiff.hpp:13-21 */
#define SOIL_TIFFTAG_GEOTIEPOINTS 33922
#define SOIL_TIFFTAG_GEOKEYDIRECTORY 34735
#define SOIL_TIFFTAG_GEODOUBLEPARAMS 34736
#define SOIL_TIFFTAG_GEOASCIIPARAMS 34737
#define SOIL_TIFFTAG_GDAL_METADATA 42112
#define SOIL_TIFFTAG_GDAL_NODATA 42113

typedef struct soil_tiff_info { /* what tiff::peek / geotiff::peek learn (tiff.hpp:69-99) */
  uint32_t width, height;       /* ImageWidth, ImageLength                          */
  uint32_t bits;                /* BitsPerSample                                    */
  uint32_t sample_format;       /* 1 unsigned, 2 signed, 3 IEEE float               */
  uint32_t samples;             /* SamplesPerPixel                                  */
  uint32_t tiled, tile_width, tile_height;
  uint32_t compression, predictor;
  /* element counts of the GeoTIFF / GDAL tags present (0 = absent), for soil_tiff_tag */
  uint32_t n_scale, n_tiepoints, n_params, n_keydir, n_ascii, n_metadata, n_nodata;
} soil_tiff_info;

typedef struct soil_geotiff_tags { /* geotiff::meta_t as written by geotiff::write (:199-213) */
  const double* scale;     uint32_t n_scale;      /* GeoPixelScale   */
  const double* tiepoints; uint32_t n_tiepoints;  /* GeoTiePoints    */
  const double* params;    uint32_t n_params;     /* GeoDoubleParams */
  const int16_t* keydir;   uint32_t n_keydir;     /* GeoKeyDirectory */
  const char* ascii;       /* GeoAsciiParams, NUL-terminated or NULL */
  const char* metadata;    /* GDAL_METADATA                          */
  const char* nodata;      /* GDAL_NODATA                            */
} soil_geotiff_tags;

/* tiff::peek + geotiff::peek: SOIL_ERR_IO when the file is missing (the
 * reference throws silt::error::missing_file) or is not a TIFF. */
int soil_tiff_peek(const char* filename, soil_tiff_info* info);
/* Payload of one tag: doubles (8 B each), shorts (2 B) or the raw bytes of an
 * ASCII tag including its NUL.  *written_bytes = 0 when the tag is absent. */
int soil_tiff_tag(const char* filename, int tag, void* dst, uint64_t capacity_bytes,
                  uint64_t* written_bytes);
/* tiff::read (tiff.hpp:102-213): width*height samples in scanline order into
 * `dst`: float64 when the file holds 64-bit samples, float32 otherwise
 * (tiff.hpp:116-124).  Integer and half-float samples are converted to
 * float32 (the reference leaves the 16-bit case unfilled). */
int soil_tiff_read(const char* filename, void* dst, uint64_t dst_bytes);
/* tiff::write / geotiff::write (tiff.hpp:215-241, geotiff.hpp:183-226):
 * uncompressed little-endian IEEE-float strips, ROWSPERSTRIP = width (what
 * TIFFDefaultStripSize(tif, width) returns); `geo` may be NULL.  Images beyond
 * 4 GiB are written as BigTIFF (libtiff would fail). */
int soil_tiff_write(const char* filename, const void* data, uint32_t width, uint32_t height,
                    uint32_t bits, const soil_geotiff_tags* geo);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* SOIL_HIP_H */
