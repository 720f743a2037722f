// particles_common.hpp — pieces shared by the particle-transport launch shapes
// (erosion_particles.hip: direct / staged; erosion_particles_tiled.hip: tiled).
#pragma once

#include "cell_math.hpp"

namespace soil {

__device__ __forceinline__ bool oob(const Dom& d, float px, float py) {  // erosion_map.cu:29-40
  if (px < 0) return true;
  if (py < 0) return true;
  if (px >= static_cast<float>(d.H)) return true;
  if (py >= static_cast<float>(d.W)) return true;
  return false;
}

// local rows whose 5-point stencil lies inside the rows this slab holds
__device__ __host__ __forceinline__ int64_t stencil_lo(const Dom& d) { return (d.x0 == 0) ? 0 : 1; }
__device__ __host__ __forceinline__ int64_t stencil_hi(const Dom& d) {  // inclusive
  return (d.x0 + d.rows == d.H) ? d.rows - 1 : d.rows - 2;
}
// A slab traces a particle only while its cell's stencil is available
// (soil_hip.h, soil_particles_*_slab).
__device__ __forceinline__ bool slab_escape(const Dom& d, int64_t gx) {
  const int64_t lx = gx - d.x0;
  return lx < stencil_lo(d) || lx > stencil_hi(d);
}

__device__ __forceinline__ bool owns_spawn(const Dom& d, float px) {
  const int64_t sx = cell_of(px) - d.x0;
  return sx >= d.r0 && sx < d.r1;
}
// first two draws of particle n: spawn position (erosion.cu:56-59 / :269-272).  The row
// decides who traces the particle: a slab that does not own it (7 of 8 streams on an
// 8-GPU run) leaves the second draw out — the stream still moves on by two.
__device__ __forceinline__ float2 spawn_position(soil_rng* __restrict__ rng, int64_t n,
                                                 const Dom& d) {
  soil_rng st = rng[n];
  const float u1 = rng_uniform_at(st.seed, static_cast<uint64_t>(n), st.offset);
  const float x = 0.5f + u1 * static_cast<float>(d.H - 1);
  float y = 0.0f;
  if (owns_spawn(d, x))
    y = 0.5f + rng_uniform_at(st.seed, static_cast<uint64_t>(n), st.offset + 1) * static_cast<float>(d.W - 1);
  st.offset += 2;
  rng[n] = st;  // the state persists in the tensor, like curandState
  return make_float2(x, y);
}

// Where a launch's streams of draws come from.  The reference keeps one generator state per particle
// (silt::rng = curandState, erosion.cu:57); a launch reads every state, draws, and writes it back.
// `uniform`: every stream's state is {seed, offset} — a tensor that was seeded for this very launch
// and is seeded again before the next, which is what the library's own step drivers do.  Nothing is
// read or written then, and only the particles this slab owns get a record slot: the replay of the
// other ranks' streams (7 of 8 on an 8-GPU run) costs one Philox draw per stream and no memory
// traffic, where the tensor form moves 36 bytes per stream (csrc/slab_runner.hip, HipOps).
struct Streams {
  soil_rng* rng;
  bool uniform;
  uint64_t seed, offset;
};
inline Streams streams_of(soil_rng* rng) { return Streams{rng, false, 0, 0}; }
// spawn position of particle n from the two first draws of its stream (see spawn_position)
__device__ __forceinline__ float2 spawn_position(const Streams& st, int64_t n, const Dom& d) {
  if (!st.uniform) return spawn_position(st.rng, n, d);
  const float u1 = rng_uniform_at(st.seed, static_cast<uint64_t>(n), st.offset);
  const float x = 0.5f + u1 * static_cast<float>(d.H - 1);
  float y = 0.0f;
  if (owns_spawn(d, x))
    y = 0.5f + rng_uniform_at(st.seed, static_cast<uint64_t>(n), st.offset + 1) * static_cast<float>(d.W - 1);
  return make_float2(x, y);
}
// Where a NaN walker's deposits for GLOBAL cell (0, 0) go when that cell lies on another rank (soil_hip.h:
// soil_particles_*_slab's remote0): `phys` float[8] (fluvial water, mass, velocity.x/.y | debris mass,
// velocity.x/.y), `colour` float[6] (fluvial | debris colour; the slab launches with colour planes only).
// Either may be null.
struct Remote0 {
  float* phys;
  float* colour;
};
// Walkers handed over at the slab's edge (SURVEY.md 8e option B; the slab runner's `migrate` mode,
// round 5): a walker that steps off the rows this launch may walk on, inside the grid and with life
// left, is written — state untouched, at the top of an iteration, as at a tile edge — into the box of
// the side it left through instead of being dropped (the deep-halo runner never lets one get there).
// 64-byte records (erosion_particles_tiled.hip: PRec), global coordinates: the neighbour injects them
// into its own queues as they are.  count[0] / count[1]: records written up / down (may exceed `cap`:
// the caller checks).
struct MigrateBox {
  void* up = nullptr;
  void* down = nullptr;
  uint32_t* count = nullptr;
  uint32_t cap = 0;
};

// the two kinds of particle launch
enum Kind { FLUVIAL = 0, DEBRIS = 1, BOTH_KINDS = 2 };

// One particle launch, or the pair of launches, of a step: what every launch shape and entry point hands on.
// Each launch takes its kind's planes of P and, with `C`, its kind's colour flux plane and C->albedo_surface;
// the per-op entries (soil_transport_*, soil_particles_*_slab with albedo planes) pass a C that holds only
// those two.  `remote0`: the NaN walkers' physics deposits for global (0, 0) (float[8], Remote0::phys),
// `remote_colour` their colour deposits (float[6], Remote0::colour); either may be null.  `overwrite`: the
// physics flux planes hold stale values (SOIL_FLUX_OVERWRITE, soil_hip.h): the pair launch leaves them holding
// its deposits only.
struct Launch {
  const soil_erosion_planes* P;
  const soil_colour_planes* C = nullptr;  // null: physics only
  Streams fluvial{}, debris{};
  int64_t N = 0;
  float* remote0 = nullptr;
  float* remote_colour = nullptr;
  Dom d;
  Scale3 s;
  Param p;
  hipStream_t st;
  bool overwrite = false;
};

// Zeroes, over `cells` = local rows x W, the flux planes the launches of `kind` (or BOTH_KINDS) add to: the
// five physics flux planes of P (both kinds; when P is not null) and that kind's colour flux plane(s) of C
// (when C is not null).
int clear_flux(const soil_erosion_planes* P, const soil_colour_planes* C, int kind, int64_t cells, hipStream_t st);

// The launches behind the entry points (erosion_particles.hip).  Each picks the launch shape (use_tiled_launch,
// soil_set_particle_mode); the small-N shapes seed uniform streams into their tensor first.  A single-kind
// launch walks every debris walker to the end and clears no plane.  The pair clears the colour flux planes
// first (with C, also when N == 0) and, on `overwrite`, the physics ones where it cannot store its first round;
// the small-N shapes run the two launches one after the other.
int particles_fluvial(const Launch& L);
int particles_debris(const Launch& L);
int particles_pair(const Launch& L);

// the launch shape a launch of N particles on domain d gets (erosion_particles.hip)
bool use_tiled_launch(int64_t N, const Dom& d);
int debris_retire_mode();    // soil_set_debris_retire / SOIL_DEBRIS_RETIRE (erosion_particles.hip): 0 off, 1 on, 2 watched
bool particle_arith_fast();  // soil_set_particle_arith(1) / SOIL_PARTICLE_DIV=fast (erosion_particles.hip)

// tiled launch shape (erosion_particles_tiled.hip)
// One launch of `kind` (FLUVIAL, DEBRIS) in the tiled shape whatever N: from the streams' spawns (`inbox` null)
// or from `n_in` handed-over records; leavers into `box` (none: dropped).
int launch_pass_tiled(int kind, const Launch& L, const void* inbox = nullptr, uint32_t n_in = 0, MigrateBox box = {});
// Both launches of a step overlapped on two internal streams forked from / joined into L.st.  With L.C: the
// colour flux planes are cleared first and spent debris walkers are retired (TiledRun::retire_colour).
// (inboxes: both launches start from handed-over records instead of the streams' spawns — the immigrants of
// both kinds walked on side by side, slab runner's migrate mode; the pack pass of the step's spawn launches
// stands)
int launch_pair_tiled(const Launch& L, MigrateBox box_fluvial = {}, MigrateBox box_debris = {},
                      const void* inbox_fluvial = nullptr, uint32_t n_fluvial = 0, const void* inbox_debris = nullptr,
                      uint32_t n_debris = 0);

}  // namespace soil
