// flats.hip — routing across flats and filled lakes (soil_hip.h, "flow graphs: conditioning").
//
// soil_fill_depressions (conditioning.hip) returns a surface on which every lake is level, and on a level surface
// steepest and random_weighted give no receiver: every cell of a filled lake is a terminal.  The reference leaves the
// remedy to the third-party pysheds as well (example/dem_condition.py:35-41, resolve_flats), which adds epsilon
// increments to fp64 heights.  Here the remedy is a pair of integer planes: the flat distance of every cell, and
// receivers that walk it down.
//
// Definition.  A non-NaN cell is a seed if a neighbour position is off the grid, a neighbour is NaN, or a neighbour is
// strictly lower: it can drain.  dist is 0 on a seed, otherwise 1 + the least dist over the equal-height neighbours
// that have one, and -1 where no chain of equal cells reaches a seed (and on NaN cells): the shortest-path distance
// inside the flat.  It is the least fixed point of
//        d(c) <- min(d(c), 1 + min over the equal neighbours n of d(n))
// started from "seeds 0, everything else unknown".  An update only lowers a value, and never below the shortest-path
// distance (a value is always the length of a walk from a seed: induction over the updates); a fixed point that is
// reached this way has d(c) <= 1 + d(n) along every shortest path, so it is the distance itself.  Only +1 and min on
// integers are involved, so an iteration in any order ends on the same integers: the kernel settles 64x64 tiles in LDS
// (chaotic inside a tile, Jacobi across tiles per launch) and the host repeats launches until no tile moved, the
// scheme of conditioning.hip without its pyramid — lakes are local, there is nothing to bring in from afar.
//
// Unknown is stored as -1 and compared as unsigned, where it is the largest value: min lowers it like any other
// value and no closing pass is needed.  The +1 is guarded (unknown + 1 would wrap to 0, a seed).
//
// Inside a tile the iteration is the plain one: every cell takes 1 + the least of its equal neighbours, all cells at
// once, until nothing in the tile moves (or 4 x 64 steps; the next launch goes on).  The fill's whole-line form was
// built and measured as well — along a line d'_j = min(d_j, d'_{j-1} + 1) where j and j-1 are equal is, with
// e_j = d_j - j, a segmented prefix minimum, six DPP steps for 64 cells; rows there and back, columns there and back,
// then the plain step — and it lost on every bench DEM: at 4096^2 10.9 ms against 4.3 ms on the filled c3 DEM and
// 13.5 against 4.2 ms on the quantised one, at 8192^2 32.7 against 16.5 and 66.0 against 20.8 ms
// (profiles/resolve_flats/bench.jsonl, "form": "scan").  Lakes of real terrain are a few cells deep in most tiles: a
// plain step that touches only the cells that can still move costs less than four line passes over all 64 lines.
//
// The first launch makes the seeds from the heights and keeps, per cell, the mask of the neighbours that are in the
// grid and equal (one byte a cell in the workspace); later launches read that byte and dist, never the heights.  A
// tile in which no cell can ever move — every cell a seed, NaN or without an equal neighbour, as nearly every tile
// of real terrain — is marked in that launch and returns at once in every later one.  (Not "a tile without an
// unknown cell": a known distance can still be lowered by a shorter way through a neighbouring tile.)
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <utility>

#include "common.hpp"
#include "flow_host.hpp"

namespace soil {

constexpr int kLT = 64;            // tile edge
constexpr int kLH = kLT + 2;       // with its one-cell apron
constexpr int kLRelax = 1024;      // threads of a relaxing work-group, kLCells cells each
constexpr int kLCells = kLT * kLT / kLRelax;
constexpr int kLBlock = 256;
constexpr uint32_t kUnknown = 0xffffffffu;

constexpr int kLDX[8] = {-1, 0, 0, 1, -1, -1, 1, 1};  // graph.hip: kDX / kDY
constexpr int kLDY[8] = {0, -1, 1, 0, -1, 1, -1, 1};

__device__ __forceinline__ uint32_t flat_next(uint32_t d) { return d == kUnknown ? kUnknown : d + 1u; }

// One tile of one model.  `first`: the call's first launch — every tile takes part, makes seeds and masks from the
// heights, relaxes without its apron (the neighbours' seeds are not known yet) and marks itself inert or not.
template <int K>
__device__ __forceinline__ void flat_tile(uint32_t* sd, int* s_flag, int* s_any,
                                          int32_t* __restrict__ dist, unsigned char* __restrict__ mask,
                                          const float* __restrict__ z, int H, int W, int tile, int tiles_w,
                                          int tiles_h, int inner_max, int* __restrict__ changed,
                                          const unsigned char* __restrict__ dirty_prev,
                                          unsigned char* __restrict__ dirty_next, unsigned char* __restrict__ inert,
                                          int first) {
  const int tid = threadIdx.x;
  const int tx = tile / tiles_w, ty = tile % tiles_w;
  if (!first) {
    bool live = inert[tile] == 0;
    if (live) {  // a tile can only move if it or one of its 8 neighbours moved in the previous launch
      live = false;
      for (int dx = -1; dx <= 1; ++dx)
        for (int dy = -1; dy <= 1; ++dy) {
          const int nx = tx + dx, ny = ty + dy;
          if (nx >= 0 && ny >= 0 && nx < tiles_h && ny < tiles_w) live = live || dirty_prev[nx * tiles_w + ny] != 0;
        }
    }
    if (!live) {
      if (tid == 0) dirty_next[tile] = 0;  // (every tile writes its mark: no clearing pass)
      return;
    }
  }
  const int row0 = tx * kLT, col0 = ty * kLT;  // (H, W <= INT32_MAX, and a tile starts inside the grid: 32-bit coordinates)
  auto at = [W](int x, int y) { return static_cast<int64_t>(x) * W + y; };
  float* const sz = reinterpret_cast<float*>(sd);  // the first launch holds the heights here until the seeds are made
  for (int i = tid; i < kLH * kLH; i += kLRelax) {
    const int x = row0 + i / kLH - 1, y = col0 + i % kLH - 1;
    const bool in = x >= 0 && y >= 0 && x < H && y < W;
    if (first) sz[i] = in ? z[at(x, y)] : __builtin_nanf("");
    else sd[i] = in ? static_cast<uint32_t>(dist[at(x, y)]) : kUnknown;
  }
  uint32_t mk[kLCells];
  bool in[kLCells];
  if (tid == 0) *s_any = 0, *s_flag = 0;
  if (first) {
    __syncthreads();
    uint32_t d0[kLCells];
#pragma unroll
    for (int j = 0; j < kLCells; ++j) {
      const int c = tid + j * kLRelax;
      const int x = row0 + c / kLT, y = col0 + c % kLT;
      const int p = (c / kLT + 1) * kLH + (c % kLT + 1);
      in[j] = x < H && y < W;
      const float h = sz[p];
      uint32_t m = 0;
      bool seed = false;
      if (in[j] && h == h) {
#pragma unroll
        for (int k = 0; k < K; ++k) {  // (a position off the grid reads as NaN: an outlet either way)
          const float hn = sz[p + kLDX[k] * kLH + kLDY[k]];
          seed = seed || hn != hn || hn < h;
          if (hn == h) m |= 1u << k;
        }
      }
      mk[j] = m;
      d0[j] = seed ? 0u : kUnknown;
      if (in[j]) mask[at(x, y)] = static_cast<unsigned char>(m);
      if (!seed && m != 0) *s_flag = 1;  // a cell that can move: the tile is not inert
    }
    __syncthreads();
    const bool is_inert = *s_flag == 0;
    for (int i = tid; i < kLH * kLH; i += kLRelax) sd[i] = kUnknown;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kLCells; ++j) {
      const int c = tid + j * kLRelax;
      sd[(c / kLT + 1) * kLH + (c % kLT + 1)] = d0[j];
    }
    if (is_inert) {  // nothing to relax, now or ever
#pragma unroll
      for (int j = 0; j < kLCells; ++j) {
        const int c = tid + j * kLRelax;
        const int x = row0 + c / kLT, y = col0 + c % kLT;
        if (in[j]) dist[at(x, y)] = static_cast<int32_t>(d0[j]);
      }
      if (tid == 0) inert[tile] = 1, dirty_next[tile] = 0;
      return;
    }
    if (tid == 0) inert[tile] = 0;
  } else {
#pragma unroll
    for (int j = 0; j < kLCells; ++j) {
      const int c = tid + j * kLRelax;
      const int x = row0 + c / kLT, y = col0 + c % kLT;
      in[j] = x < H && y < W;
      mk[j] = in[j] ? mask[at(x, y)] : 0u;
    }
  }
  __syncthreads();
  for (int it = 0; it < inner_max; ++it) {
    if (tid == 0) *s_flag = 0;
    __syncthreads();
    bool moved = false;
    // every equal neighbour, one step
#pragma unroll
    for (int j = 0; j < kLCells; ++j) {
      const int c = tid + j * kLRelax;
      const int p = (c / kLT + 1) * kLH + (c % kLT + 1);
      const uint32_t cur = sd[p];
      if (mk[j] == 0 || cur == 0) continue;  // nothing to take from, or nothing below a seed
      uint32_t m = kUnknown;
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (mk[j] >> k & 1) {
          const uint32_t v = sd[p + kLDX[k] * kLH + kLDY[k]];
          m = v < m ? v : m;
        }
      const uint32_t v = flat_next(m);
      if (v < cur) {
        sd[p] = v;
        moved = true;
      }
    }
    if (moved) *s_flag = 1;
    __syncthreads();
    if (*s_flag == 0) break;
    if (tid == 0) *s_any = 1;
    __syncthreads();
  }
  __syncthreads();
  if (*s_any || first) {
#pragma unroll
    for (int j = 0; j < kLCells; ++j) {
      const int c = tid + j * kLRelax;
      const int x = row0 + c / kLT, y = col0 + c % kLT;
      if (in[j]) dist[at(x, y)] = static_cast<int32_t>(sd[(c / kLT + 1) * kLH + (c % kLT + 1)]);
    }
  }
  if (tid == 0) {
    // (the first launch saw no apron: whatever it did, the tile has to look at its neighbours once)
    if (*s_any || first) *changed = 1;
    dirty_next[tile] = (*s_any || first) ? 1 : 0;
  }
}

// grid.x the tile, grid.y the model (a work-group of a batch above 65535 models takes several): model b's planes start
// at b * H * W, in int64; its marks at b * tiles.
template <int K>
__global__ void __launch_bounds__(kLRelax)
    k_flat_relax(int32_t* __restrict__ dist, unsigned char* __restrict__ mask, const float* __restrict__ z, int64_t B,
                 int64_t H, int64_t W, int tiles_w, int tiles_h, int inner_max, int* __restrict__ changed,
                 const unsigned char* __restrict__ dirty_prev, unsigned char* __restrict__ dirty_next,
                 unsigned char* __restrict__ inert, int first) {
  __shared__ uint32_t sd[kLH * kLH];
  __shared__ int s_flag, s_any;
  const int64_t hw = H * W, tiles = static_cast<int64_t>(tiles_w) * tiles_h;
  for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
    flat_tile<K>(sd, &s_flag, &s_any, dist + b * hw, mask + b * hw, z + b * hw, static_cast<int>(H), static_cast<int>(W),
                 static_cast<int>(blockIdx.x),
                 tiles_w, tiles_h, inner_max, changed, dirty_prev + b * tiles, dirty_next + b * tiles,
                 inert + b * tiles, first);
    __syncthreads();  // the next model takes the LDS over
  }
}

// Flat receivers: one thread per cell, grid.z the model.  A cell reads its own graph entry and nothing else of the
// graph, so out == in is allowed; the neighbours are looked at only where in < 0 && dist > 0.
template <int K>
__global__ void __launch_bounds__(kLBlock)
    k_flat_receivers(int32_t* out_, const int32_t* in_, const float* __restrict__ height_,
                     const int32_t* __restrict__ dist_, int64_t B, int64_t H, int64_t W) {
  const int64_t y = static_cast<int64_t>(blockIdx.x) * kLBlock + threadIdx.x;
  if (y >= W) return;
  const int64_t hw = H * W;
  for (int64_t b = blockIdx.z; b < B; b += gridDim.z) {
    // (out and in may be the same plane, so neither is __restrict__: each thread reads in[n] before it writes out[n],
    // and no thread reads another cell's entry)
    int32_t* const out = out_ + b * hw;
    const int32_t* const in = in_ + b * hw;
    const float* const height = height_ + b * hw;
    const int32_t* const dist = dist_ + b * hw;
    SOIL_ROW_LOOP(x, H) {
      const int64_t n = x * W + y;
      int32_t r = in[n];
      if (r < 0) {
        const int32_t d = dist[n];
        if (d > 0) {
          const float h = height[n];
#pragma unroll
          for (int k = 0; k < K; ++k) {
            const int64_t nx = x + kLDX[k], ny = y + kLDY[k];
            if (nx < 0 || ny < 0 || nx >= H || ny >= W) continue;
            const int64_t nb = nx * W + ny;
            if (height[nb] == h && dist[nb] == d - 1) {
              r = static_cast<int32_t>(nb);
              break;
            }
          }
        }
      }
      out[n] = r;
    }
  }
}

// What the last call of soil_flat_distance(_batch) on this host thread did (soil_flat_distance_info)
struct FlatsInfo {
  int64_t launches, tiles, models, looks;
};
static thread_local FlatsInfo t_flats_info{0, 0, 0, 0};

template <int K>
static int flat_distance_run(int32_t* dist, const float* height, int64_t B, int64_t H, int64_t W, hipStream_t st) {
  const int tiles_w = static_cast<int>((W + kLT - 1) / kLT);
  const int tiles_h = static_cast<int>((H + kLT - 1) / kLT);
  const size_t ntiles = static_cast<size_t>(tiles_w) * tiles_h;
  t_flats_info = FlatsInfo{0, static_cast<int64_t>(ntiles), B, 0};
  const size_t b_marks = align256(ntiles * static_cast<size_t>(B));
  void* base = nullptr;
  if (int rc = workspace_get(WS_FLATS, 3 * b_marks + static_cast<size_t>(B) * H * W, &base); rc != SOIL_OK) return rc;
  unsigned char* dirty_prev = static_cast<unsigned char*>(base);
  unsigned char* dirty_next = dirty_prev + b_marks;
  unsigned char* const inert = dirty_next + b_marks;
  unsigned char* const mask = inert + b_marks;
  // "some tile moved in this launch": a pinned, device-mapped word the tiles write straight into (one per host
  // thread and device, as in conditioning.hip)
  static thread_local ThreadOwned<PinnedWord> t_flags;  // (goes with the thread: common.hpp)
  int dev = 0;
  SOIL_HIP(hipGetDevice(&dev));
  PinnedWord& fl = t_flags[dev];
  SOIL_HIP(fl.ensure());
  int *const flag_host = fl.host, *const flag_dev = fl.dev;
  // The fill's bound (conditioning.hip: fill_level): a value reaches a cell along a shortest path inside the flat, a
  // simple path, and a launch finishes in every tile the stretch of it inside the tile up to the next seam, or
  // 4 kLT cells of it.  The models of a batch run side by side: the bound is one model's.
  const int64_t max_launches = static_cast<int64_t>(ntiles) * (4 * kLT + kLT / 4) + 16;
  const char* const e = std::getenv("SOIL_FLATS_PER_CHECK");  // read per call
  const int per_env = e ? std::atoi(e) : 3;
  const int per_check = per_env >= 1 ? per_env : 3;
  const dim3 grid(static_cast<unsigned>(ntiles), static_cast<unsigned>(B < 65535 ? B : 65535));
  for (int64_t launch = 0; launch < max_launches; launch += per_check) {
    *flag_host = 0;  // the stream is idle here: the previous launches were waited for
    for (int k = 0; k < per_check; ++k) {
      k_flat_relax<K><<<grid, kLRelax, 0, st>>>(dist, mask, height, B, H, W, tiles_w, tiles_h, 4 * kLT, flag_dev,
                                                dirty_prev, dirty_next, inert, launch + k == 0 ? 1 : 0);
      std::swap(dirty_prev, dirty_next);
    }
    SOIL_LAUNCH_CHECK();
    SOIL_HIP(hipStreamSynchronize(st));
    t_flats_info.launches += per_check;
    t_flats_info.looks += 1;
    if (!__atomic_load_n(flag_host, __ATOMIC_ACQUIRE)) return SOIL_OK;
  }
  return fail(SOIL_ERR_HIP, "flat_distance: did not converge");
}

// What the entries refuse before any device work, under the entry's name
static int check_flats(const char* what, bool pointers, int64_t B, int64_t H, int64_t W, int edge) {
  const std::string w(what);
  SOIL_REQUIRE(pointers, w + ": null tensor");
  return check_grid_batch(w, B, H, W, edge);
}

static int flat_receivers_run(int32_t* out, const int32_t* in, const float* height, const int32_t* dist, int64_t B,
                              int64_t H, int64_t W, int edge, hipStream_t st) {
  dim3 grid = grid_rows(H, W, kLBlock);
  grid.z = static_cast<unsigned>(B < 65535 ? B : 65535);
  if (edge == SOIL_D4) k_flat_receivers<4><<<grid, kLBlock, 0, st>>>(out, in, height, dist, B, H, W);
  else k_flat_receivers<8><<<grid, kLBlock, 0, st>>>(out, in, height, dist, B, H, W);
  SOIL_LAUNCH_CHECK();
  return SOIL_OK;
}

}  // namespace soil

using namespace soil;

extern "C" {

int soil_flat_distance(int32_t* dist, const float* height, int64_t H, int64_t W, int edge, void* stream) {
  if (int rc = check_flats("flat_distance", dist && height, 1, H, W, edge); rc != SOIL_OK) return rc;
  SOIL_DEVICE();
  return edge == SOIL_D4 ? flat_distance_run<4>(dist, height, 1, H, W, as_stream(stream))
                         : flat_distance_run<8>(dist, height, 1, H, W, as_stream(stream));
}

int soil_flat_distance_batch(int32_t* dist, const float* height, int64_t B, int64_t H, int64_t W, int edge,
                             void* stream) {
  if (int rc = check_flats("flat_distance_batch", dist && height, B, H, W, edge); rc != SOIL_OK) return rc;
  SOIL_DEVICE();
  return edge == SOIL_D4 ? flat_distance_run<4>(dist, height, B, H, W, as_stream(stream))
                         : flat_distance_run<8>(dist, height, B, H, W, as_stream(stream));
}

int soil_flat_receivers(int32_t* out, const int32_t* in, const float* height, const int32_t* dist, int64_t H,
                        int64_t W, int edge, void* stream) {
  if (int rc = check_flats("flat_receivers", out && in && height && dist, 1, H, W, edge); rc != SOIL_OK) return rc;
  SOIL_DEVICE();
  return flat_receivers_run(out, in, height, dist, 1, H, W, edge, as_stream(stream));
}

int soil_flat_receivers_batch(int32_t* out, const int32_t* in, const float* height, const int32_t* dist, int64_t B,
                              int64_t H, int64_t W, int edge, void* stream) {
  if (int rc = check_flats("flat_receivers_batch", out && in && height && dist, B, H, W, edge); rc != SOIL_OK)
    return rc;
  SOIL_DEVICE();
  return flat_receivers_run(out, in, height, dist, B, H, W, edge, as_stream(stream));
}

int soil_flat_distance_info(int64_t info[4]) {
  SOIL_REQUIRE(info, "flat_distance_info: null info");
  info[0] = t_flats_info.launches, info[1] = t_flats_info.tiles;
  info[2] = t_flats_info.models, info[3] = t_flats_info.looks;
  return SOIL_OK;
}

}  // extern "C"
