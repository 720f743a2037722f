// slope_limit.hip — threshold hillslopes: the slope-limited surface of a DEM (soil_hip.h, "flow graphs: conditioning").
//
// soil_slope_limit returns the greatest surface w <= h in which no cell stands higher above a neighbour than a
// critical slope times the distance allows:
//        w[n] <= w[k] (+) c_k[n]   for every neighbour k of n in the grid,
// c_k[n] = (float)((double)slope[n] * L_k) — one fp64 product rounded once, L_k the fp64 length flow_length uses for
// that kind of edge — and (+) one fp32 addition, round to nearest, denormals kept.  The slope that binds an edge is
// the slope of the cell being lowered.  It is the third tile relaxation of the library, after the fill
// (conditioning.hip) and the flat distance (flats.hip), and the fixed point that
//        w[n] <- cand   if cand < w[n],   cand = w[k] (+) c_k[n]
// reaches from w = h in any order of updates:
//   - The operator T(w)[n] = min(w[n], min_k w[k] (+) c_k[n]) is monotone (u <= v cell by cell gives T(u) <= T(v)),
//     because round-to-nearest addition is monotone in each argument and min is.
//   - It only lowers values.
//   - The greatest fixed point w* below h exists (the cell-wise maximum of two surfaces that satisfy the constraints
//     satisfies them, by monotonicity).  Every chaotic iteration from h — single updates in any order, also from a
//     neighbour's value that has since been lowered further — stays on or above w*: w >= w* gives
//     w[k] (+) c >= w*[k] (+) c >= w*[n].  Where it ends, no update lowers anything, so it ends on a fixed point below
//     h and above w*: on w*.
//   - It ends: the values are floats between min h and h, a finite set, and c >= 0 means a value only ever comes from
//     a smaller or equal one (w (+) c >= w); a cell is lowered finitely often.
// The same argument as a shortest path: w*[n] is the least value of h[m] (+) c (+) c ... along a way m -> n, and
// because w (+) c >= w a heap-based Dijkstra finds it (tests/slope_limit_ref.py holds both restatements).
//
// One definite bit pattern.  Strict <: a tie keeps the bits the cell has.  c is never -0 (a product that is zero is
// taken as +0), so no candidate is ever -0 either: x (+) c is +0 whenever it is zero.  Two candidates of one value
// have therefore the same bits, and a -0 in the result is a -0 of h that was not lowered.  A NaN height is a void: never
// lowered (cand < NaN is false), lowering nobody (NaN (+) c is NaN), NaN in the result; a position off the grid is
// loaded as NaN and binds nothing the same way.  A slope entry that is not >= 0 (NaN, negative) means "no limit at
// this cell": c = +inf there, what a slope of +inf gives by arithmetic alone; the cell keeps its height
// (w[k] + inf is +inf, or NaN for w[k] = -inf) and still binds its neighbours through their own c.  +-inf heights go
// through the arithmetic as they are.
//
// What the kernel may not do.  The fill's whole-line DPP scans compose clamps exactly; here a scan that pre-adds two
// steps would compute w (+) (c + c), which is not (w (+) c) (+) c, can land below the fixed point and would make the
// result depend on the path.  Every update a cell sees is the one rounded addition above (__fadd_rn: no contraction,
// no reassociation) on a value that some cell holds or held — a stale, higher value is a legal chaotic update.
//
// Scheme (that of flats.hip): 64 x 64 tiles with a one-cell apron in LDS, chaotic inside a tile (the plain step: every
// cell takes the least candidate of its neighbours, all cells at once, until nothing in the tile moves or kSInner
// steps have run), Jacobi across tiles per launch.  Every tile writes its own dirty mark (no clearing pass); a tile
// runs only if it or one of its eight neighbours moved in the previous launch; the host looks at a pinned "changed"
// word every SOIL_SLOPE_LIMIT_PER_CHECK launches.  The first launch reads h (apron included: unlike the flat distance
// the start is known everywhere) and the slope plane, later launches read and write w (and re-read the slope plane of
// live tiles: the steps are three products a cell, cheaper than a plane of their own).
//
// Inert tiles.  A tile is marked inert in the first launch, and returns at once in every later one, only if no cell
// of it can be lowered whatever happens around it: every cell in the grid is NaN, -inf, or has no finite step (all
// c = +inf).  NOT "every constraint holds in the tile and on its apron": the apron can come down later — a pit three
// tiles away lowers it — and then the tile has to follow.  Nothing about the apron's future is provable from one
// tile's view in launch one, so tiles that merely hold their constraints are left to the dirty marks, which wake them
// when a neighbour moves.
//
// The launch bound.  Let p_0 .. p_L = n be a way that realises w*[n] (p_0 a cell that keeps its height, each p_i+1
// lowered from p_i; Dijkstra's tree, so the way is simple).  If p_i holds its final value when a launch starts, the
// tile T of p_i+1 runs in that launch (p_i became final by a move of its tile, T or one of T's neighbours, in the
// launch before, or is final from the start and the first launch runs every tile), loads p_i, and the plain step
// makes p_i+1 final in its first sweep, p_i+2 in the second, ... as long as the way stays inside T and the kSInner
// sweeps last; a tile that stops at kSInner has moved and marks itself dirty.  So a launch finishes the stretch of the
// way inside a tile up to the next seam, or kSInner cells of it.  A stretch ends on a border cell of its tile, and a
// simple way visits each of the < 4 kST border cells of a tile once: at most 4 kST stretches a tile, and the ceil of a
// stretch's length over kSInner sums to at most that plus kST kST / kSInner a tile.  One more launch sees that
// nothing moved.  Hence launches <= tiles * (4 kST + kST kST / kSInner) + 2 for every legal input (the models of a
// batch run side by side: the bound is one model's); the loop's groups of per-check launches may overshoot it by less
// than one group.
//
// The in-tile form is the plain step.  The serial line walks were built and measured as well — before every plain
// step one wave walks the 64 rows there and back, a thread a row, cell j from the updated cell j - 1 (legal: the
// operator itself, applied in line order), then the columns, and the plain step takes the diagonals — gave the same
// bits on every test and lost at every size on the bench terrain: 0.38 against 0.11 ms at 256^2, 1.60 against 0.31 ms
// at 1024^2, 22.8 against 3.0 ms at 4096^2 (profiles/slope_limit/bench_forms.jsonl).  A walk is 256 dependent LDS
// round trips by 64 of the 1024 threads, the price of some thirty plain steps, and the cones of real terrain are a
// few tens of cells wide: the plain step, which costs nothing where nothing moves, gets there sooner.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <utility>

#include "common.hpp"
#include "flow_host.hpp"

namespace soil {

constexpr int kST = 64;            // tile edge
constexpr int kSH = kST + 2;       // with its one-cell apron
constexpr int kSRelax = 1024;      // threads of a relaxing work-group, kSCells cells each
constexpr int kSCells = kST * kST / kSRelax;
constexpr int kSInner = 4 * kST;   // sweeps of a tile per launch (flats.hip's value; not measured for this operator)
constexpr int kSBlock = 256;

constexpr int kSDX[8] = {-1, 0, 0, 1, -1, -1, 1, 1};  // graph.hip: kDX / kDY
constexpr int kSDY[8] = {0, -1, 1, 0, -1, 1, -1, 1};

// A model's step lengths (fp64: sx, sy, sqrt(sx sx + sy sy), as flow_length has them) and, for a scalar slope, the
// three steps c made from them on the host
struct SlopeRec {
  double lx, ly, ld;
  float cx, cy, cd, pad;
};

inline float slope_step(double slope, double len) {  // one fp64 product, rounded once; never -0
  const float c = static_cast<float>(slope * len);
  return c == 0.0f ? 0.0f : c;
}

// grid.x the tile, grid.y the model (BATCH; a work-group of a batch above 65535 models takes several): model b's
// planes start at b * H * W, in int64; its marks at b * tiles.  `first`: the call's first launch — every tile takes
// part, reads h instead of w and marks itself inert or not.  PLANE: c from slope[n]; otherwise from the record.
template <int K, bool PLANE, bool BATCH>
__global__ void __launch_bounds__(kSRelax)
    k_slope_relax(float* w_, const float* __restrict__ h_, const float* __restrict__ slope_, SlopeRec one,
                  const SlopeRec* __restrict__ recs, int64_t B, int H, int W, int tiles_w, int tiles_h, int inner_max,
                  int* __restrict__ changed, const unsigned char* __restrict__ dirty_prev_,
                  unsigned char* __restrict__ dirty_next_, unsigned char* __restrict__ inert_, int first) {
  __shared__ float sd[kSH * kSH];
  __shared__ int s_flag, s_any;
  const int tid = threadIdx.x;
  const int tile = static_cast<int>(blockIdx.x);
  const int tx = tile / tiles_w, ty = tile % tiles_w;
  const int row0 = tx * kST, col0 = ty * kST;  // (a tile starts inside the grid: 32-bit coordinates)
  const int64_t hw = static_cast<int64_t>(H) * W, tiles = static_cast<int64_t>(tiles_w) * tiles_h;
  auto at = [W](int x, int y) { return static_cast<int64_t>(x) * W + y; };
  const float inf = __builtin_inff();
  for (int64_t b = BATCH ? blockIdx.y : 0; b < (BATCH ? B : 1); b += BATCH ? gridDim.y : 1) {
    __syncthreads();  // (the model before has left the LDS)
    const unsigned char* const dirty_prev = dirty_prev_ + b * tiles;
    unsigned char* const dirty_next = dirty_next_ + b * tiles;
    unsigned char* const inert = inert_ + b * tiles;
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
        continue;
      }
    }
    float* const w = w_ + b * hw;
    const float* const src = first ? h_ + b * hw : w;
    for (int i = tid; i < kSH * kSH; i += kSRelax) {
      const int x = row0 + i / kSH - 1, y = col0 + i % kSH - 1;
      sd[i] = (x >= 0 && y >= 0 && x < H && y < W) ? src[at(x, y)] : __builtin_nanf("");
    }
    const SlopeRec rec = BATCH && recs ? recs[b] : one;
    // the steps of this thread's cells: toward a row neighbour, a column neighbour, a diagonal one
    float cx[kSCells], cy[kSCells], cd[kSCells];
    bool in[kSCells];
#pragma unroll
    for (int j = 0; j < kSCells; ++j) {
      const int c = tid + j * kSRelax;
      const int x = row0 + c / kST, y = col0 + c % kST;
      in[j] = x < H && y < W;
      if (PLANE) {
        const float s = in[j] ? slope_[b * hw + at(x, y)] : -1.0f;
        if (s >= 0.0f) {
          const double s64 = static_cast<double>(s);
          cx[j] = __double2float_rn(__dmul_rn(s64, rec.lx));
          cy[j] = __double2float_rn(__dmul_rn(s64, rec.ly));
          cd[j] = __double2float_rn(__dmul_rn(s64, rec.ld));
          cx[j] = cx[j] == 0.0f ? 0.0f : cx[j];  // never -0
          cy[j] = cy[j] == 0.0f ? 0.0f : cy[j];
          cd[j] = cd[j] == 0.0f ? 0.0f : cd[j];
        } else {
          cx[j] = cy[j] = cd[j] = inf;  // NaN or negative: no limit at this cell
        }
      } else {
        cx[j] = rec.cx, cy[j] = rec.cy, cd[j] = rec.cd;
      }
    }
    if (tid == 0) s_any = 0, s_flag = 0;
    __syncthreads();
    // a cell that can never be lowered: off the grid, NaN or -inf, or without a finite step
    bool mv[kSCells];
#pragma unroll
    for (int j = 0; j < kSCells; ++j) {
      const int c = tid + j * kSRelax;
      const float cur = sd[(c / kST + 1) * kSH + (c % kST + 1)];
      float cmin = cx[j] < cy[j] ? cx[j] : cy[j];
      if (K == 8) cmin = cd[j] < cmin ? cd[j] : cmin;
      mv[j] = in[j] && cur > -inf && cmin < inf;
      if (first && mv[j]) s_flag = 1;
    }
    if (first) {
      __syncthreads();
      const bool is_inert = s_flag == 0;
      if (tid == 0) inert[tile] = is_inert ? 1 : 0;
      if (is_inert) {  // nothing to relax, now or ever: w = h
#pragma unroll
        for (int j = 0; j < kSCells; ++j) {
          const int c = tid + j * kSRelax;
          if (in[j]) w[at(row0 + c / kST, col0 + c % kST)] = sd[(c / kST + 1) * kSH + (c % kST + 1)];
        }
        if (tid == 0) dirty_next[tile] = 0;
        continue;
      }
      __syncthreads();  // (s_flag is read above and cleared below)
    }
    for (int it = 0; it < inner_max; ++it) {
      if (tid == 0) s_flag = 0;
      __syncthreads();
      bool moved = false;
#pragma unroll
      for (int j = 0; j < kSCells; ++j) {
        if (!mv[j]) continue;
        const int c = tid + j * kSRelax;
        const int p = (c / kST + 1) * kSH + (c % kST + 1);
        const float cur = sd[p];
        float best = cur;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float step = k >= 4 ? cd[j] : (kSDX[k] != 0 ? cx[j] : cy[j]);
          const float cand = __fadd_rn(sd[p + kSDX[k] * kSH + kSDY[k]], step);
          best = cand < best ? cand : best;  // strict: a tie keeps what is there
        }
        if (best < cur) {
          sd[p] = best;
          moved = true;
        }
      }
      if (moved) s_flag = 1;
      __syncthreads();
      if (s_flag == 0) break;
      if (tid == 0) s_any = 1;
      __syncthreads();
    }
    __syncthreads();
    const bool any = s_any != 0;
    if (any || first) {
#pragma unroll
      for (int j = 0; j < kSCells; ++j) {
        const int c = tid + j * kSRelax;
        if (in[j]) w[at(row0 + c / kST, col0 + c % kST)] = sd[(c / kST + 1) * kSH + (c % kST + 1)];
      }
    }
    if (tid == 0) {
      if (any) *changed = 1;  // one word for the whole batch: any tile of any model
      dirty_next[tile] = any ? 1 : 0;
    }
  }
}

// excess = h (-) w, one fp32 subtraction a cell: +0 where the cell was not lowered (+-inf cells that stayed
// included), NaN on voids
__global__ void __launch_bounds__(kSBlock)
    k_slope_excess(float* __restrict__ excess, const float* __restrict__ h, const float* __restrict__ w, int64_t n) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kSBlock + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kSBlock) {
    const float a = h[i], c = w[i];
    excess[i] = c < a ? __fsub_rn(a, c) : (a != a ? a : 0.0f);
  }
}

// What the last call of soil_slope_limit(_batch) on this host thread did (soil_slope_limit_info)
struct SlopeLimitInfo {
  int64_t launches, tiles, models, looks;
};
static thread_local SlopeLimitInfo t_slope_info{0, 0, 0, 0};

template <int K, bool PLANE, bool BATCH>
static int slope_limit_run(float* out, float* excess, const float* height, const float* slope_plane, double slope,
                           int64_t B, int64_t H, int64_t W, const float* scales, int64_t n_scales, hipStream_t st) {
  const int tiles_w = static_cast<int>((W + kST - 1) / kST);
  const int tiles_h = static_cast<int>((H + kST - 1) / kST);
  const size_t ntiles = static_cast<size_t>(tiles_w) * tiles_h;
  t_slope_info = SlopeLimitInfo{0, static_cast<int64_t>(ntiles), B, 0};
  const bool per_model = n_scales > 1;
  const size_t b_recs = per_model ? align256(sizeof(SlopeRec) * static_cast<size_t>(B)) : 0;
  const size_t b_marks = align256(ntiles * static_cast<size_t>(B));
  void* base = nullptr;
  if (int rc = workspace_get(WS_SLOPE_LIMIT, b_recs + 3 * b_marks, &base); rc != SOIL_OK) return rc;
  auto make = [slope](const float* pair) {
    const double sx = static_cast<double>(pair[0]), sy = static_cast<double>(pair[1]);
    SlopeRec r{sx, sy, std::sqrt(sx * sx + sy * sy), 0.0f, 0.0f, 0.0f, 0.0f};  // (flow_paths.hpp: path_scale)
    if (!PLANE) r.cx = slope_step(slope, r.lx), r.cy = slope_step(slope, r.ly), r.cd = slope_step(slope, r.ld);
    return r;
  };
  const SlopeRec* recs = nullptr;
  if (per_model) {
    if (int rc = upload_scale_records(base, scales, B, make, st); rc != SOIL_OK) return rc;
    recs = static_cast<const SlopeRec*>(base);
  }
  unsigned char* dirty_prev = static_cast<unsigned char*>(base) + b_recs;
  unsigned char* dirty_next = dirty_prev + b_marks;
  unsigned char* const inert = dirty_next + b_marks;
  // "some tile moved in this launch": a pinned, device-mapped word the tiles write straight into (one per host
  // thread and device, as in conditioning.hip and flats.hip)
  static thread_local ThreadOwned<PinnedWord> t_flags;  // (goes with the thread: common.hpp)
  int dev = 0;
  SOIL_HIP(hipGetDevice(&dev));
  PinnedWord& fl = t_flags[dev];
  SOIL_HIP(fl.ensure());
  int *const flag_host = fl.host, *const flag_dev = fl.dev;
  // the bound of the file's header
  const int64_t max_launches = static_cast<int64_t>(ntiles) * (4 * kST + kST * kST / kSInner) + 2;
  const char* const e = std::getenv("SOIL_SLOPE_LIMIT_PER_CHECK");  // read per call
  const int per_env = e ? std::atoi(e) : 3;
  const int per_check = per_env >= 1 ? per_env : 3;
  const dim3 grid(static_cast<unsigned>(ntiles), static_cast<unsigned>(B < 65535 ? B : 65535));
  bool settled = false;
  for (int64_t launch = 0; launch < max_launches && !settled; launch += per_check) {
    *flag_host = 0;  // the stream is idle here: the previous launches were waited for
    for (int k = 0; k < per_check; ++k) {
      k_slope_relax<K, PLANE, BATCH><<<grid, kSRelax, 0, st>>>(
          out, height, slope_plane, make(scales), recs, B, static_cast<int>(H), static_cast<int>(W), tiles_w, tiles_h,
          kSInner, flag_dev, dirty_prev, dirty_next, inert, launch + k == 0 ? 1 : 0);
      std::swap(dirty_prev, dirty_next);
    }
    SOIL_LAUNCH_CHECK();
    SOIL_HIP(hipStreamSynchronize(st));
    t_slope_info.launches += per_check;
    t_slope_info.looks += 1;
    settled = !__atomic_load_n(flag_host, __ATOMIC_ACQUIRE);
  }
  if (!settled) return fail(SOIL_ERR_HIP, "slope_limit: did not converge");
  if (excess) {
    const int64_t n = B * H * W;
    const int64_t blocks = (n + kSBlock - 1) / kSBlock;
    k_slope_excess<<<static_cast<unsigned>(blocks < 65535 * 16 ? blocks : 65535 * 16), kSBlock, 0, st>>>(excess, height,
                                                                                                      out, n);
    SOIL_LAUNCH_CHECK();
    SOIL_HIP(hipStreamSynchronize(st));
  }
  return SOIL_OK;
}

// What the entries refuse before any device work, under the entry's name
static int check_slope_limit(const char* what, const float* out, const float* excess, const float* height,
                             const float* slope_plane, double slope, int64_t B, int64_t H, int64_t W,
                             const float* scales, int64_t n_scales, int edge) {
  const std::string w(what);
  SOIL_REQUIRE(out && height, w + ": null tensor");
  SOIL_REQUIRE(scales, w + ": null scale");
  if (int rc = check_grid_batch(w, B, H, W, edge, n_scales, ""); rc != SOIL_OK) return rc;
  const size_t cells = plane_cells(B, H * W);
  for (const void* q : {static_cast<const void*>(height), static_cast<const void*>(slope_plane)})
    SOIL_REQUIRE(!overlaps(out, 4 * cells, q, 4 * cells) && !overlaps(excess, 4 * cells, q, 4 * cells),
                 w + ": an output aliases an input plane");
  SOIL_REQUIRE(!overlaps(out, 4 * cells, excess, 4 * cells), w + ": out and excess overlap");
  if (int rc = check_scales_positive(w, scales, n_scales); rc != SOIL_OK) return rc;
  SOIL_REQUIRE(slope_plane || (slope >= 0.0 && std::isfinite(slope)),
               w + ": slope must be finite and >= 0 (or a slope plane given)");
  return SOIL_OK;
}

template <bool BATCH>
static int slope_limit_dispatch(float* out, float* excess, const float* height, const float* slope_plane, double slope,
                                int64_t B, int64_t H, int64_t W, const float* scales, int64_t n_scales, int edge,
                                hipStream_t st) {
  if (edge == SOIL_D4)
    return slope_plane ? slope_limit_run<4, true, BATCH>(out, excess, height, slope_plane, slope, B, H, W, scales, n_scales, st)
                       : slope_limit_run<4, false, BATCH>(out, excess, height, slope_plane, slope, B, H, W, scales, n_scales, st);
  return slope_plane ? slope_limit_run<8, true, BATCH>(out, excess, height, slope_plane, slope, B, H, W, scales, n_scales, st)
                     : slope_limit_run<8, false, BATCH>(out, excess, height, slope_plane, slope, B, H, W, scales, n_scales, st);
}

}  // namespace soil

using namespace soil;

extern "C" {

int soil_slope_limit(float* out, float* excess, const float* height, const float* slope_plane, double slope, int64_t H,
                     int64_t W, const float scale[2], int edge, void* stream) {
  if (int rc = check_slope_limit("slope_limit", out, excess, height, slope_plane, slope, 1, H, W, scale, 1, edge);
      rc != SOIL_OK)
    return rc;
  SOIL_DEVICE();
  return slope_limit_dispatch<false>(out, excess, height, slope_plane, slope, 1, H, W, scale, 1, edge,
                                     as_stream(stream));
}

int soil_slope_limit_batch(float* out, float* excess, const float* height, const float* slope_plane, double slope,
                           int64_t B, int64_t H, int64_t W, const float* scales, int64_t n_scales, int edge,
                           void* stream) {
  if (int rc = check_slope_limit("slope_limit_batch", out, excess, height, slope_plane, slope, B, H, W, scales,
                                 n_scales, edge);
      rc != SOIL_OK)
    return rc;
  SOIL_DEVICE();
  return slope_limit_dispatch<true>(out, excess, height, slope_plane, slope, B, H, W, scales, n_scales, edge,
                                    as_stream(stream));
}

int soil_slope_limit_info(int64_t info[4]) {
  SOIL_REQUIRE(info, "slope_limit_info: null info");
  info[0] = t_slope_info.launches, info[1] = t_slope_info.tiles;
  info[2] = t_slope_info.models, info[3] = t_slope_info.looks;
  return SOIL_OK;
}

}  // extern "C"
