// mfd.hip — exact multiple-flow accumulation: the limit of multiflow in one call (soil_hip.h, "flow graphs: exact
// multiple-flow accumulation").
//
// soil_multiflow averages the accumulations of K random_weighted graphs.  Every cell of such a graph draws its receiver
// independently, neighbour k with the Gibbs share w_k = P_k / Z, and every edge goes strictly downhill, so a walk
// never meets a cell twice and the expectation of the accumulation is the solution of the sparse triangular system
//        a[n] = source[n] + sum over donors d of w(d -> n) a[d].
// With the weights P_k = (drop / length)^p the same system is the deterministic multiple-flow accumulation of Freeman,
// Quinn and Holmgren.  soil_mfd_weights writes the shares, soil_mfd_accumulate solves the system; soil_hip.h states
// the arithmetic of both in full, tests/mfd_ref.py restates it in numpy.
//
// One bit pattern, whatever the schedule.  The graph of the non-zero shares is acyclic: a Gibbs or power share is
// non-zero only where diff = h[n] (-) h[k] > 0, that is h[n] > h[k]; a flat edge (share 1 along `dist`) keeps the
// height and lowers dist by one; so every edge strictly lowers the pair (height, dist) in lexicographic order,
// whatever `dist` holds.  (A NaN diff gives a NaN weight, a NaN Z and a terminal, for both kinds: pow(NaN, 0) is 1,
// and two NaN cells that fed each other would be a cycle, so the power kind tests for the NaN itself.)  On a DAG the
// value of a cell is one fixed expression of its donors' final values — the sum in table order, one rounded fp64
// product and one rounded fp64 sum a donor — so every iteration that ends, ends on the same bits: whole-grid Jacobi,
// the tiles below, any order.
//
// Scheme (that of slope_limit.hip and flats.hip): 64 x 64 tiles with a one-cell apron, here of doubles (66 x 66 x 8 =
// 34 848 bytes of LDS), 1024 threads with four cells each.  A thread holds the incoming shares of its cells in
// registers: share k of cell n is the outgoing share of neighbour k towards n, plane kMOpp[k] of the weights at the
// neighbour's index, loaded once a launch.  Jacobi sweeps inside a tile (every cell from the values of the sweep
// before: read, barrier, write, barrier) until no bit of the tile changes or kMInner sweeps have run; Jacobi across
// tiles per launch.  Every tile writes its own dirty mark; a tile runs only if it or one of its eight neighbours
// moved in the previous launch; a tile that stops at kMInner has moved in its last sweep and is dirty by that.  The
// host looks at a pinned "changed" word every SOIL_MFD_PER_CHECK launches.  The first launch reads the source (apron
// included) and marks a tile inert if no cell of it receives anything: such a tile holds the source for ever.
//
// The launch bound.  Call a cell final once it holds its last value.  A cell without donors is final from the start
// (a = source).  A cell is final one sweep after the last of its donors: all donors final in LDS or on the apron, the
// sweep evaluates the fixed expression.  Follow from a cell n its last-finalised donor, from that one its own, and so
// on back to a cell without donors: the critical chain of n, p_0 .. p_L = n, a way along edges of a DAG and therefore
// simple.  If p_i is final when a launch starts, the tile T of p_i+1 runs in that launch — p_i became final by a move
// of its tile, which is T or one of T's eight neighbours, in the launch before, or it is final from the start and the
// first launch runs every tile — and T loads p_i, and every other donor of p_i+1, final (they were final no later
// than p_i).  Its first sweep makes p_i+1 final, its second p_i+2, ... as long as the chain stays inside T and the
// kMInner sweeps last; a tile that stops at kMInner marks itself dirty and goes on in the next launch.  So a launch
// finishes the stretch of the chain inside a tile up to the next seam, or kMInner cells of it.  A stretch ends on a
// border cell of its tile and a simple way visits each of the < 4 kMT border cells of a tile once: at most 4 kMT
// stretches a tile, and the ceil of a stretch's length over kMInner sums to at most that plus kMT kMT / kMInner a
// tile.  One more launch sees that nothing moved.  Hence
//        launches <= tiles * (4 kMT + kMT kMT / kMInner) + 2 = tiles * 272 + 2
// for every input (the models of a batch run side by side: the bound is one model's); the loop's groups of per-check
// launches may overshoot it by less than one group.  Reaching it is an internal error, not a property of the input.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <utility>

#include "common.hpp"
#include "flow_host.hpp"

namespace soil {

constexpr int kMT = 64;            // tile edge
constexpr int kMH = kMT + 2;       // with its one-cell apron
constexpr int kMRelax = 1024;      // threads of a relaxing work-group, kMCells cells each
constexpr int kMCells = kMT * kMT / kMRelax;
constexpr int kMInner = 4 * kMT;   // sweeps of a tile per launch
constexpr int kMBlock = 256;

constexpr int kMDX[8] = {-1, 0, 0, 1, -1, -1, 1, 1};  // graph.hip: kDX / kDY
constexpr int kMDY[8] = {0, -1, 1, 0, -1, 1, -1, 1};
constexpr int kMOpp[8] = {3, 2, 1, 0, 7, 6, 5, 4};     // the neighbour's direction back to the cell

// What makes the raw weights: the Gibbs constants (rw_const) or the exponent, and a model's fp64 step lengths (sx, sy,
// sqrt(sx sx + sy sy), as flow_length has them; read by the power kind only)
struct MfdLen {
  double lx, ly, ld;
};
struct MfdKind {
  RwConst rc;
  double p;
};

// The K outgoing shares of a cell (soil_hip.h states each step).  hn[k], dn[k]: neighbour k's height and dist where
// ok[k], anything otherwise; d the cell's own dist (DIST only).
template <int K, bool POWER, bool DIST>
__device__ __forceinline__ void mfd_shares(float w[K], float h, int32_t d, const float hn[K], const int32_t dn[K],
                                           const bool ok[K], const MfdKind& kind, const MfdLen& len) {
  float P[K];
  float Z = 0.0f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float diff = h - hn[k];
    float p;
    if (diff <= 0.0f) {
      p = 0.0f;
    } else if (POWER) {
      const double L = k >= 4 ? len.ld : (kMDX[k] != 0 ? len.lx : len.ly);
      p = diff != diff ? diff : __double2float_rn(sp_pow(__ddiv_rn(static_cast<double>(diff), L), kind.p));
    } else {
      p = rw_exp2(diff, k < 4 ? kind.rc.straight : kind.rc.diagonal);
    }
    if (!ok[k]) p = 0.0f;
    P[k] = p;
    Z += p;  // ((P_0 + P_1) + ...), as rw_cdf sums it
  }
  const bool sends = Z > 0.0f && Z < __builtin_inff();
#pragma unroll
  for (int k = 0; k < K; ++k) w[k] = sends ? __fdiv_rn(P[k], Z) : 0.0f;
  if (DIST && !sends && Z == 0.0f && d > 0) {  // a flat: flat_receivers' rule, share 1
    bool found = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const bool take = !found && ok[k] && hn[k] == h && dn[k] == d - 1;
      if (take) w[k] = 1.0f;
      found = found || take;
    }
  }
}

// One thread a cell, a work-group a band of rows (SOIL_ROW_LOOP), grid.z the model.  Model b's heights start at
// b * H * W and its K share planes at b * K * H * W, in int64.
template <int K, bool POWER, bool DIST>
__global__ void __launch_bounds__(kMBlock)
    k_mfd_weights(float* __restrict__ weights_, const float* __restrict__ height_, const int32_t* __restrict__ dist_,
                  MfdKind kind, MfdLen one, const MfdLen* __restrict__ lens, int64_t B, int64_t H, int64_t W) {
  const int64_t y = static_cast<int64_t>(blockIdx.x) * kMBlock + threadIdx.x;
  if (y >= W) return;
  const int64_t hw = H * W;
  for (int64_t b = blockIdx.z; b < B; b += gridDim.z) {
    float* const weights = weights_ + b * K * hw;
    const float* const height = height_ + b * hw;
    const int32_t* const dist = DIST ? dist_ + b * hw : nullptr;
    const MfdLen len = lens ? lens[b] : one;
    SOIL_ROW_LOOP(x, H) {
      const int64_t n = x * W + y;
      float hn[K], w[K];
      int32_t dn[K];
      bool ok[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int64_t nx = x + kMDX[k], ny = y + kMDY[k];
        ok[k] = !(nx < 0 || ny < 0 || nx >= H || ny >= W);
        hn[k] = ok[k] ? height[nx * W + ny] : 0.0f;
        dn[k] = DIST && ok[k] ? dist[nx * W + ny] : 0;
      }
      mfd_shares<K, POWER, DIST>(w, height[n], DIST ? dist[n] : 0, hn, dn, ok, kind, len);
#pragma unroll
      for (int k = 0; k < K; ++k) weights[k * hw + n] = w[k];
    }
  }
}

__device__ __forceinline__ uint64_t mfd_bits(double v) { return static_cast<uint64_t>(__double_as_longlong(v)); }

// grid.x the tile, grid.y the model (a work-group of a batch above 65535 models takes several): model b's planes start
// at b * H * W, its shares at b * K * H * W, in int64; its marks at b * tiles.  `first`: the call's first launch —
// every tile takes part, reads the source instead of a and marks itself inert or not.
template <int K>
__global__ void __launch_bounds__(kMRelax)
    k_mfd_relax(double* a_, const float* __restrict__ source_, const float* __restrict__ weights_, int64_t B, int H,
                int W, int tiles_w, int tiles_h, int inner_max, int* __restrict__ changed,
                const unsigned char* __restrict__ dirty_prev_, unsigned char* __restrict__ dirty_next_,
                unsigned char* __restrict__ inert_, int first) {
  __shared__ double sd[kMH * kMH];
  __shared__ int s_flag[2];
  const int tile = static_cast<int>(blockIdx.x);
  const int tx = tile / tiles_w, ty = tile % tiles_w;
  const int row0 = tx * kMT, col0 = ty * kMT;  // (a tile starts inside the grid: 32-bit coordinates)
  const int64_t hw = static_cast<int64_t>(H) * W, tiles = static_cast<int64_t>(tiles_w) * tiles_h;
  auto at = [W](int x, int y) { return static_cast<int64_t>(x) * W + y; };
  for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
    __syncthreads();  // (the model before has left the LDS)
    // (what a thread derives from its number is made anew for every model: held over the loop it costs the registers
    // that the shares need)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
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
    double* const a = a_ + b * hw;
    const float* const source = source_ ? source_ + b * hw : nullptr;
    const float* const weights = weights_ + b * K * hw;
    for (int i = tid; i < kMH * kMH; i += kMRelax) {
      const int x = row0 + i / kMH - 1, y = col0 + i % kMH - 1;
      double v = 0.0;  // (a position off the grid has no share towards anybody: never read)
      if (x >= 0 && y >= 0 && x < H && y < W)
        v = first ? (source ? static_cast<double>(source[at(x, y)]) : 1.0) : a[at(x, y)];
      if (v != v) v = __builtin_nan("");  // (a NaN source, which a cell without donors keeps: the canonical one)
      sd[i] = v;
    }
    // this thread's cells: their sources and the shares that come in, neighbour k's plane kMOpp[k] at k's index
    float win[kMCells][K];
    float src[kMCells];
    bool in[kMCells], mv[kMCells];
    bool any_in = false;
#pragma unroll
    for (int j = 0; j < kMCells; ++j) {
      const int c = tid + j * kMRelax;
      const int x = row0 + c / kMT, y = col0 + c % kMT;
      in[j] = x < H && y < W;
      mv[j] = false;
      src[j] = in[j] && source ? source[at(x, y)] : 1.0f;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int nx = x + kMDX[k], ny = y + kMDY[k];
        const bool okk = in[j] && nx >= 0 && ny >= 0 && nx < H && ny < W;
        win[j][k] = okk ? weights[kMOpp[k] * hw + at(nx, ny)] : 0.0f;
        mv[j] = mv[j] || win[j][k] != 0.0f;  // (a NaN share cannot be: a share is P / Z of a finite Z > 0, 0 or 1)
      }
      any_in = any_in || mv[j];
    }
    if (tid == 0) s_flag[0] = 0, s_flag[1] = 0;
    __syncthreads();
    if (first) {
      if (any_in) s_flag[0] = 1;
      __syncthreads();
      const bool is_inert = s_flag[0] == 0;
      __syncthreads();  // (s_flag[0] is read above and cleared below)
      if (tid == 0) inert[tile] = is_inert ? 1 : 0, s_flag[0] = 0;
      if (is_inert) {  // nothing arrives, now or ever: a = source
#pragma unroll
        for (int j = 0; j < kMCells; ++j) {
          const int c = tid + j * kMRelax;
          if (in[j]) a[at(row0 + c / kMT, col0 + c % kMT)] = sd[(c / kMT + 1) * kMH + (c % kMT + 1)];
        }
        if (tid == 0) dirty_next[tile] = 0;
        continue;
      }
      __syncthreads();
    }
    bool any = false;
    for (int it = 0; it < inner_max; ++it) {
      double nv[kMCells];
      bool moved = false;
#pragma unroll
      for (int j = 0; j < kMCells; ++j) {
        if (!mv[j]) continue;
        const int c = tid + j * kMRelax;
        const int p = (c / kMT + 1) * kMH + (c % kMT + 1);
        double s = static_cast<double>(src[j]);
#pragma unroll
        for (int k = 0; k < K; ++k)
          if (win[j][k] != 0.0f)  // a zero share is skipped: an infinite donor never makes inf * 0
            s = __dadd_rn(s, __dmul_rn(sd[p + kMDX[k] * kMH + kMDY[k]], static_cast<double>(win[j][k])));
        if (s != s) s = __builtin_nan("");  // the canonical quiet NaN
        nv[j] = s;
        moved = moved || mfd_bits(s) != mfd_bits(sd[p]);
      }
      __syncthreads();  // every cell has read the sweep before
      if (tid == 0) s_flag[(it + 1) & 1] = 0;  // (last read before this barrier, next set after the one below)
      if (moved) {
#pragma unroll
        for (int j = 0; j < kMCells; ++j) {
          const int c = tid + j * kMRelax;
          if (mv[j]) sd[(c / kMT + 1) * kMH + (c % kMT + 1)] = nv[j];
        }
        s_flag[it & 1] = 1;
      }
      __syncthreads();
      if (s_flag[it & 1] == 0) break;
      any = true;
    }
    if (any || first) {
#pragma unroll
      for (int j = 0; j < kMCells; ++j) {
        const int c = tid + j * kMRelax;
        if (in[j]) a[at(row0 + c / kMT, col0 + c % kMT)] = sd[(c / kMT + 1) * kMH + (c % kMT + 1)];
      }
    }
    if (tid == 0) {
      if (any) *changed = 1;  // one word for the whole batch: any tile of any model
      dirty_next[tile] = any ? 1 : 0;
    }
  }
}

// out = the double rounded once to float
__global__ void __launch_bounds__(kMBlock)
    k_mfd_round(float* __restrict__ out, const double* __restrict__ a, int64_t n) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kMBlock + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kMBlock)
    out[i] = __double2float_rn(a[i]);
}

// What the last call of soil_mfd_accumulate(_batch) on this host thread did (soil_mfd_info)
struct MfdInfo {
  int64_t launches, tiles, models, looks;
};
static thread_local MfdInfo t_mfd_info{0, 0, 0, 0};

struct MfdCall {
  const float* height;
  const int32_t* dist;
  int kind;
  double param;
  int64_t B, H, W;
  const float* scales;
  int64_t n_scales;
  int edge;
  hipStream_t st;
};

inline MfdLen mfd_len(const float* pair) {
  if (!pair) return MfdLen{1.0, 1.0, 1.0};  // (the Gibbs kind reads none)
  const double sx = static_cast<double>(pair[0]), sy = static_cast<double>(pair[1]);
  return MfdLen{sx, sy, std::sqrt(sx * sx + sy * sy)};  // (flow_paths.hpp: path_scale)
}

template <int K, bool POWER, bool DIST>
static int mfd_weights_launch(float* weights, const MfdCall& c, const MfdLen* lens) {
  MfdKind kind{RwConst{0.0f, 0.0f}, c.param};
  if (!POWER) kind.rc = rw_const(static_cast<float>(c.param));
  dim3 grid = grid_rows(c.H, c.W, kMBlock);
  grid.z = static_cast<unsigned>(c.B < 65535 ? c.B : 65535);
  k_mfd_weights<K, POWER, DIST><<<grid, kMBlock, 0, c.st>>>(weights, c.height, c.dist, kind, mfd_len(c.scales), lens,
                                                           c.B, c.H, c.W);
  SOIL_LAUNCH_CHECK();
  return SOIL_OK;
}

// The weights pass of a call, stream-ordered.  `recs`: room for B MfdLen records on the device (read only with B
// pairs of scales and the power kind).
static int mfd_weights_run(float* weights, const MfdCall& c, void* recs) {
  const bool power = c.kind == SOIL_MFD_POWER;
  const MfdLen* lens = nullptr;
  if (power && c.n_scales > 1) {
    if (int rc = upload_scale_records(recs, c.scales, c.B, mfd_len, c.st); rc != SOIL_OK) return rc;
    lens = static_cast<const MfdLen*>(recs);
  }
  const int which = (c.edge == SOIL_D8 ? 4 : 0) + (power ? 2 : 0) + (c.dist ? 1 : 0);
  switch (which) {
    case 0: return mfd_weights_launch<4, false, false>(weights, c, lens);
    case 1: return mfd_weights_launch<4, false, true>(weights, c, lens);
    case 2: return mfd_weights_launch<4, true, false>(weights, c, lens);
    case 3: return mfd_weights_launch<4, true, true>(weights, c, lens);
    case 4: return mfd_weights_launch<8, false, false>(weights, c, lens);
    case 5: return mfd_weights_launch<8, false, true>(weights, c, lens);
    case 6: return mfd_weights_launch<8, true, false>(weights, c, lens);
    default: return mfd_weights_launch<8, true, true>(weights, c, lens);
  }
}

static size_t mfd_rec_bytes(const MfdCall& c) {
  return c.kind == SOIL_MFD_POWER && c.n_scales > 1 ? align256(sizeof(MfdLen) * static_cast<size_t>(c.B)) : 0;
}

template <int K>
static int mfd_accumulate_run(float* out, double* out64, const float* source, const MfdCall& c) {
  const int64_t B = c.B, H = c.H, W = c.W;
  hipStream_t st = c.st;
  const int tiles_w = static_cast<int>((W + kMT - 1) / kMT);
  const int tiles_h = static_cast<int>((H + kMT - 1) / kMT);
  const size_t ntiles = static_cast<size_t>(tiles_w) * tiles_h;
  t_mfd_info = MfdInfo{0, static_cast<int64_t>(ntiles), B, 0};
  const size_t cells = static_cast<size_t>(B) * static_cast<size_t>(H * W);
  const size_t b_recs = mfd_rec_bytes(c);
  const size_t b_marks = align256(ntiles * static_cast<size_t>(B));
  const size_t b_weights = align256(sizeof(float) * K * cells);
  const size_t b_iter = out64 ? 0 : align256(sizeof(double) * cells);
  void* base = nullptr;
  if (int rc = workspace_get(WS_MFD, b_recs + 3 * b_marks + b_weights + b_iter, &base); rc != SOIL_OK) return rc;
  unsigned char* dirty_prev = static_cast<unsigned char*>(base) + b_recs;
  unsigned char* dirty_next = dirty_prev + b_marks;
  unsigned char* const inert = dirty_next + b_marks;
  float* const weights = reinterpret_cast<float*>(inert + b_marks);
  double* const a = out64 ? out64 : reinterpret_cast<double*>(reinterpret_cast<char*>(weights) + b_weights);
  if (int rc = mfd_weights_run(weights, c, base); rc != SOIL_OK) return rc;
  // "some tile moved in this launch": a pinned, device-mapped word the tiles write straight into (one per host
  // thread and device, as in slope_limit.hip)
  static thread_local ThreadOwned<PinnedWord> t_flags;  // (goes with the thread: common.hpp)
  int dev = 0;
  SOIL_HIP(hipGetDevice(&dev));
  PinnedWord& fl = t_flags[dev];
  SOIL_HIP(fl.ensure());
  int *const flag_host = fl.host, *const flag_dev = fl.dev;
  // the bound of the file's header
  const int64_t max_launches = static_cast<int64_t>(ntiles) * (4 * kMT + kMT * kMT / kMInner) + 2;
  const char* const e = std::getenv("SOIL_MFD_PER_CHECK");  // read per call
  const int per_env = e ? std::atoi(e) : 4;
  const int per_check = per_env >= 1 ? per_env : 4;
  const dim3 grid(static_cast<unsigned>(ntiles), static_cast<unsigned>(B < 65535 ? B : 65535));
  bool settled = false;
  for (int64_t launch = 0; launch < max_launches && !settled; launch += per_check) {
    *flag_host = 0;  // the stream is idle here: the previous launches were waited for
    for (int k = 0; k < per_check; ++k) {
      k_mfd_relax<K><<<grid, kMRelax, 0, st>>>(a, source, weights, B, static_cast<int>(H), static_cast<int>(W), tiles_w,
                                              tiles_h, kMInner, flag_dev, dirty_prev, dirty_next, inert,
                                              launch + k == 0 ? 1 : 0);
      std::swap(dirty_prev, dirty_next);
    }
    SOIL_LAUNCH_CHECK();
    SOIL_HIP(hipStreamSynchronize(st));
    t_mfd_info.launches += per_check;
    t_mfd_info.looks += 1;
    settled = !__atomic_load_n(flag_host, __ATOMIC_ACQUIRE);
  }
  if (!settled) return fail(SOIL_ERR_HIP, "mfd_accumulate: internal error: the launch bound was reached");
  if (out) {
    const int64_t n = static_cast<int64_t>(cells);
    const int64_t blocks = (n + kMBlock - 1) / kMBlock;
    k_mfd_round<<<static_cast<unsigned>(blocks < 65535 * 16 ? blocks : 65535 * 16), kMBlock, 0, st>>>(out, a, n);
    SOIL_LAUNCH_CHECK();
    SOIL_HIP(hipStreamSynchronize(st));
  }
  return SOIL_OK;
}

// What the entries refuse before any device work, under the entry's name
static int check_mfd(const std::string& w, const MfdCall& c) {
  SOIL_REQUIRE(c.height, w + ": null tensor");
  if (int rc = check_grid_batch(w, c.B, c.H, c.W, c.edge, c.n_scales, ""); rc != SOIL_OK) return rc;
  SOIL_REQUIRE(c.kind == SOIL_MFD_GIBBS || c.kind == SOIL_MFD_POWER, w + ": invalid kind enumerator");
  if (c.kind == SOIL_MFD_GIBBS) {
    SOIL_REQUIRE(rw_temperature_ok(static_cast<float>(c.param)), w + ": T must be 0 or a normal positive float");
  } else {  // (the Gibbs kind reads no scale)
    SOIL_REQUIRE(c.param >= 0.0 && c.param <= 16.0, w + ": p must be a finite number in 0 .. 16");
    SOIL_REQUIRE(c.scales, w + ": null scale (kind power needs the spacings)");
    if (int rc = check_scales_positive(w, c.scales, c.n_scales); rc != SOIL_OK) return rc;
  }
  return SOIL_OK;
}

static int mfd_weights_entry(const char* what, float* weights, const MfdCall& c) {
  const std::string w(what);
  SOIL_REQUIRE(weights, w + ": null tensor");
  if (int rc = check_mfd(w, c); rc != SOIL_OK) return rc;
  const size_t cells = plane_cells(c.B, c.H * c.W);
  const size_t k = c.edge == SOIL_D8 ? 8 : 4;
  for (const void* q : {static_cast<const void*>(c.height), static_cast<const void*>(c.dist)})
    SOIL_REQUIRE(!overlaps(weights, 4 * k * cells, q, 4 * cells), w + ": an output aliases an input plane");
  SOIL_DEVICE();
  void* recs = nullptr;
  if (const size_t bytes = mfd_rec_bytes(c); bytes)
    if (int rc = workspace_get(WS_MFD, bytes, &recs); rc != SOIL_OK) return rc;
  return mfd_weights_run(weights, c, recs);
}

static int mfd_accumulate_entry(const char* what, float* out, double* out64, const float* source, const MfdCall& c) {
  const std::string w(what);
  SOIL_REQUIRE(out || out64, w + ": both outputs are null");
  if (int rc = check_mfd(w, c); rc != SOIL_OK) return rc;
  if (int rc = check_outputs_apart(w, out, out64, plane_cells(c.B, c.H * c.W), {c.height, source, c.dist});
      rc != SOIL_OK)
    return rc;
  SOIL_DEVICE();
  return c.edge == SOIL_D4 ? mfd_accumulate_run<4>(out, out64, source, c) : mfd_accumulate_run<8>(out, out64, source, c);
}

}  // namespace soil

using namespace soil;

extern "C" {

int soil_mfd_weights(float* weights, const float* height, const int32_t* dist, int kind, double param, int64_t H,
                     int64_t W, const float scale[2], int edge, void* stream) {
  return mfd_weights_entry("mfd_weights", weights,
                           MfdCall{height, dist, kind, param, 1, H, W, scale, 1, edge, as_stream(stream)});
}

int soil_mfd_weights_batch(float* weights, const float* height, const int32_t* dist, int kind, double param, int64_t B,
                           int64_t H, int64_t W, const float* scales, int64_t n_scales, int edge, void* stream) {
  return mfd_weights_entry("mfd_weights_batch", weights,
                           MfdCall{height, dist, kind, param, B, H, W, scales, n_scales, edge, as_stream(stream)});
}

int soil_mfd_accumulate(float* out, double* out64, const float* height, const float* source, const int32_t* dist,
                        int kind, double param, int64_t H, int64_t W, const float scale[2], int edge, void* stream) {
  return mfd_accumulate_entry("mfd_accumulate", out, out64, source,
                              MfdCall{height, dist, kind, param, 1, H, W, scale, 1, edge, as_stream(stream)});
}

int soil_mfd_accumulate_batch(float* out, double* out64, const float* height, const float* source, const int32_t* dist,
                              int kind, double param, int64_t B, int64_t H, int64_t W, const float* scales,
                              int64_t n_scales, int edge, void* stream) {
  return mfd_accumulate_entry("mfd_accumulate_batch", out, out64, source,
                              MfdCall{height, dist, kind, param, B, H, W, scales, n_scales, edge, as_stream(stream)});
}

int soil_mfd_info(int64_t info[4]) {
  SOIL_REQUIRE(info, "mfd_info: null info");
  info[0] = t_mfd_info.launches, info[1] = t_mfd_info.tiles;
  info[2] = t_mfd_info.models, info[3] = t_mfd_info.looks;
  return SOIL_OK;
}

}  // extern "C"
