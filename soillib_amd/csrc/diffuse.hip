// diffuse.hip — hillslope diffusion: one locally one-dimensional backward-Euler step of dh/dt = div(kappa grad h) + u
// (soil_diffuse / soil_diffuse_batch, soil_hip.h "hillslope diffusion").  The reference has no diffusion of any kind;
// its example/dem_process.py carries a commented-out explicit diffuse().
//
// A step is two sweeps, one along each axis, and a sweep is a tridiagonal (Thomas) solve per grid line: forward
//
//   den = b - p g[i-1],  e[i] = (d[i] + p e[i-1]) / den,  g[i] = q / den
//
// and back x[i] = e[i] + g[i] x[i+1], every operation a single correctly rounded fp64 operation in the order
// soil_hip.h writes down, so the result is one definite bit pattern.  The recurrence is serial along a line; the
// lines are independent, and a sweep is ONE launch of k_diff_cols in which a thread owns a column, walks it forward —
// e and g go to two fp64 scratch planes in the cells' own order, 16 bytes a cell — and walks it back over what it
// wrote.  The back-substitution is in place: x goes where e was.  Lanes stand on adjacent columns, so every row step
// of a wave is one coalesced access per plane; the planes' loads do not depend on the recurrence and run a block of
// kAhead rows ahead of the division chain.  A thread reads back from the scratch planes exactly the words it wrote
// itself: no pass depends on another thread's global stores within a launch.
//
// The sweep along axis 1 is the same kernel on the transposed planes.  A thread per row would read with a stride of
// W; a first version staged 64 x 64 tiles of the rows through LDS inside the sweep (one wave a row block, e and g
// carried across tiles) and took 4.5 to 6 times the column sweep's time, a single wave having nobody to hide its
// tile loads behind.  Instead k_diff_transpose moves the planes through padded 32 x 33 LDS tiles,
// coalesced on both sides and bound by bandwidth, not by latency; the arithmetic of a line is the same whichever way
// the plane lies, so the bits are the same.  With first_axis == 0: column sweep, transposes (h, k, fixed; x),
// column sweep on the transposed planes, k_diff_output (transposes x back and writes out / out64).  With
// first_axis == 1: transposes (h, k, fixed, u), column sweep there, transpose of x, column sweep that writes the
// outputs itself.  Five and four launches a chunk, whatever B is.
//
// The model is on grid.y of the sweeps and grid.z of the transposes (a batch's chunk: at most 65535 whole models), its
// planes reached through a uniform base, so the single grid pays nothing for the batch form: B == 1 is one model of
// the same kernels.  Within a model a cell is addressed by a 32-bit byte offset where 8 H W < 2^32, by a 64-bit
// index otherwise (IDX).
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "common.hpp"
#include "flow_host.hpp"

namespace soil {

constexpr int kDiffLanes = 64;   // work-group of k_diff_cols: one wave
constexpr int kAhead = 8;        // k_diff_cols: rows to a block; the loads run a block ahead of the chain
constexpr int kTrTile = 32;      // k_diff_transpose, k_diff_output: a tile's rows and columns, 32 x 8 threads
constexpr int64_t kDiffMaxGridY = 65535;

struct DiffScale {  // the squares of the spacings along axis 0 and axis 1, made on the host in double
  double ss0, ss1;
};
struct DiffScales {
  const DiffScale* per_model;  // null: `one` for every model
  DiffScale one;
};
struct DiffArgs {
  const float* h;
  const float* k;        // diffusivity plane or null (kappa)
  const float* u;        // uplift or null
  const int32_t* fixed;  // or null
  double* E;             // scratch: e, then x in place
  double* G;             // scratch: g
  float* out;            // the second sweep's outputs, either may be null
  double* out64;
  int64_t H, W;         // of the planes as this launch sees them: (W, H) of the call on the transposed planes
  int axis;             // the call's axis this sweep runs along: which spacing
  double kappa, dt;
  int border;
  bool has_k, has_u, has_fixed;  // an absent plane's pointer stands on `h` in the kernels: see model_of
  DiffScales scales;
};

template <typename IDX, typename T>
__device__ __forceinline__ T* cell_at(T* base, IDX n) {
  if constexpr (sizeof(IDX) == 4) {
    using Byte = std::conditional_t<std::is_const_v<T>, const char, char>;
    return reinterpret_cast<T*>(reinterpret_cast<Byte*>(base) + static_cast<uint32_t>(n * static_cast<uint32_t>(sizeof(T))));
  } else {
    return base + n;
  }
}

// The face weight between two cells: (kf dt) / ss, the product rounded, then the quotient
__device__ __forceinline__ double face_weight(float ka, float kb, double dt, double ss) {
  const double kf = __dmul_rn(0.5, __dadd_rn(static_cast<double>(ka), static_cast<double>(kb)));
  return __ddiv_rn(__dmul_rn(kf, dt), ss);
}

// The carried state of a line's forward pass and one cell of it.  `free`: the cell is free; `link_next`: it is linked
// to the next cell of the line; wq: the weight of the face between them (read only where both hold).
struct Fwd {
  double e = 0.0, g = 0.0, w = 0.0;  // of the cell before: e, g and the weight of the face towards this one
  bool link = false;                 // whether the cell before is linked to this one
};
__device__ __forceinline__ void fwd_cell(Fwd& s, double d, double wq, bool free, bool link_next, double& e, double& g) {
  const bool lp = free && s.link;
  const double p = lp ? s.w : 0.0;
  const double q = (free && link_next) ? wq : 0.0;
  const double b = __dadd_rn(__dadd_rn(1.0, p), q);
  const double den = lp ? __dsub_rn(b, __dmul_rn(p, s.g)) : b;
  const double num = lp ? __dadd_rn(d, __dmul_rn(p, s.e)) : d;
  e = __ddiv_rn(num, den);
  g = __ddiv_rn(q, den);
  s.e = e, s.g = g, s.w = wq, s.link = link_next;
}

__device__ __forceinline__ bool on_border(int border, int64_t x, int64_t y, int64_t H, int64_t W) {
  return border != 0 && (x == 0 || x == H - 1 || y == 0 || y == W - 1);
}

__device__ __forceinline__ void write_out(float* out, double* out64, double x) {
  const bool nan = x != x;
  if (out) *out = nan ? bits2f(0x7fc00000u) : __double2float_rn(x);
  if (out64) *out64 = nan ? __hiloint2double(0x7ff80000, 0) : x;
}

// The model of this work-group: its planes and its squared spacing along the sweep's axis.  The pointer of an absent
// plane is put on the heights: every load of the kernels is then unconditional — no branch stands between the loads
// of a block, and the counters of outstanding loads stay exact, which is what lets them run ahead of the chain —
// and what was read through it is dropped by a select on has_*.
__device__ __forceinline__ double model_of(DiffArgs& a) {
  const int64_t first = static_cast<int64_t>(blockIdx.y) * a.H * a.W;
  a.h += first;
  a.k = a.has_k ? a.k + first : a.h;
  a.u = a.has_u ? a.u + first : a.h;
  a.fixed = a.has_fixed ? a.fixed + first : reinterpret_cast<const int32_t*>(a.h);
  a.E += first, a.G += first;
  if (a.out) a.out += first;
  if (a.out64) a.out64 += first;
  const DiffScale s = a.scales.per_model ? a.scales.per_model[blockIdx.y] : a.scales.one;
  return a.axis == 0 ? s.ss0 : s.ss1;
}

// ---- a sweep: a thread per column --------------------------------------------------------------------------------

struct ColCell {  // what the forward pass reads of one cell
  float h, k, u;
  int32_t fx;
  double d;  // the second sweep: the first sweep's x
};
// Row x of column y, without a branch: a row past the end is read from the last row and made void (linked to nothing)
template <typename IDX, bool FIRST>
__device__ __forceinline__ ColCell col_load(const DiffArgs& a, int64_t x, int64_t y) {
  const bool past = x >= a.H;
  const IDX n = static_cast<IDX>(y) + static_cast<IDX>(past ? a.H - 1 : x) * static_cast<IDX>(a.W);
  ColCell c;
  c.h = *cell_at<IDX>(a.h, n);
  c.k = *cell_at<IDX>(a.k, n);
  c.fx = *cell_at<IDX>(a.fixed, n);
  c.u = 0.0f, c.d = 0.0;
  if constexpr (FIRST) c.u = *cell_at<IDX>(a.u, n);
  else c.d = *cell_at<IDX>(a.E, n);
  c.h = past ? bits2f(0x7fc00000u) : c.h;
  c.fx = a.has_fixed ? c.fx : 0;
  return c;
}

struct BackCell {  // what the way back reads of one cell
  double e, g;
  float h;
  int32_t fx;
};
template <typename IDX>
__device__ __forceinline__ BackCell back_load(const DiffArgs& a, int64_t x, int64_t y) {
  const IDX n = static_cast<IDX>(y) + static_cast<IDX>(x < 0 ? 0 : x) * static_cast<IDX>(a.W);  // (x < 0: never used)
  BackCell c;
  c.e = *cell_at<IDX>(a.E, n);
  c.g = *cell_at<IDX>(a.G, n);
  c.h = *cell_at<IDX>(a.h, n);
  c.fx = *cell_at<IDX>(a.fixed, n);
  c.fx = a.has_fixed ? c.fx : 0;
  return c;
}

// MODE 0: the first sweep (d from the heights and the uplift, x left in E); 1: the second sweep with x left in E (the
// transposed planes: k_diff_output writes the outputs); 2: the second sweep writing out / out64 itself.
template <typename IDX, int MODE>
__global__ void __launch_bounds__(kDiffLanes) k_diff_cols(DiffArgs a) {
  constexpr bool FIRST = MODE == 0;
  const int64_t y = static_cast<int64_t>(blockIdx.x) * kDiffLanes + threadIdx.x;
  if (y >= a.W) return;
  const double ss = model_of(a);
  const int64_t H = a.H, W = a.W;
  const double w_const = __ddiv_rn(__dmul_rn(a.kappa, a.dt), ss);
  const IDX step = static_cast<IDX>(W);

  // forward: cell x from its own words and the height and diffusivity of cell x + 1
  Fwd s;
  auto forward = [&](int64_t x, const ColCell& cur, const ColCell& next) {
    const bool isvoid = cur.h != cur.h;
    const bool link_next = !isvoid && !(next.h != next.h);
    const bool free = !isvoid && cur.fx == 0 && !on_border(a.border, x, y, H, W);
    const double wq = a.has_k ? face_weight(cur.k, next.k, a.dt, ss) : w_const;
    double d;
    if constexpr (FIRST) {
      const double h = static_cast<double>(cur.h);
      d = (free && a.has_u) ? __dadd_rn(h, __dmul_rn(a.dt, static_cast<double>(cur.u))) : h;
    } else {
      d = cur.d;
    }
    double e, g;
    fwd_cell(s, d, wq, free, link_next, e, g);
    const IDX n = static_cast<IDX>(y) + static_cast<IDX>(x) * step;
    *cell_at<IDX>(a.E, n) = e;
    *cell_at<IDX>(a.G, n) = g;
  };
  // Whole blocks of kAhead rows, the loads a block ahead: while the chain walks the rows of `nx`, the rows of the block
  // after it are on their way (`nn`).  The second sweep reads a row's d from E before that row's e goes there: loads
  // only ever run ahead of the stores.  Then the rows that are left, one at a time.
  ColCell cur = col_load<IDX, FIRST>(a, 0, y);
  int64_t x0 = 0;
  if (H >= kAhead) {
    ColCell nx[kAhead];
#pragma unroll
    for (int j = 0; j < kAhead; ++j) nx[j] = col_load<IDX, FIRST>(a, j + 1, y);
    for (; x0 + kAhead <= H; x0 += kAhead) {
      ColCell nn[kAhead];
#pragma unroll
      for (int j = 0; j < kAhead; ++j) nn[j] = col_load<IDX, FIRST>(a, x0 + kAhead + j + 1, y);
#pragma unroll
      for (int j = 0; j < kAhead; ++j) {
        forward(x0 + j, cur, nx[j]);
        cur = nx[j];
      }
#pragma unroll
      for (int j = 0; j < kAhead; ++j) nx[j] = nn[j];
    }
  }
  for (; x0 < H; ++x0) {
    const ColCell next = col_load<IDX, FIRST>(a, x0 + 1, y);
    forward(x0, cur, next);
    cur = next;
  }

  // back, in place: x[i] = e[i] + g[i] x[i + 1] where cell i is free and linked to cell i + 1; blocks as above
  double x_next = 0.0;
  float h_next = bits2f(0x7fc00000u);
  auto back = [&](int64_t x, const BackCell& c) {
    const bool use = !(c.h != c.h) && !(h_next != h_next) && c.fx == 0 && !on_border(a.border, x, y, H, W);
    const double v = use ? __dadd_rn(c.e, __dmul_rn(c.g, x_next)) : c.e;
    const IDX n = static_cast<IDX>(y) + static_cast<IDX>(x) * step;
    if constexpr (MODE != 2) *cell_at<IDX>(a.E, n) = v;
    else write_out(a.out ? cell_at<IDX>(a.out, n) : nullptr, a.out64 ? cell_at<IDX>(a.out64, n) : nullptr, v);
    x_next = v, h_next = c.h;
  };
  int64_t x1 = H;
  if (H >= kAhead) {
    BackCell bc[kAhead];
#pragma unroll
    for (int j = 0; j < kAhead; ++j) bc[j] = back_load<IDX>(a, H - 1 - j, y);
    for (; x1 - kAhead >= 0; x1 -= kAhead) {
      BackCell bn[kAhead];
#pragma unroll
      for (int j = 0; j < kAhead; ++j) bn[j] = back_load<IDX>(a, x1 - 1 - kAhead - j, y);
#pragma unroll
      for (int j = 0; j < kAhead; ++j) back(x1 - 1 - j, bc[j]);
#pragma unroll
      for (int j = 0; j < kAhead; ++j) bc[j] = bn[j];
    }
  }
  for (; x1 > 0; --x1) back(x1 - 1, back_load<IDX>(a, x1 - 1, y));
}

// ---- transposes ------------------------------------------------------------------------------------------------

// Up to four planes of (H, W) elements of type T, each to its (W, H) transpose, the model on grid.z.  Tiles of 32 x 32
// through a padded LDS image; the tiles of the longer side are on grid.x (`rows_on_x`: those of the rows), the other
// side has at most 2^15.5 / 32 of them.
struct TrJobs {
  const void* src[4];
  void* dst[4];
  int n;
};
struct TrTile {
  int64_t x0, y0;
  int tx, ty;
};
__device__ __forceinline__ TrTile tr_tile(bool rows_on_x) {
  const int64_t bx = blockIdx.x, by = blockIdx.y;
  return TrTile{(rows_on_x ? bx : by) * kTrTile, (rows_on_x ? by : bx) * kTrTile, static_cast<int>(threadIdx.x & 31u),
                static_cast<int>(threadIdx.x >> 5)};
}
template <typename T>
__global__ void __launch_bounds__(256) k_diff_transpose(TrJobs jobs, int64_t H, int64_t W, bool rows_on_x) {
  __shared__ T tile[kTrTile][kTrTile + 1];
  const TrTile t = tr_tile(rows_on_x);
  const int64_t first = static_cast<int64_t>(blockIdx.z) * H * W;
  for (int j = 0; j < jobs.n; ++j) {
    const T* const src = static_cast<const T*>(jobs.src[j]) + first;
    T* const dst = static_cast<T*>(jobs.dst[j]) + first;
    for (int r = t.ty; r < kTrTile; r += 8) {
      const int64_t x = t.x0 + r, y = t.y0 + t.tx;
      if (x < H && y < W) tile[r][t.tx] = src[x * W + y];
    }
    __syncthreads();
    for (int r = t.ty; r < kTrTile; r += 8) {
      const int64_t y = t.y0 + r, x = t.x0 + t.tx;
      if (x < H && y < W) dst[y * H + x] = tile[t.tx][r];
    }
    __syncthreads();
  }
}
// x of the second sweep, (Hs, Ws) = (W, H) of the call, back to the call's order and out: out64 = x, out = (float)x,
// the canonical NaN words
__global__ void __launch_bounds__(256) k_diff_output(const double* __restrict__ xs, float* __restrict__ out,
                                                    double* __restrict__ out64, int64_t Hs, int64_t Ws, bool rows_on_x) {
  __shared__ double tile[kTrTile][kTrTile + 1];
  const TrTile t = tr_tile(rows_on_x);
  const int64_t first = static_cast<int64_t>(blockIdx.z) * Hs * Ws;
  for (int r = t.ty; r < kTrTile; r += 8) {
    const int64_t x = t.x0 + r, y = t.y0 + t.tx;
    if (x < Hs && y < Ws) tile[r][t.tx] = xs[first + x * Ws + y];
  }
  __syncthreads();
  for (int r = t.ty; r < kTrTile; r += 8) {
    const int64_t y = t.y0 + r, x = t.x0 + t.tx;
    if (x < Hs && y < Ws) {
      const int64_t n = first + y * Hs + x;
      write_out(out ? out + n : nullptr, out64 ? out64 + n : nullptr, tile[t.tx][r]);
    }
  }
}

// ---- host -------------------------------------------------------------------------------------------------------

struct DiffInfo {  // soil_diffuse_info
  int64_t launches, chunks, idx64_chunks, scratch_bytes;
};
static thread_local DiffInfo t_diff_info{0, 0, 0, 0};

static dim3 tr_grid(int64_t H, int64_t W, int64_t models, bool* rows_on_x) {
  const unsigned th = blocks_for(H, kTrTile), tw = blocks_for(W, kTrTile);
  *rows_on_x = th > tw;
  return dim3(th > tw ? th : tw, th > tw ? tw : th, static_cast<unsigned>(models));
}
template <typename T>
static void diff_transpose(const TrJobs& jobs, int64_t H, int64_t W, int64_t models, hipStream_t st) {
  bool rows_on_x = false;
  const dim3 grid = tr_grid(H, W, models, &rows_on_x);
  k_diff_transpose<T><<<grid, 256, 0, st>>>(jobs, H, W, rows_on_x);
}

// The scratch planes of a chunk: e / x and g, x transposed, and the transposed inputs
struct DiffScratch {
  double *E, *G, *ET;
  float *hT, *kT, *uT;
  int32_t* fT;
};

// The launches of one chunk of `models` models; `a` holds the call's planes and shape.  Returns their number.
template <typename IDX>
static int diff_launch(const DiffArgs& a, const DiffScratch& w, int64_t models, int first_axis, hipStream_t st) {
  const int64_t H = a.H, W = a.W;
  const dim3 cols(blocks_for(W, kDiffLanes), static_cast<unsigned>(models));
  const dim3 colsT(blocks_for(H, kDiffLanes), static_cast<unsigned>(models));
  DiffArgs n = a, t = a;  // the sweep on the planes as they lie, and on the transposed ones
  n.axis = 0, n.E = w.E, n.G = w.G;
  t.axis = 1, t.H = W, t.W = H, t.E = w.ET, t.G = w.G;
  t.h = w.hT, t.k = a.has_k ? w.kT : nullptr, t.u = a.has_u ? w.uT : nullptr, t.fixed = a.has_fixed ? w.fT : nullptr;
  t.out = nullptr, t.out64 = nullptr;
  TrJobs in{{a.h, nullptr, nullptr, nullptr}, {w.hT, nullptr, nullptr, nullptr}, 1};
  auto add = [&](const void* src, void* dst) { in.src[in.n] = src, in.dst[in.n] = dst, ++in.n; };
  if (a.has_k) add(a.k, w.kT);
  if (a.has_fixed) add(a.fixed, w.fT);
  if (first_axis == 0) {
    k_diff_cols<IDX, 0><<<cols, kDiffLanes, 0, st>>>(n);
    diff_transpose<uint32_t>(in, H, W, models, st);
    diff_transpose<double>(TrJobs{{w.E, nullptr, nullptr, nullptr}, {w.ET, nullptr, nullptr, nullptr}, 1}, H, W, models, st);
    k_diff_cols<IDX, 1><<<colsT, kDiffLanes, 0, st>>>(t);
    bool rows_on_x = false;
    const dim3 grid = tr_grid(W, H, models, &rows_on_x);
    k_diff_output<<<grid, 256, 0, st>>>(w.ET, a.out, a.out64, W, H, rows_on_x);
    return 5;
  }
  if (a.has_u) add(a.u, w.uT);
  diff_transpose<uint32_t>(in, H, W, models, st);
  k_diff_cols<IDX, 0><<<colsT, kDiffLanes, 0, st>>>(t);
  diff_transpose<double>(TrJobs{{w.ET, nullptr, nullptr, nullptr}, {w.E, nullptr, nullptr, nullptr}, 1}, W, H, models, st);
  k_diff_cols<IDX, 2><<<cols, kDiffLanes, 0, st>>>(n);
  return 4;
}

// What both entries refuse before any device work, under the entry's name
static int check_diffuse(const char* what, const void* out, const void* out64, const float* height,
                         const float* diffusivity, const float* uplift, const int32_t* fixed, int64_t B, int64_t H,
                         int64_t W, const float* scales, int64_t n_scales, double kappa, double dt, int border,
                         int first_axis) {
  const std::string w(what);
  SOIL_REQUIRE(height, w + ": null height");
  SOIL_REQUIRE(out || out64, w + ": no output asked for (out and out64 are both null)");
  SOIL_REQUIRE(scales, w + ": null scale");
  if (int rc = check_grid_batch(w, B, H, W, SOIL_D8, n_scales, ""); rc != SOIL_OK) return rc;
  if (int rc = check_scales_positive(w, scales, n_scales); rc != SOIL_OK) return rc;
  if (int rc = check_dt(w, dt); rc != SOIL_OK) return rc;
  SOIL_REQUIRE(diffusivity || (kappa >= 0.0 && std::isfinite(kappa)),
               w + ": kappa must be finite and >= 0 where there is no diffusivity plane");
  SOIL_REQUIRE(border == 0 || border == 1, w + ": border must be 0 or 1");
  SOIL_REQUIRE(first_axis == 0 || first_axis == 1, w + ": first_axis must be 0 or 1");
  return check_outputs_apart(w, out, out64, plane_cells(B, H * W), {height, diffusivity, uplift, fixed});
}

static DiffScale diff_scale(const float pair[2]) {
  const double sx = static_cast<double>(pair[0]), sy = static_cast<double>(pair[1]);
  return DiffScale{sx * sx, sy * sy};  // (the square of a float is exact in fp64)
}

// A call: chunks of whole models one after the other on `st`, five or four launches a chunk, through one block of
// workspace slot WS_DIFFUSE: the per-model scale records first, then the chunk's scratch planes.
static int diffuse_run(float* out, double* out64, const float* height, const float* diffusivity, const float* uplift,
                       const int32_t* fixed, int64_t B, int64_t H, int64_t W, const float* scales, int64_t n_scales,
                       double kappa, double dt, int border, int first_axis, hipStream_t st) {
  // Models per chunk: whole models, at most 2^28 - 1 cells (4 GiB of e and g), at most a launch's grid.y
  const int64_t hw = H * W, per = chunk_models((int64_t{1} << 28) - 1, hw, kDiffMaxGridY);
  const int64_t first_chunk = B < per ? B : per;
  const bool per_model = n_scales > 1;
  const size_t b_scales = per_model ? align256(sizeof(DiffScale) * static_cast<size_t>(B)) : 0;
  // 40 bytes a cell of a chunk: e / x, g and the transposed x (8 each), the transposed h, k, fixed and u (4 each)
  const size_t cells = static_cast<size_t>(first_chunk * hw);
  const size_t b8 = align256(sizeof(double) * cells), b4 = align256(sizeof(float) * cells);
  const size_t bytes = b_scales + 3 * b8 + 4 * b4;
  t_diff_info = DiffInfo{0, 0, 0, static_cast<int64_t>(bytes)};
  void* base = nullptr;
  if (int rc = workspace_get(WS_DIFFUSE, bytes, &base); rc != SOIL_OK) return rc;
  DiffScales sc{nullptr, diff_scale(scales)};
  if (per_model) {
    if (int rc = upload_scale_records(base, scales, B, diff_scale, st); rc != SOIL_OK) return rc;
    sc.per_model = static_cast<const DiffScale*>(base);
  }
  char* const p = static_cast<char*>(base) + b_scales;
  const DiffScratch w{reinterpret_cast<double*>(p), reinterpret_cast<double*>(p + b8), reinterpret_cast<double*>(p + 2 * b8),
                      reinterpret_cast<float*>(p + 3 * b8), reinterpret_cast<float*>(p + 3 * b8 + b4),
                      reinterpret_cast<float*>(p + 3 * b8 + 2 * b4), reinterpret_cast<int32_t*>(p + 3 * b8 + 3 * b4)};
  // (64-bit offsets: the form a model of 2^29 cells or more takes, or SOIL_PATHS_IDX64)
  const bool idx32 = static_cast<uint64_t>(hw) * sizeof(double) < (1ull << 32) && !force_idx64();
  for (int64_t b0 = 0; b0 < B; b0 += per) {
    const int64_t nb = B - b0 < per ? B - b0 : per, at = b0 * hw;
    DiffArgs a;
    a.h = height + at;
    a.k = diffusivity ? diffusivity + at : nullptr;
    a.u = uplift ? uplift + at : nullptr;
    a.fixed = fixed ? fixed + at : nullptr;
    a.E = a.G = nullptr;
    a.out = out ? out + at : nullptr;
    a.out64 = out64 ? out64 + at : nullptr;
    a.H = H, a.W = W, a.axis = 0, a.kappa = kappa, a.dt = dt, a.border = border;
    a.has_k = diffusivity != nullptr, a.has_u = uplift != nullptr, a.has_fixed = fixed != nullptr;
    a.scales = sc;
    if (a.scales.per_model) a.scales.per_model += b0;
    t_diff_info.launches += idx32 ? diff_launch<uint32_t>(a, w, nb, first_axis, st) : diff_launch<int64_t>(a, w, nb, first_axis, st);
    SOIL_LAUNCH_CHECK();
    t_diff_info.chunks += 1;
    t_diff_info.idx64_chunks += idx32 ? 0 : 1;
  }
  return SOIL_OK;
}

}  // namespace soil

using namespace soil;

extern "C" {

int soil_diffuse(float* out, double* out64, const float* height, const float* diffusivity, const float* uplift,
                 const int32_t* fixed, int64_t H, int64_t W, const float scale[2], double kappa, double dt,
                 int border, int first_axis, void* stream) {
  if (int rc = check_diffuse("diffuse", out, out64, height, diffusivity, uplift, fixed, 1, H, W, scale, 1, kappa, dt,
                             border, first_axis);
      rc != SOIL_OK)
    return rc;
  SOIL_DEVICE();
  return diffuse_run(out, out64, height, diffusivity, uplift, fixed, 1, H, W, scale, 1, kappa, dt, border, first_axis,
                     as_stream(stream));
}

int soil_diffuse_batch(float* out, double* out64, const float* height, const float* diffusivity, const float* uplift,
                       const int32_t* fixed, int64_t B, int64_t H, int64_t W, const float* scales, int64_t n_scales,
                       double kappa, double dt, int border, int first_axis, void* stream) {
  if (int rc = check_diffuse("diffuse_batch", out, out64, height, diffusivity, uplift, fixed, B, H, W, scales,
                             n_scales, kappa, dt, border, first_axis);
      rc != SOIL_OK)
    return rc;
  SOIL_DEVICE();
  return diffuse_run(out, out64, height, diffusivity, uplift, fixed, B, H, W, scales, n_scales, kappa, dt, border,
                     first_axis, as_stream(stream));
}

int soil_diffuse_info(int64_t info[4]) {
  SOIL_REQUIRE(info, "diffuse_info: null info");
  info[0] = t_diff_info.launches, info[1] = t_diff_info.chunks, info[2] = t_diff_info.idx64_chunks;
  info[3] = t_diff_info.scratch_bytes;
  return SOIL_OK;
}

}  // extern "C"
