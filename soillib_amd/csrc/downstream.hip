// downstream.hip — a value carried DOWN a receiver graph: the linear recurrence
//
//   x[n] = t[n]                         n a terminal
//   x[n] = a[n] L(n) + b[n] x[r(n)]     n has an edge to r(n), of length L(n)
//
// (soil_downstream / soil_downstream_batch, soil_hip.h: chi, travel time, the outlet's height, what survives a decay)
// and the implicit stream-power step of Braun & Willett, the same recurrence with coefficients made from the planes
// (soil_stream_power / soil_stream_power_batch).  The reference has neither; its example/dem_process.py names the
// solver.
//
// The composition of affine maps is associative, so this is the pointer doubling of flow_paths.hip with other
// records: where that file adds three counters, a round here composes x -> A + B x with the map of the cell the
// pointer stands on,
//
//   A' = A + (B * A_p),  B' = B * B_p,  ptr' = ptr_p        fp64, the product rounded, then the sum
//
// over 16-byte records {ptr | kFinal, edges walked, A} — the dwordx4 gather of a flow_paths round — and, only where B
// is not 1 throughout (`b` given, or the stream-power step), a plane of 8-byte B beside them: HASB.  Without it a round moves
// exactly what a flow_paths round moves, with it half as much again.  B of a cell that is not final is the product of
// the b along the edges walked so far; with b == 1 everywhere that is 1.0 and 1.0 * A_p is A_p, bit for bit, so the
// instantiation without the plane gives the bits of b == 1.  A terminal is final with B = 0; a final record is a
// fixed point and is copied from buffer to buffer with its B, which the cells that still point at it read.
//
// Everything else is flow_paths.hip's, through flow_paths.hpp: kFinal and the round count ceil(log2(H W)) of ONE
// model, the dense round that writes down the pending cells, the listed rounds, device-side control words, chunks of
// whole models on 32-bit byte offsets (64-bit for a single model above them), the model on grid.z in init and final.
// A cell that never gets the bit — on a cycle, or draining into one — gets the quiet NaN.
//
// The result is one definite bit pattern: every operand of a round comes from the round before, every operation is
// a single correctly rounded fp64 operation (-ffp-contract=off, and the intrinsics say so), and neither lists nor
// offsets nor chunks change which operations a cell sees.
#include <algorithm>
#include <cstdlib>

#include "common.hpp"
#include "flow_paths.hpp"

namespace soil {

// The edge rule of soil_hip.h (flow_paths.hip path_record) for cell (x, y) with graph entry g: the kind of the edge,
// 0 a row step, 1 a column step, 2 a diagonal, or -1 where g is no edge.
template <int K>
__device__ __forceinline__ int down_edge(int32_t g, int64_t x, int64_t y, int64_t H, int64_t W) {
  const int64_t d = static_cast<int64_t>(g) - (x * W + y);
  int kind = -1;
#pragma unroll
  for (int rd = -1; rd <= 1; ++rd) {
    const int64_t cd = d - rd * W;
    const bool ok = cd >= -1 && cd <= 1 && (rd != 0 || cd != 0) && x + rd >= 0 && x + rd < H && y + cd >= 0 &&
                    y + cd < W && (K == 8 || rd == 0 || cd == 0);
    if (ok) kind = rd == 0 ? 1 : (cd == 0 ? 0 : 2);
  }
  return kind;
}

// {ptr | kFinal, edges walked, A}.  The second word is not part of the result; it is carried (an integer add a round,
// at most 2^31 as in flow_paths.hip) so that every word of a record read is used: the compiler narrows a 16-byte load
// whose second word goes unused to a dword and a dwordx2, two gathers a record instead of one, and the rounds of
// the bench graph at 4096^2 ran 9 % longer that way.
__device__ __forceinline__ uint4 down_rec(uint32_t ptr, uint32_t edges, double A) {
  return make_uint4(ptr, edges, static_cast<uint32_t>(__double2loint(A)), static_cast<uint32_t>(__double2hiint(A)));
}
__device__ __forceinline__ double down_a(const uint4& r) {
  return __hiloint2double(static_cast<int>(r.w), static_cast<int>(r.z));
}

// B of cell n, at a 32-bit byte offset like the records (rec_at)
template <typename IDX>
__device__ __forceinline__ double* b_at(double* base, IDX n) {
  if constexpr (sizeof(IDX) == 4)
    return reinterpret_cast<double*>(reinterpret_cast<char*>(base) + static_cast<uint32_t>(n * 8u));
  else
    return base + n;
}
template <typename IDX>
__device__ __forceinline__ const double* b_at(const double* base, IDX n) {
  if constexpr (sizeof(IDX) == 4)
    return reinterpret_cast<const double*>(reinterpret_cast<const char*>(base) + static_cast<uint32_t>(n * 8u));
  else
    return base + n;
}

// The planes of a call.  kSum (soil_downstream): p0 = a, p1 = b, p2 = t, each may be null (1, 1, 0).  kPower
// (soil_stream_power): p0 = height, p1 = erosivity, p2 = uplift (may be null), and dt.
enum DownMode { kSum = 0, kPower = 1 };
struct DownPlanes {
  const int32_t* graph;
  const int32_t* stop;
  const float *p0, *p1, *p2;
  double dt;
};

// The record of one cell, and its B.  Each operation is rounded once, as soil_hip.h writes them down.
template <int K, int MODE, bool HASB>
__device__ __forceinline__ void down_init_cell(uint4* __restrict__ rec, double* __restrict__ bcoef, int64_t n,
                                               int32_t g, bool stop, float v0, float v1, float v2, bool has2,
                                               int64_t x, int64_t y, int64_t H, int64_t W, uint32_t first,
                                               const PathScale& s, double dt) {
  const int kind = stop ? -1 : down_edge<K>(g, x, y, H, W);
  double A, B = 0.0;
  uint32_t ptr = (first + static_cast<uint32_t>(n)) | kFinal;
  if (kind < 0) {
    A = static_cast<double>(MODE == kSum ? v2 : v0);  // t, or the height of the base level
  } else {
    ptr = first + static_cast<uint32_t>(g);
    const double L = kind == 0 ? s.sx : (kind == 1 ? s.sy : s.dd);
    if constexpr (MODE == kSum) {
      A = __dmul_rn(static_cast<double>(v0), L);  // (without a scale L is 1.0: the product is a, exactly)
      B = static_cast<double>(v1);
    } else {
      const double F = __ddiv_rn(__dmul_rn(static_cast<double>(v1), dt), L);
      const double d = __dadd_rn(1.0, F);
      const double h = static_cast<double>(v0);
      A = __ddiv_rn(has2 ? __dadd_rn(h, __dmul_rn(dt, static_cast<double>(v2))) : h, d);
      B = __ddiv_rn(F, d);
    }
  }
  rec[n] = down_rec(ptr, kind < 0 ? 0u : 1u, A);
  if constexpr (HASB) bcoef[n] = B;
}

// Init: flow_paths.hip k_paths_init — threads along the row, a band of rows per work-group, grid.z the model.  VEC:
// four cells per thread, every plane as a 16-byte load (W a multiple of four, the planes 16-byte aligned).
template <int K, bool VEC, int MODE, bool HASB>
__global__ void __launch_bounds__(kPBlock)
    k_down_init(uint4* __restrict__ rec, double* __restrict__ bcoef, DownPlanes in, int64_t H, int64_t W,
                PathScales scales, int* __restrict__ flags) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x < kPathFlags)
    flags[threadIdx.x] = threadIdx.x == 0 ? 1 : 0;
  const int64_t y = (static_cast<int64_t>(blockIdx.x) * kPBlock + threadIdx.x) * (VEC ? 4 : 1);
  if (y >= W) return;
  const int64_t first64 = static_cast<int64_t>(blockIdx.z) * H * W;
  const uint32_t first = static_cast<uint32_t>(first64);
  const PathScale s = scales.per_model ? scales.per_model[blockIdx.z] : scales.one;
  rec += first64;
  if constexpr (HASB) bcoef += first64;
  const int32_t* const graph = in.graph + first64;
  const int32_t* const stop = in.stop ? in.stop + first64 : nullptr;
  const float* const p0 = in.p0 ? in.p0 + first64 : nullptr;
  const float* const p1 = in.p1 ? in.p1 + first64 : nullptr;
  const float* const p2 = in.p2 ? in.p2 + first64 : nullptr;
  const float d0 = MODE == kSum ? 1.0f : 0.0f, d1 = MODE == kSum ? 1.0f : 0.0f;  // a, b == 1; t == 0
  SOIL_ROW_LOOP(x, H) {
    const int64_t n = x * W + y;
    if constexpr (VEC) {
      const int4 g = *reinterpret_cast<const int4*>(graph + n);
      const int4 st = stop ? *reinterpret_cast<const int4*>(stop + n) : make_int4(0, 0, 0, 0);
      const float4 v0 = p0 ? *reinterpret_cast<const float4*>(p0 + n) : make_float4(d0, d0, d0, d0);
      const float4 v1 = p1 ? *reinterpret_cast<const float4*>(p1 + n) : make_float4(d1, d1, d1, d1);
      const float4 v2 = p2 ? *reinterpret_cast<const float4*>(p2 + n) : make_float4(0.f, 0.f, 0.f, 0.f);
      down_init_cell<K, MODE, HASB>(rec, bcoef, n + 0, g.x, st.x != 0, v0.x, v1.x, v2.x, p2 != nullptr, x, y + 0, H,
                                    W, first, s, in.dt);
      down_init_cell<K, MODE, HASB>(rec, bcoef, n + 1, g.y, st.y != 0, v0.y, v1.y, v2.y, p2 != nullptr, x, y + 1, H,
                                    W, first, s, in.dt);
      down_init_cell<K, MODE, HASB>(rec, bcoef, n + 2, g.z, st.z != 0, v0.z, v1.z, v2.z, p2 != nullptr, x, y + 2, H,
                                    W, first, s, in.dt);
      down_init_cell<K, MODE, HASB>(rec, bcoef, n + 3, g.w, st.w != 0, v0.w, v1.w, v2.w, p2 != nullptr, x, y + 3, H,
                                    W, first, s, in.dt);
    } else {
      down_init_cell<K, MODE, HASB>(rec, bcoef, n, graph[n], stop ? stop[n] != 0 : false, p0 ? p0[n] : d0,
                                    p1 ? p1[n] : d1, p2 ? p2[n] : 0.0f, p2 != nullptr, x, y, H, W, first, s, in.dt);
    }
  }
}

// One cell of one round, `in` -> `out` (flow_paths.hip path_cell).  Returns whether the cell has to be looked at
// again: it wrote a new record.
template <typename IDX, bool HASB>
__device__ __forceinline__ bool down_cell(uint4* __restrict__ out, const uint4* __restrict__ in,
                                          double* __restrict__ bout, const double* __restrict__ bin, IDX n) {
  const uint4 r = *rec_at<IDX>(in, n);
  if (r.x & kFinal) {  // final in `in`: both buffers hold it, and its B, from here on
    *rec_at<IDX>(out, n) = r;
    if constexpr (HASB) *b_at<IDX>(bout, n) = *b_at<IDX>(bin, n);
    return false;
  }
  const IDX p = static_cast<IDX>(r.x);
  const uint4 q = *rec_at<IDX>(in, p);
  if constexpr (HASB) {
    const double B = *b_at<IDX>(bin, n);
    *rec_at<IDX>(out, n) = down_rec(q.x, r.y + q.y, __dadd_rn(down_a(r), __dmul_rn(B, down_a(q))));
    *b_at<IDX>(bout, n) = __dmul_rn(B, *b_at<IDX>(bin, p));
  } else {
    *rec_at<IDX>(out, n) = down_rec(q.x, r.y + q.y, __dadd_rn(down_a(r), down_a(q)));  // B == 1.0: 1.0 * A_p is A_p
  }
  return true;
}

// A dense round (flow_paths.hip k_paths_round): a grid of a few work-groups per CU strides over the cells; a round
// that wrote no new record ends the work of the dense rounds after it; `list_out`: the pending cells, work-group b
// into segment b.
template <typename IDX, bool HASB>
__global__ void __launch_bounds__(kPBlock)
    k_down_round(uint4* __restrict__ out, const uint4* __restrict__ in, double* __restrict__ bout,
                 const double* __restrict__ bin, int64_t elem64, int* __restrict__ flags, int round,
                 uint32_t* __restrict__ list_out, uint32_t* __restrict__ fill_out, uint32_t seg) {
  const IDX elem = static_cast<IDX>(elem64);
  __shared__ uint32_t s_fill;
  if (blockIdx.x == 0 && threadIdx.x == 0) flags[(round + 2) % 3] = 0;
  if (flags[round % 3] == 0) {
    if (list_out && threadIdx.x == 0) fill_out[blockIdx.x] = 0;
    return;
  }
  if (list_out) {
    if (threadIdx.x == 0) s_fill = 0;
    __syncthreads();
  }
  uint32_t* const segment = list_out ? list_out + static_cast<size_t>(blockIdx.x) * seg : nullptr;
  bool pending = false;
  for (IDX n = static_cast<IDX>(blockIdx.x) * kPBlock + threadIdx.x; n < elem;
       n += static_cast<IDX>(gridDim.x) * kPBlock) {
    const bool again = down_cell<IDX, HASB>(out, in, bout, bin, n);
    pending = pending || again;
    if (list_out) path_append<IDX>(again, n, segment, &s_fill);
  }
  if (__any(pending) && (threadIdx.x & 63) == 0) flags[(round + 1) % 3] = 1;
  if (list_out) {
    __syncthreads();
    if (threadIdx.x == 0) fill_out[blockIdx.x] = s_fill;
  }
}

// A round over the lists (flow_paths.hip k_paths_list)
template <typename IDX, bool HASB>
__global__ void __launch_bounds__(kPBlock)
    k_down_list(uint4* __restrict__ out, const uint4* __restrict__ in, double* __restrict__ bout,
                const double* __restrict__ bin, const uint32_t* __restrict__ list_in,
                const uint32_t* __restrict__ fill_in, uint32_t* __restrict__ list_out,
                uint32_t* __restrict__ fill_out, uint32_t seg) {
  const uint32_t n_in = fill_in[blockIdx.x];
  if (n_in == 0) {
    if (threadIdx.x == 0) fill_out[blockIdx.x] = 0;
    return;
  }
  __shared__ uint32_t s_fill;
  if (threadIdx.x == 0) s_fill = 0;
  __syncthreads();
  const uint32_t* const mine = list_in + static_cast<size_t>(blockIdx.x) * seg;
  uint32_t* const segment = list_out + static_cast<size_t>(blockIdx.x) * seg;
  for (uint32_t i = threadIdx.x; i < n_in; i += kPBlock) {
    const IDX n = static_cast<IDX>(mine[i]);
    const bool again = down_cell<IDX, HASB>(out, in, bout, bin, n);
    path_append<IDX>(again, n, segment, &s_fill);
  }
  __syncthreads();
  if (threadIdx.x == 0) fill_out[blockIdx.x] = s_fill;
}

// Final: a cell per thread, grid.z the model, no gather.  A, or the quiet NaN for any NaN and for a cell that never
// became final.
__global__ void __launch_bounds__(kPBlock)
    k_down_final(float* __restrict__ out, double* __restrict__ out64, const uint4* __restrict__ rec, int64_t cells) {
  const int64_t first64 = static_cast<int64_t>(blockIdx.z) * cells;
  for (int64_t n = static_cast<int64_t>(blockIdx.x) * kPBlock + threadIdx.x; n < cells;
       n += static_cast<int64_t>(gridDim.x) * kPBlock) {
    const uint4 r = rec[first64 + n];
    const double A = down_a(r);
    const bool nan = (r.x & kFinal) == 0 || A != A;
    if (out) out[first64 + n] = nan ? bits2f(0x7fc00000u) : __double2float_rn(A);
    if (out64) out64[first64 + n] = nan ? __hiloint2double(0x7ff80000, 0) : A;
  }
}

// Models per chunk, as flow_paths.hip counts them: whole models on 32-bit offsets (16 bytes a cell under 4 GiB; B's 8
// bytes a cell lie below that anyway) in one init launch, at least one; SOIL_FLOW_BATCH_CELLS lowers the cap.
static int64_t down_chunk_models(int64_t cells_per_model) {
  const char* const e = std::getenv("SOIL_FLOW_BATCH_CELLS");
  const int64_t cap_env = e ? std::atoll(e) : 0ll;
  int64_t cap = static_cast<int64_t>((1ull << 32) / sizeof(uint4)) - 1;
  if (cap_env > 0 && cap_env < cap) cap = cap_env;
  const int64_t per = cap / cells_per_model;
  return per < 1 ? 1 : (per > kPathsMaxGridZ ? kPathsMaxGridZ : per);
}

// What the last call of one of the four entries on this host thread did (soil_downstream_info)
struct DownInfo {
  int64_t chunks, vec_chunks, idx64_chunks, rounds;
};
static thread_local DownInfo t_down_info{0, 0, 0, 0};

struct DownLayout {  // the scratch of a chunk: two record buffers, two B planes (HASB), two lists, their fills, flags
  unsigned groups;
  size_t seg, b_rec, b_coef, b_list, b_fill;
  size_t bytes() const { return 2 * b_rec + 2 * b_coef + 2 * b_list + 2 * b_fill + 256; }
};
static DownLayout down_layout(int64_t elem, bool has_b) {
  static const unsigned groups_env = [] {
    const char* e = std::getenv("SOIL_PATHS_GROUPS");
    return e && std::atoi(e) > 0 ? static_cast<unsigned>(std::atoi(e)) : 256u * 32u;
  }();
  DownLayout L;
  L.groups = std::min(blocks_for(elem, kPBlock), groups_env);
  L.seg = ((static_cast<size_t>(elem) + L.groups - 1) / L.groups + 255) / 256 * 256;
  L.b_rec = align256(sizeof(uint4) * static_cast<size_t>(elem));
  L.b_coef = has_b ? align256(sizeof(double) * static_cast<size_t>(elem)) : 0;
  L.b_list = align256(sizeof(uint32_t) * L.seg * L.groups);
  L.b_fill = align256(sizeof(uint32_t) * L.groups);
  return L;
}

struct DownOut {
  float* out;
  double* out64;
};

// One chunk of `models` models of (H, W), stream-ordered: init, the rounds of ONE model, final.
template <int K, int MODE, bool HASB>
static int down_chunk(DownOut o, const DownPlanes& in, int64_t models, int64_t H, int64_t W, const PathScales& scales,
                      char* scratch, hipStream_t st) {
  const int64_t hw = H * W, elem = models * hw;
  const DownLayout L = down_layout(elem, HASB);
  char* p = scratch;
  uint4* const rec[2] = {reinterpret_cast<uint4*>(p), reinterpret_cast<uint4*>(p + L.b_rec)};
  p += 2 * L.b_rec;
  double* const coef[2] = {HASB ? reinterpret_cast<double*>(p) : nullptr,
                           HASB ? reinterpret_cast<double*>(p + L.b_coef) : nullptr};
  p += 2 * L.b_coef;
  uint32_t* const list[2] = {reinterpret_cast<uint32_t*>(p), reinterpret_cast<uint32_t*>(p + L.b_list)};
  p += 2 * L.b_list;
  uint32_t* const fill[2] = {reinterpret_cast<uint32_t*>(p), reinterpret_cast<uint32_t*>(p + L.b_fill)};
  p += 2 * L.b_fill;
  int* const flags = reinterpret_cast<int*>(p);

  const unsigned z = static_cast<unsigned>(models);
  const uintptr_t planes = reinterpret_cast<uintptr_t>(in.graph) | reinterpret_cast<uintptr_t>(in.stop) |
                           reinterpret_cast<uintptr_t>(in.p0) | reinterpret_cast<uintptr_t>(in.p1) |
                           reinterpret_cast<uintptr_t>(in.p2);
  const bool vec = W % 4 == 0 && (planes & 15) == 0;
  if (vec) {
    dim3 grid = grid_rows(H, W / 4, kPBlock);
    grid.z = z;
    k_down_init<K, true, MODE, HASB><<<grid, kPBlock, 0, st>>>(rec[0], coef[0], in, H, W, scales, flags);
  } else {
    dim3 grid = grid_rows(H, W, kPBlock);
    grid.z = z;
    k_down_init<K, false, MODE, HASB><<<grid, kPBlock, 0, st>>>(rec[0], coef[0], in, H, W, scales, flags);
  }
  SOIL_LAUNCH_CHECK();
  t_down_info.chunks += 1;
  t_down_info.vec_chunks += vec ? 1 : 0;

  // The knobs of flow_paths.hip, read per call: SOIL_PATHS_LIST_FROM, the first round over the lists (0, or beyond
  // the last round: dense rounds throughout), and SOIL_PATHS_IDX64=1, 64-bit offsets whatever the size.
  const char* const e = std::getenv("SOIL_PATHS_LIST_FROM");
  const int list_from_env = e ? std::atoi(e) : 1;
  const int rounds = ceil_log2(hw);
  const int list_from = (list_from_env >= 1 && list_from_env < rounds) ? list_from_env : rounds;
  const char* const e64 = std::getenv("SOIL_PATHS_IDX64");
  const bool idx32 = static_cast<uint64_t>(elem) * sizeof(uint4) < (1ull << 32) && !(e64 && std::atoi(e64) == 1);
  t_down_info.idx64_chunks += idx32 ? 0 : 1;
  t_down_info.rounds = rounds;
  const uint32_t seg32 = static_cast<uint32_t>(L.seg);
  for (int r = 0; r < rounds; ++r) {
    uint4* const ro = rec[(r + 1) & 1];
    const uint4* const ri = rec[r & 1];
    double* const bo = coef[(r + 1) & 1];
    const double* const bi = coef[r & 1];
    if (r >= list_from) {
      const uint32_t *li = list[r & 1], *fi = fill[r & 1];
      uint32_t *lo = list[(r + 1) & 1], *fo = fill[(r + 1) & 1];
      if (idx32) k_down_list<uint32_t, HASB><<<L.groups, kPBlock, 0, st>>>(ro, ri, bo, bi, li, fi, lo, fo, seg32);
      else k_down_list<int64_t, HASB><<<L.groups, kPBlock, 0, st>>>(ro, ri, bo, bi, li, fi, lo, fo, seg32);
      continue;
    }
    uint32_t* const lo = list_from < rounds && r + 1 == list_from ? list[(r + 1) & 1] : nullptr;
    uint32_t* const fo = fill[(r + 1) & 1];
    if (idx32) k_down_round<uint32_t, HASB><<<L.groups, kPBlock, 0, st>>>(ro, ri, bo, bi, elem, flags, r, lo, fo, seg32);
    else k_down_round<int64_t, HASB><<<L.groups, kPBlock, 0, st>>>(ro, ri, bo, bi, elem, flags, r, lo, fo, seg32);
  }
  SOIL_LAUNCH_CHECK();

  const int64_t per_model = (hw + kPBlock - 1) / kPBlock;
  const int64_t want = (8192 + models - 1) / models;
  dim3 grid(static_cast<unsigned>(per_model < want ? per_model : want), 1, z);
  k_down_final<<<grid, kPBlock, 0, st>>>(o.out, o.out64, rec[rounds & 1], hw);
  SOIL_LAUNCH_CHECK();
  return SOIL_OK;
}

// Whether [p, p + pb) and [q, q + qb) share a byte (a null pointer shares nothing)
static bool overlaps(const void* p, size_t pb, const void* q, size_t qb) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return p && q && a < b + qb && b < a + pb;
}

// What the four entries refuse before any device work, under the entry's name.  `planes`: the float inputs.
static int check_downstream(const char* what, int mode, const void* out, const void* out64, const DownPlanes& in,
                            const float* scales, int64_t B, int64_t H, int64_t W, int edge, int64_t n_scales) {
  const std::string w(what);
  SOIL_REQUIRE(in.graph, w + ": null graph");
  SOIL_REQUIRE(out || out64, w + ": no output asked for (out and out64 are both null)");
  if (mode == kPower) {
    SOIL_REQUIRE(in.p0, w + ": null height");
    SOIL_REQUIRE(in.p1, w + ": null erosivity");
    SOIL_REQUIRE(scales, w + ": the stream-power step needs a scale");
  }
  SOIL_REQUIRE(B >= 1, w + ": B must be >= 1");
  SOIL_REQUIRE(H >= 1 && W >= 1, w + ": empty grid");
  SOIL_REQUIRE(H <= INT32_MAX / W, w + ": a model must have 1..2^31-1 cells (int32 graph)");
  SOIL_REQUIRE(n_scales == 1 || n_scales == B, w + ": n_scales must be 1 or B");
  SOIL_REQUIRE(edge == SOIL_D4 || edge == SOIL_D8, w + ": invalid edge enumerator");
  if (mode == kPower) {
    for (int64_t i = 0; i < 2 * n_scales; ++i)
      SOIL_REQUIRE(scales[i] > 0.0f && std::isfinite(scales[i]), w + ": a scale must be a positive finite float");
    SOIL_REQUIRE(in.dt >= 0.0 && std::isfinite(in.dt), w + ": dt must be finite and >= 0");
  }
  // (cells counted so that the byte counts below cannot wrap: a batch this large fails its allocation anyway)
  const int64_t hw = H * W;
  const size_t cells = static_cast<size_t>(B > (int64_t{1} << 58) / hw ? (int64_t{1} << 58) : B * hw);
  const void* const inputs[] = {in.graph, in.stop, in.p0, in.p1, in.p2};
  for (const void* q : inputs)
    SOIL_REQUIRE(!overlaps(out, 4 * cells, q, 4 * cells) && !overlaps(out64, 8 * cells, q, 4 * cells),
                 w + ": an output aliases an input plane");
  SOIL_REQUIRE(!overlaps(out, 4 * cells, out64, 8 * cells), w + ": out and out64 overlap");
  return SOIL_OK;
}

// Chunks of whole models, one after the other on `st` through one block of workspace slot WS_DOWNSTREAM (the
// entries' own: they return with their work in flight): the B scale records first, then the chunk's scratch.
static int downstream_run(int mode, DownOut o, const DownPlanes& in, int64_t B, int64_t H, int64_t W, int edge,
                          const float* scales, int64_t n_scales, hipStream_t st) {
  const int64_t hw = H * W, per = down_chunk_models(hw);
  t_down_info = DownInfo{0, 0, 0, 0};
  const bool has_b = mode == kPower || in.p1 != nullptr;
  const bool per_model = scales && n_scales > 1;
  const size_t b_scales = per_model ? align256(sizeof(PathScale) * static_cast<size_t>(B)) : 0;
  const int64_t first_chunk = B < per ? B : per;
  void* base = nullptr;
  if (int rc = workspace_get(WS_DOWNSTREAM, b_scales + down_layout(first_chunk * hw, has_b).bytes(), &base);
      rc != SOIL_OK)
    return rc;
  PathScales sc{nullptr, PathScale{1.0, 1.0, 1.0}};  // no scale: L == 1
  if (scales) sc.one = path_scale(scales);
  if (per_model) {
    std::vector<PathScale> host(static_cast<size_t>(B));
    for (int64_t b = 0; b < B; ++b) host[static_cast<size_t>(b)] = path_scale(scales + 2 * b);
    if (int rc = batch_upload(base, host.data(), sizeof(PathScale) * host.size(), st); rc != SOIL_OK) return rc;
    sc.per_model = static_cast<const PathScale*>(base);
  }
  char* const scratch = static_cast<char*>(base) + b_scales;
  const bool d4 = edge == SOIL_D4;
  auto go = mode == kPower ? (d4 ? down_chunk<4, kPower, true> : down_chunk<8, kPower, true>)
            : has_b        ? (d4 ? down_chunk<4, kSum, true> : down_chunk<8, kSum, true>)
                           : (d4 ? down_chunk<4, kSum, false> : down_chunk<8, kSum, false>);
  for (int64_t b0 = 0; b0 < B; b0 += per) {
    const int64_t nb = B - b0 < per ? B - b0 : per, at = b0 * hw;
    PathScales s = sc;
    if (s.per_model) s.per_model += b0;
    const DownPlanes part{in.graph + at, in.stop ? in.stop + at : nullptr, in.p0 ? in.p0 + at : nullptr,
                          in.p1 ? in.p1 + at : nullptr, in.p2 ? in.p2 + at : nullptr, in.dt};
    if (int rc = go(DownOut{o.out ? o.out + at : nullptr, o.out64 ? o.out64 + at : nullptr}, part, nb, H, W, s,
                    scratch, st);
        rc != SOIL_OK)
      return rc;
  }
  return SOIL_OK;
}

}  // namespace soil

using namespace soil;

extern "C" {

int soil_downstream(float* out, double* out64, const int32_t* graph, const float* a, const float* b, const float* t,
                    const int32_t* stop, int64_t H, int64_t W, int edge, const float scale[2], void* stream) {
  const DownPlanes in{graph, stop, a, b, t, 0.0};
  if (int rc = check_downstream("downstream", kSum, out, out64, in, scale, 1, H, W, edge, 1); rc != SOIL_OK) return rc;
  SOIL_DEVICE();
  return downstream_run(kSum, DownOut{out, out64}, in, 1, H, W, edge, scale, 1, as_stream(stream));
}

int soil_downstream_batch(float* out, double* out64, const int32_t* graph, const float* a, const float* b,
                          const float* t, const int32_t* stop, int64_t B, int64_t H, int64_t W, int edge,
                          const float* scales, int64_t n_scales, void* stream) {
  const DownPlanes in{graph, stop, a, b, t, 0.0};
  if (int rc = check_downstream("downstream_batch", kSum, out, out64, in, scales, B, H, W, edge, n_scales);
      rc != SOIL_OK)
    return rc;
  SOIL_DEVICE();
  return downstream_run(kSum, DownOut{out, out64}, in, B, H, W, edge, scales, n_scales, as_stream(stream));
}

int soil_stream_power(float* out, double* out64, const float* height, const int32_t* graph, const float* erosivity,
                      const float* uplift, const int32_t* stop, int64_t H, int64_t W, int edge, const float scale[2],
                      double dt, void* stream) {
  const DownPlanes in{graph, stop, height, erosivity, uplift, dt};
  if (int rc = check_downstream("stream_power", kPower, out, out64, in, scale, 1, H, W, edge, 1); rc != SOIL_OK)
    return rc;
  SOIL_DEVICE();
  return downstream_run(kPower, DownOut{out, out64}, in, 1, H, W, edge, scale, 1, as_stream(stream));
}

int soil_stream_power_batch(float* out, double* out64, const float* height, const int32_t* graph,
                            const float* erosivity, const float* uplift, const int32_t* stop, int64_t B, int64_t H,
                            int64_t W, int edge, const float* scales, int64_t n_scales, double dt, void* stream) {
  const DownPlanes in{graph, stop, height, erosivity, uplift, dt};
  if (int rc = check_downstream("stream_power_batch", kPower, out, out64, in, scales, B, H, W, edge, n_scales);
      rc != SOIL_OK)
    return rc;
  SOIL_DEVICE();
  return downstream_run(kPower, DownOut{out, out64}, in, B, H, W, edge, scales, n_scales, as_stream(stream));
}

int soil_downstream_info(int64_t info[4]) {
  SOIL_REQUIRE(info, "downstream_info: null info");
  info[0] = t_down_info.chunks, info[1] = t_down_info.vec_chunks;
  info[2] = t_down_info.idx64_chunks, info[3] = t_down_info.rounds;
  return SOIL_OK;
}

}  // extern "C"
