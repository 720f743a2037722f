// downstream.hip — a value carried DOWN a receiver graph: the linear recurrence
//
//   x[n] = t[n]                         n a terminal
//   x[n] = a[n] L(n) + b[n] x[r(n)]     n has an edge to r(n), of length L(n)
//
// (soil_downstream / soil_downstream_batch, soil_hip.h: chi, travel time, the outlet's height, what survives a decay)
// and the implicit stream-power step of Braun & Willett, the same recurrence with coefficients made from the planes
// (soil_stream_power / soil_stream_power_batch).  The reference has neither; its example/dem_process.py names the
// solver.  At the end of the file, the stream-power step with a deposition term (soil_stream_power_deposit /
// soil_stream_power_deposit_batch): the same rounds inside a fixed-point iteration with graph.hip's accumulation; and
// the step with a slope exponent above 1 (soil_stream_power_n / soil_stream_power_n_batch): the same rounds inside a
// Newton iteration, whose linearisation about an iterate is an affine recurrence again; and the two in one step
// (soil_stream_power_deposit_n / soil_stream_power_deposit_n_batch): the deposit step's driver with an init pass that
// writes both sets of coefficients.
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
// Everything else is the engine of flow_paths.hpp, as flow_paths.hip's header explains it: kFinal and the round count
// ceil(log2(H W)) of ONE model, the dense round that writes down the pending cells, the listed rounds, device-side
// control words, chunks of whole models on 32-bit byte offsets (64-bit for a single model above them), the model on
// grid.z in init and final.  This file has the records, the per-cell operation, init, final and the refusals.
// A cell that never gets the bit — on a cycle, or draining into one — gets the quiet NaN.
//
// The result is one definite bit pattern: every operand of a round comes from the round before, every operation is
// a single correctly rounded fp64 operation (-ffp-contract=off, and the intrinsics say so), and neither lists nor
// offsets nor chunks change which operations a cell sees.
#include "common.hpp"
#include "flow_paths.hpp"

namespace soil {

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
  DownPlanes at(int64_t off) const {  // the planes from cell `off` on: a chunk's
    return {graph + off, soil::at(stop, off), soil::at(p0, off), soil::at(p1, off), soil::at(p2, off), dt};
  }
};

// The record of one cell, and its B.  Each operation is rounded once, as soil_hip.h writes them down.
template <int K, int MODE, bool HASB>
__device__ __forceinline__ void down_init_cell(uint4* __restrict__ rec, double* __restrict__ bcoef, int64_t n,
                                               int32_t g, bool stop, float v0, float v1, float v2, bool has2,
                                               int64_t x, int64_t y, int64_t H, int64_t W, uint32_t first,
                                               const PathScale& s, double dt) {
  const int kind = stop ? -1 : edge_kind<K>(g, x, y, H, W);
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

// Init, as k_paths_init of flow_paths.hip: threads along the row, a band of rows per work-group, grid.z the model.  VEC:
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

// The dense and the listed round (flow_paths.hpp ptr_round, ptr_list) over down_cell
template <typename IDX, bool HASB>
__global__ void __launch_bounds__(kPBlock)
    k_down_round(uint4* __restrict__ out, const uint4* __restrict__ in, double* __restrict__ bout,
                 const double* __restrict__ bin, int64_t elem64, int* __restrict__ flags, int round,
                 uint32_t* __restrict__ list_out, uint32_t* __restrict__ fill_out, uint32_t seg) {
  ptr_round<IDX>([=](IDX n) { return down_cell<IDX, HASB>(out, in, bout, bin, n); }, elem64, flags, round, list_out,
                 fill_out, seg);
}
template <typename IDX, bool HASB>
__global__ void __launch_bounds__(kPBlock)
    k_down_list(uint4* __restrict__ out, const uint4* __restrict__ in, double* __restrict__ bout,
                const double* __restrict__ bin, const uint32_t* __restrict__ list_in,
                const uint32_t* __restrict__ fill_in, uint32_t* __restrict__ list_out,
                uint32_t* __restrict__ fill_out, uint32_t seg) {
  ptr_list<IDX>([=](IDX n) { return down_cell<IDX, HASB>(out, in, bout, bin, n); }, list_in, fill_in, list_out,
                fill_out, seg);
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

static thread_local PtrInfo t_down_info{0, 0, 0, 0};  // soil_downstream_info

struct DownOut {
  float* out;
  double* out64;
};

// One round of a chunk (flow_paths.hpp ptr_chunk), dense or listed, on 32- or 64-bit offsets by the chunk
template <bool HASB>
static void down_launch_round(const PtrChunk& c, const PtrRound& q, hipStream_t st) {
  ptr_launch_round(c, q, st, k_down_list<uint32_t, HASB>, k_down_list<int64_t, HASB>, k_down_round<uint32_t, HASB>,
                   k_down_round<int64_t, HASB>, static_cast<double*>(c.extra[(q.r + 1) & 1]),
                   static_cast<const double*>(c.extra[q.r & 1]));
}

// One chunk of `models` models (flow_paths.hpp ptr_chunk) with this file's launches; HASB: the chunk's extra planes
// are the two B planes, 8 bytes a cell.
template <int K, int MODE, bool HASB>
static int down_chunk(DownOut o, const DownPlanes& in, int64_t models, int64_t H, int64_t W, const PathScales& scales,
                      char* scratch, hipStream_t st) {
  auto init = [&](const PtrChunk& c) {
    const bool vec = ptr_vec_init(W, in.graph, in.stop, in.p0, in.p1, in.p2);
    launch_vec(vec, k_down_init<K, true, MODE, HASB>, k_down_init<K, false, MODE, HASB>, ptr_init_grid(c, H, W, vec),
               st, c.rec[0], static_cast<double*>(c.extra[0]), in, H, W, scales, c.flags);
    return vec;
  };
  auto round = [&](const PtrChunk& c, const PtrRound& q) { down_launch_round<HASB>(c, q, st); };
  auto fin = [&](const PtrChunk&, dim3 grid, const uint4* rec) {
    k_down_final<<<grid, kPBlock, 0, st>>>(o.out, o.out64, rec, H * W);
  };
  return ptr_chunk(t_down_info, models, H, W, HASB ? sizeof(double) : 0, scratch, init, round, fin);
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
  if (int rc = check_grid_batch(w, B, H, W, edge, n_scales); rc != SOIL_OK) return rc;
  if (mode == kPower) {
    if (int rc = check_scales_positive(w, scales, n_scales); rc != SOIL_OK) return rc;
    if (int rc = check_dt(w, in.dt); rc != SOIL_OK) return rc;
  }
  return check_outputs_apart(w, out, out64, plane_cells(B, H * W), {in.graph, in.stop, in.p0, in.p1, in.p2});
}

// A call under the entry's name, through workspace slot WS_DOWNSTREAM (flow_paths.hpp ptr_run); without a scale L == 1
static int downstream_run(const char* what, int mode, DownOut o, const DownPlanes& in, int64_t B, int64_t H, int64_t W,
                          int edge, const float* scales, int64_t n_scales, void* stream) {
  if (int rc = check_downstream(what, mode, o.out, o.out64, in, scales, B, H, W, edge, n_scales); rc != SOIL_OK)
    return rc;
  SOIL_DEVICE();
  const hipStream_t st = as_stream(stream);
  const bool has_b = mode == kPower || in.p1 != nullptr;
  const bool d4 = edge == SOIL_D4;
  auto go = mode == kPower ? (d4 ? down_chunk<4, kPower, true> : down_chunk<8, kPower, true>)
            : has_b        ? (d4 ? down_chunk<4, kSum, true> : down_chunk<8, kSum, true>)
                           : (d4 ? down_chunk<4, kSum, false> : down_chunk<8, kSum, false>);
  return ptr_run(WS_DOWNSTREAM, t_down_info, B, H, W, has_b ? sizeof(double) : 0, scales, n_scales,
                 PathScale{1.0, 1.0, 1.0}, st, [&](int64_t b0, int64_t nb, const PathScales& s, char* scratch) {
                   const int64_t off = b0 * H * W;
                   return go(DownOut{at(o.out, off), at(o.out64, off)}, in.at(off), nb, H, W, s, scratch, st);
                 });
}

// ---- erosion-deposition: the stream-power step with a deposition term fed by an upstream sum -------------------
//
// soil_stream_power_deposit(_batch), soil_hip.h "flow graphs: erosion-deposition".  A fixed number of iterations,
// each: q = (float)(b - x) of the iterate before (k_dep_q), Qs = its upstream sum (graph.hip's rake-compress engine
// through rake_accumulate, as it is), the coefficients of the recurrence from the planes, Qs and q (k_dep_init), the
// rounds above (k_down_round / k_down_list with B, untouched), and k_dep_final, which keeps the fp64 iterate in
// scratch and on the last iteration makes the outputs and the per-model residual.  Per chunk of whole models, all on
// the caller's stream: nothing synchronises.

struct DepPlanes {
  const int32_t* graph;
  const float *height, *erosivity, *uplift, *deposition;
  double dt;
  DepPlanes at(int64_t off) const {
    return {graph + off, height + off, erosivity + off, soil::at(uplift, off), deposition + off, dt};
  }
};
// A chunk's planes between the iterations (workspace slot WS_DEPOSIT_PLANES): the iterate, q and Qs
struct DepWork {
  double* x;
  float *q, *qs;
};

// b of a cell: the lifted height, soil_stream_power's expression
__device__ __forceinline__ double dep_lifted(float h, float u, bool has_u, double dt) {
  const double hd = static_cast<double>(h);
  return has_u ? __dadd_rn(hd, __dmul_rn(dt, static_cast<double>(u))) : hd;
}

// One cell of the q pass.  FIRST: x^0 (b on a cell with an edge, the height on a terminal) and the +0 planes the
// first iteration reads in place of q and Qs — zeros accumulate to +0, so that iteration has no accumulation.
template <int K, bool FIRST>
__device__ __forceinline__ void dep_q_cell(const DepWork& w, int64_t n, int32_t g, float h, float u, bool has_u,
                                           int64_t x, int64_t y, int64_t H, int64_t W, double dt) {
  const bool has_edge = edge_kind<K>(g, x, y, H, W) >= 0;
  const double b = has_edge ? dep_lifted(h, u, has_u, dt) : static_cast<double>(h);
  if constexpr (FIRST) {
    w.x[n] = b;
    w.q[n] = 0.0f;
    w.qs[n] = 0.0f;
  } else {
    const float q = __double2float_rn(__dsub_rn(b, w.x[n]));
    w.q[n] = has_edge && q - q == 0.0f ? q : 0.0f;  // (q - q: zero for a finite float, NaN otherwise)
  }
}

// The q pass, in k_down_init's shape: threads along the row, a band of rows per work-group, grid.z the model; VEC:
// four cells per thread on 16-byte loads and stores.
template <int K, bool VEC, bool FIRST>
__global__ void __launch_bounds__(kPBlock) k_dep_q(DepWork w, DepPlanes in, int64_t H, int64_t W) {
  const int64_t y = (static_cast<int64_t>(blockIdx.x) * kPBlock + threadIdx.x) * (VEC ? 4 : 1);
  if (y >= W) return;
  const int64_t first64 = static_cast<int64_t>(blockIdx.z) * H * W;
  w.x += first64, w.q += first64, w.qs += first64;
  const int32_t* const graph = in.graph + first64;
  const float* const height = in.height + first64;
  const float* const uplift = in.uplift ? in.uplift + first64 : nullptr;
  SOIL_ROW_LOOP(x, H) {
    const int64_t n = x * W + y;
    if constexpr (VEC) {
      const int4 g = *reinterpret_cast<const int4*>(graph + n);
      const float4 h = *reinterpret_cast<const float4*>(height + n);
      const float4 u = uplift ? *reinterpret_cast<const float4*>(uplift + n) : make_float4(0.f, 0.f, 0.f, 0.f);
      dep_q_cell<K, FIRST>(w, n + 0, g.x, h.x, u.x, uplift != nullptr, x, y + 0, H, W, in.dt);
      dep_q_cell<K, FIRST>(w, n + 1, g.y, h.y, u.y, uplift != nullptr, x, y + 1, H, W, in.dt);
      dep_q_cell<K, FIRST>(w, n + 2, g.z, h.z, u.z, uplift != nullptr, x, y + 2, H, W, in.dt);
      dep_q_cell<K, FIRST>(w, n + 3, g.w, h.w, u.w, uplift != nullptr, x, y + 3, H, W, in.dt);
    } else {
      dep_q_cell<K, FIRST>(w, n, graph[n], height[n], uplift ? uplift[n] : 0.0f, uplift != nullptr, x, y, H, W, in.dt);
    }
  }
}

// The record of one cell of the deposit mode, and its B: soil_hip.h's operations in its order, each rounded once
template <int K>
__device__ __forceinline__ void dep_init_cell(uint4* __restrict__ rec, double* __restrict__ bcoef, int64_t n,
                                              int32_t gr, float h, float e, float u, bool has_u, float dep, float qs,
                                              float q, int64_t x, int64_t y, int64_t H, int64_t W, uint32_t first,
                                              const PathScale& s, double dt) {
  const int kind = edge_kind<K>(gr, x, y, H, W);
  double A = static_cast<double>(h), B = 0.0;  // a terminal: the height of the base level
  uint32_t ptr = (first + static_cast<uint32_t>(n)) | kFinal;
  if (kind >= 0) {
    ptr = first + static_cast<uint32_t>(gr);
    const double L = kind == 0 ? s.sx : (kind == 1 ? s.sy : s.dd);
    const double F = __ddiv_rn(__dmul_rn(static_cast<double>(e), dt), L);
    const double g = static_cast<double>(dep);
    const double d = __dadd_rn(__dadd_rn(1.0, F), g);
    const double b = dep_lifted(h, u, has_u, dt);
    const double Qup = __dsub_rn(static_cast<double>(qs), static_cast<double>(q));
    A = __ddiv_rn(__dadd_rn(__dmul_rn(__dadd_rn(1.0, g), b), __dmul_rn(g, Qup)), d);
    B = __ddiv_rn(F, d);
  }
  rec[n] = down_rec(ptr, kind < 0 ? 0u : 1u, A);
  bcoef[n] = B;
}

// The init pass of the deposit mode, as k_down_init: seven planes, each a 16-byte load in the VEC form
template <int K, bool VEC>
__global__ void __launch_bounds__(kPBlock)
    k_dep_init(uint4* __restrict__ rec, double* __restrict__ bcoef, DepPlanes in, const float* __restrict__ qs,
               const float* __restrict__ q, int64_t H, int64_t W, PathScales scales, int* __restrict__ flags) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x < kPathFlags)
    flags[threadIdx.x] = threadIdx.x == 0 ? 1 : 0;
  const int64_t y = (static_cast<int64_t>(blockIdx.x) * kPBlock + threadIdx.x) * (VEC ? 4 : 1);
  if (y >= W) return;
  const int64_t first64 = static_cast<int64_t>(blockIdx.z) * H * W;
  const uint32_t first = static_cast<uint32_t>(first64);
  const PathScale s = scales.per_model ? scales.per_model[blockIdx.z] : scales.one;
  rec += first64, bcoef += first64, qs += first64, q += first64;
  const int32_t* const graph = in.graph + first64;
  const float* const height = in.height + first64;
  const float* const erosivity = in.erosivity + first64;
  const float* const deposition = in.deposition + first64;
  const float* const uplift = in.uplift ? in.uplift + first64 : nullptr;
  const bool has_u = uplift != nullptr;
  SOIL_ROW_LOOP(x, H) {
    const int64_t n = x * W + y;
    if constexpr (VEC) {
      const int4 g = *reinterpret_cast<const int4*>(graph + n);
      const float4 h = *reinterpret_cast<const float4*>(height + n);
      const float4 e = *reinterpret_cast<const float4*>(erosivity + n);
      const float4 u = uplift ? *reinterpret_cast<const float4*>(uplift + n) : make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 dp = *reinterpret_cast<const float4*>(deposition + n);
      const float4 s4 = *reinterpret_cast<const float4*>(qs + n);
      const float4 q4 = *reinterpret_cast<const float4*>(q + n);
      dep_init_cell<K>(rec, bcoef, n + 0, g.x, h.x, e.x, u.x, has_u, dp.x, s4.x, q4.x, x, y + 0, H, W, first, s, in.dt);
      dep_init_cell<K>(rec, bcoef, n + 1, g.y, h.y, e.y, u.y, has_u, dp.y, s4.y, q4.y, x, y + 1, H, W, first, s, in.dt);
      dep_init_cell<K>(rec, bcoef, n + 2, g.z, h.z, e.z, u.z, has_u, dp.z, s4.z, q4.z, x, y + 2, H, W, first, s, in.dt);
      dep_init_cell<K>(rec, bcoef, n + 3, g.w, h.w, e.w, u.w, has_u, dp.w, s4.w, q4.w, x, y + 3, H, W, first, s, in.dt);
    } else {
      dep_init_cell<K>(rec, bcoef, n, graph[n], height[n], erosivity[n], uplift ? uplift[n] : 0.0f, has_u,
                       deposition[n], qs[n], q[n], x, y, H, W, first, s, in.dt);
    }
  }
}

// Final of an iteration, k_down_final's shape: the iterate (A, or the quiet NaN as k_down_final writes it) replaces
// the one before in `x`; the last iteration also makes the outputs and, asked for, the residual of its model
// (grid.z): max |x - x_before| over the cells where that is no NaN, as the largest WORD of a non-negative double — an
// integer max through LDS and one global atomic a work-group, no floating-point atomic, any order the same bits.
__global__ void __launch_bounds__(kPBlock)
    k_dep_final(float* __restrict__ out, double* __restrict__ out64, double* __restrict__ x,
                unsigned long long* __restrict__ residual, const uint4* __restrict__ rec, int64_t cells) {
  __shared__ unsigned long long s_max;
  if (residual) {
    if (threadIdx.x == 0) s_max = 0ull;
    __syncthreads();
  }
  const int64_t first64 = static_cast<int64_t>(blockIdx.z) * cells;
  unsigned long long mine = 0ull;
  for (int64_t n = static_cast<int64_t>(blockIdx.x) * kPBlock + threadIdx.x; n < cells;
       n += static_cast<int64_t>(gridDim.x) * kPBlock) {
    const uint4 r = rec[first64 + n];
    const double A = down_a(r);
    const bool nan = (r.x & kFinal) == 0 || A != A;
    const double xn = nan ? __hiloint2double(0x7ff80000, 0) : A;
    if (residual) {
      const double diff = fabs(__dsub_rn(xn, x[first64 + n]));
      const unsigned long long w = static_cast<unsigned long long>(__double_as_longlong(diff));
      if (diff == diff && w > mine) mine = w;
    }
    x[first64 + n] = xn;
    if (out) out[first64 + n] = nan ? bits2f(0x7fc00000u) : __double2float_rn(A);
    if (out64) out64[first64 + n] = xn;
  }
  if (residual) {
    if (mine) atomicMax(&s_max, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_max) atomicMax(residual + blockIdx.z, s_max);
  }
}

// The outputs of an iterated step, each may be null; `flux` is the deposit step's alone
struct StepOut {
  float* out;
  double* out64;
  float* flux;
  double* residual;  // a word a model
  StepOut at(int64_t off, int64_t b0) const {
    return {soil::at(out, off), soil::at(out64, off), soil::at(flux, off), soil::at(residual, b0)};
  }
};
// soil_stream_power_deposit_info: launches, chunks, iterations, bytes of scratch
struct DepInfo {
  int64_t launches, chunks, iters, bytes;
};
static thread_local DepInfo t_dep_info{0, 0, 0, 0};

// One solve of an iterated step over a chunk (flow_paths.hpp ptr_chunk): `init` makes the records and B from the
// iterate before, the rounds are the recurrence's with B, and k_dep_final leaves the new iterate in `x`.  `o`: the
// outputs on the step's last pass, nothing before it.  Adds what it launched to `launches`.
template <typename Init>
static int solve_pass(int64_t& launches, int64_t models, int64_t H, int64_t W, char* scratch, hipStream_t st, Init init,
                      double* x, const StepOut& o) {
  PtrInfo pinfo{0, 0, 0, 0};
  auto round = [&](const PtrChunk& c, const PtrRound& q) { down_launch_round<true>(c, q, st); };
  auto fin = [&](const PtrChunk&, dim3 grid, const uint4* rec) {
    k_dep_final<<<grid, kPBlock, 0, st>>>(o.out, o.out64, x, reinterpret_cast<unsigned long long*>(o.residual), rec,
                                          H * W);
  };
  if (int rc = ptr_chunk(pinfo, models, H, W, sizeof(double), scratch, init, round, fin); rc != SOIL_OK) return rc;
  launches += 2 + pinfo.rounds;
  return SOIL_OK;
}

template <int K>
static void dep_launch_q(DepInfo& info, const DepWork& w, const DepPlanes& in, int64_t models, int64_t H, int64_t W,
                         bool first, hipStream_t st) {
  const bool vec = ptr_vec_init(W, in.graph, in.height, in.uplift, w.x, w.q, w.qs);
  dim3 grid = grid_rows(H, vec ? W / 4 : W, kPBlock);
  grid.z = static_cast<unsigned>(models);
  if (first) launch_vec(vec, k_dep_q<K, true, true>, k_dep_q<K, false, true>, grid, st, w, in, H, W);
  else launch_vec(vec, k_dep_q<K, true, false>, k_dep_q<K, false, false>, grid, st, w, in, H, W);
  info.launches += 1;
}

// Neither the flux (4 bytes a cell) nor the residual (8 bytes a model) shares a byte with one of `planes` (4 bytes a
// cell), with out64 or with the other; `msg` names the two an entry has
static int check_side_outputs_apart(const std::string& msg, const StepOut& o, int64_t B, size_t cells,
                                    std::initializer_list<const void*> planes) {
  const size_t b_res = 8 * static_cast<size_t>(B);
  for (const void* p : planes)
    SOIL_REQUIRE(!overlaps(o.flux, 4 * cells, p, 4 * cells) && !overlaps(o.residual, b_res, p, 4 * cells), msg);
  SOIL_REQUIRE(!overlaps(o.flux, 4 * cells, o.out64, 8 * cells) && !overlaps(o.residual, b_res, o.out64, 8 * cells) &&
                   !overlaps(o.flux, 4 * cells, o.residual, b_res),
               msg);
  return SOIL_OK;
}

// What the deposit entries refuse before any device work: soil_stream_power's refusals and their own.  `n`: the
// slope exponent, 1.0 from the entries that take none.
static int check_deposit(const char* what, const StepOut& o, const DepPlanes& in, double n, int iters,
                         const float* scales, int64_t B, int64_t H, int64_t W, int edge, int64_t n_scales) {
  const std::string w(what);
  const DownPlanes power{in.graph, nullptr, in.height, in.erosivity, in.uplift, in.dt};
  if (int rc = check_downstream(what, kPower, o.out, o.out64, power, scales, B, H, W, edge, n_scales); rc != SOIL_OK)
    return rc;
  SOIL_REQUIRE(in.deposition, w + ": null deposition");
  SOIL_REQUIRE(std::isfinite(n) && n >= 1.0 && n <= 16.0,
               w + ": n must be a finite slope exponent in 1 .. 16 (n < 1 makes the per-cell equation concave: it needs "
                   "a safeguarded solve per cell, which no affine map expresses)");
  SOIL_REQUIRE(iters >= 1, w + ": iters must be >= 1");
  const size_t cells = plane_cells(B, H * W);
  // (out and out64 are apart: check_downstream saw to it)
  if (int rc = check_outputs_apart(w, o.out, o.out64, cells, {in.deposition}); rc != SOIL_OK) return rc;
  return check_side_outputs_apart(w + ": flux or residual aliases another plane", o, B, cells,
                                  {in.graph, in.height, in.erosivity, in.uplift, in.deposition, o.out});
}

// What the two iterated drivers set up before ptr_run: the planes a chunk keeps between its passes (`side`: the bytes
// a cell of each, 0 for none; sized for the call's first chunk, each padded to 256 bytes) in workspace `slot`, the
// residual cleared in stream order, and the bytes of scratch of the call, those planes and ptr_run's block
struct IterSetup {
  char* plane[3];
  int64_t bytes;
};
static int iter_setup(IterSetup& s, WorkspaceSlot slot, const size_t (&side)[3], double* residual, int64_t B, int64_t H,
                      int64_t W, const float* scales, int64_t n_scales, hipStream_t st) {
  const PtrBlock blk = ptr_block(B, H * W, sizeof(double), scales, n_scales);
  size_t total = 0, off[3];
  for (int i = 0; i < 3; ++i) off[i] = total, total += align256(side[i] * static_cast<size_t>(blk.cells));
  void* base = nullptr;
  if (total)
    if (int rc = workspace_get(slot, total, &base); rc != SOIL_OK) return rc;
  for (int i = 0; i < 3; ++i) s.plane[i] = static_cast<char*>(base) + off[i];
  if (residual) SOIL_HIP(hipMemsetAsync(residual, 0, sizeof(double) * static_cast<size_t>(B), st));
  s.bytes = static_cast<int64_t>(total + blk.b_scales + blk.b_chunk);
  return SOIL_OK;
}

// ---- slope exponents above 1: Newton steps on the whole triangular system, each one solve of the rounds above ---
//
// soil_stream_power_n(_batch), soil_hip.h "flow graphs: slope exponents above 1".  x^0 is soil_stream_power's solve
// (k_down_init<kPower>, the rounds, k_dep_final keeping the fp64 iterate); then `iters` times the coefficients of the
// linearisation about the iterate before (k_pn_init: the receiver's value an 8-byte gather, a slope raised to a
// power), the rounds untouched, and k_dep_final, which on the last iteration makes the outputs and the residual.  Per
// chunk of whole models, all on the caller's stream: nothing synchronises.

struct PnPlanes {
  const int32_t* graph;
  const int32_t* stop;
  const float *height, *erosivity, *uplift;
  double dt, n, n1;  // n1 = n - 1, made once on the host
  PnPlanes at(int64_t off) const {
    return {graph + off, soil::at(stop, off), height + off, erosivity + off, soil::at(uplift, off), dt, n, n1};
  }
};

// The record of one cell of the Newton mode, and its B: soil_hip.h's operations in its order, each rounded once.
// `xit`: the iterate before of the cell's model, xi its value at the cell; a valid edge_kind puts gr inside the model.
template <int K>
__device__ __forceinline__ void pn_init_cell(uint4* __restrict__ rec, double* __restrict__ bcoef, int64_t n,
                                             int32_t gr, bool stop, float h, float e, float u, bool has_u, double xi,
                                             const double* __restrict__ xit, int64_t x, int64_t y, int64_t H,
                                             int64_t W, uint32_t first, const PathScale& s, const PnPlanes& in) {
  const int kind = stop ? -1 : edge_kind<K>(gr, x, y, H, W);
  double A = static_cast<double>(h), B = 0.0;  // a terminal: the height of the base level
  uint32_t ptr = (first + static_cast<uint32_t>(n)) | kFinal;
  if (kind >= 0) {
    ptr = first + static_cast<uint32_t>(gr);
    const double L = kind == 0 ? s.sx : (kind == 1 ? s.sy : s.dd);
    const double d = __dsub_rn(xi, xit[gr]);
    const double S = d <= 0.0 ? 0.0 : __ddiv_rn(d, L);  // (a NaN d is not <= 0: it stays a NaN)
    const double P = in.n == 2.0 ? S : sp_pow(S, in.n1);
    const double kd = __dmul_rn(static_cast<double>(e), in.dt);
    const double F = __dmul_rn(__ddiv_rn(__dmul_rn(in.n, kd), L), P);
    const double c = __dmul_rn(__dmul_rn(kd, in.n1), __dmul_rn(P, S));
    const double b = dep_lifted(h, u, has_u, in.dt);
    const double D = __dadd_rn(1.0, F);
    A = __ddiv_rn(__dadd_rn(b, c), D);
    B = __ddiv_rn(F, D);
  }
  rec[n] = down_rec(ptr, kind < 0 ? 0u : 1u, A);
  bcoef[n] = B;
}

// The init pass of the Newton mode, as k_dep_init: five planes and the iterate, each a 16-byte load in the VEC form
// (the iterate two of them), and the gather of the receiver's iterate.  The gather hangs on the load of the graph
// entry, two memory latencies in a row for every row a thread walks, so the band of rows is kPnBand, shorter than
// kRowBand: at 256^2 sixteen rows a work-group left sixteen work-groups on the device, each waiting out thirty-two
// latencies.
constexpr int kPnBand = 4;
template <int K, bool VEC>
__global__ void __launch_bounds__(kPBlock)
    k_pn_init(uint4* __restrict__ rec, double* __restrict__ bcoef, PnPlanes in, const double* __restrict__ xit,
              int64_t H, int64_t W, PathScales scales, int* __restrict__ flags) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x < kPathFlags)
    flags[threadIdx.x] = threadIdx.x == 0 ? 1 : 0;
  const int64_t y = (static_cast<int64_t>(blockIdx.x) * kPBlock + threadIdx.x) * (VEC ? 4 : 1);
  if (y >= W) return;
  const int64_t first64 = static_cast<int64_t>(blockIdx.z) * H * W;
  const uint32_t first = static_cast<uint32_t>(first64);
  const PathScale s = scales.per_model ? scales.per_model[blockIdx.z] : scales.one;
  rec += first64, bcoef += first64, xit += first64;
  const int32_t* const graph = in.graph + first64;
  const int32_t* const stop = in.stop ? in.stop + first64 : nullptr;
  const float* const height = in.height + first64;
  const float* const erosivity = in.erosivity + first64;
  const float* const uplift = in.uplift ? in.uplift + first64 : nullptr;
  const bool has_u = uplift != nullptr;
  for (int64_t band = blockIdx.y; band * kPnBand < H; band += gridDim.y) {
    for (int64_t x = band * kPnBand, end = x + kPnBand < H ? x + kPnBand : H; x < end; ++x) {
      const int64_t n = x * W + y;
      if constexpr (VEC) {
        const int4 g = *reinterpret_cast<const int4*>(graph + n);
        const int4 st = stop ? *reinterpret_cast<const int4*>(stop + n) : make_int4(0, 0, 0, 0);
        const float4 h = *reinterpret_cast<const float4*>(height + n);
        const float4 e = *reinterpret_cast<const float4*>(erosivity + n);
        const float4 u = uplift ? *reinterpret_cast<const float4*>(uplift + n) : make_float4(0.f, 0.f, 0.f, 0.f);
        const double2 x01 = *reinterpret_cast<const double2*>(xit + n);
        const double2 x23 = *reinterpret_cast<const double2*>(xit + n + 2);
        pn_init_cell<K>(rec, bcoef, n + 0, g.x, st.x != 0, h.x, e.x, u.x, has_u, x01.x, xit, x, y + 0, H, W, first, s, in);
        pn_init_cell<K>(rec, bcoef, n + 1, g.y, st.y != 0, h.y, e.y, u.y, has_u, x01.y, xit, x, y + 1, H, W, first, s, in);
        pn_init_cell<K>(rec, bcoef, n + 2, g.z, st.z != 0, h.z, e.z, u.z, has_u, x23.x, xit, x, y + 2, H, W, first, s, in);
        pn_init_cell<K>(rec, bcoef, n + 3, g.w, st.w != 0, h.w, e.w, u.w, has_u, x23.y, xit, x, y + 3, H, W, first, s, in);
      } else {
        pn_init_cell<K>(rec, bcoef, n, graph[n], stop ? stop[n] != 0 : false, height[n], erosivity[n],
                        uplift ? uplift[n] : 0.0f, has_u, xit[n], xit, x, y, H, W, first, s, in);
      }
    }
  }
}

// The grid of an init pass on bands of kPnBand rows: ptr_init_grid's, grid.y the shorter bands
static dim3 pn_init_grid(const PtrChunk& c, int64_t H, int64_t W, bool vec) {
  const dim3 grid = ptr_init_grid(c, H, W, vec);
  const int64_t bands = (H + kPnBand - 1) / kPnBand;
  return dim3(grid.x, static_cast<unsigned>(bands < 65535 ? bands : 65535), grid.z);
}

// The planes of soil_stream_power_deposit_n: the deposit step's and the slope exponent, n1 = n - 1 made once on the host
struct DnPlanes {
  DepPlanes dep;
  double n, n1;
  DnPlanes at(int64_t off) const { return {dep.at(off), n, n1}; }
};

// The record of one cell of the deposit step at a slope exponent (soil_stream_power_deposit_n), and its B:
// soil_hip.h's operations in its order, each rounded once.  pn_init_cell's slope, power, F and c; dep_init_cell's g,
// Qup and the self-implicit (1 + g) and + g.  There is no stop plane, as in the deposit step.
template <int K>
__device__ __forceinline__ void dn_init_cell(uint4* __restrict__ rec, double* __restrict__ bcoef, int64_t n,
                                             int32_t gr, float h, float e, float u, bool has_u, float dep, float qs,
                                             float q, double xi, const double* __restrict__ xit, int64_t x, int64_t y,
                                             int64_t H, int64_t W, uint32_t first, const PathScale& s,
                                             const DnPlanes& in) {
  const int kind = edge_kind<K>(gr, x, y, H, W);
  double A = static_cast<double>(h), B = 0.0;  // a terminal: the height of the base level
  uint32_t ptr = (first + static_cast<uint32_t>(n)) | kFinal;
  if (kind >= 0) {
    ptr = first + static_cast<uint32_t>(gr);
    const double dt = in.dep.dt;
    const double L = kind == 0 ? s.sx : (kind == 1 ? s.sy : s.dd);
    const double Qup = __dsub_rn(static_cast<double>(qs), static_cast<double>(q));
    const double d = __dsub_rn(xi, xit[gr]);
    const double S = d <= 0.0 ? 0.0 : __ddiv_rn(d, L);  // (a NaN d is not <= 0: it stays a NaN)
    const double P = in.n == 2.0 ? S : sp_pow(S, in.n1);
    const double kd = __dmul_rn(static_cast<double>(e), dt);
    const double F = __dmul_rn(__ddiv_rn(__dmul_rn(in.n, kd), L), P);
    const double c = __dmul_rn(__dmul_rn(kd, in.n1), __dmul_rn(P, S));
    const double g = static_cast<double>(dep);
    const double b = dep_lifted(h, u, has_u, dt);
    const double D = __dadd_rn(__dadd_rn(1.0, F), g);
    A = __ddiv_rn(__dadd_rn(__dadd_rn(__dmul_rn(__dadd_rn(1.0, g), b), __dmul_rn(g, Qup)), c), D);
    B = __ddiv_rn(F, D);
  }
  rec[n] = down_rec(ptr, kind < 0 ? 0u : 1u, A);
  bcoef[n] = B;
}

// The init pass of the deposit step at a slope exponent: k_dep_init's seven planes and k_pn_init's iterate with the
// gather of the receiver's value, on k_pn_init's bands of kPnBand rows for the reason given there.
template <int K, bool VEC>
__global__ void __launch_bounds__(kPBlock)
    k_dn_init(uint4* __restrict__ rec, double* __restrict__ bcoef, DnPlanes in, const float* __restrict__ qs,
              const float* __restrict__ q, const double* __restrict__ xit, int64_t H, int64_t W, PathScales scales,
              int* __restrict__ flags) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x < kPathFlags)
    flags[threadIdx.x] = threadIdx.x == 0 ? 1 : 0;
  const int64_t y = (static_cast<int64_t>(blockIdx.x) * kPBlock + threadIdx.x) * (VEC ? 4 : 1);
  if (y >= W) return;
  const int64_t first64 = static_cast<int64_t>(blockIdx.z) * H * W;
  const uint32_t first = static_cast<uint32_t>(first64);
  const PathScale s = scales.per_model ? scales.per_model[blockIdx.z] : scales.one;
  rec += first64, bcoef += first64, qs += first64, q += first64, xit += first64;
  const int32_t* const graph = in.dep.graph + first64;
  const float* const height = in.dep.height + first64;
  const float* const erosivity = in.dep.erosivity + first64;
  const float* const deposition = in.dep.deposition + first64;
  const float* const uplift = in.dep.uplift ? in.dep.uplift + first64 : nullptr;
  const bool has_u = uplift != nullptr;
  for (int64_t band = blockIdx.y; band * kPnBand < H; band += gridDim.y) {
    for (int64_t x = band * kPnBand, end = x + kPnBand < H ? x + kPnBand : H; x < end; ++x) {
      const int64_t n = x * W + y;
      if constexpr (VEC) {
        const int4 g = *reinterpret_cast<const int4*>(graph + n);
        const float4 h = *reinterpret_cast<const float4*>(height + n);
        const float4 e = *reinterpret_cast<const float4*>(erosivity + n);
        const float4 u = uplift ? *reinterpret_cast<const float4*>(uplift + n) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 dp = *reinterpret_cast<const float4*>(deposition + n);
        const float4 s4 = *reinterpret_cast<const float4*>(qs + n);
        const float4 q4 = *reinterpret_cast<const float4*>(q + n);
        const double2 x01 = *reinterpret_cast<const double2*>(xit + n);
        const double2 x23 = *reinterpret_cast<const double2*>(xit + n + 2);
        dn_init_cell<K>(rec, bcoef, n + 0, g.x, h.x, e.x, u.x, has_u, dp.x, s4.x, q4.x, x01.x, xit, x, y + 0, H, W,
                        first, s, in);
        dn_init_cell<K>(rec, bcoef, n + 1, g.y, h.y, e.y, u.y, has_u, dp.y, s4.y, q4.y, x01.y, xit, x, y + 1, H, W,
                        first, s, in);
        dn_init_cell<K>(rec, bcoef, n + 2, g.z, h.z, e.z, u.z, has_u, dp.z, s4.z, q4.z, x23.x, xit, x, y + 2, H, W,
                        first, s, in);
        dn_init_cell<K>(rec, bcoef, n + 3, g.w, h.w, e.w, u.w, has_u, dp.w, s4.w, q4.w, x23.y, xit, x, y + 3, H, W,
                        first, s, in);
      } else {
        dn_init_cell<K>(rec, bcoef, n, graph[n], height[n], erosivity[n], uplift ? uplift[n] : 0.0f, has_u,
                        deposition[n], qs[n], q[n], xit[n], xit, x, y, H, W, first, s, in);
      }
    }
  }
}

static thread_local DepInfo t_pn_info{0, 0, 0, 0};  // soil_stream_power_n_info

// One chunk of `models` models: the start (soil_stream_power's init), then `iters` times k_pn_init, each a solve
// pass.  iters == 0 (n == 1): the start alone, with soil_stream_power's final.  `in`, `o` and `x` are the chunk's own.
template <int K>
static int pn_chunk(StepOut o, const PnPlanes& in, double* x, int iters, int64_t models, int64_t H, int64_t W,
                    const PathScales& scales, char* scratch, hipStream_t st) {
  t_pn_info.chunks += 1;
  const DownPlanes power{in.graph, in.stop, in.height, in.erosivity, in.uplift, in.dt};
  const bool vec = ptr_vec_init(W, in.graph, in.stop, in.height, in.erosivity, in.uplift, x);
  auto start = [&](const PtrChunk& c) {
    launch_vec(vec, k_down_init<K, true, kPower, true>, k_down_init<K, false, kPower, true>,
               ptr_init_grid(c, H, W, vec), st, c.rec[0], static_cast<double*>(c.extra[0]), power, H, W, scales,
               c.flags);
    return vec;
  };
  auto init = [&](const PtrChunk& c) {
    launch_vec(vec, k_pn_init<K, true>, k_pn_init<K, false>, pn_init_grid(c, H, W, vec), st, c.rec[0],
               static_cast<double*>(c.extra[0]), in, x, H, W, scales, c.flags);
    return vec;
  };
  if (iters == 0) {
    PtrInfo pinfo{0, 0, 0, 0};
    auto round = [&](const PtrChunk& c, const PtrRound& q) { down_launch_round<true>(c, q, st); };
    auto fin = [&](const PtrChunk&, dim3 grid, const uint4* rec) {
      k_down_final<<<grid, kPBlock, 0, st>>>(o.out, o.out64, rec, H * W);
    };
    if (int rc = ptr_chunk(pinfo, models, H, W, sizeof(double), scratch, start, round, fin); rc != SOIL_OK) return rc;
    t_pn_info.launches += 2 + pinfo.rounds;
    return SOIL_OK;
  }
  if (int rc = solve_pass(t_pn_info.launches, models, H, W, scratch, st, start, x, StepOut{}); rc != SOIL_OK) return rc;
  for (int j = 1; j <= iters; ++j)
    if (int rc = solve_pass(t_pn_info.launches, models, H, W, scratch, st, init, x, j == iters ? o : StepOut{});
        rc != SOIL_OK)
      return rc;
  return SOIL_OK;
}

// What the two entries refuse before any device work: soil_stream_power's refusals and their own
static int check_power_n(const char* what, const StepOut& o, const PnPlanes& in, int iters, const float* scales,
                         int64_t B, int64_t H, int64_t W, int edge, int64_t n_scales) {
  const std::string w(what);
  const DownPlanes power{in.graph, in.stop, in.height, in.erosivity, in.uplift, in.dt};
  if (int rc = check_downstream(what, kPower, o.out, o.out64, power, scales, B, H, W, edge, n_scales); rc != SOIL_OK)
    return rc;
  SOIL_REQUIRE(std::isfinite(in.n) && in.n >= 1.0 && in.n <= 16.0,
               w + ": n must be a finite slope exponent in 1 .. 16 (n < 1 makes the per-cell equation concave: it needs "
                   "a safeguarded solve per cell, which no affine map expresses)");
  SOIL_REQUIRE(iters >= 1, w + ": iters must be >= 1");
  return check_side_outputs_apart(w + ": residual aliases another plane", o, B, plane_cells(B, H * W),
                                  {in.graph, in.stop, in.height, in.erosivity, in.uplift, o.out});
}

// A call, under the entry's name: the chunks of ptr_run through slot WS_POWER_N, the chunk's iterate in
// WS_POWER_N_ITERATE beside them
static int power_n_run(const char* what, StepOut o, const PnPlanes& in, int iters, int64_t B, int64_t H, int64_t W,
                       int edge, const float* scales, int64_t n_scales, void* stream) {
  if (int rc = check_power_n(what, o, in, iters, scales, B, H, W, edge, n_scales); rc != SOIL_OK) return rc;
  SOIL_DEVICE();
  const hipStream_t st = as_stream(stream);
  if (in.n == 1.0) iters = 0;  // soil_stream_power's single solve and nothing else
  t_pn_info = DepInfo{0, 0, iters, 0};
  IterSetup s;
  if (int rc = iter_setup(s, WS_POWER_N_ITERATE, {iters ? sizeof(double) : 0, 0, 0}, o.residual, B, H, W, scales,
                          n_scales, st);
      rc != SOIL_OK)
    return rc;
  double* const x = reinterpret_cast<double*>(s.plane[0]);  // (null with iters == 0)
  PtrInfo pinfo{0, 0, 0, 0};
  auto go = edge == SOIL_D4 ? pn_chunk<4> : pn_chunk<8>;
  const int rc = ptr_run(WS_POWER_N, pinfo, B, H, W, sizeof(double), scales, n_scales, PathScale{1.0, 1.0, 1.0}, st,
                         [&](int64_t b0, int64_t nb, const PathScales& sc, char* scratch) {
                           const int64_t off = b0 * H * W;
                           return go(o.at(off, b0), in.at(off), x, iters, nb, H, W, sc, scratch, st);
                         });
  t_pn_info.bytes = s.bytes;
  return rc;
}

// ---- the deposit driver: soil_stream_power_deposit and, with a slope exponent, soil_stream_power_deposit_n ----
//
// Below the init passes of both sections, which a chunk launches: k_dep_init at n == 1, k_dn_init at any other n.

// One chunk of `models` models: x^0, then `iters` times q, Qs and a solve pass from them, then the flux of the
// returned iterate.  `in`, `o` and `w` are the chunk's own.  in.n == 1: x^0 = b from the first q pass, whose zero
// planes stand in for the first iteration's q and Qs, and k_dep_init.  Any other n (soil_stream_power_deposit_n):
// x^0 is soil_stream_power's solve, every iteration has its q pass and accumulation, and the init pass is k_dn_init.
template <int K>
static int dep_chunk(DepInfo& info, StepOut o, const DnPlanes& in, const DepWork& w, int iters, int64_t models,
                     int64_t H, int64_t W, int edge, const PathScales& scales, char* scratch, RakeStats& rake,
                     hipStream_t st) {
  info.chunks += 1;
  const DepPlanes& dep = in.dep;
  const bool newton = in.n != 1.0;
  const bool vec = ptr_vec_init(W, dep.graph, dep.height, dep.erosivity, dep.uplift, dep.deposition, w.qs, w.q, w.x);
  auto init = [&](const PtrChunk& c) {
    launch_vec(vec, k_dep_init<K, true>, k_dep_init<K, false>, ptr_init_grid(c, H, W, vec), st, c.rec[0],
               static_cast<double*>(c.extra[0]), dep, w.qs, w.q, H, W, scales, c.flags);
    return vec;
  };
  auto init_n = [&](const PtrChunk& c) {
    launch_vec(vec, k_dn_init<K, true>, k_dn_init<K, false>, pn_init_grid(c, H, W, vec), st, c.rec[0],
               static_cast<double*>(c.extra[0]), in, w.qs, w.q, w.x, H, W, scales, c.flags);
    return vec;
  };
  if (newton) {
    const DownPlanes power{dep.graph, nullptr, dep.height, dep.erosivity, dep.uplift, dep.dt};
    auto start = [&](const PtrChunk& c) {
      launch_vec(vec, k_down_init<K, true, kPower, true>, k_down_init<K, false, kPower, true>,
                 ptr_init_grid(c, H, W, vec), st, c.rec[0], static_cast<double*>(c.extra[0]), power, H, W, scales,
                 c.flags);
      return vec;
    };
    if (int rc = solve_pass(info.launches, models, H, W, scratch, st, start, w.x, StepOut{}); rc != SOIL_OK) return rc;
  } else {
    dep_launch_q<K>(info, w, dep, models, H, W, true, st);
    SOIL_LAUNCH_CHECK();
  }
  for (int k = 1; k <= iters; ++k) {
    if (k > 1 || newton) {
      dep_launch_q<K>(info, w, dep, models, H, W, false, st);
      SOIL_LAUNCH_CHECK();
      if (int rc = rake_accumulate(w.qs, dep.graph, w.q, models, H, W, edge, st, WS_DEPOSIT_RAKE, &rake); rc != SOIL_OK)
        return rc;
    }
    const StepOut ok = k == iters ? o : StepOut{};
    if (int rc = newton ? solve_pass(info.launches, models, H, W, scratch, st, init_n, w.x, ok)
                        : solve_pass(info.launches, models, H, W, scratch, st, init, w.x, ok);
        rc != SOIL_OK)
      return rc;
  }
  if (o.flux) {
    dep_launch_q<K>(info, w, dep, models, H, W, false, st);
    SOIL_LAUNCH_CHECK();
    if (int rc = rake_accumulate(o.flux, dep.graph, w.q, models, H, W, edge, st, WS_DEPOSIT_RAKE, &rake); rc != SOIL_OK)
      return rc;
  }
  return SOIL_OK;
}

static thread_local DepInfo t_dn_info{0, 0, 0, 0};  // soil_stream_power_deposit_n_info

// A call, under the entry's name: the chunks of ptr_run through slot WS_DEPOSIT, the chunk's planes in
// WS_DEPOSIT_PLANES beside them.  `info`: the record of the entry's family; the deposit step at a slope exponent
// shares the slots, as a thread's calls of one entry do.
static int deposit_run(const char* what, DepInfo& info, StepOut o, const DnPlanes& in, int iters, int64_t B, int64_t H,
                       int64_t W, int edge, const float* scales, int64_t n_scales, void* stream) {
  if (int rc = check_deposit(what, o, in.dep, in.n, iters, scales, B, H, W, edge, n_scales); rc != SOIL_OK) return rc;
  SOIL_DEVICE();
  const hipStream_t st = as_stream(stream);
  info = DepInfo{0, 0, iters, 0};
  IterSetup s;
  if (int rc = iter_setup(s, WS_DEPOSIT_PLANES, {8, 4, 4}, o.residual, B, H, W, scales, n_scales, st); rc != SOIL_OK)
    return rc;
  const DepWork w{reinterpret_cast<double*>(s.plane[0]), reinterpret_cast<float*>(s.plane[1]),
                  reinterpret_cast<float*>(s.plane[2])};
  RakeStats rake{0, 0};
  PtrInfo pinfo{0, 0, 0, 0};
  auto go = edge == SOIL_D4 ? dep_chunk<4> : dep_chunk<8>;
  const int rc = ptr_run(WS_DEPOSIT, pinfo, B, H, W, sizeof(double), scales, n_scales, PathScale{1.0, 1.0, 1.0}, st,
                         [&](int64_t b0, int64_t nb, const PathScales& sc, char* scratch) {
                           const int64_t off = b0 * H * W;
                           return go(info, o.at(off, b0), in.at(off), w, iters, nb, H, W, edge, sc, scratch, rake, st);
                         });
  info.launches += rake.launches;
  info.bytes = s.bytes + rake.bytes;
  return rc;
}

}  // namespace soil

using namespace soil;

extern "C" {

// (each grid entry is its batch twin's call with B = 1 and one scale pair, under its own name)

int soil_downstream(float* out, double* out64, const int32_t* graph, const float* a, const float* b, const float* t,
                    const int32_t* stop, int64_t H, int64_t W, int edge, const float scale[2], void* stream) {
  return downstream_run("downstream", kSum, DownOut{out, out64}, DownPlanes{graph, stop, a, b, t, 0.0}, 1, H, W, edge,
                        scale, 1, stream);
}

int soil_downstream_batch(float* out, double* out64, const int32_t* graph, const float* a, const float* b,
                          const float* t, const int32_t* stop, int64_t B, int64_t H, int64_t W, int edge,
                          const float* scales, int64_t n_scales, void* stream) {
  return downstream_run("downstream_batch", kSum, DownOut{out, out64}, DownPlanes{graph, stop, a, b, t, 0.0}, B, H, W,
                        edge, scales, n_scales, stream);
}

int soil_stream_power(float* out, double* out64, const float* height, const int32_t* graph, const float* erosivity,
                      const float* uplift, const int32_t* stop, int64_t H, int64_t W, int edge, const float scale[2],
                      double dt, void* stream) {
  return downstream_run("stream_power", kPower, DownOut{out, out64}, DownPlanes{graph, stop, height, erosivity, uplift, dt},
                        1, H, W, edge, scale, 1, stream);
}

int soil_stream_power_batch(float* out, double* out64, const float* height, const int32_t* graph,
                            const float* erosivity, const float* uplift, const int32_t* stop, int64_t B, int64_t H,
                            int64_t W, int edge, const float* scales, int64_t n_scales, double dt, void* stream) {
  return downstream_run("stream_power_batch", kPower, DownOut{out, out64},
                        DownPlanes{graph, stop, height, erosivity, uplift, dt}, B, H, W, edge, scales, n_scales, stream);
}

int soil_stream_power_deposit(float* out, double* out64, float* flux, double* residual, const float* height,
                              const int32_t* graph, const float* erosivity, const float* deposition,
                              const float* uplift, int64_t H, int64_t W, int edge, const float scale[2], double dt,
                              int iters, void* stream) {
  return deposit_run("stream_power_deposit", t_dep_info, StepOut{out, out64, flux, residual},
                     DnPlanes{{graph, height, erosivity, uplift, deposition, dt}, 1.0, 0.0}, iters, 1, H, W, edge, scale,
                     1, stream);
}

int soil_stream_power_deposit_batch(float* out, double* out64, float* flux, double* residual, const float* height,
                                    const int32_t* graph, const float* erosivity, const float* deposition,
                                    const float* uplift, int64_t B, int64_t H, int64_t W, int edge,
                                    const float* scales, int64_t n_scales, double dt, int iters, void* stream) {
  return deposit_run("stream_power_deposit_batch", t_dep_info, StepOut{out, out64, flux, residual},
                     DnPlanes{{graph, height, erosivity, uplift, deposition, dt}, 1.0, 0.0}, iters, B, H, W, edge, scales,
                     n_scales, stream);
}

int soil_stream_power_deposit_info(int64_t info[4]) {
  SOIL_REQUIRE(info, "stream_power_deposit_info: null info");
  info[0] = t_dep_info.launches, info[1] = t_dep_info.chunks, info[2] = t_dep_info.iters, info[3] = t_dep_info.bytes;
  return SOIL_OK;
}

int soil_stream_power_deposit_n(float* out, double* out64, float* flux, double* residual, const float* height,
                                const int32_t* graph, const float* erosivity, const float* deposition,
                                const float* uplift, int64_t H, int64_t W, int edge, const float scale[2], double dt,
                                double n, int iters, void* stream) {
  return deposit_run("stream_power_deposit_n", t_dn_info, StepOut{out, out64, flux, residual},
                     DnPlanes{{graph, height, erosivity, uplift, deposition, dt}, n, n - 1.0}, iters, 1, H, W, edge,
                     scale, 1, stream);
}

int soil_stream_power_deposit_n_batch(float* out, double* out64, float* flux, double* residual, const float* height,
                                      const int32_t* graph, const float* erosivity, const float* deposition,
                                      const float* uplift, int64_t B, int64_t H, int64_t W, int edge,
                                      const float* scales, int64_t n_scales, double dt, double n, int iters,
                                      void* stream) {
  return deposit_run("stream_power_deposit_n_batch", t_dn_info, StepOut{out, out64, flux, residual},
                     DnPlanes{{graph, height, erosivity, uplift, deposition, dt}, n, n - 1.0}, iters, B, H, W, edge,
                     scales, n_scales, stream);
}

int soil_stream_power_deposit_n_info(int64_t info[4]) {
  SOIL_REQUIRE(info, "stream_power_deposit_n_info: null info");
  info[0] = t_dn_info.launches, info[1] = t_dn_info.chunks, info[2] = t_dn_info.iters, info[3] = t_dn_info.bytes;
  return SOIL_OK;
}

int soil_stream_power_n(float* out, double* out64, double* residual, const float* height, const int32_t* graph,
                        const float* erosivity, const float* uplift, const int32_t* stop, int64_t H, int64_t W,
                        int edge, const float scale[2], double dt, double n, int iters, void* stream) {
  return power_n_run("stream_power_n", StepOut{out, out64, nullptr, residual},
                     PnPlanes{graph, stop, height, erosivity, uplift, dt, n, n - 1.0}, iters, 1, H, W, edge, scale, 1,
                     stream);
}

int soil_stream_power_n_batch(float* out, double* out64, double* residual, const float* height, const int32_t* graph,
                              const float* erosivity, const float* uplift, const int32_t* stop, int64_t B, int64_t H,
                              int64_t W, int edge, const float* scales, int64_t n_scales, double dt, double n,
                              int iters, void* stream) {
  return power_n_run("stream_power_n_batch", StepOut{out, out64, nullptr, residual},
                     PnPlanes{graph, stop, height, erosivity, uplift, dt, n, n - 1.0}, iters, B, H, W, edge, scales,
                     n_scales, stream);
}

int soil_stream_power_n_info(int64_t info[4]) {
  SOIL_REQUIRE(info, "stream_power_n_info: null info");
  info[0] = t_pn_info.launches, info[1] = t_pn_info.chunks, info[2] = t_pn_info.iters, info[3] = t_pn_info.bytes;
  return SOIL_OK;
}

int soil_downstream_info(int64_t info[4]) {
  SOIL_REQUIRE(info, "downstream_info: null info");
  t_down_info.store(info);
  return SOIL_OK;
}

}  // extern "C"
