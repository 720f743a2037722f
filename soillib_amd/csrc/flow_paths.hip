// flow_paths.hip — the downstream half of a drainage analysis: where every cell of a receiver graph drains to, how
// many edges away that is and how long the way is (soil_flow_paths / soil_flow_paths_batch, soil_hip.h).  The
// reference names these — `upstream` and `distance` sit commented out in its model.cpp — and implements neither.
//
// Pointer doubling over 16-byte records {ptr, n_row, n_col, n_diag}, one dwordx4 load or store per record
// (tools/microbench/gather16.hip: the gather shape of a round):
//
//   init    one record per cell from the edge rule and the stop plane.  A terminal points to itself with zero
//           counts and carries kFinal; any other cell points to its receiver with one count set.
//   rounds  rec'[n] = {rec[p].ptr, counts[n] + counts[p]}, p = rec[n].ptr, ceil(log2(H W)) times, between two
//           buffers (`in` is only read, a cell's record in `out` is written by that cell alone: no access of a round
//           can meet a store to the same record).
//   final   terminal / steps / length from the records; -1 / -1 / NaN where the pointer is no terminal.
//
// kFinal, bit 31 of `ptr` (a cell index is below 2^31): "this pointer is a terminal".  Only init sets it, on the
// terminals themselves; a round copies rec[p].ptr with the bit, so it reaches cell n in the round that brings n's
// pointer onto a terminal's record.  Once set, the record is the cell's last: the terminal's record is a fixed point
// with zero counts.  The final pass therefore needs no gather, and a cell on a cycle, or one that drains into a
// cycle, never gets the bit — its pointer may well come back to the cell itself (a two-cell cycle after one round),
// which is why "points to itself" alone does not say terminal.
//
// Round count.  A record without the bit has walked exactly 2^k edges after k rounds (init: one), and one with a
// path of L edges to its terminal gets the bit in the first round with 2^k > L.  L <= H W - 1, so
// floor(log2(H W - 1)) + 1 = ceil(log2(H W)) rounds resolve every cell of an acyclic graph, and one round less does
// not resolve the cell at the head of a chain through every cell.  The counts of a record without the bit sum to
// 2^k <= 2^31: the unsigned words never wrap; the final pass overwrites them anyway.
//
// Work set, as in k_rake_compress / k_rake_list (graph.hip).  A cell that finds the bit in `in` copies its record to
// `out` — both buffers hold it from then on (rake_cell's `was_final`) — and leaves the work set.  Dense rounds stride
// over every cell and return at once when a device-side word says that the round before wrote no new record; from
// round SOIL_PATHS_LIST_FROM on (default 1: the dense round 0 makes the first lists) a round runs over per-work-group
// lists of the cells that do not hold the bit in both buffers yet.  Nothing looks at the host in between.
//
// A batch is ONE stacked array of records with pointers into that array: init takes its model from grid.z, as the
// donor pass does, and adds the model's first cell to the receiver; the rounds never look at H, W or the model.
#include "common.hpp"
#include "flow_paths.hpp"  // the round bodies, the edge rule and the host driver: shared with downstream.hip

namespace soil {

// The record of cell (x, y) of a (H, W) model with graph entry g under the edge rule (edge_kind), `first` the model's
// first cell in the stacked array.
template <int K>
__device__ __forceinline__ uint4 path_record(int32_t g, bool stop, int64_t x, int64_t y, int64_t H, int64_t W,
                                             uint32_t first) {
  const uint4 self = make_uint4((first + static_cast<uint32_t>(x * W + y)) | kFinal, 0u, 0u, 0u);
  if (stop) return self;
  const int kind = edge_kind<K>(g, x, y, H, W);
  return kind < 0 ? self
                  : make_uint4(first + static_cast<uint32_t>(g), kind == 0 ? 1u : 0u, kind == 1 ? 1u : 0u,
                               kind == 2 ? 1u : 0u);
}

// Init: threads along the row, a work-group walks a band of rows (SOIL_ROW_LOOP), grid.z is the model.  VEC: four
// cells per thread, the graph and the stop plane as 16-byte loads (W a multiple of four, the planes 16-byte aligned).
template <int K, bool VEC>
__global__ void __launch_bounds__(kPBlock)
    k_paths_init(uint4* __restrict__ rec, const int32_t* __restrict__ graph, const int32_t* __restrict__ stop,
                 int64_t H, int64_t W, int* __restrict__ flags) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x < kPathFlags)
    flags[threadIdx.x] = threadIdx.x == 0 ? 1 : 0;
  const int64_t y = (static_cast<int64_t>(blockIdx.x) * kPBlock + threadIdx.x) * (VEC ? 4 : 1);
  if (y >= W) return;
  const int64_t first64 = static_cast<int64_t>(blockIdx.z) * H * W;
  const uint32_t first = static_cast<uint32_t>(first64);
  rec += first64, graph += first64;
  if (stop) stop += first64;
  SOIL_ROW_LOOP(x, H) {
    const int64_t n = x * W + y;
    if constexpr (VEC) {
      const int4 g = *reinterpret_cast<const int4*>(graph + n);
      const int4 s = stop ? *reinterpret_cast<const int4*>(stop + n) : make_int4(0, 0, 0, 0);
      rec[n + 0] = path_record<K>(g.x, s.x != 0, x, y + 0, H, W, first);
      rec[n + 1] = path_record<K>(g.y, s.y != 0, x, y + 1, H, W, first);
      rec[n + 2] = path_record<K>(g.z, s.z != 0, x, y + 2, H, W, first);
      rec[n + 3] = path_record<K>(g.w, s.w != 0, x, y + 3, H, W, first);
    } else {
      rec[n] = path_record<K>(graph[n], stop ? stop[n] != 0 : false, x, y, H, W, first);
    }
  }
}

// One cell of one round, `in` -> `out`.  Returns whether the cell has to be looked at again: it wrote a new record
// (if that one carries the bit, the other buffer still holds the stale one).
template <typename IDX>
__device__ __forceinline__ bool path_cell(uint4* __restrict__ out, const uint4* __restrict__ in, IDX n) {
  const uint4 r = *rec_at<IDX>(in, n);
  if (r.x & kFinal) {  // final in `in`: both buffers hold it from here on
    *rec_at<IDX>(out, n) = r;
    return false;
  }
  const uint4 q = *rec_at<IDX>(in, static_cast<IDX>(r.x));
  *rec_at<IDX>(out, n) = make_uint4(q.x, r.y + q.y, r.z + q.z, r.w + q.w);
  return true;
}

// The dense and the listed round (flow_paths.hpp ptr_round, ptr_list) over path_cell
template <typename IDX>
__global__ void __launch_bounds__(kPBlock)
    k_paths_round(uint4* __restrict__ out, const uint4* __restrict__ in, int64_t elem64, int* __restrict__ flags,
                  int round, uint32_t* __restrict__ list_out, uint32_t* __restrict__ fill_out, uint32_t seg) {
  ptr_round<IDX>([=](IDX n) { return path_cell<IDX>(out, in, n); }, elem64, flags, round, list_out, fill_out, seg);
}
template <typename IDX>
__global__ void __launch_bounds__(kPBlock)
    k_paths_list(uint4* __restrict__ out, const uint4* __restrict__ in, const uint32_t* __restrict__ list_in,
                 const uint32_t* __restrict__ fill_in, uint32_t* __restrict__ list_out,
                 uint32_t* __restrict__ fill_out, uint32_t seg) {
  ptr_list<IDX>([=](IDX n) { return path_cell<IDX>(out, in, n); }, list_in, fill_in, list_out, fill_out, seg);
}

// Final: a cell per thread, grid.z is the model.  length = (float)((n_row sx + n_col sy) + n_diag dd) in fp64, one
// rounding per operation, as soil_hip.h states it.
__global__ void __launch_bounds__(kPBlock)
    k_paths_final(int32_t* __restrict__ terminal, int32_t* __restrict__ steps, float* __restrict__ length,
                  const uint4* __restrict__ rec, int64_t cells, PathScales scales) {
  const int64_t first64 = static_cast<int64_t>(blockIdx.z) * cells;
  const uint32_t first = static_cast<uint32_t>(first64);
  PathScale s = scales.one;
  if (length && scales.per_model) s = scales.per_model[blockIdx.z];
  for (int64_t n = static_cast<int64_t>(blockIdx.x) * kPBlock + threadIdx.x; n < cells;
       n += static_cast<int64_t>(gridDim.x) * kPBlock) {
    const uint4 r = rec[first64 + n];
    const bool resolved = (r.x & kFinal) != 0;
    if (terminal) terminal[first64 + n] = resolved ? static_cast<int32_t>((r.x & ~kFinal) - first) : -1;
    if (steps) steps[first64 + n] = resolved ? static_cast<int32_t>(r.y + r.z + r.w) : -1;
    if (length) {
      const double rows = __dmul_rn(static_cast<double>(r.y), s.sx);
      const double cols = __dmul_rn(static_cast<double>(r.z), s.sy);
      const double diag = __dmul_rn(static_cast<double>(r.w), s.dd);
      const float len = __double2float_rn(__dadd_rn(__dadd_rn(rows, cols), diag));
      length[first64 + n] = resolved ? len : bits2f(0x7fc00000u);
    }
  }
}

static thread_local PtrInfo t_paths_info{0, 0, 0, 0};  // soil_flow_paths_info

// One chunk of `models` models (flow_paths.hpp ptr_chunk) with this file's launches
template <int K>
static int paths_chunk(int32_t* terminal, int32_t* steps, float* length, const int32_t* graph, const int32_t* stop,
                       int64_t models, int64_t H, int64_t W, const PathScales& scales, char* scratch, hipStream_t st) {
  auto init = [&](const PtrChunk& c) {
    const bool vec = ptr_vec_init(W, graph, stop);
    launch_vec(vec, k_paths_init<K, true>, k_paths_init<K, false>, ptr_init_grid(c, H, W, vec), st, c.rec[0], graph,
               stop, H, W, c.flags);
    return vec;
  };
  auto round = [&](const PtrChunk& c, const PtrRound& q) {
    ptr_launch_round(c, q, st, k_paths_list<uint32_t>, k_paths_list<int64_t>, k_paths_round<uint32_t>,
                     k_paths_round<int64_t>);
  };
  auto fin = [&](const PtrChunk&, dim3 grid, const uint4* rec) {
    k_paths_final<<<grid, kPBlock, 0, st>>>(terminal, steps, length, rec, H * W, scales);
  };
  return ptr_chunk(t_paths_info, models, H, W, 0, scratch, init, round, fin);
}

// What both entries refuse before any device work, under the entry's name
static int check_flow_paths(const char* what, const void* terminal, const void* steps, const void* length,
                            const void* graph, const void* scale, int64_t B, int64_t H, int64_t W, int edge,
                            int64_t n_scales) {
  const std::string w(what);
  SOIL_REQUIRE(graph, w + ": null graph");
  SOIL_REQUIRE(terminal || steps || length, w + ": no output asked for (terminal, steps and length are all null)");
  SOIL_REQUIRE(!length || scale, w + ": length needs a scale");
  return check_grid_batch(w, B, H, W, edge, n_scales);
}

// A call, under the entry's name, through workspace slot WS_FLOW_PATHS (flow_paths.hpp ptr_run); the scales are read
// only for `length`
static int flow_paths_run(const char* what, int32_t* terminal, int32_t* steps, float* length, const int32_t* graph,
                          const int32_t* stop, int64_t B, int64_t H, int64_t W, int edge, const float* scales,
                          int64_t n_scales, void* stream) {
  if (int rc = check_flow_paths(what, terminal, steps, length, graph, scales, B, H, W, edge, n_scales); rc != SOIL_OK)
    return rc;
  SOIL_DEVICE();
  const hipStream_t st = as_stream(stream);
  auto go = edge == SOIL_D4 ? paths_chunk<4> : paths_chunk<8>;
  return ptr_run(WS_FLOW_PATHS, t_paths_info, B, H, W, 0, length ? scales : nullptr, n_scales,
                 PathScale{0.0, 0.0, 0.0}, st, [&](int64_t b0, int64_t nb, const PathScales& s, char* scratch) {
                   const int64_t off = b0 * H * W;
                   return go(at(terminal, off), at(steps, off), at(length, off), graph + off, at(stop, off), nb, H, W,
                             s, scratch, st);
                 });
}

}  // namespace soil

using namespace soil;

extern "C" {

int soil_flow_paths(int32_t* terminal, int32_t* steps, float* length, const int32_t* graph, const int32_t* stop,
                    int64_t H, int64_t W, int edge, const float scale[2], void* stream) {
  return flow_paths_run("flow_paths", terminal, steps, length, graph, stop, 1, H, W, edge, scale, 1, stream);
}

int soil_flow_paths_batch(int32_t* terminal, int32_t* steps, float* length, const int32_t* graph,
                          const int32_t* stop, int64_t B, int64_t H, int64_t W, int edge, const float* scales,
                          int64_t n_scales, void* stream) {
  return flow_paths_run("flow_paths_batch", terminal, steps, length, graph, stop, B, H, W, edge, scales, n_scales,
                        stream);
}

int soil_flow_paths_info(int64_t info[4]) {
  SOIL_REQUIRE(info, "flow_paths_info: null info");
  t_paths_info.store(info);
  return SOIL_OK;
}

}  // extern "C"
