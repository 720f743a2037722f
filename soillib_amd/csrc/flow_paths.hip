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
#include <algorithm>
#include <cstdlib>

#include "common.hpp"
#include "flow_paths.hpp"  // the records' pointer word, rec_at, path_append, PathScale: shared with downstream.hip

namespace soil {

// The edge rule of soil_hip.h for cell (x, y) of a (H, W) model with graph entry g: the record of the cell, `first`
// the model's first cell in the stacked array.  g is an edge iff it is the index of one of the cell's K neighbours
// inside the model: of the three row steps rd the one (if any) whose column step cd = g - n - rd W lies in -1 .. 1
// with the neighbour in the grid — at most one does, the decomposition of an index into row and column being
// unique —, so no division is needed, and any other int32 is no edge.  64-bit differences: g may be INT32_MIN.
template <int K>
__device__ __forceinline__ uint4 path_record(int32_t g, bool stop, int64_t x, int64_t y, int64_t H, int64_t W,
                                             uint32_t first) {
  const int64_t n = x * W + y;
  const int64_t d = static_cast<int64_t>(g) - n;
  uint4 rec = make_uint4((first + static_cast<uint32_t>(n)) | kFinal, 0u, 0u, 0u);
  if (stop) return rec;
#pragma unroll
  for (int rd = -1; rd <= 1; ++rd) {
    const int64_t cd = d - rd * W;
    const bool ok = cd >= -1 && cd <= 1 && (rd != 0 || cd != 0) && x + rd >= 0 && x + rd < H && y + cd >= 0 &&
                    y + cd < W && (K == 8 || rd == 0 || cd == 0);
    if (ok) {
      const bool diag = rd != 0 && cd != 0;
      rec = make_uint4(first + static_cast<uint32_t>(g), (rd != 0 && !diag) ? 1u : 0u, (rd == 0) ? 1u : 0u,
                       diag ? 1u : 0u);
    }
  }
  return rec;
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

// A dense round: a grid of a few work-groups per CU strides over the cells.  A cell that holds the bit is copied
// across (a dense round keeps no word that says "final in both buffers"; the listed rounds do not come back to such
// a cell at all), so when a dense round writes no new record every record is final in both buffers and the rounds
// after it have nothing to do.  `list_out`: the dense round in front of the listed rounds writes down its pending
// cells, work-group b into segment b (`seg` entries: its share of the cells).
template <typename IDX>
__global__ void __launch_bounds__(kPBlock)
    k_paths_round(uint4* __restrict__ out, const uint4* __restrict__ in, int64_t elem64, int* __restrict__ flags,
                  int round, uint32_t* __restrict__ list_out, uint32_t* __restrict__ fill_out, uint32_t seg) {
  const IDX elem = static_cast<IDX>(elem64);
  __shared__ uint32_t s_fill;
  // the word round + 2 will read is cleared either way (k_rake_compress)
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
  // (the trip count is uniform over the work-group but for the last trip; the ballots of path_append are per wave)
  for (IDX n = static_cast<IDX>(blockIdx.x) * kPBlock + threadIdx.x; n < elem;
       n += static_cast<IDX>(gridDim.x) * kPBlock) {
    const bool again = path_cell<IDX>(out, in, n);
    pending = pending || again;
    if (list_out) path_append<IDX>(again, n, segment, &s_fill);
  }
  if (__any(pending) && (threadIdx.x & 63) == 0) flags[(round + 1) % 3] = 1;
  if (list_out) {
    __syncthreads();
    if (threadIdx.x == 0) fill_out[blockIdx.x] = s_fill;
  }
}

// A round over the lists: work-group b reads segment b of the lists the round before made and makes segment b of
// the next; a work-group whose segment is empty returns at once.
template <typename IDX>
__global__ void __launch_bounds__(kPBlock)
    k_paths_list(uint4* __restrict__ out, const uint4* __restrict__ in, const uint32_t* __restrict__ list_in,
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
    const bool again = path_cell<IDX>(out, in, n);
    path_append<IDX>(again, n, segment, &s_fill);
  }
  __syncthreads();
  if (threadIdx.x == 0) fill_out[blockIdx.x] = s_fill;
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

// Models per chunk: as many whole models as keep the rounds on 32-bit offsets (16 bytes a cell under 4 GiB) and one
// init launch (grid.z), at least one.  SOIL_FLOW_BATCH_CELLS lowers the cap on the cells of a chunk, as it does for
// soil_accumulate_batch (read per call).
static int64_t paths_chunk_models(int64_t cells_per_model) {
  const char* const e = std::getenv("SOIL_FLOW_BATCH_CELLS");
  const int64_t cap_env = e ? std::atoll(e) : 0ll;
  int64_t cap = static_cast<int64_t>((1ull << 32) / sizeof(uint4)) - 1;
  if (cap_env > 0 && cap_env < cap) cap = cap_env;
  const int64_t per = cap / cells_per_model;
  return per < 1 ? 1 : (per > kPathsMaxGridZ ? kPathsMaxGridZ : per);
}

// What the last call of either entry on this host thread did (soil_flow_paths_info): the tests hold the chunking,
// the choice of the init form and of the offsets to it.
struct PathsInfo {
  int64_t chunks, vec_chunks, idx64_chunks, rounds;
};
static thread_local PathsInfo t_paths_info{0, 0, 0, 0};

struct PathsWork {  // the scratch of a chunk, carved out of the call's block
  uint4* rec[2];
  uint32_t* list[2];
  uint32_t* fill[2];
  int* flags;
};
struct PathsLayout {
  unsigned groups;
  size_t seg, b_rec, b_list, b_fill;
  size_t bytes() const { return 2 * b_rec + 2 * b_list + 2 * b_fill + 256; }
};
static PathsLayout paths_layout(int64_t elem) {
  static const unsigned groups_env = [] {
    const char* e = std::getenv("SOIL_PATHS_GROUPS");
    return e && std::atoi(e) > 0 ? static_cast<unsigned>(std::atoi(e)) : 256u * 32u;
  }();
  PathsLayout L;
  L.groups = std::min(blocks_for(elem, kPBlock), groups_env);
  // a work-group's segment of the lists: its share of the cells, in whole work-groups' worth of entries
  L.seg = ((static_cast<size_t>(elem) + L.groups - 1) / L.groups + 255) / 256 * 256;
  L.b_rec = align256(sizeof(uint4) * static_cast<size_t>(elem));
  L.b_list = align256(sizeof(uint32_t) * L.seg * L.groups);
  L.b_fill = align256(sizeof(uint32_t) * L.groups);
  return L;
}

// One chunk of `models` models of (H, W), stream-ordered: init, the rounds of ONE model, final.
template <int K>
static int paths_chunk(int32_t* terminal, int32_t* steps, float* length, const int32_t* graph, const int32_t* stop,
                int64_t models, int64_t H, int64_t W, const PathScales& scales, char* scratch, hipStream_t st) {
  const int64_t hw = H * W, elem = models * hw;
  const PathsLayout L = paths_layout(elem);
  PathsWork w;
  char* p = scratch;
  w.rec[0] = reinterpret_cast<uint4*>(p), w.rec[1] = reinterpret_cast<uint4*>(p + L.b_rec), p += 2 * L.b_rec;
  w.list[0] = reinterpret_cast<uint32_t*>(p), w.list[1] = reinterpret_cast<uint32_t*>(p + L.b_list), p += 2 * L.b_list;
  w.fill[0] = reinterpret_cast<uint32_t*>(p), w.fill[1] = reinterpret_cast<uint32_t*>(p + L.b_fill), p += 2 * L.b_fill;
  w.flags = reinterpret_cast<int*>(p);

  const unsigned z = static_cast<unsigned>(models);
  const bool vec = W % 4 == 0 &&
                   ((reinterpret_cast<uintptr_t>(graph) | reinterpret_cast<uintptr_t>(stop)) & 15) == 0;
  if (vec) {
    dim3 grid = grid_rows(H, W / 4, kPBlock);
    grid.z = z;
    k_paths_init<K, true><<<grid, kPBlock, 0, st>>>(w.rec[0], graph, stop, H, W, w.flags);
  } else {
    dim3 grid = grid_rows(H, W, kPBlock);
    grid.z = z;
    k_paths_init<K, false><<<grid, kPBlock, 0, st>>>(w.rec[0], graph, stop, H, W, w.flags);
  }
  SOIL_LAUNCH_CHECK();
  t_paths_info.chunks += 1;
  t_paths_info.vec_chunks += vec ? 1 : 0;

  // Rounds from `list_from` on run over the lists; the dense round in front of them makes the first lists.
  // SOIL_PATHS_LIST_FROM: that round (0, or beyond the last round: dense rounds throughout), read per call.
  const char* const e = std::getenv("SOIL_PATHS_LIST_FROM");
  const int list_from_env = e ? std::atoi(e) : 1;
  const int rounds = ceil_log2(hw);
  const int list_from = (list_from_env >= 1 && list_from_env < rounds) ? list_from_env : rounds;
  // SOIL_PATHS_IDX64=1 (read per call): 64-bit offsets whatever the size — the form a single model of 2^28 cells or
  // more takes, reached by the tests at small shapes through it.
  const char* const e64 = std::getenv("SOIL_PATHS_IDX64");
  const bool idx32 = static_cast<uint64_t>(elem) * sizeof(uint4) < (1ull << 32) && !(e64 && std::atoi(e64) == 1);
  t_paths_info.idx64_chunks += idx32 ? 0 : 1;
  t_paths_info.rounds = rounds;
  const uint32_t seg32 = static_cast<uint32_t>(L.seg);
  for (int r = 0; r < rounds; ++r) {
    uint4* const o = w.rec[(r + 1) & 1];
    const uint4* const in = w.rec[r & 1];
    if (r >= list_from) {
      const uint32_t *li = w.list[r & 1], *fi = w.fill[r & 1];
      uint32_t *lo = w.list[(r + 1) & 1], *fo = w.fill[(r + 1) & 1];
      if (idx32) k_paths_list<uint32_t><<<L.groups, kPBlock, 0, st>>>(o, in, li, fi, lo, fo, seg32);
      else k_paths_list<int64_t><<<L.groups, kPBlock, 0, st>>>(o, in, li, fi, lo, fo, seg32);
      continue;
    }
    // (list_from == rounds: dense rounds throughout, and the last of them has nobody to make lists for)
    uint32_t* const lo = list_from < rounds && r + 1 == list_from ? w.list[(r + 1) & 1] : nullptr;
    uint32_t* const fo = w.fill[(r + 1) & 1];
    if (idx32) k_paths_round<uint32_t><<<L.groups, kPBlock, 0, st>>>(o, in, elem, w.flags, r, lo, fo, seg32);
    else k_paths_round<int64_t><<<L.groups, kPBlock, 0, st>>>(o, in, elem, w.flags, r, lo, fo, seg32);
  }
  SOIL_LAUNCH_CHECK();

  const int64_t per_model = (hw + kPBlock - 1) / kPBlock;
  // (a few thousand work-groups in all stride over the cells; a batch of many small models has one per model)
  const int64_t want = (8192 + models - 1) / models;
  dim3 grid(static_cast<unsigned>(per_model < want ? per_model : want), 1, z);
  k_paths_final<<<grid, kPBlock, 0, st>>>(terminal, steps, length, w.rec[rounds & 1], hw, scales);
  SOIL_LAUNCH_CHECK();
  return SOIL_OK;
}

// What both entries refuse before any device work, under the entry's name
static int check_flow_paths(const char* what, const void* terminal, const void* steps, const void* length,
                     const void* graph, const void* scale, int64_t B, int64_t H, int64_t W, int edge,
                     int64_t n_scales) {
  const std::string w(what);
  SOIL_REQUIRE(graph, w + ": null graph");
  SOIL_REQUIRE(terminal || steps || length, w + ": no output asked for (terminal, steps and length are all null)");
  SOIL_REQUIRE(!length || scale, w + ": length needs a scale");
  SOIL_REQUIRE(B >= 1, w + ": B must be >= 1");
  SOIL_REQUIRE(H >= 1 && W >= 1, w + ": empty grid");
  SOIL_REQUIRE(H <= INT32_MAX / W, w + ": a model must have 1..2^31-1 cells (int32 graph)");
  SOIL_REQUIRE(n_scales == 1 || n_scales == B, w + ": n_scales must be 1 or B");
  SOIL_REQUIRE(edge == SOIL_D4 || edge == SOIL_D8, w + ": invalid edge enumerator");
  return SOIL_OK;
}

// Chunks of whole models, one after the other on `st` through one block of workspace slot WS_FLOW_PATHS (the
// entries' own: they return with their work in flight): the B scale records first, then the chunk's scratch.
static int flow_paths_run(int32_t* terminal, int32_t* steps, float* length, const int32_t* graph, const int32_t* stop,
                   int64_t B, int64_t H, int64_t W, int edge, const float* scales, int64_t n_scales,
                   hipStream_t st) {
  const int64_t hw = H * W, per = paths_chunk_models(hw);
  t_paths_info = PathsInfo{0, 0, 0, 0};
  const bool per_model = length && n_scales > 1;
  const size_t b_scales = per_model ? align256(sizeof(PathScale) * static_cast<size_t>(B)) : 0;
  const int64_t first_chunk = B < per ? B : per;
  void* base = nullptr;
  if (int rc = workspace_get(WS_FLOW_PATHS, b_scales + paths_layout(first_chunk * hw).bytes(), &base); rc != SOIL_OK)
    return rc;
  PathScales sc{nullptr, PathScale{0.0, 0.0, 0.0}};
  if (length) sc.one = path_scale(scales);
  if (per_model) {
    std::vector<PathScale> host(static_cast<size_t>(B));
    for (int64_t b = 0; b < B; ++b) host[static_cast<size_t>(b)] = path_scale(scales + 2 * b);
    if (int rc = batch_upload(base, host.data(), sizeof(PathScale) * host.size(), st); rc != SOIL_OK) return rc;
    sc.per_model = static_cast<const PathScale*>(base);
  }
  char* const scratch = static_cast<char*>(base) + b_scales;
  for (int64_t b0 = 0; b0 < B; b0 += per) {
    const int64_t nb = B - b0 < per ? B - b0 : per, at = b0 * hw;
    PathScales s = sc;
    if (s.per_model) s.per_model += b0;
    auto go = edge == SOIL_D4 ? paths_chunk<4> : paths_chunk<8>;
    if (int rc = go(terminal ? terminal + at : nullptr, steps ? steps + at : nullptr, length ? length + at : nullptr,
                    graph + at, stop ? stop + at : nullptr, nb, H, W, s, scratch, st);
        rc != SOIL_OK)
      return rc;
  }
  return SOIL_OK;
}

}  // namespace soil

using namespace soil;

extern "C" {

int soil_flow_paths(int32_t* terminal, int32_t* steps, float* length, const int32_t* graph, const int32_t* stop,
                    int64_t H, int64_t W, int edge, const float scale[2], void* stream) {
  if (int rc = check_flow_paths("flow_paths", terminal, steps, length, graph, scale, 1, H, W, edge, 1); rc != SOIL_OK)
    return rc;
  SOIL_DEVICE();
  return flow_paths_run(terminal, steps, length, graph, stop, 1, H, W, edge, scale, 1, as_stream(stream));
}

int soil_flow_paths_batch(int32_t* terminal, int32_t* steps, float* length, const int32_t* graph,
                          const int32_t* stop, int64_t B, int64_t H, int64_t W, int edge, const float* scales,
                          int64_t n_scales, void* stream) {
  if (int rc = check_flow_paths("flow_paths_batch", terminal, steps, length, graph, scales, B, H, W, edge, n_scales);
      rc != SOIL_OK)
    return rc;
  SOIL_DEVICE();
  return flow_paths_run(terminal, steps, length, graph, stop, B, H, W, edge, scales, n_scales, as_stream(stream));
}

int soil_flow_paths_info(int64_t info[4]) {
  SOIL_REQUIRE(info, "flow_paths_info: null info");
  info[0] = t_paths_info.chunks, info[1] = t_paths_info.vec_chunks;
  info[2] = t_paths_info.idx64_chunks, info[3] = t_paths_info.rounds;
  return SOIL_OK;
}

}  // extern "C"
