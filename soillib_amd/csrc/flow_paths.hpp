// flow_paths.hpp — the pointer-doubling engine along a receiver graph, once: flow_paths.hip (terminal, steps, length)
// and downstream.hip (the linear recurrence x[n] = a L + b x[r(n)]) run it over 16-byte records whose first word is
// the pointer with kFinal in bit 31; upstream.hip (minima and maxima UP the graph) runs it over 4-byte records, the
// pointer alone, beside one plane of 8 bytes a cell (PtrSizes).  Here are
//
//   device  rec_at, the edge rule (edge_kind), the append to a work-group's list (path_append) and the bodies of the
//           dense and the listed round (ptr_round, ptr_list) over a per-cell operation `bool cell(IDX n)`: "one round
//           for cell n, in -> out; true where it wrote a new record".  Each file's __global__ round kernels are one
//           statement: the body over a lambda around its path_cell / down_cell.
//   host    models per chunk, the layout and carving of a chunk's scratch (ptr_carve), the round plan (ptr_rounds), the
//           chunk (init, rounds, final) and the loop over the chunks of a call (ptr_chunk, ptr_run), the call's info
//           record.  stream_order.hip runs the rounds once per level between passes of its own: it takes ptr_carve,
//           ptr_rounds and ptr_run and leaves ptr_chunk.  Each file
//           hands in its launches as callables and keeps its workspace slot and info instance.  The shape refusals,
//           the chunk-size rule and the knobs read per call are flow_host.hpp's.
//
// The records' other words, the per-cell operation, the init and the final kernels are each file's own.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "flow_host.hpp"

namespace soil {

constexpr int kPBlock = 256;
constexpr uint32_t kFinal = 0x80000000u;
constexpr int64_t kPathsMaxGridZ = 65535;  // models per init / final launch, and so per chunk

// A record at a 32-bit BYTE offset from a uniform base where the chunk's records are under 4 GiB (a scalar base and
// one offset register per lane, graph.hip word_at), at a 64-bit index otherwise.
template <typename IDX>
__device__ __forceinline__ uint4* rec_at(uint4* base, IDX n) {
  if constexpr (sizeof(IDX) == 4)
    return reinterpret_cast<uint4*>(reinterpret_cast<char*>(base) + static_cast<uint32_t>(n * 16u));
  else
    return base + n;
}
template <typename IDX>
__device__ __forceinline__ const uint4* rec_at(const uint4* base, IDX n) {
  if constexpr (sizeof(IDX) == 4)
    return reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(base) + static_cast<uint32_t>(n * 16u));
  else
    return base + n;
}

// The edge rule of soil_hip.h for cell (x, y) of a (H, W) model with graph entry g: the kind of the edge, 0 a row
// step, 1 a column step, 2 a diagonal, or -1 where g is no edge.  g is an edge iff it is the index of one of the
// cell's K neighbours inside the model: of the three row steps rd the one (if any) whose column step
// cd = g - n - rd W lies in -1 .. 1 with the neighbour in the grid — at most one does, the decomposition of an index
// into row and column being unique —, so no division is needed, and any other int32 is no edge.  64-bit differences:
// g may be INT32_MIN.
template <int K>
__device__ __forceinline__ int edge_kind(int32_t g, int64_t x, int64_t y, int64_t H, int64_t W) {
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

// Control words of the dense rounds (graph.hip kRakeFlags): flags[round % 3] = "work left"; init sets {1, 0, 0}
constexpr int kPathFlags = 4;

// graph.hip rake_append: the entries of a wave side by side in its work-group's segment, one LDS atomic per wave.
// The ballot is per wave: every lane of a wave must come here the same number of times.
template <typename IDX>
__device__ __forceinline__ void path_append(bool again, IDX n, uint32_t* __restrict__ segment, uint32_t* s_fill) {
  const uint64_t m = __ballot(again);
  if (m == 0) return;
  const int lane = static_cast<int>(threadIdx.x & 63u), leader = __ffsll(static_cast<long long>(m)) - 1;
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(s_fill, static_cast<uint32_t>(__popcll(m)));
  base = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(base), leader));
  if (again) segment[base + static_cast<uint32_t>(__popcll(m & ((1ull << lane) - 1ull)))] = static_cast<uint32_t>(n);
}

// A dense round: a grid of a few work-groups per CU strides over the cells.  A cell that holds the bit is copied
// across (a dense round keeps no word that says "final in both buffers"; the listed rounds do not come back to such
// a cell at all), so when a dense round writes no new record every record is final in both buffers and the rounds
// after it have nothing to do: they return at once on flags[round % 3].  `list_out`: the dense round in front of the
// listed rounds writes down its pending cells, work-group b into segment b (`seg` entries: its share of the cells).
template <typename IDX, typename Cell>
__device__ __forceinline__ void ptr_round(Cell cell, int64_t elem64, int* __restrict__ flags, int round,
                                          uint32_t* __restrict__ list_out, uint32_t* __restrict__ fill_out,
                                          uint32_t seg) {
  const IDX elem = static_cast<IDX>(elem64);
  __shared__ uint32_t s_fill;
  // the word round + 2 will read is cleared either way: a round that returns at once must not leave its
  // predecessor's "work left" standing for the round three launches on (k_rake_compress)
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
    const bool again = cell(n);
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
template <typename IDX, typename Cell>
__device__ __forceinline__ void ptr_list(Cell cell, const uint32_t* __restrict__ list_in,
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
    const bool again = cell(n);
    path_append<IDX>(again, n, segment, &s_fill);
  }
  __syncthreads();
  if (threadIdx.x == 0) fill_out[blockIdx.x] = s_fill;
}

// The scale of a model as the kernels read it: the floats widened, and dd = sqrt(sx sx + sy sy) made on the host
struct PathScale {
  double sx, sy, dd;
};
struct PathScales {
  const PathScale* per_model;  // null: `one` for every model
  PathScale one;
};

inline PathScale path_scale(const float pair[2]) {
  const double sx = static_cast<double>(pair[0]), sy = static_cast<double>(pair[1]);
  return PathScale{sx, sy, std::sqrt(sx * sx + sy * sy)};  // (the squares of two floats are exact in fp64)
}

inline int ceil_log2(int64_t v) {  // ceil(log2(v)), v >= 1, in integers
  int k = 0;
  while ((int64_t{1} << k) < v) ++k;
  return k;
}

// ---- the host driver ------------------------------------------------------------------------------------------

// What the last call of an entry on this host thread did (soil_flow_paths_info, soil_downstream_info; each file has
// its own thread_local instance): the tests hold the chunking, the choice of the init form and of the offsets to it.
struct PtrInfo {
  int64_t chunks, vec_chunks, idx64_chunks, rounds;
  void store(int64_t info[4]) const { info[0] = chunks, info[1] = vec_chunks, info[2] = idx64_chunks, info[3] = rounds; }
};

// Models per chunk: as many whole models as keep the rounds on 32-bit offsets (16 bytes a cell under 4 GiB; an extra
// plane's 8 bytes a cell lie below that anyway) and one init launch (grid.z), at least one.  SOIL_FLOW_BATCH_CELLS
// lowers the cap on the cells of a chunk, as it does for soil_accumulate_batch (flow_host.hpp chunk_models).
inline int64_t ptr_chunk_models(int64_t cells_per_model) {
  return chunk_models(static_cast<int64_t>((1ull << 32) / sizeof(uint4)) - 1, cells_per_model, kPathsMaxGridZ);
}

// What a file keeps per cell: two record buffers of `rec` bytes a cell (16 unless the file says otherwise; the chunk
// rule and the choice of the offsets stay those of 16-byte records either way, so that every file cuts a batch alike)
// and `planes` planes of `extra` bytes a cell (0: none).  A bare byte count is downstream.hip's B: two planes.
struct PtrSizes {
  size_t extra, rec;
  int planes;
  PtrSizes(size_t extra_bytes, size_t rec_bytes = sizeof(uint4), int n_planes = 2)
      : extra(extra_bytes), rec(rec_bytes), planes(n_planes) {}
};

// The scratch of a chunk of `elem` cells, in this order: two record buffers, the planes of `extra` bytes a cell
// (0: none; downstream.hip's B), two lists of `groups` segments, their fills, the control words.
struct PtrLayout {
  unsigned groups;
  size_t seg, b_rec, b_extra, b_list, b_fill;
  int planes;
  size_t bytes() const { return 2 * b_rec + planes * b_extra + 2 * b_list + 2 * b_fill + 256; }
};
inline PtrLayout ptr_layout(int64_t elem, PtrSizes sizes) {
  static const unsigned groups_env = [] {
    const char* e = std::getenv("SOIL_PATHS_GROUPS");
    return e && std::atoi(e) > 0 ? static_cast<unsigned>(std::atoi(e)) : 256u * 32u;
  }();
  PtrLayout L;
  L.groups = std::min(blocks_for(elem, kPBlock), groups_env);
  // a work-group's segment of the lists: its share of the cells, in whole work-groups' worth of entries
  L.seg = ((static_cast<size_t>(elem) + L.groups - 1) / L.groups + 255) / 256 * 256;
  L.b_rec = align256(sizes.rec * static_cast<size_t>(elem));
  L.b_extra = align256(sizes.extra * static_cast<size_t>(elem));
  L.planes = sizes.planes;
  L.b_list = align256(sizeof(uint32_t) * L.seg * L.groups);
  L.b_fill = align256(sizeof(uint32_t) * L.groups);
  return L;
}

// One chunk at work: its buffers carved out of the call's block, its launch shapes and its round plan
struct PtrChunk {
  uint4* rec[2];   // (records of PtrSizes::rec bytes: a file with other records than uint4 casts)
  void* extra[2];  // null without the plane
  uint32_t* list[2];
  uint32_t* fill[2];
  int* flags;
  unsigned groups;  // work-groups of a round
  uint32_t seg;
  int64_t elem;  // cells of the chunk
  unsigned z;    // its models: grid.z of init and final
  int rounds;
  bool idx32;
};
// One round, as the file's launch sees it: records (and planes) [r & 1] -> [(r + 1) & 1]; `list_in` null: dense
struct PtrRound {
  int r;
  const uint32_t *list_in, *fill_in;
  uint32_t *list_out, *fill_out;
};

// A plane from cell `off` on — a chunk's part of a batch's plane —, null for a plane that is not given
template <typename T>
T* at(T* p, int64_t off) { return p ? p + off : nullptr; }

// The init form: four cells per thread where W is a multiple of four and every plane (the OR of their addresses) is
// 16-byte aligned; the grid of either form
inline bool ptr_vec_init(int64_t W, uintptr_t planes) { return W % 4 == 0 && (planes & 15) == 0; }
template <typename... P>
bool ptr_vec_init(int64_t W, const P*... planes) { return ptr_vec_init(W, (reinterpret_cast<uintptr_t>(planes) | ...)); }
inline dim3 ptr_init_grid(const PtrChunk& c, int64_t H, int64_t W, bool vec) {
  dim3 grid = grid_rows(H, vec ? W / 4 : W, kPBlock);
  grid.z = c.z;
  return grid;
}
// An init-shaped kernel in its 16-byte form or its scalar one (two instantiations of one signature), same arguments
template <typename Kernel, typename... Args>
void launch_vec(bool vec, Kernel* k_vec, Kernel* k_scalar, dim3 grid, hipStream_t st, Args... args) {
  (vec ? k_vec : k_scalar)<<<grid, kPBlock, 0, st>>>(args...);
}

// One round of a chunk, dense or listed, on 32- or 64-bit offsets by the chunk: the file's four round kernels, and
// `planes`, what its kernels take between the two record buffers and the engine's own arguments (downstream.hip's B)
template <typename List, typename Round, typename... Planes>
void ptr_launch_round(const PtrChunk& c, const PtrRound& q, hipStream_t st, List* list32, List* list64, Round* round32,
                      Round* round64, Planes... planes) {
  uint4* const out = c.rec[(q.r + 1) & 1];
  const uint4* const in = c.rec[q.r & 1];
  if (q.list_in)
    (c.idx32 ? list32 : list64)<<<c.groups, kPBlock, 0, st>>>(out, in, planes..., q.list_in, q.fill_in, q.list_out,
                                                              q.fill_out, c.seg);
  else
    (c.idx32 ? round32 : round64)<<<c.groups, kPBlock, 0, st>>>(out, in, planes..., c.elem, c.flags, q.r, q.list_out,
                                                                q.fill_out, c.seg);
}

// The buffers of one chunk of `models` models of (H, W) carved out of `scratch` in ptr_layout's order, its launch
// shapes and its round count; a file with more than two planes finds plane k at extra[0] + k * ptr_layout().b_extra
inline PtrChunk ptr_carve(int64_t models, int64_t H, int64_t W, PtrSizes sizes, char* scratch) {
  const int64_t hw = H * W, elem = models * hw;
  const size_t extra = sizes.extra;
  const PtrLayout L = ptr_layout(elem, sizes);
  PtrChunk c;
  char* p = scratch;
  c.rec[0] = reinterpret_cast<uint4*>(p), c.rec[1] = reinterpret_cast<uint4*>(p + L.b_rec), p += 2 * L.b_rec;
  c.extra[0] = extra ? p : nullptr, c.extra[1] = extra && L.planes > 1 ? p + L.b_extra : nullptr;
  p += L.planes * L.b_extra;
  c.list[0] = reinterpret_cast<uint32_t*>(p), c.list[1] = reinterpret_cast<uint32_t*>(p + L.b_list), p += 2 * L.b_list;
  c.fill[0] = reinterpret_cast<uint32_t*>(p), c.fill[1] = reinterpret_cast<uint32_t*>(p + L.b_fill), p += 2 * L.b_fill;
  c.flags = reinterpret_cast<int*>(p);
  c.groups = L.groups, c.seg = static_cast<uint32_t>(L.seg), c.elem = elem, c.z = static_cast<unsigned>(models);
  c.rounds = ceil_log2(hw);
  // (64-bit offsets: the form a single model of 2^28 cells or more takes, or SOIL_PATHS_IDX64)
  c.idx32 = static_cast<uint64_t>(elem) * sizeof(uint4) < (1ull << 32) && !force_idx64();
  return c;
}

// The rounds of a chunk from records rec[0] (and flags {1, 0, 0}) on: rounds from `list_from` on run over the lists;
// the dense round in front of them makes the first lists.  SOIL_PATHS_LIST_FROM: that round (0, or beyond the last
// round: dense rounds throughout), read per call.
template <typename Round>
void ptr_rounds(const PtrChunk& c, Round round) {
  const char* const e = std::getenv("SOIL_PATHS_LIST_FROM");
  const int list_from_env = e ? std::atoi(e) : 1;
  const int list_from = (list_from_env >= 1 && list_from_env < c.rounds) ? list_from_env : c.rounds;
  for (int r = 0; r < c.rounds; ++r) {
    uint32_t* const fo = c.fill[(r + 1) & 1];
    if (r >= list_from)
      round(c, PtrRound{r, c.list[r & 1], c.fill[r & 1], c.list[(r + 1) & 1], fo});
    else  // (list_from == rounds: dense rounds throughout, and the last of them has nobody to make lists for)
      round(c, PtrRound{r, nullptr, nullptr, list_from < c.rounds && r + 1 == list_from ? c.list[(r + 1) & 1] : nullptr,
                        fo});
  }
}

// The grid of a final pass: a few thousand work-groups in all stride over the cells; a batch of many small models
// has one per model
inline dim3 ptr_final_grid(const PtrChunk& c, int64_t hw) {
  const int64_t per_model = (hw + kPBlock - 1) / kPBlock;
  const int64_t want = (8192 + static_cast<int64_t>(c.z) - 1) / static_cast<int64_t>(c.z);
  return dim3(static_cast<unsigned>(per_model < want ? per_model : want), 1, c.z);
}

// One chunk of `models` models of (H, W), stream-ordered: init, the rounds of ONE model, final.
//   init(chunk) -> bool       launches the file's init on rec[0] (extra[0], flags); whether it took the vector form
//   round(chunk, PtrRound)    launches the file's dense or listed round, 32- or 64-bit by chunk.idx32
//   final(chunk, grid, rec)   launches the file's final pass over `rec`
template <typename Init, typename Round, typename Final>
int ptr_chunk(PtrInfo& info, int64_t models, int64_t H, int64_t W, PtrSizes sizes, char* scratch, Init init,
              Round round, Final fin) {
  const PtrChunk c = ptr_carve(models, H, W, sizes, scratch);
  const bool vec = init(c);
  SOIL_LAUNCH_CHECK();
  info.chunks += 1;
  info.vec_chunks += vec ? 1 : 0;
  info.idx64_chunks += c.idx32 ? 0 : 1;
  info.rounds = c.rounds;
  ptr_rounds(c, round);
  SOIL_LAUNCH_CHECK();
  fin(c, ptr_final_grid(c, H * W), c.rec[c.rounds & 1]);
  SOIL_LAUNCH_CHECK();
  return SOIL_OK;
}

// A call: chunks of whole models, one after the other on `st` through one block of workspace `slot` (the entries'
// own: they return with their work in flight): the B scale records first (`scales` with n_scales > 1; null: `none`
// for every model), then the chunk's scratch.  chunk(b0, nb, scales of the chunk, scratch) runs models b0 .. b0 + nb.
// PtrBlock: the models of a chunk, the cells of the first chunk, the largest, and the two parts of the block in bytes;
// a driver that keeps planes of its own beside the block (downstream.hip iter_setup) sizes them by it.
struct PtrBlock {
  int64_t per, cells;
  size_t b_scales, b_chunk;
};
inline PtrBlock ptr_block(int64_t B, int64_t hw, PtrSizes sizes, const float* scales, int64_t n_scales) {
  const int64_t per = ptr_chunk_models(hw), cells = (B < per ? B : per) * hw;
  const bool per_model = scales && n_scales > 1;
  return PtrBlock{per, cells, per_model ? align256(sizeof(PathScale) * static_cast<size_t>(B)) : 0,
                  ptr_layout(cells, sizes).bytes()};
}
template <typename Chunk>
int ptr_run(WorkspaceSlot slot, PtrInfo& info, int64_t B, int64_t H, int64_t W, PtrSizes sizes, const float* scales,
            int64_t n_scales, PathScale none, hipStream_t st, Chunk chunk) {
  const auto [per, cells, b_scales, b_chunk] = ptr_block(B, H * W, sizes, scales, n_scales);
  info = PtrInfo{0, 0, 0, 0};
  const bool per_model = b_scales != 0;
  void* base = nullptr;
  if (int rc = workspace_get(slot, b_scales + b_chunk, &base); rc != SOIL_OK) return rc;
  PathScales sc{nullptr, scales ? path_scale(scales) : none};
  if (per_model) {
    if (int rc = upload_scale_records(base, scales, B, path_scale, st); rc != SOIL_OK) return rc;
    sc.per_model = static_cast<const PathScale*>(base);
  }
  char* const scratch = static_cast<char*>(base) + b_scales;
  for (int64_t b0 = 0; b0 < B; b0 += per) {
    PathScales s = sc;
    if (s.per_model) s.per_model += b0;
    if (int rc = chunk(b0, B - b0 < per ? B - b0 : per, s, scratch); rc != SOIL_OK) return rc;
  }
  return SOIL_OK;
}

}  // namespace soil
