// upstream.hip — minima and maxima UP a receiver graph (soil_upstream_extreme / soil_upstream_extreme_batch,
// soil_hip.h): out[n] = the least (the greatest) value[u] over every cell u that reaches n, and the cell that holds
// it.  Breaching a DEM along its conditioned graph is the minimum of the heights; the longest flow path and the
// catchment relief are maxima.
//
// Order.  Values are compared as integer keys (erosion_quantiles.hip key_of: -inf < .. < -0 < +0 < .. < +inf < NaN,
// every NaN one key), never as floats.  A cell's word is (key << 32) | index-within-the-model, so ONE unsigned 64-bit
// minimum carries the value and its `arg`, ties going to the smallest index.  The maximum is the minimum of the
// negated values (the sign bit flipped before the key is made), negated back in the final pass.
//
// Pointer doubling on the engine of flow_paths.hpp, over 4-byte records — the pointer J with kFinal in bit 31,
// double-buffered as there — and one plane M of packed words, updated IN PLACE by atomic minima:
//
//   init    J[n] = n | kFinal for a terminal, the receiver otherwise (the edge rule and `stop` of soil_flow_paths);
//           M[n] = (key(value[n]) << 32) | n.
//   round   a cell u in the work set, with pointer j = J[u]:  M[j] <- min(M[j], M[u])  by one atomic;  then, if j
//           carries kFinal, u copies j across and leaves the work set, else J'[u] = J[j].
//   final   out = the float of the key (negated for max, the quiet NaN kept), arg = the index, -1 where NaN.
//
// Why the rounds give the definition.  Write r for the receiver map made total by r(t) = t on a terminal, and d(w, n)
// for the number of edges from w to n along it.  At the start of round k, J[u] = r^(2^k)(u).  Claim: at that point
// M[n] holds min{value[w] : r^i(w) = n for some i <= 2^k - 1}.  True for k = 0.  Round k: every u with
// r^(2^k)(u) = n pushes M[u], which covers the w with r^i(w) = u, i <= 2^k - 1, so r^(i + 2^k)(w) = n: together with
// M[n] itself every exponent 0 .. 2^(k+1) - 1 is covered, and nothing that does not reach n is ever pushed to it.
// Any u that reaches n does so within H W - 1 edges (a walk that is longer has met a cell twice), and after
// ceil(log2(H W)) rounds the exponents go up to 2^rounds - 1 >= H W - 1: M[n] is the minimum over everything that
// reaches n, on cycles as anywhere else — no cell is special.  One round less does not carry the head of a chain
// through every cell to its foot.
//
// Leaving the work set.  A cell u at d >= 1 edges from its terminal t finds kFinal on its pointer first in the round
// k with 2^k > d (flow_paths.hip, "Round count"), pushes into t in that round too and leaves; its pointer is t from
// the first round with 2^k >= d on.  Nothing is lost by its leaving: a source w at D edges from t,
// 2^k <= D < 2^(k+1), is carried to t by v = r^(D - 2^k)(w), which lies exactly 2^k edges from t, has w within
// 2^k - 1 edges above it — so M[v] holds value[w] at the start of round k by the claim — and is still in the work set
// in round k: it leaves in round k + 1.  What arrives at u after it left is delivered by its senders' own jumps in
// the same way.  (Pushing into t in more than one round is idempotent.)  A dense round runs over every cell, also
// those that left: their push is repeated, and skipped by the rule below.
//
// Reading M while it is written.  A round reads M[u] and M[j] while other cells' atomics fall on them.  This rests on
// one assumption, stated here: an aligned 8-byte word is read WHOLE, never as the key of one word beside the index of
// another — a torn (key_new, index_old) of the target could skip a push that was needed, a torn word of the cell's own
// could push a word that never was.  The loads are therefore relaxed atomic loads of device scope (up_load: one
// global_load_dwordx2, as a plain load would be; no ordering is asked for and none is needed).  Any word read is at
// most the word at the start of the launch (a word only ever falls) and at least the final minimum, and it is the
// minimum of values that reach the cell: pushing it is never wrong, and the claim needs only that it is no greater
// than the word at the start of the launch.  min is monotone and idempotent, so neither a stale read nor a fresher
// one changes the result: one definite bit pattern under any schedule.
//
// Push rule.  The atomic is skipped where that load of M[j] is already <= the cell's own word: the target only
// falls, so the atomic would have changed nothing.  A river outlet that millions of cells point at in the late rounds
// takes an atomic only from the cells that still see it above their own word, not one from each.
//
// A batch is one stacked array, as in flow_paths.hip: pointers are indices into the chunk, the index in a packed word
// is the cell's index within its model, and a pointer never leaves its model.
#include "common.hpp"
#include "flow_paths.hpp"

namespace soil {

using u64 = unsigned long long;

constexpr uint32_t kNanKey = 0xFFC00000u;  // key_of of every NaN: the greatest key

// erosion_quantiles.hip key_of / bits_of: the order of the floats as unsigned integers, every NaN one key
__device__ __forceinline__ uint32_t up_key(uint32_t u) {
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) u = 0x7FC00000u;
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint32_t up_bits(uint32_t key) { return (key >> 31) ? (key & 0x7FFFFFFFu) : ~key; }

// The pointer of cell (x, y) with graph entry g (flow_paths.hip path_record's first word) and its packed word;
// `flip`: 0x80000000 for the maximum (the value negated), 0 for the minimum
template <int K>
__device__ __forceinline__ uint32_t up_pointer(int32_t g, bool stop, int64_t x, int64_t y, int64_t H, int64_t W,
                                               uint32_t first) {
  if (stop || edge_kind<K>(g, x, y, H, W) < 0) return (first + static_cast<uint32_t>(x * W + y)) | kFinal;
  return first + static_cast<uint32_t>(g);
}
__device__ __forceinline__ u64 up_word(float v, uint32_t flip, int64_t n) {
  return (static_cast<u64>(up_key(__float_as_uint(v) ^ flip)) << 32) | static_cast<u64>(static_cast<uint32_t>(n));
}

// Init: k_paths_init's shape.  VEC: four cells per thread, the three planes as 16-byte loads, the four pointers as
// one 16-byte store and the four words as two (W a multiple of four, the planes 16-byte aligned; a model's first
// cell is then a multiple of four as well).
template <int K, bool VEC>
__global__ void __launch_bounds__(kPBlock)
    k_up_init(uint32_t* __restrict__ J, u64* __restrict__ M, const int32_t* __restrict__ graph,
              const float* __restrict__ value, const int32_t* __restrict__ stop, int64_t H, int64_t W, uint32_t flip,
              int* __restrict__ flags) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x < kPathFlags)
    flags[threadIdx.x] = threadIdx.x == 0 ? 1 : 0;
  const int64_t y = (static_cast<int64_t>(blockIdx.x) * kPBlock + threadIdx.x) * (VEC ? 4 : 1);
  if (y >= W) return;
  const int64_t first64 = static_cast<int64_t>(blockIdx.z) * H * W;
  const uint32_t first = static_cast<uint32_t>(first64);
  J += first64, M += first64, graph += first64, value += first64;
  if (stop) stop += first64;
  SOIL_ROW_LOOP(x, H) {
    const int64_t n = x * W + y;
    if constexpr (VEC) {
      const int4 g = *reinterpret_cast<const int4*>(graph + n);
      const int4 s = stop ? *reinterpret_cast<const int4*>(stop + n) : make_int4(0, 0, 0, 0);
      const float4 v = *reinterpret_cast<const float4*>(value + n);
      *reinterpret_cast<uint4*>(J + n) =
          make_uint4(up_pointer<K>(g.x, s.x != 0, x, y + 0, H, W, first), up_pointer<K>(g.y, s.y != 0, x, y + 1, H, W, first),
                     up_pointer<K>(g.z, s.z != 0, x, y + 2, H, W, first), up_pointer<K>(g.w, s.w != 0, x, y + 3, H, W, first));
      *reinterpret_cast<ulonglong2*>(M + n) = make_ulonglong2(up_word(v.x, flip, n), up_word(v.y, flip, n + 1));
      *reinterpret_cast<ulonglong2*>(M + n + 2) = make_ulonglong2(up_word(v.z, flip, n + 2), up_word(v.w, flip, n + 3));
    } else {
      J[n] = up_pointer<K>(graph[n], stop ? stop[n] != 0 : false, x, y, H, W, first);
      M[n] = up_word(value[n], flip, n);
    }
  }
}

// A word of M read while atomics fall on it: a relaxed atomic load of device scope, one global_load_dwordx2, which the
// compiler may neither split nor merge with its neighbour's — the word is read whole
__device__ __forceinline__ u64 up_load(const u64* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One cell of one round: the push, then the jump Jin -> Jout.  Returns whether the cell stays in the work set (it
// wrote a new pointer; if that one carries the bit, the next round is the one in which it pushes into its terminal).
template <typename IDX>
__device__ __forceinline__ bool up_cell(uint32_t* __restrict__ Jout, const uint32_t* __restrict__ Jin, u64* M, IDX n) {
  const uint32_t j = Jin[n];
  const IDX t = static_cast<IDX>(j & ~kFinal);
  if (t != n) {  // (a terminal, or a cell whose pointer has come round its cycle to itself: nothing to push)
    const u64 mine = up_load(M + n);
    if (mine < up_load(M + t)) atomicMin(M + t, mine);  // the push rule: the target only falls
  }
  if (j & kFinal) {  // both buffers hold the pointer from here on
    Jout[n] = j;
    return false;
  }
  Jout[n] = Jin[t];
  return true;
}

// The dense and the listed round (flow_paths.hpp ptr_round, ptr_list) over up_cell; the record buffers are the
// engine's, 4 bytes a cell here
template <typename IDX>
__global__ void __launch_bounds__(kPBlock)
    k_up_round(uint4* out, const uint4* in, u64* M, int64_t elem64, int* __restrict__ flags, int round,
               uint32_t* __restrict__ list_out, uint32_t* __restrict__ fill_out, uint32_t seg) {
  uint32_t* const Jout = reinterpret_cast<uint32_t*>(out);
  const uint32_t* const Jin = reinterpret_cast<const uint32_t*>(in);
  ptr_round<IDX>([=](IDX n) { return up_cell<IDX>(Jout, Jin, M, n); }, elem64, flags, round, list_out, fill_out, seg);
}
template <typename IDX>
__global__ void __launch_bounds__(kPBlock)
    k_up_list(uint4* out, const uint4* in, u64* M, const uint32_t* __restrict__ list_in,
              const uint32_t* __restrict__ fill_in, uint32_t* __restrict__ list_out, uint32_t* __restrict__ fill_out,
              uint32_t seg) {
  uint32_t* const Jout = reinterpret_cast<uint32_t*>(out);
  const uint32_t* const Jin = reinterpret_cast<const uint32_t*>(in);
  ptr_list<IDX>([=](IDX n) { return up_cell<IDX>(Jout, Jin, M, n); }, list_in, fill_in, list_out, fill_out, seg);
}

// Final: a cell per thread, grid.z is the model
__global__ void __launch_bounds__(kPBlock)
    k_up_final(float* __restrict__ out, int32_t* __restrict__ arg, const u64* __restrict__ M, int64_t cells,
               uint32_t flip) {
  const int64_t first64 = static_cast<int64_t>(blockIdx.z) * cells;
  for (int64_t n = static_cast<int64_t>(blockIdx.x) * kPBlock + threadIdx.x; n < cells;
       n += static_cast<int64_t>(gridDim.x) * kPBlock) {
    const u64 m = M[first64 + n];
    const uint32_t key = static_cast<uint32_t>(m >> 32);
    const bool nan = key == kNanKey;
    if (out) out[first64 + n] = __uint_as_float(nan ? 0x7FC00000u : up_bits(key) ^ flip);
    if (arg) arg[first64 + n] = nan ? -1 : static_cast<int32_t>(static_cast<uint32_t>(m));
  }
}

static thread_local PtrInfo t_up_info{0, 0, 0, 0};  // soil_upstream_extreme_info

// One chunk of `models` models (flow_paths.hpp ptr_chunk) with this file's launches
template <int K>
static int up_chunk(float* out, int32_t* arg, const int32_t* graph, const float* value, const int32_t* stop,
                    int64_t models, int64_t H, int64_t W, uint32_t flip, char* scratch, hipStream_t st) {
  auto init = [&](const PtrChunk& c) {
    const bool vec = ptr_vec_init(W, graph, stop, value);
    launch_vec(vec, k_up_init<K, true>, k_up_init<K, false>, ptr_init_grid(c, H, W, vec), st,
               reinterpret_cast<uint32_t*>(c.rec[0]), static_cast<u64*>(c.extra[0]), graph, value, stop, H, W, flip,
               c.flags);
    return vec;
  };
  auto round = [&](const PtrChunk& c, const PtrRound& q) {
    ptr_launch_round(c, q, st, k_up_list<uint32_t>, k_up_list<int64_t>, k_up_round<uint32_t>, k_up_round<int64_t>,
                     static_cast<u64*>(c.extra[0]));
  };
  auto fin = [&](const PtrChunk& c, dim3 grid, const uint4*) {
    k_up_final<<<grid, kPBlock, 0, st>>>(out, arg, static_cast<const u64*>(c.extra[0]), H * W, flip);
  };
  return ptr_chunk(t_up_info, models, H, W, PtrSizes(sizeof(u64), sizeof(uint32_t), 1), scratch, init, round, fin);
}

// What both entries refuse before any device work, under the entry's name
static int check_upstream(const char* what, const void* out, const void* arg, const void* graph, const void* value,
                          const void* stop, int64_t B, int64_t H, int64_t W, int edge, int op) {
  const std::string w(what);
  SOIL_REQUIRE(graph, w + ": null graph");
  SOIL_REQUIRE(value, w + ": null value");
  SOIL_REQUIRE(out || arg, w + ": no output asked for (out and arg are both null)");
  if (int rc = check_grid_batch(w, B, H, W, edge); rc != SOIL_OK) return rc;
  SOIL_REQUIRE(op == 0 || op == 1, w + ": op must be 0 (min) or 1 (max)");
  const size_t bytes = 4 * plane_cells(B, H * W);
  for (const void* q : {graph, value, stop})
    SOIL_REQUIRE(!overlaps(out, bytes, q, bytes) && !overlaps(arg, bytes, q, bytes),
                 w + ": an output aliases an input plane");
  SOIL_REQUIRE(!overlaps(out, bytes, arg, bytes), w + ": out and arg overlap");
  return SOIL_OK;
}

// A call, under the entry's name, through workspace slot WS_UPSTREAM (flow_paths.hpp ptr_run)
static int upstream_run(const char* what, float* out, int32_t* arg, const int32_t* graph, const float* value,
                        const int32_t* stop, int64_t B, int64_t H, int64_t W, int edge, int op, void* stream) {
  if (int rc = check_upstream(what, out, arg, graph, value, stop, B, H, W, edge, op); rc != SOIL_OK) return rc;
  SOIL_DEVICE();
  const hipStream_t st = as_stream(stream);
  const uint32_t flip = op == 1 ? 0x80000000u : 0u;
  auto go = edge == SOIL_D4 ? up_chunk<4> : up_chunk<8>;
  return ptr_run(WS_UPSTREAM, t_up_info, B, H, W, PtrSizes(sizeof(u64), sizeof(uint32_t), 1), nullptr, 1,
                 PathScale{0.0, 0.0, 0.0}, st, [&](int64_t b0, int64_t nb, const PathScales&, char* scratch) {
                   const int64_t off = b0 * H * W;
                   return go(at(out, off), at(arg, off), graph + off, value + off, at(stop, off), nb, H, W, flip,
                             scratch, st);
                 });
}

}  // namespace soil

using namespace soil;

extern "C" {

int soil_upstream_extreme(float* out, int32_t* arg, const int32_t* graph, const float* value, const int32_t* stop,
                          int64_t H, int64_t W, int edge, int op, void* stream) {
  return upstream_run("upstream_extreme", out, arg, graph, value, stop, 1, H, W, edge, op, stream);
}

int soil_upstream_extreme_batch(float* out, int32_t* arg, const int32_t* graph, const float* value,
                                const int32_t* stop, int64_t B, int64_t H, int64_t W, int edge, int op, void* stream) {
  return upstream_run("upstream_extreme_batch", out, arg, graph, value, stop, B, H, W, edge, op, stream);
}

int soil_upstream_extreme_info(int64_t info[4]) {
  SOIL_REQUIRE(info, "upstream_extreme_info: null info");
  t_up_info.store(info);
  return SOIL_OK;
}

}  // extern "C"
