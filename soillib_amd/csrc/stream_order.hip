// stream_order.hip — the channel network of a receiver graph (soil_stream_order / soil_stream_order_batch,
// soil_hip.h): which cells are channels, the Strahler order of each, the donors of each, where links and Strahler
// streams end, and the graph restricted to the channels.
//
// The order is no idempotent reduction — two donors of order k make k + 1, one does not — so upstream.hip's single
// closure cannot give it.  It stratifies by level, though (soil_hip.h: M_1 the channel cells, J_k the cells with two
// donors in M_k, M_{k+1} everything J_k reaches, order = the largest k with the cell in M_k), and each level is a
// max-closure of exactly upstream.hip's kind.  Per chunk, on the engine of flow_paths.hpp over 4-byte pointers:
//
//   init     P[n] = the receiver where the channel-graph edge n -> r exists (the edge rule and `stop` of
//            soil_flow_paths, n and r both channel cells), n | kFinal elsewhere; L[n] = 1 on a channel cell, 0 off.
//   seed i   (gather, no atomics) a cell c with L[c] >= i looks at its K neighbours; n is a donor iff P[n] = c.  With
//            s = min(i, the second-largest L among the donors): if s >= 1, L[c] <- max(L[c], s + 1).  A cell that rose
//            ORs into a pinned word the host looks at.  The pass also resets the working pointers J <- P for the
//            closure, and pass 1 writes the donor counts D.
//   closure  ceil(log2(H W)) rounds of upstream.hip's up_cell with a 32-bit atomicMax: a cell u in the work set with
//            pointer j = J[u]: L[j] <- max(L[j], L[u]); then, if j carries kFinal, u copies j across and leaves the
//            work set, else J'[u] = J[j].
//   final    order = L, donors = D, and from ONE gather of the receiver's L and D the foot planes; channel_graph from P.
//
// and the host runs  seed 1, look, closure, seed 2, look, closure, ...  until a seed pass raises nothing.
//
// Invariant.  Before seed pass i, L = min(order, i) everywhere: {L >= k} = M_k for every k <= i, and L <= order.
//   i = 1: L is 1 on M_1 and 0 off it.
//   Seed i.  A donor's L read during the pass is its value before the pass or the i + 1 the pass has just given it;
//   capped at i both are min(order, i): the pass is a Jacobi sweep without a second plane, and what it writes does
//   not depend on the schedule.  s = i iff two donors lie in M_i iff c is in J_i; then L[c] was i (J_i lies in
//   M_i: M_i is closed downstream for i >= 2, and J_1 in M_1 by definition) and becomes i + 1.  Where s < i the cell
//   lies in M_{s+1} at least and L[c] >= s + 1 already.  So the pass raises exactly J_i, by one, and raises nothing
//   iff J_i is empty iff M_{i+1} is empty iff no order exceeds i.  (A cell with L[c] < i or fewer than two donors
//   cannot lie in J_i and is not looked at from pass 2 on.)
//   Closure i.  The proof of upstream.hip's header carries over with max for min — max is as idempotent, monotone and
//   order-free; a word only ever rises; any L read is at least the word at the start of the launch and at most the
//   final maximum —: afterwards L[n] = the greatest L over everything that reaches n along the channel graph, which
//   is i + 1 exactly on what J_i reaches, M_{i+1}, and unchanged elsewhere: L = min(order, i + 1).
// What differs from upstream.hip: the words are 4 bytes (an aligned 32-bit load is whole by itself; the loads are
// relaxed atomic loads all the same), there is no index beside the value, the closure is run once per level on
// pointers reset from P, and the push is skipped where the target is already as HIGH.
//
// Levels.  `levels` (soil_stream_order_info, info[4]) is the number of seed passes run: the greatest order, or 1
// where there is no channel cell; the closures run are levels - 1, the last seed pass having raised nothing.  A cell
// of order k has 2^(k-1) distinct heads above it on a forest, and on any graph M_{k+1} non-empty needs a cell with two
// donors in M_k, distinct cells whose own certificates are disjoint up to the same count: 2^(levels-1) <= H W, at
// most floor(log2(H W)) + 1 levels.  A call that would run more has met an internal error and says so.
//
// Narrowing.  At level i >= 2 a cell with L < i is final and never pushes again, and since M_i is closed downstream
// no pointer of a cell of M_i leads through it: seed i gives it n | kFinal, the dense round 0 drops it, and the
// listed rounds run over M_i alone.  SOIL_STREAM_ORDER_NARROW=0 (read per call) turns this off for the A/B of
// DESIGN.md 3.5; the result does not depend on it.
//
// One host look per level (hipStreamSynchronize, as the fill's): the call is NOT free of synchronisation.  In a batch
// all models of a chunk iterate together, and the level count is that of the model that needs most.
#include <map>

#include "common.hpp"
#include "flow_paths.hpp"

namespace soil {

constexpr int kSoPlanes = 3;  // P, L, D: 4 bytes a cell each, beside the two pointer buffers

// The init and the seed pass walk SOIL_ROW_LOOP's bands of consecutive rows, a work-group per band and 256 columns,
// but with the band's height chosen per call: kRowBand rows where that still leaves a few thousand work-groups, fewer
// on a small grid — at 256 x 256 whole bands are 16 work-groups on 256 CUs, each walking its rows one after the other.
inline int so_band(int64_t models, int64_t H, int64_t W) {
  const int64_t groups_of_a_row = models * ((W + kPBlock - 1) / kPBlock);
  const int64_t band = H * groups_of_a_row / 2048;  // rows a work-group, for about 2048 work-groups
  return static_cast<int>(band < 1 ? 1 : (band > kRowBand ? kRowBand : band));
}
inline dim3 so_grid(const PtrChunk& c, int64_t H, int64_t W, bool vec, int band) {
  const int64_t bands = (H + band - 1) / band;
  return dim3(blocks_for(vec ? W / 4 : W, kPBlock), static_cast<unsigned>(bands < 65535 ? bands : 65535), c.z);
}
#define SO_ROW_LOOP(x, H, band)                                                                  \
  for (int64_t x##_band = blockIdx.y; x##_band * (band) < (H); x##_band += gridDim.y)            \
    for (int64_t x = x##_band * (band), x##_end = (x + (band) < (H)) ? x + (band) : (H); x < x##_end; ++x)

__device__ __forceinline__ int32_t so_load(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Whether cell m of the model is a channel cell (soil_hip.h): a float comparison, so a NaN area fails
__device__ __forceinline__ bool so_channel(const int32_t* __restrict__ channel, const float* __restrict__ area,
                                           float threshold, int64_t m) {
  return (!channel || channel[m] != 0) && (!area || area[m] >= threshold);
}

// The base pointer of cell (x, y) with graph entry g, itself a channel cell or not (`mine`)
template <int K>
__device__ __forceinline__ uint32_t so_pointer(int32_t g, bool stop, bool mine, const int32_t* __restrict__ channel,
                                               const float* __restrict__ area, float threshold, int64_t x, int64_t y,
                                               int64_t H, int64_t W, uint32_t first) {
  const uint32_t self = (first + static_cast<uint32_t>(x * W + y)) | kFinal;
  if (!mine || stop || edge_kind<K>(g, x, y, H, W) < 0) return self;
  return so_channel(channel, area, threshold, g) ? first + static_cast<uint32_t>(g) : self;
}

// Init: k_up_init's shape.  VEC: four cells per thread, the planes as 16-byte loads, P and L as 16-byte stores (W a
// multiple of four, the planes given 16-byte aligned).
template <int K, bool VEC>
__global__ void __launch_bounds__(kPBlock)
    k_so_init(uint32_t* __restrict__ P, int32_t* __restrict__ L, const int32_t* __restrict__ graph,
              const int32_t* __restrict__ channel, const float* __restrict__ area, float threshold,
              const int32_t* __restrict__ stop, int64_t H, int64_t W, int band) {
  const int64_t y = (static_cast<int64_t>(blockIdx.x) * kPBlock + threadIdx.x) * (VEC ? 4 : 1);
  if (y >= W) return;
  const int64_t first64 = static_cast<int64_t>(blockIdx.z) * H * W;
  const uint32_t first = static_cast<uint32_t>(first64);
  P += first64, L += first64, graph += first64;
  if (channel) channel += first64;
  if (area) area += first64;
  if (stop) stop += first64;
  SO_ROW_LOOP(x, H, band) {
    const int64_t n = x * W + y;
    if constexpr (VEC) {
      const int4 g = *reinterpret_cast<const int4*>(graph + n);
      const int4 s = stop ? *reinterpret_cast<const int4*>(stop + n) : make_int4(0, 0, 0, 0);
      const int4 c = channel ? *reinterpret_cast<const int4*>(channel + n) : make_int4(1, 1, 1, 1);
      const float4 a = area ? *reinterpret_cast<const float4*>(area + n) : make_float4(0.f, 0.f, 0.f, 0.f);
      const bool m0 = c.x != 0 && (!area || a.x >= threshold), m1 = c.y != 0 && (!area || a.y >= threshold),
                 m2 = c.z != 0 && (!area || a.z >= threshold), m3 = c.w != 0 && (!area || a.w >= threshold);
      *reinterpret_cast<uint4*>(P + n) =
          make_uint4(so_pointer<K>(g.x, s.x != 0, m0, channel, area, threshold, x, y + 0, H, W, first),
                     so_pointer<K>(g.y, s.y != 0, m1, channel, area, threshold, x, y + 1, H, W, first),
                     so_pointer<K>(g.z, s.z != 0, m2, channel, area, threshold, x, y + 2, H, W, first),
                     so_pointer<K>(g.w, s.w != 0, m3, channel, area, threshold, x, y + 3, H, W, first));
      *reinterpret_cast<int4*>(L + n) = make_int4(m0 ? 1 : 0, m1 ? 1 : 0, m2 ? 1 : 0, m3 ? 1 : 0);
    } else {
      const bool mine = so_channel(channel, area, threshold, n);
      P[n] = so_pointer<K>(graph[n], stop ? stop[n] != 0 : false, mine, channel, area, threshold, x, y, H, W, first);
      L[n] = mine ? 1 : 0;
    }
  }
}

// Seed pass `level` (the header's "seed i"): gather over the K neighbours, no atomics.  It also resets the engine's
// control words to {1, 0, 0} and the working pointers J <- P (narrowed: n | kFinal below the level), and pass 1
// writes the donor counts.
template <int K>
__global__ void __launch_bounds__(kPBlock)
    k_so_seed(uint32_t* __restrict__ J, int32_t* L, int32_t* __restrict__ D, const uint32_t* __restrict__ P, int64_t H,
              int64_t W, int band, int level, int narrow, int* __restrict__ flags, int* __restrict__ changed) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x < kPathFlags)
    flags[threadIdx.x] = threadIdx.x == 0 ? 1 : 0;
  const int64_t y = static_cast<int64_t>(blockIdx.x) * kPBlock + threadIdx.x;
  const int64_t first64 = static_cast<int64_t>(blockIdx.z) * H * W;
  const uint32_t first = static_cast<uint32_t>(first64);
  J += first64, L += first64, D += first64, P += first64;
  bool raised = false;
  if (y < W) {
    SO_ROW_LOOP(x, H, band) {
      const int64_t n = x * W + y;
      const uint32_t me = first + static_cast<uint32_t>(n);
      int32_t l = so_load(L + n);
      // (from pass 2 on only a cell of M_level with two donors can rise)
      if (l > 0 && (level == 1 || (l >= level && D[n] >= 2))) {
        int32_t top = 0, second = 0, count = 0;
#pragma unroll
        for (int rd = -1; rd <= 1; ++rd) {
#pragma unroll
          for (int cd = -1; cd <= 1; ++cd) {
            if ((rd == 0 && cd == 0) || (K == 4 && rd != 0 && cd != 0)) continue;
            const int64_t xx = x + rd, yy = y + cd;
            if (xx < 0 || xx >= H || yy < 0 || yy >= W) continue;
            const int64_t m = xx * W + yy;
            if (P[m] != me) continue;  // (a pointer with kFinal is never `me`)
            const int32_t v = so_load(L + m);
            ++count;
            if (v > top) second = top, top = v;
            else if (v > second) second = v;
          }
        }
        if (level == 1) D[n] = count;
        const int32_t s = second < level ? second : level;
        if (s >= 1 && s + 1 > l) {
          l = s + 1;
          __hip_atomic_store(L + n, l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          raised = true;
        }
      } else if (level == 1) {
        D[n] = 0;
      }
      J[n] = (narrow && l < level) ? (me | kFinal) : P[n];
    }
  }
  if (__any(raised) && (threadIdx.x & 63) == 0) *changed = 1;
}

// One cell of one closure round: upstream.hip's up_cell over 32-bit words and a maximum.  The push is skipped where
// the target already stands as high: it only rises.
template <typename IDX>
__device__ __forceinline__ bool so_cell(uint32_t* __restrict__ Jout, const uint32_t* __restrict__ Jin, int32_t* L,
                                        IDX n) {
  const uint32_t j = Jin[n];
  const IDX t = static_cast<IDX>(j & ~kFinal);
  if (t != n) {
    const int32_t mine = so_load(L + n);
    if (mine > so_load(L + t)) atomicMax(L + t, mine);
  }
  if (j & kFinal) {
    Jout[n] = j;
    return false;
  }
  Jout[n] = Jin[t];
  return true;
}

template <typename IDX>
__global__ void __launch_bounds__(kPBlock)
    k_so_round(uint4* out, const uint4* in, int32_t* L, int64_t elem64, int* __restrict__ flags, int round,
               uint32_t* __restrict__ list_out, uint32_t* __restrict__ fill_out, uint32_t seg) {
  uint32_t* const Jout = reinterpret_cast<uint32_t*>(out);
  const uint32_t* const Jin = reinterpret_cast<const uint32_t*>(in);
  ptr_round<IDX>([=](IDX n) { return so_cell<IDX>(Jout, Jin, L, n); }, elem64, flags, round, list_out, fill_out, seg);
}
template <typename IDX>
__global__ void __launch_bounds__(kPBlock)
    k_so_list(uint4* out, const uint4* in, int32_t* L, const uint32_t* __restrict__ list_in,
              const uint32_t* __restrict__ fill_in, uint32_t* __restrict__ list_out, uint32_t* __restrict__ fill_out,
              uint32_t seg) {
  uint32_t* const Jout = reinterpret_cast<uint32_t*>(out);
  const uint32_t* const Jin = reinterpret_cast<const uint32_t*>(in);
  ptr_list<IDX>([=](IDX n) { return so_cell<IDX>(Jout, Jin, L, n); }, list_in, fill_in, list_out, fill_out, seg);
}

// Final: a cell per thread, grid.z is the model; one gather of the receiver's L and D
__global__ void __launch_bounds__(kPBlock)
    k_so_final(int32_t* __restrict__ order, int32_t* __restrict__ donors, int32_t* __restrict__ link_foot,
               int32_t* __restrict__ order_foot, int32_t* __restrict__ channel_graph, const uint32_t* __restrict__ P,
               const int32_t* __restrict__ L, const int32_t* __restrict__ D, int64_t cells) {
  const int64_t first64 = static_cast<int64_t>(blockIdx.z) * cells;
  const uint32_t first = static_cast<uint32_t>(first64);
  for (int64_t n = static_cast<int64_t>(blockIdx.x) * kPBlock + threadIdx.x; n < cells;
       n += static_cast<int64_t>(gridDim.x) * kPBlock) {
    const int64_t i = first64 + n;
    const uint32_t p = P[i];
    const int32_t o = L[i];
    const bool edge = !(p & kFinal);
    int32_t lr = 0, dr = 0;
    if (edge && (link_foot || order_foot)) lr = L[p], dr = D[p];
    if (order) order[i] = o;
    if (donors) donors[i] = D[i];
    if (link_foot) link_foot[i] = (o > 0 && (!edge || dr >= 2)) ? 1 : 0;
    if (order_foot) order_foot[i] = (o > 0 && (!edge || lr > o)) ? 1 : 0;
    if (channel_graph) channel_graph[i] = edge ? static_cast<int32_t>(p - first) : -1;
  }
}

struct SoInfo {
  PtrInfo ptr;
  int64_t levels;
};
static thread_local SoInfo t_so_info{{0, 0, 0, 0}, 0};  // soil_stream_order_info

struct SoPlanes {  // the planes of a call, from the chunk's first cell on
  int32_t *order, *donors, *link_foot, *order_foot, *channel_graph;
  const int32_t *graph, *channel;
  const float* area;
  const int32_t* stop;
  SoPlanes from(int64_t off) const {
    return SoPlanes{at(order, off),      at(donors, off), at(link_foot, off), at(order_foot, off),
                    at(channel_graph, off), graph + off,  at(channel, off),   at(area, off),
                    at(stop, off)};
  }
};

inline PtrSizes so_sizes() { return PtrSizes(sizeof(int32_t), sizeof(uint32_t), kSoPlanes); }

// "a cell rose in this seed pass": a pinned, device-mapped word the waves write straight into, one per host thread
// and device (conditioning.hip, flats.hip)
static int so_changed_word(int** host, int** dev) {
  static thread_local ThreadOwned<PinnedWord> t_words;  // (goes with the thread: common.hpp)
  int d = 0;
  SOIL_HIP(hipGetDevice(&d));
  PinnedWord& w = t_words[d];
  SOIL_HIP(w.ensure());
  *host = w.host, *dev = w.dev;
  return SOIL_OK;
}

// One chunk of `models` models: init, the level loop, final
template <int K>
static int so_chunk(const char* what, const SoPlanes& q, float threshold, int64_t models, int64_t H, int64_t W,
                    char* scratch, hipStream_t st) {
  const PtrChunk c = ptr_carve(models, H, W, so_sizes(), scratch);
  const size_t b_plane = ptr_layout(c.elem, so_sizes()).b_extra;
  uint32_t* const J = reinterpret_cast<uint32_t*>(c.rec[0]);
  uint32_t* const P = static_cast<uint32_t*>(c.extra[0]);
  int32_t* const L = reinterpret_cast<int32_t*>(static_cast<char*>(c.extra[0]) + b_plane);
  int32_t* const D = reinterpret_cast<int32_t*>(static_cast<char*>(c.extra[0]) + 2 * b_plane);
  int *changed_host = nullptr, *changed_dev = nullptr;
  if (int rc = so_changed_word(&changed_host, &changed_dev); rc != SOIL_OK) return rc;
  const char* const e = std::getenv("SOIL_STREAM_ORDER_NARROW");  // read per call
  const int narrow = e && std::atoi(e) == 0 ? 0 : 1;

  const bool vec = ptr_vec_init(W, q.graph, q.stop, q.channel, q.area);
  const int band = so_band(models, H, W);
  launch_vec(vec, k_so_init<K, true>, k_so_init<K, false>, so_grid(c, H, W, vec, band), st, P, L, q.graph, q.channel,
             q.area, threshold, q.stop, H, W, band);
  SOIL_LAUNCH_CHECK();
  t_so_info.ptr.chunks += 1;
  t_so_info.ptr.vec_chunks += vec ? 1 : 0;
  t_so_info.ptr.idx64_chunks += c.idx32 ? 0 : 1;
  t_so_info.ptr.rounds = c.rounds;

  auto round = [&](const PtrChunk& cc, const PtrRound& r) {
    ptr_launch_round(cc, r, st, k_so_list<uint32_t>, k_so_list<int64_t>, k_so_round<uint32_t>, k_so_round<int64_t>, L);
  };
  int max_levels = 1;  // floor(log2(H W)) + 1
  while ((int64_t{2} << (max_levels - 1)) <= H * W) ++max_levels;
  const dim3 seed_grid = so_grid(c, H, W, false, band);
  for (int level = 1;; ++level) {
    if (level > max_levels)
      return fail(SOIL_ERR_HIP, std::string(what) + ": internal error: more levels than floor(log2(H W)) + 1");
    *changed_host = 0;  // the stream's own work on this word was waited for
    k_so_seed<K><<<seed_grid, kPBlock, 0, st>>>(J, L, D, P, H, W, band, level, narrow, c.flags, changed_dev);
    SOIL_LAUNCH_CHECK();
    SOIL_HIP(hipStreamSynchronize(st));
    if (t_so_info.levels < level) t_so_info.levels = level;
    if (!__atomic_load_n(changed_host, __ATOMIC_ACQUIRE)) break;
    ptr_rounds(c, round);
    SOIL_LAUNCH_CHECK();
  }
  k_so_final<<<ptr_final_grid(c, H * W), kPBlock, 0, st>>>(q.order, q.donors, q.link_foot, q.order_foot,
                                                           q.channel_graph, P, L, D, H * W);
  SOIL_LAUNCH_CHECK();
  return SOIL_OK;
}

// What both entries refuse before any device work, under the entry's name
static int check_stream_order(const char* what, const SoPlanes& q, float threshold, int64_t B, int64_t H, int64_t W,
                              int edge) {
  const std::string w(what);
  SOIL_REQUIRE(q.graph, w + ": null graph");
  SOIL_REQUIRE(q.order || q.donors || q.link_foot || q.order_foot || q.channel_graph,
               w + ": no output asked for (order, donors, link_foot, order_foot and channel_graph are all null)");
  if (int rc = check_grid_batch(w, B, H, W, edge); rc != SOIL_OK) return rc;
  SOIL_REQUIRE(!q.area || threshold == threshold, w + ": threshold is NaN");
  const size_t bytes = 4 * plane_cells(B, H * W);
  const void* const outs[5] = {q.order, q.donors, q.link_foot, q.order_foot, q.channel_graph};
  for (int i = 0; i < 5; ++i) {
    for (const void* in : {static_cast<const void*>(q.graph), static_cast<const void*>(q.channel),
                           static_cast<const void*>(q.area), static_cast<const void*>(q.stop)})
      SOIL_REQUIRE(!overlaps(outs[i], bytes, in, bytes), w + ": an output aliases an input plane");
    for (int k = i + 1; k < 5; ++k)
      SOIL_REQUIRE(!overlaps(outs[i], bytes, outs[k], bytes), w + ": two outputs overlap");
  }
  return SOIL_OK;
}

// A call, under the entry's name, through workspace slot WS_STREAM_ORDER (flow_paths.hpp ptr_run)
static int stream_order_run(const char* what, const SoPlanes& q, float threshold, int64_t B, int64_t H, int64_t W,
                            int edge, void* stream) {
  if (int rc = check_stream_order(what, q, threshold, B, H, W, edge); rc != SOIL_OK) return rc;
  SOIL_DEVICE();
  const hipStream_t st = as_stream(stream);
  auto go = edge == SOIL_D4 ? so_chunk<4> : so_chunk<8>;
  t_so_info.levels = 0;
  return ptr_run(WS_STREAM_ORDER, t_so_info.ptr, B, H, W, so_sizes(), nullptr, 1, PathScale{0.0, 0.0, 0.0}, st,
                 [&](int64_t b0, int64_t nb, const PathScales&, char* scratch) {
                   return go(what, q.from(b0 * H * W), threshold, nb, H, W, scratch, st);
                 });
}

}  // namespace soil

using namespace soil;

extern "C" {

int soil_stream_order(int32_t* order, int32_t* donors, int32_t* link_foot, int32_t* order_foot, int32_t* channel_graph,
                      const int32_t* graph, const int32_t* channel, const float* area, float threshold,
                      const int32_t* stop, int64_t H, int64_t W, int edge, void* stream) {
  return stream_order_run("stream_order",
                          SoPlanes{order, donors, link_foot, order_foot, channel_graph, graph, channel, area, stop},
                          threshold, 1, H, W, edge, stream);
}

int soil_stream_order_batch(int32_t* order, int32_t* donors, int32_t* link_foot, int32_t* order_foot,
                            int32_t* channel_graph, const int32_t* graph, const int32_t* channel, const float* area,
                            float threshold, const int32_t* stop, int64_t B, int64_t H, int64_t W, int edge,
                            void* stream) {
  return stream_order_run("stream_order_batch",
                          SoPlanes{order, donors, link_foot, order_foot, channel_graph, graph, channel, area, stop},
                          threshold, B, H, W, edge, stream);
}

int soil_stream_order_info(int64_t info[5]) {
  SOIL_REQUIRE(info, "stream_order_info: null info");
  t_so_info.ptr.store(info);
  info[4] = t_so_info.levels;
  return SOIL_OK;
}

}  // extern "C"
