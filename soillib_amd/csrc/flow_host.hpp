// flow_host.hpp — what the host side of the flow solvers shares (flow_paths.hpp and through it flow_paths.hip and
// downstream.hip; diffuse.hip, flats.hip, conditioning.hip, graph.hip): the refusals of a batch's shape, of aliased
// outputs, of scales and dt, the models of a chunk, the two knobs read per call, and the upload of per-model scale
// records.  Host code only: nothing here is seen by a kernel.
#pragma once
#include <cmath>
#include <cstdlib>
#include <initializer_list>
#include <string>
#include <vector>

#include "common.hpp"

namespace soil {

inline size_t align256(size_t b) { return (b + 255) & ~static_cast<size_t>(255); }

// The shape refusals every batch entry shares, under the entry's name `w`, in this order.  An entry without scales
// leaves n_scales at 1, one without an edge passes SOIL_D8; `cells_note` ends the message about the cells of a model.
inline int check_grid_batch(const std::string& w, int64_t B, int64_t H, int64_t W, int edge, int64_t n_scales = 1,
                            const char* cells_note = " (int32 graph)") {
  SOIL_REQUIRE(B >= 1, w + ": B must be >= 1");
  SOIL_REQUIRE(H >= 1 && W >= 1, w + ": empty grid");
  SOIL_REQUIRE(H <= INT32_MAX / W, w + ": a model must have 1..2^31-1 cells" + cells_note);
  SOIL_REQUIRE(n_scales == 1 || n_scales == B, w + ": n_scales must be 1 or B");
  SOIL_REQUIRE(edge == SOIL_D4 || edge == SOIL_D8, w + ": invalid edge enumerator");
  return SOIL_OK;
}

// Whether [p, p + pb) and [q, q + qb) share a byte (a null pointer shares nothing)
inline bool overlaps(const void* p, size_t pb, const void* q, size_t qb) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return p && q && a < b + qb && b < a + pb;
}

// The cells of B planes of hw cells, counted so that the byte counts of the alias checks cannot wrap: a batch this
// large fails its allocation anyway
inline size_t plane_cells(int64_t B, int64_t hw) {
  return static_cast<size_t>(B > (int64_t{1} << 58) / hw ? (int64_t{1} << 58) : B * hw);
}

// Neither output shares a byte with one of `inputs` (4 bytes a cell), nor with the other
inline int check_outputs_apart(const std::string& w, const void* out, const void* out64, size_t cells,
                               std::initializer_list<const void*> inputs) {
  for (const void* q : inputs)
    SOIL_REQUIRE(!overlaps(out, 4 * cells, q, 4 * cells) && !overlaps(out64, 8 * cells, q, 4 * cells),
                 w + ": an output aliases an input plane");
  SOIL_REQUIRE(!overlaps(out, 4 * cells, out64, 8 * cells), w + ": out and out64 overlap");
  return SOIL_OK;
}

inline int check_scales_positive(const std::string& w, const float* scales, int64_t n_scales) {
  for (int64_t i = 0; i < 2 * n_scales; ++i)
    SOIL_REQUIRE(scales[i] > 0.0f && std::isfinite(scales[i]), w + ": a scale must be a positive finite float");
  return SOIL_OK;
}

inline int check_dt(const std::string& w, double dt) {
  SOIL_REQUIRE(dt >= 0.0 && std::isfinite(dt), w + ": dt must be finite and >= 0");
  return SOIL_OK;
}

// Models per chunk: as many whole models of hw cells as `cap_cells` holds — the most that keep an entry's offsets
// on 32 bits — or what SOIL_FLOW_BATCH_CELLS lowers that to (read per call: the tests reach the chunking with tiny
// shapes through it), at most `max_grid`, a launch's grid.y or grid.z, at least one.
inline int64_t chunk_models(int64_t cap_cells, int64_t hw, int64_t max_grid) {
  const char* const e = std::getenv("SOIL_FLOW_BATCH_CELLS");
  const int64_t cap_env = e ? std::atoll(e) : 0ll;
  const int64_t cap = cap_env > 0 && cap_env < cap_cells ? cap_env : cap_cells;
  const int64_t per = cap / hw;
  return per < 1 ? 1 : (per > max_grid ? max_grid : per);
}

// SOIL_PATHS_IDX64=1 (read per call): 64-bit offsets whatever the size, the form only a very large model takes
// otherwise, reached by the tests at small shapes through it.
inline bool force_idx64() {
  const char* const e = std::getenv("SOIL_PATHS_IDX64");
  return e && std::atoi(e) == 1;
}

// The records make(pair) of the B scale pairs of `scales`, copied to `dst` in stream order
template <typename Make>
int upload_scale_records(void* dst, const float* scales, int64_t B, Make make, hipStream_t st) {
  std::vector<decltype(make(scales))> host(static_cast<size_t>(B));
  for (int64_t b = 0; b < B; ++b) host[static_cast<size_t>(b)] = make(scales + 2 * b);
  return batch_upload(dst, host.data(), sizeof(host[0]) * host.size(), st);
}

}  // namespace soil
