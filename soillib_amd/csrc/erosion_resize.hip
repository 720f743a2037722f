// erosion_resize.hip — soil_erode_resize_batch: every plane of every model of a batch resampled to a new
// resolution by one kernel (include/soil_hip.h, "erosion: changing resolution").
//
// The arithmetic is k_resize's (stencil.hip), plane by plane: resize_pos, the clamped corner indices, the weights
// written 1 + -1*w and 0 + 1*w, columns interpolated first, then rows, all under -ffp-contract=off, so every
// value carries the bits soil_resize gives that plane alone.  What the fusion saves is everything around the
// arithmetic: the column index and weight are computed once per thread and the row index and weight once per row
// for all 12 (24 with colour) floats of a cell, `height` is rebuilt and the five flux planes are cleared in the
// same pass, and the model rides in grid.z, so a batch takes one launch where the single-plane route takes 15 B.
#include "common.hpp"

#include <type_traits>

namespace soil {
namespace {

constexpr int kRBlock = 256;
constexpr int64_t kMaxModels = 65535;  // grid.z

struct ResizePhysics {  // the planes of soil_erosion_planes the resample reads (src) and writes (dst), typed
  const float2* src_layers;
  const float* src_uplift;
  const float* src_rainfall;
  const float* src_waterHeight;
  const float* src_mass;
  const float* src_debris;
  const float2* src_velocity;
  const float2* src_debrisVelocity;
  float2* layers;
  float* height;  // may be null
  float* uplift;
  float* rainfall;
  float* waterHeight;
  float* mass;
  float* debris;
  float2* velocity;
  float2* debrisVelocity;
  // written zero
  float* waterFlux;
  float* massFlux;
  float* debrisFlux;
  float2* velocityFlux;
  float2* debrisVelocityFlux;
};
struct ResizeColour {  // soil_colour_planes in its order, vec3 AoS
  const float* src_albedo[4];
  float* albedo[4];
};
struct NoColour {};
// one by-value kernel argument; the physics-only kernel does not carry the 8 colour pointers
template <bool COLOUR>
struct ResizeArgs : ResizePhysics, std::conditional_t<COLOUR, ResizeColour, NoColour> {};

typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void store_nt(float* p, float v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ void store_nt(float2* p, float2 v) {  // one 8-byte store
  __builtin_nontemporal_store(v2f{v.x, v.y}, reinterpret_cast<v2f*>(p));
}

// the four corners of one output cell in a source plane and their weights (k_resize's, in its order)
struct Corners {
  int64_t i00, i01, i10, i11;
  float ay, by, ax, bx;
  __device__ __forceinline__ float mix(float v00, float v01, float v10, float v11) const {
    const float l0 = ay * v00 + by * v01;
    const float l1 = ay * v10 + by * v11;
    return ax * l0 + bx * l1;
  }
  __device__ __forceinline__ float at(const float* __restrict__ src) const {
    return mix(src[i00], src[i01], src[i10], src[i11]);
  }
  __device__ __forceinline__ float2 at(const float2* __restrict__ src) const {
    const float2 v00 = src[i00], v01 = src[i01], v10 = src[i10], v11 = src[i11];
    return make_float2(mix(v00.x, v01.x, v10.x, v11.x), mix(v00.y, v01.y, v10.y, v11.y));
  }
};

// One thread per output column, a band of rows per work-group (SOIL_ROW_LOOP), grid.z = the model.
template <bool COLOUR>
__global__ void __launch_bounds__(kRBlock)
    k_erode_resize(ResizeArgs<COLOUR> A, int64_t Hn, int64_t Wn, int64_t Ho, int64_t Wo) {
  const int64_t y = static_cast<int64_t>(blockIdx.x) * kRBlock + threadIdx.x;
  if (y >= Wn) return;
  const int64_t so = static_cast<int64_t>(blockIdx.z) * Ho * Wo;  // this model's first cell, old and new
  const int64_t dn = static_cast<int64_t>(blockIdx.z) * Hn * Wn;
  Corners c;
  const float py = resize_pos(y, Wn, Wo);
  int64_t iy = static_cast<int64_t>(py);
  if (iy > Wo - 2) iy = Wo - 2;
  if (iy < 0) iy = 0;  // Wo == 1
  const int64_t jy = (Wo > 1) ? iy + 1 : iy;
  const float wy = py - static_cast<float>(iy);
  c.ay = 1.0f + -1.0f * wy, c.by = 0.0f + 1.0f * wy;
  SOIL_ROW_LOOP(x, Hn) {
    const float px = resize_pos(x, Hn, Ho);
    int64_t ix = static_cast<int64_t>(px);
    if (ix > Ho - 2) ix = Ho - 2;
    if (ix < 0) ix = 0;
    const int64_t jx = (Ho > 1) ? ix + 1 : ix;
    const float wx = px - static_cast<float>(ix);
    c.ax = 1.0f + -1.0f * wx, c.bx = 0.0f + 1.0f * wx;
    c.i00 = so + ix * Wo + iy, c.i01 = so + ix * Wo + jy, c.i10 = so + jx * Wo + iy, c.i11 = so + jx * Wo + jy;
    const int64_t n = dn + x * Wn + y;

    const float2 layers = c.at(A.src_layers);
    const float2 velocity = c.at(A.src_velocity), debrisVelocity = c.at(A.src_debrisVelocity);
    const float uplift = c.at(A.src_uplift), rainfall = c.at(A.src_rainfall);
    const float waterHeight = c.at(A.src_waterHeight), mass = c.at(A.src_mass), debris = c.at(A.src_debris);
    // written once and not read again here: nontemporal stores, which leave the caches to the gathers
    store_nt(A.layers + n, layers);
    if (A.height) store_nt(A.height + n, layers.x + layers.y);  // layer_merge of the new layers
    store_nt(A.uplift + n, uplift);
    store_nt(A.rainfall + n, rainfall);
    store_nt(A.waterHeight + n, waterHeight);
    store_nt(A.mass + n, mass);
    store_nt(A.debris + n, debris);
    store_nt(A.velocity + n, velocity);
    store_nt(A.debrisVelocity + n, debrisVelocity);
    store_nt(A.waterFlux + n, 0.0f);
    store_nt(A.massFlux + n, 0.0f);
    store_nt(A.debrisFlux + n, 0.0f);
    store_nt(A.velocityFlux + n, make_float2(0.0f, 0.0f));
    store_nt(A.debrisVelocityFlux + n, make_float2(0.0f, 0.0f));
    // the colour planes after the physics stores: their 48 loads in flight beside the 32 above cost about 40
    // VGPRs and two of the five waves per SIMD
    if constexpr (COLOUR) {
      float albedo[4][3];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float* __restrict__ src = A.src_albedo[k];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
          albedo[k][ch] =
              c.mix(src[3 * c.i00 + ch], src[3 * c.i01 + ch], src[3 * c.i10 + ch], src[3 * c.i11 + ch]);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) store_nt(A.albedo[k] + 3 * n + ch, albedo[k][ch]);
    }
  }
}

// the kernel's argument from model b0's first cell on (old grid: `so` cells in, new grid: `dn`)
template <bool COLOUR>
ResizeArgs<COLOUR> resize_args(const soil_erosion_planes& D, const soil_erosion_planes& S,
                               const soil_colour_planes* DC, const soil_colour_planes* SC, int64_t dn, int64_t so) {
  ResizeArgs<COLOUR> A{};
  A.src_layers = reinterpret_cast<const float2*>(S.layers) + so;
  A.src_uplift = S.uplift + so;
  A.src_rainfall = S.rainfall + so;
  A.src_waterHeight = S.waterHeight + so;
  A.src_mass = S.mass + so;
  A.src_debris = S.debris + so;
  A.src_velocity = reinterpret_cast<const float2*>(S.velocity) + so;
  A.src_debrisVelocity = reinterpret_cast<const float2*>(S.debrisVelocity) + so;
  A.layers = reinterpret_cast<float2*>(const_cast<float*>(D.layers)) + dn;  // (const for the step's sake)
  A.height = D.height ? D.height + dn : nullptr;
  A.uplift = const_cast<float*>(D.uplift) + dn;
  A.rainfall = const_cast<float*>(D.rainfall) + dn;
  A.waterHeight = D.waterHeight + dn;
  A.mass = D.mass + dn;
  A.debris = D.debris + dn;
  A.velocity = reinterpret_cast<float2*>(D.velocity) + dn;
  A.debrisVelocity = reinterpret_cast<float2*>(D.debrisVelocity) + dn;
  A.waterFlux = D.waterFlux + dn;
  A.massFlux = D.massFlux + dn;
  A.debrisFlux = D.debrisFlux + dn;
  A.velocityFlux = reinterpret_cast<float2*>(D.velocityFlux) + dn;
  A.debrisVelocityFlux = reinterpret_cast<float2*>(D.debrisVelocityFlux) + dn;
  if constexpr (COLOUR) {
    const float* src[4] = {SC->albedo_bedrock, SC->albedo_surface, SC->albedo_fluvial, SC->albedo_debris};
    float* dst[4] = {const_cast<float*>(DC->albedo_bedrock), DC->albedo_surface, DC->albedo_fluvial,
                     DC->albedo_debris};
    for (int k = 0; k < 4; ++k) A.src_albedo[k] = src[k] + 3 * so, A.albedo[k] = dst[k] + 3 * dn;
  }
  return A;
}

template <bool COLOUR>
int resize_launch(const soil_erosion_planes& D, const soil_erosion_planes& S, const soil_colour_planes* DC,
                  const soil_colour_planes* SC, int64_t B, int64_t Hn, int64_t Wn, int64_t Ho, int64_t Wo,
                  hipStream_t st) {
  dim3 grid = grid_rows(Hn, Wn, kRBlock);
  for (int64_t b0 = 0; b0 < B; b0 += kMaxModels) {
    grid.z = static_cast<unsigned>(B - b0 < kMaxModels ? B - b0 : kMaxModels);
    k_erode_resize<COLOUR><<<grid, kRBlock, 0, st>>>(resize_args<COLOUR>(D, S, DC, SC, b0 * Hn * Wn, b0 * Ho * Wo),
                                                     Hn, Wn, Ho, Wo);
    SOIL_LAUNCH_CHECK();
  }
  return SOIL_OK;
}

}  // namespace
}  // namespace soil

using namespace soil;

extern "C" {

int soil_erode_resize_batch(const soil_erosion_planes* dst, const soil_erosion_planes* src,
                            const soil_colour_planes* dst_colour, const soil_colour_planes* src_colour, int64_t B,
                            int64_t Hn, int64_t Wn, int64_t Ho, int64_t Wo, void* stream) {
  SOIL_DEVICE();
  SOIL_REQUIRE(dst && src, "erode_resize_batch: null dst or src");
  if (int rc = check_batch(B, Hn, Wn, 0, nullptr, "erode_resize_batch (new size Hn x Wn)"); rc != SOIL_OK) return rc;
  if (int rc = check_batch(B, Ho, Wo, 0, nullptr, "erode_resize_batch (old size Ho x Wo)"); rc != SOIL_OK) return rc;
  const soil_erosion_planes& D = *dst;
  const soil_erosion_planes& S = *src;
  SOIL_REQUIRE(S.layers && S.uplift && S.rainfall && S.waterHeight && S.mass && S.debris && S.velocity &&
                   S.debrisVelocity,
               "erode_resize_batch: null plane in src (the flux planes, layers_next and height are not read)");
  SOIL_REQUIRE(D.layers && D.uplift && D.rainfall && D.waterHeight && D.mass && D.debris && D.velocity &&
                   D.debrisVelocity && D.waterFlux && D.massFlux && D.velocityFlux && D.debrisFlux &&
                   D.debrisVelocityFlux,
               "erode_resize_batch: null plane in dst (only height and layers_next are optional)");
  SOIL_REQUIRE(!dst_colour == !src_colour,
               "erode_resize_batch: dst_colour and src_colour must both be NULL or both be set");
  SOIL_REQUIRE(!dst_colour || (has_colour(dst_colour) && has_colour(src_colour)),
               "erode_resize_batch: every colour plane of dst_colour and src_colour is required");
  SOIL_REQUIRE(D.layers != S.layers, "erode_resize_batch: dst->layers == src->layers (in place is not supported)");
  const hipStream_t st = as_stream(stream);
  if (dst_colour) return resize_launch<true>(D, S, dst_colour, src_colour, B, Hn, Wn, Ho, Wo, st);
  return resize_launch<false>(D, S, nullptr, nullptr, B, Hn, Wn, Ho, Wo, st);
}

}  // extern "C"
