// flow_paths.hpp — what the pointer-doubling kernels along a receiver graph share: flow_paths.hip (terminal, steps,
// length) and downstream.hip (the linear recurrence x[n] = a L + b x[r(n)]).  Both run rounds over 16-byte records
// whose first word is the pointer with kFinal in bit 31, over per-work-group lists of the cells still pending, in
// chunks of whole models; the records' other words, the init and the final pass are each file's own.
#pragma once
#include <cmath>

#include "common.hpp"

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

// Control words of the dense rounds (graph.hip kRakeFlags): flags[round % 3] = "work left"
constexpr int kPathFlags = 4;

// graph.hip rake_append: the entries of a wave side by side in its work-group's segment, one LDS atomic per wave
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

// The scale of a model as the final pass reads it: the floats widened, and dd = sqrt(sx sx + sy sy) made on the host
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

inline size_t align256(size_t b) { return (b + 255) & ~static_cast<size_t>(255); }

}  // namespace soil
