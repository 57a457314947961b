// parallel-gcn_amd/csrc/slot_items.hpp -- the scaffolding of the kernels that walk the CSR slots
// of a square pattern one wave per work item (k_gat.hip, k_sage.hip).  An item is a row, a column
// of the transposed index, or a kGatSeg-slot segment of a long one.  The wave is cut into 64 / GL
// neighbour groups of GL lanes, lane li of a group holding the float4 at column 4 * li of its
// neighbour's row:
//   d <= 4: GL 1 | <= 8: 2 | <= 16: 4 | <= 32: 8 | <= 64: 16 | <= 128: 32
// Group q takes slots q, q + 64 / GL, ... of the item; the groups meet in xor butterflies over
// the lane offsets GL .. 32 (every lane ends with the same bits).
// (Inline definitions with external linkage in namespace pgcn: both translation units see
// these same definitions, which is what keeps that sound.)
#pragma once
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"

namespace pgcn {

constexpr int kItemThreads = 256;  // 4 waves: 4 items per workgroup step
constexpr int kItemWaves = kItemThreads / kWave;
constexpr int kItemMaxBlocks = 32 * kCUs;

// the float4 at columns c0 .. c0 + 3 of a row of logical width d: columns >= d read as zero
// (the padding may hold anything)
__device__ __forceinline__ float4 row4(const float *p, int c0, int d, bool on) {
  float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (on) {
    v = *reinterpret_cast<const float4 *>(p + c0);
    if (c0 + 1 >= d) v.y = 0.0f;
    if (c0 + 2 >= d) v.z = 0.0f;
    if (c0 + 3 >= d) v.w = 0.0f;
  }
  return v;
}

// this wave's item of a launch over the direct items and the segments, grid-stride
__device__ __forceinline__ long long first_item() {
  return ((long long)blockIdx.x * kItemThreads + threadIdx.x) / kWave;
}
__device__ __forceinline__ long long item_stride() { return (long long)gridDim.x * kItemWaves; }

// sum over the groups of a wave (the lane offsets GL and above)
template <int GL>
__device__ __forceinline__ float across_groups(float v) {
#pragma unroll
  for (int off = GL; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

inline int item_gl(int d) {
  const int d4 = (d + 3) / 4;
  return d4 <= 1 ? 1 : d4 <= 2 ? 2 : d4 <= 4 ? 4 : d4 <= 8 ? 8 : d4 <= 16 ? 16 : 32;
}

inline dim3 item_grid(long long items) {
  return dim3((unsigned)std::max<long long>(
      1, std::min<long long>(ceil_div(items, kItemWaves), kItemMaxBlocks)));
}

// KERNEL<GL> for the width `d` in scope
#define ITEM_DISPATCH(KERNEL, grid, s, ...)                                                  \
  do {                                                                                       \
    switch (item_gl(d)) {                                                                    \
      case 1: PGCN_LAUNCH((KERNEL<1>), grid, dim3(kItemThreads), 0, s, __VA_ARGS__); break;   \
      case 2: PGCN_LAUNCH((KERNEL<2>), grid, dim3(kItemThreads), 0, s, __VA_ARGS__); break;   \
      case 4: PGCN_LAUNCH((KERNEL<4>), grid, dim3(kItemThreads), 0, s, __VA_ARGS__); break;   \
      case 8: PGCN_LAUNCH((KERNEL<8>), grid, dim3(kItemThreads), 0, s, __VA_ARGS__); break;   \
      case 16: PGCN_LAUNCH((KERNEL<16>), grid, dim3(kItemThreads), 0, s, __VA_ARGS__); break; \
      default: PGCN_LAUNCH((KERNEL<32>), grid, dim3(kItemThreads), 0, s, __VA_ARGS__); break; \
    }                                                                                        \
  } while (0)

}  // namespace pgcn
