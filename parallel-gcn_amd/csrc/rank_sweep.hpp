// parallel-gcn_amd/csrc/rank_sweep.hpp -- what the 1-vs-all sweeps over an embedding share
// (k_rank.hip counts against a fixed threshold, k_topk.hip selects the k best): the rank score's
// fmaf chain, the split LDS row layout, the clamped loads, the staging of a workgroup's anchors and
// candidate tiles, and the f32 MFMA product of a wave's 32 queries with a tile's 64 candidates.
// Device code only; include after common.hpp and kernels.hpp.
#pragma once

#include "common.hpp"
#include "kernels.hpp"

namespace pgcn {
namespace {
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kRankThreads = 256;

// r(a, v) over d columns of two rows (16-byte aligned, readable up to round_up4(d))
__device__ __forceinline__ float chain_score(const float *__restrict__ a,
                                             const float *__restrict__ b, int d) {
  float s = 0.0f;
  int c = 0;
  for (; c + 4 <= d; c += 4) {
    const float4 x = *reinterpret_cast<const float4 *>(a + c);
    const float4 y = *reinterpret_cast<const float4 *>(b + c);
    s = __fmaf_rn(x.x, y.x, s);
    s = __fmaf_rn(x.y, y.y, s);
    s = __fmaf_rn(x.z, y.z, s);
    s = __fmaf_rn(x.w, y.w, s);
  }
  if (c < d) {
    const float4 x = *reinterpret_cast<const float4 *>(a + c);
    const float4 y = *reinterpret_cast<const float4 *>(b + c);
    s = __fmaf_rn(x.x, y.x, s);
    if (c + 1 < d) s = __fmaf_rn(x.y, y.y, s);
    if (c + 2 < d) s = __fmaf_rn(x.z, y.z, s);
  }
  return s;
}

// the float4 at columns 4 ch .. 4 ch + 3 into a split row: even columns at [0, HD), odd at [HD, 2 HD)
template <int HD>
__device__ __forceinline__ void put_split(float *row, int ch, float4 v) {
  *reinterpret_cast<float2 *>(row + 2 * ch) = make_float2(v.x, v.z);
  *reinterpret_cast<float2 *>(row + HD + 2 * ch) = make_float2(v.y, v.w);
}

// the float4 at chunk ch of row `node` of H (always loaded, from a clamped address), zero where
// the row or the column does not exist
__device__ __forceinline__ float4 load_chunk(const float *__restrict__ H, int ld_h, int d, int n,
                                             int node, int ch) {
  const int c0 = 4 * ch, last = ((d + 3) / 4 - 1) * 4;
  const float4 r = *reinterpret_cast<const float4 *>(H + (long long)min(node, n - 1) * ld_h +
                                                     min(c0, last));
  const bool row_on = node < n;
  float4 v;
  v.x = row_on && c0 < d ? r.x : 0.0f;
  v.y = row_on && c0 + 1 < d ? r.y : 0.0f;
  v.z = row_on && c0 + 2 < d ? r.z : 0.0f;
  v.w = row_on && c0 + 3 < d ? r.w : 0.0f;
  return v;
}

// A sweep's LDS image, NV float4s a thread stages per candidate tile: rows of W = 16 NV >=
// round_up8(d) columns at stride S; kRankTQ anchor rows, then two buffers of kRankTC candidate rows
template <int NV>
struct SweepLds {
  static constexpr int W = 16 * NV, S = W + 4, HD = W / 2, CPR = 4 * NV;
  static constexpr int kFloats = (kRankTQ + 2 * kRankTC) * S;
};

// the rows of the workgroup's anchors anchor[q0 .. q0 + kRankTQ) into As (zero rows from Q on)
template <int NV>
__device__ __forceinline__ void sweep_gather_anchors(float *As, const int *__restrict__ anchor,
                                                     int q0, int Q, const float *__restrict__ H,
                                                     int ld_h, int d, int n, int tid) {
  using L = SweepLds<NV>;
#pragma unroll
  for (int i = 0; i < 2 * NV; i++) {
    const int idx = i * kRankThreads + tid, row = idx / L::CPR, ch = idx % L::CPR, q = q0 + row;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (q < Q) v = load_chunk(H, ld_h, d, n, anchor[q], ch);
    put_split<L::HD>(As + row * L::S, ch, v);
  }
}

// candidate tile t: its rows into registers (no branch: clamped addresses), registers into LDS
template <int NV>
__device__ __forceinline__ void sweep_load_tile(float4 (&stage)[NV], const float *__restrict__ H,
                                                int ld_h, int d, int n, int t, int tid) {
  using L = SweepLds<NV>;
#pragma unroll
  for (int i = 0; i < NV; i++) {
    const int idx = i * kRankThreads + tid;
    stage[i] = load_chunk(H, ld_h, d, n, t * kRankTC + idx / L::CPR, idx % L::CPR);
  }
}
template <int NV>
__device__ __forceinline__ void sweep_store_tile(float *Bt, const float4 (&stage)[NV], int tid) {
  using L = SweepLds<NV>;
#pragma unroll
  for (int i = 0; i < NV; i++) {
    const int idx = i * kRankThreads + tid;
    put_split<L::HD>(Bt + (idx / L::CPR) * L::S, idx % L::CPR, stage[i]);
  }
}

// a wave's 32 queries (a_row: this lane's row and column half of As) x a tile's 64 candidates
// (b_row: likewise of the tile): two 32 x 32 accumulators from zero, k ascending.  Accumulator
// register r of a lane is query row sweep_row(r, half) of the wave's 32, candidate lane & 31 of
// the tile (acc0) and that + 32 (acc1).
template <int S>
__device__ __forceinline__ void sweep_mfma(const float *a_row, const float *b_row, int groups,
                                           f32x16 &acc0, f32x16 &acc1) {
#pragma unroll
  for (int r = 0; r < 16; r++) acc0[r] = acc1[r] = 0.0f;
  for (int j = 0; j < groups; j++) {
    const float4 a = *reinterpret_cast<const float4 *>(a_row + 4 * j);
    const float4 b0 = *reinterpret_cast<const float4 *>(b_row + 4 * j);
    const float4 b1 = *reinterpret_cast<const float4 *>(b_row + 32 * S + 4 * j);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0.x, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b1.x, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b0.y, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1.y, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b0.z, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b1.z, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b0.w, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b1.w, acc1, 0, 0, 0);
  }
}
__host__ __device__ constexpr int sweep_row(int r, int half) {
  return (r & 3) + 8 * (r >> 2) + 4 * half;
}

// the sweep instantiation of a width: LAUNCH(NV) with 16 NV >= round_up8(d)
#define PGCN_SWEEP_BY_WIDTH(d, LAUNCH) \
  do {                                 \
    if ((d) <= 16) LAUNCH(1);          \
    else if ((d) <= 32) LAUNCH(2);     \
    else if ((d) <= 64) LAUNCH(4);     \
    else LAUNCH(8);                    \
  } while (0)
}  // namespace
}  // namespace pgcn
