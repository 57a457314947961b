// parallel-gcn_amd/csrc/rank_mlp_sweep.hpp -- what the 1-vs-all sweeps under the Hadamard-MLP
// decoder share (k_rank_mlp.hip counts against a threshold, k_topk_mlp.hip selects the k best): the
// staging of a workgroup's anchor rows and candidate chunks, and one query's score of a wave's 32
// candidates -- the MFMA loop over all unit tiles and the forward's epilogue in its one order.  The
// score is defined by that order, so both sweeps call this code instead of holding a copy each.
// Device code only; include after link_mlp_tile.hpp, in a file compiled with fp contract(off) and
// without packed fp32 ops.
#pragma once

#include "link_mlp_tile.hpp"

namespace pgcn {
namespace {
static_assert(kRankMlpTQ == kLinkMlpTile && kRankMlpTC == kLinkMlpTile,
              "the sweeps keep their chunk in the image's z rows and their block's words in G / Red");

// chunk c of the candidates into registers (no branch: clamped addresses), registers into LDS
template <int ND, int UT>
__device__ __forceinline__ void rank_mlp_load_chunk(float4 *stage, const float *__restrict__ H,
                                                    int ld_h, int d, int n, int c, int tid) {
  using L = MlpLds<ND, UT>;
#pragma unroll
  for (int i = 0; i < L::NG; i++) {
    const int idx = i * kMlpThreads + tid;
    stage[i] = load_chunk(H, ld_h, d, n, c * kRankMlpTC + idx / L::CPR, idx % L::CPR);
  }
}
template <int ND, int UT>
__device__ __forceinline__ void rank_mlp_store_rows(float *rows, const float4 *stage, int tid) {
  using L = MlpLds<ND, UT>;
#pragma unroll
  for (int i = 0; i < L::NG; i++) {
    const int idx = i * kMlpThreads + tid;
    put_split<L::HD>(rows + (idx / L::CPR) * L::S, idx % L::CPR, stage[i]);
  }
}

// the rows of the block's anchors anchor[q0 .. q0 + kRankMlpTQ) into As (zero rows from Q on);
// stage is scratch
template <int ND, int UT>
__device__ __forceinline__ void rank_mlp_gather_anchors(float *As, float4 *stage,
                                                        const int *__restrict__ anchor, int q0,
                                                        int Q, const float *__restrict__ H,
                                                        int ld_h, int d, int n, int tid) {
  using L = MlpLds<ND, UT>;
#pragma unroll
  for (int i = 0; i < L::NG; i++) {
    const int idx = i * kMlpThreads + tid, q = q0 + idx / L::CPR;
    const float4 r = load_chunk(H, ld_h, d, n, anchor[min(q, Q - 1)], idx % L::CPR);
    stage[i] = q < Q ? r : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  rank_mlp_store_rows<ND, UT>(As, stage, tid);
}

// One query against a wave's 32 candidates.  a_row: the query's anchor row, c_row: this lane's
// candidate row, w_row: this lane's W1^T row of unit tile 0 -- each at the lane's column half.  The
// MFMA's B operand is formed on the fly (a v_mul of an anchor float4, a broadcast read, and its
// candidate float4) and ALL UT unit tiles run here, so the sum over units never leaves the wave:
// accumulators acc[uh][q] are the forward's wave uh, tile uh + 2 q; the two lane sums take
// mlp_lane_sum, each its __shfl_xor(32), then red[0] + red[1], then + b2 as mlp_tile_score has
// them.  Both lane halves return the score of candidate lane & 31.
template <int ND, int UT>
__device__ __forceinline__ float rank_mlp_query_score(const float *lds, const float *a_row,
                                                      const float *c_row, const float *w_row,
                                                      int groups, float b2, int half) {
  using L = MlpLds<ND, UT>;
  f32x16 acc[2][L::NQ];
#pragma unroll
  for (int u = 0; u < 2; u++)
#pragma unroll
    for (int q = 0; q < L::NQ; q++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[u][q][r] = 0.0f;
  for (int j = 0; j < groups; j++) {
    const float4 a = *reinterpret_cast<const float4 *>(a_row + 4 * j);
    const float4 b = *reinterpret_cast<const float4 *>(c_row + 4 * j);
    const float zx = a.x * b.x, zy = a.y * b.y, zz = a.z * b.z, zw = a.w * b.w;
#pragma unroll
    for (int ut = 0; ut < UT; ut++) {
      const float4 w = *reinterpret_cast<const float4 *>(w_row + 32 * ut * L::S + 4 * j);
      f32x16 &t = acc[ut & 1][ut >> 1];
      t = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, zx, t, 0, 0, 0);
      t = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, zy, t, 0, 0, 0);
      t = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, zz, t, 0, 0, 0);
      t = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, zw, t, 0, 0, 0);
    }
  }
  // the forward's epilogue: wave uh's lane sum and exchange, red[0] + red[1], + b2
  float s = mlp_lane_sum<ND, UT>(lds, acc[0], 0, half);
  s = s + __shfl_xor(s, 32, 64);
  if (UT > 1) {
    float s1 = mlp_lane_sum<ND, UT>(lds, acc[1], 1, half);
    s1 = s1 + __shfl_xor(s1, 32, 64);
    s = s + s1;
  }
  return s + b2;
}
}  // namespace
}  // namespace pgcn
