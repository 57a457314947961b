// parallel-gcn_amd/csrc/link_mlp_tile.hpp -- the tile code the Hadamard-MLP decoder's kernels share
// (k_link_mlp.hip: the pair forward and backward; k_rank_mlp.hip: the 1-vs-all sweep and its filter
// correction): the LDS image, the staging of W1^T, b1 and w2, the f32 MFMA contraction mlp_pre and
// the forward epilogue's per-lane sum.  A score is defined by the ORDER of these operations, so
// every kernel that has to agree with k_link_mlp_fwd bit for bit is built from them.
// Device code only; include after common.hpp, kernels.hpp and rank_sweep.hpp, in a file compiled
// with fp contract(off) and without packed fp32 ops.
#pragma once

#include "common.hpp"
#include "kernels.hpp"
#include "rank_sweep.hpp"

namespace pgcn {
namespace {
constexpr int kMlpThreads = 256;
constexpr int kMlpLdsBudget = 150 * 1024;

// LDS image of the pair kernels, in floats: W1^T [WU][S], z [kLinkMlpTile][S], b1 [WU], w2 [WU],
// G [tile], the forward's cross-wave partials [2][tile]; the backward's dhid [tile][SU] behind
template <int ND, int UT>
struct MlpLds {
  static constexpr int S = ND + 4, HD = ND / 2, CPR = ND / 4, NG = kLinkMlpTile * CPR / kMlpThreads;
  static constexpr int WU = 32 * UT, SU = WU + 4, HDU = WU / 2;
  static constexpr int oW1 = 0, oZ = oW1 + WU * S, oB1 = oZ + kLinkMlpTile * S, oW2 = oB1 + WU,
                       oG = oW2 + WU, oRed = oG + kLinkMlpTile, oD = oRed + 2 * kLinkMlpTile;
  static constexpr int kFwdFloats = oD, kBwdFloats = oD + kLinkMlpTile * SU;
  static constexpr int IT = ND / 32, NQ = (UT + 1) / 2, NI = (IT + 1) / 2;
};

// where column c sits in a split row of half width HD
template <int HD>
__device__ __forceinline__ int split_pos(int c) {
  return (c & 1) * HD + (c >> 1);
}

// W1^T, b1 and w2 into LDS, zero beyond (d, h)
template <int ND, int UT>
__device__ __forceinline__ void mlp_stage_params(float *lds, const float *__restrict__ P, int ld_p,
                                                 int d, int h, int tid) {
  using L = MlpLds<ND, UT>;
  for (int idx = tid; idx < L::WU * ND; idx += kMlpThreads) {
    const int u = idx % L::WU, i = idx / L::WU;
    lds[L::oW1 + u * L::S + split_pos<L::HD>(i)] =
        (i < d && u < h) ? P[(long long)i * ld_p + u] : 0.0f;
  }
  for (int u = tid; u < L::WU; u += kMlpThreads) {
    lds[L::oB1 + u] = u < h ? P[(long long)d * ld_p + u] : 0.0f;
    lds[L::oW2 + u] = u < h ? P[(long long)(d + 1) * ld_p + u] : 0.0f;
  }
}

// acc[q][r] = sum_i z[pair][i] W1[i][unit], i ascending from zero: pair (wave & 1) * 32 + lane & 31
// of the tile, unit 32 ut + sweep_row(r, half) with ut = (wave >> 1) + 2 q (nothing for ut >= UT)
template <int ND, int UT>
__device__ __forceinline__ void mlp_pre(const float *lds, int groups, int wave, int lane,
                                        f32x16 *acc) {
  using L = MlpLds<ND, UT>;
  const int half = lane >> 5, col = lane & 31, pb = wave & 1, uh = wave >> 1;
  const float *b_row = lds + L::oZ + (pb * 32 + col) * L::S + half * L::HD;
  const float *a_row = lds + L::oW1 + col * L::S + half * L::HD;
#pragma unroll
  for (int q = 0; q < L::NQ; q++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[q][r] = 0.0f;
  for (int j = 0; j < groups; j++) {
    const float4 b = *reinterpret_cast<const float4 *>(b_row + 4 * j);
#pragma unroll
    for (int q = 0; q < L::NQ; q++) {
      const int ut = uh + 2 * q;
      if (ut < UT) {
        const float4 a = *reinterpret_cast<const float4 *>(a_row + 32 * ut * L::S + 4 * j);
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc[q], 0, 0, 0);
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc[q], 0, 0, 0);
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc[q], 0, 0, 0);
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc[q], 0, 0, 0);
      }
    }
  }
}

__device__ __forceinline__ float f4at(const float4 &v, int k) {
  return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w;
}

// the forward epilogue's per-lane sum: w2[u] * max(acc + b1[u], 0) over the lane's registers and
// the unit tiles ut = uh, uh + 2 (acc[q] is tile uh + 2 q), in that order, from zero
template <int ND, int UT>
__device__ __forceinline__ float mlp_lane_sum(const float *lds, const f32x16 *acc, int uh,
                                              int half) {
  using L = MlpLds<ND, UT>;
  float s = 0.0f;
#pragma unroll
  for (int q = 0; q < L::NQ; q++) {
    const int ut = uh + 2 * q;
    if (ut < UT) {
#pragma unroll
      for (int g4 = 0; g4 < 4; g4++) {
        const int u0 = 32 * ut + 8 * g4 + 4 * half;
        const float4 b1v = *reinterpret_cast<const float4 *>(lds + L::oB1 + u0);
        const float4 w2v = *reinterpret_cast<const float4 *>(lds + L::oW2 + u0);
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const float pre = acc[q][4 * g4 + k] + f4at(b1v, k);
          const float hid = fmaxf(pre, 0.0f);
          const float term = f4at(w2v, k) * hid;
          s = s + term;
        }
      }
    }
  }
  return s;
}

// a tile's scores from its lanes' sums, in the forward's order: one exchange across the lane halves,
// the two waves of a pair block through LDS (a barrier inside: every thread calls), + b2.  Thread
// tid < kLinkMlpTile returns the score of the tile's pair tid.
template <int ND, int UT>
__device__ __forceinline__ float mlp_tile_score(float *lds, float s, float b2, int wave, int lane,
                                                int tid) {
  using L = MlpLds<ND, UT>;
  const int half = lane >> 5, col = lane & 31, pb = wave & 1, uh = wave >> 1;
  s = s + __shfl_xor(s, 32, 64);
  if (half == 0) lds[L::oRed + uh * kLinkMlpTile + pb * 32 + col] = s;
  __syncthreads();
  float v = 0.0f;
  if (tid < kLinkMlpTile) {
    v = lds[L::oRed + tid];
    if (UT > 1) v = v + lds[L::oRed + kLinkMlpTile + tid];
    v = v + b2;
  }
  return v;
}

// the instantiation of a shape: row width class ND >= d, unit tiles UT with 32 UT >= h
inline int mlp_nd(int d) { return d <= 32 ? 32 : d <= 64 ? 64 : 128; }
inline int mlp_ut(int h) { return h <= 32 ? 1 : h <= 64 ? 2 : 4; }

#define MLP_BY_SHAPE(d, h, LAUNCH)                                  \
  do {                                                              \
    const int nd_ = mlp_nd(d), ut_ = mlp_ut(h);                     \
    if (nd_ == 32) {                                                \
      if (ut_ == 1) LAUNCH(32, 1); else if (ut_ == 2) LAUNCH(32, 2); else LAUNCH(32, 4);    \
    } else if (nd_ == 64) {                                         \
      if (ut_ == 1) LAUNCH(64, 1); else if (ut_ == 2) LAUNCH(64, 2); else LAUNCH(64, 4);    \
    } else {                                                        \
      if (ut_ == 1) LAUNCH(128, 1); else if (ut_ == 2) LAUNCH(128, 2); else LAUNCH(128, 4); \
    }                                                               \
  } while (0)
}  // namespace
}  // namespace pgcn
