// parallel-gcn_amd/csrc/k_gat.hip -- additive graph attention over the CSR slots of a square
// pattern, for gfx950 (GAT; the reference has no such module): K heads inside the width d, the
// per-row, per-head softmax of the slot scores fused with the weighted row gather, dropout on the
// attention weights, and the backward without float atomics.
//
// Layout (every gather kernel): one wave per work item -- a row (forward, backward row pass) or
// a column of the transposed index (backward column pass) -- cut into 64 / GL neighbour groups
// of GL lanes as slot_items.hpp describes, so 64 / GL neighbours are in flight per step (16 at
// d <= 16).  Head h owns columns [h dh, (h + 1) dh) with dh = d / K in {4 .. 128}: the hl = dh / 4
// lanes [h hl, (h + 1) hl) of every group, so a lane's float4 belongs to one head and the dot
// products (u, v, t, c) are butterflies over the lane offsets below hl.  u, v are [n][K], alpha,
// dx and the mask bits [nnz][K].  A row's per-head score maximum and exponent sum are taken in
// the gather layout (group q over slots q, q + 64 / GL, ..., then the offsets GL .. 32): one pass
// over the row's index serves every head.  The groups' sums meet in xor butterflies over the
// lane offsets GL .. 32 (every lane ends with the same bits).
// ONE = a single head over any d in 1 .. 128 (K = 1, hl = GL): the dot products are butterflies
// over the whole group with their offsets known at compile time, and a row's scalars (its score
// maximum and exponent sum, du_i) are summed one slot per lane, then over the wave.
//
// Items longer than kGatSeg slots (hub rows and hub columns of a power-law graph) are cut into
// kGatSeg-slot segments, each summed by a wave of its own in the same launch as the short items:
//   forward: a segment leaves {max[32], sum[32], its unnormalised partial row[128]}; a second
//   launch merges a row's segments in segment order (every segment's wave: the row's max and sum,
//   then its own alpha; the first segment's wave also Z);
//   backward column pass: a segment leaves {dv[32], -, its partial dP row[128]}; a second launch
//   sums a column's segments in order.  The backward row pass needs no merge: dx is per slot, and
//   du_i is summed from dx by the column pass (the wave of column i).
// da_dst / da_src go through per-workgroup partials and one reducing launch (the shape of
// k_layernorm_bwd).  Every order depends on the pattern, d and K only: bit-reproducible.
//
// Dropout: the weight of slot s, head h is kept when bit base + s K + h of the mask is set, times
// the scale in Z and in the backward; alpha holds the weights before dropout.  A null mask skips
// the factor (not a multiplication by one), so it costs nothing where there is no dropout.
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"
#include "slot_items.hpp"

#pragma clang fp contract(off)

namespace pgcn {

namespace {
constexpr int kGatDaBlocks = 256;  // da partials: one reducing chain of <= 256 per element

__device__ __forceinline__ float leaky(float x, float slope) { return x > 0.0f ? x : slope * x; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// sum over the hl lanes of a head (hl a power of two <= GL; ONE: the whole group)
template <int GL, bool ONE>
__device__ __forceinline__ float head_sum(float v, int hl) {
  if constexpr (ONE) {
#pragma unroll
    for (int off = GL / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  } else {
    for (int off = hl >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  }
  return v;
}

template <int GL>
__device__ __forceinline__ float across_groups_max(float v) {
#pragma unroll
  for (int off = GL; off < 64; off <<= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

template <int GL>
__device__ __forceinline__ float4 across_groups4(float4 a) {
  a.x = across_groups<GL>(a.x);
  a.y = across_groups<GL>(a.y);
  a.z = across_groups<GL>(a.z);
  a.w = across_groups<GL>(a.w);
  return a;
}

__device__ __forceinline__ float4 cols4(const float *p, int c0, int d) {
  float4 v;
  v.x = c0 < d ? p[c0] : 0.0f;
  v.y = c0 + 1 < d ? p[c0 + 1] : 0.0f;
  v.z = c0 + 2 < d ? p[c0 + 2] : 0.0f;
  v.w = c0 + 3 < d ? p[c0 + 3] : 0.0f;
  return v;
}

__device__ __forceinline__ float dot4(float4 a, float4 b) {
  return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w);
}

__device__ __forceinline__ void axpy4(float4 &acc, float w, float4 p) {
  acc.x += w * p.x;
  acc.y += w * p.y;
  acc.z += w * p.z;
  acc.w += w * p.w;
}

struct GatDrop {
  const uint64_t *mask;  // bit base + s K + h: the weight of slot s, head h is kept; null: all
  long long base;
  float scale;
};

// the factor m'_s^h: 1 without a mask
__device__ __forceinline__ float drop_factor(const GatDrop &dr, long long e) {
  if (!dr.mask) return 1.0f;
  const long long b = dr.base + e;
  return (dr.mask[b >> 6] >> (b & 63)) & 1ull ? dr.scale : 0.0f;
}

// a lane's place: its head (clamped on the idle lanes past column d, which store nothing) and
// whether it writes its head's scalars
template <int GL, bool ONE>
struct HeadLane {
  int q, li, c0, hd;
  bool lead;
  __device__ HeadLane(int lane, int d, int K, int hl) {
    q = lane / GL;
    li = lane % GL;
    c0 = 4 * li;
    hd = ONE ? 0 : min(li / hl, K - 1);
    lead = ONE ? li == 0 : (li % hl == 0 && c0 < d);
  }
};

// this lane's head over slots [b, e) of row i's index list: the score maximum and the sum of
// exp(score - max); every lane of the wave takes part
template <int GL, bool ONE>
__device__ __forceinline__ void slot_stats(const int *__restrict__ idx, const float *__restrict__ v,
                                           int K, int hd, float ui, float slope, int b, int e,
                                           int lane, float *m, float *s) {
  if constexpr (ONE) {  // one slot per lane, then the wave
    float mx = -INFINITY;
    for (int k = b + lane; k < e; k += kWave) mx = fmaxf(mx, leaky(ui + v[idx[k]], slope));
    mx = wave_max(mx);
    float sm = 0.0f;
    for (int k = b + lane; k < e; k += kWave) sm += expf(leaky(ui + v[idx[k]], slope) - mx);
    *m = mx;
    *s = wave_sum(sm);
  } else {  // one slot per group, then the groups
    constexpr int NB = kWave / GL;
    const int q = lane / GL;
    float mx = -INFINITY;
    for (int k = b + q; k < e; k += NB)
      mx = fmaxf(mx, leaky(ui + v[(long long)idx[k] * K + hd], slope));
    mx = across_groups_max<GL>(mx);
    float sm = 0.0f;
    for (int k = b + q; k < e; k += NB)
      sm += expf(leaky(ui + v[(long long)idx[k] * K + hd], slope) - mx);
    *m = mx;
    *s = across_groups<GL>(sm);
  }
}

// sum over slots [b, e) of m'_s w_s P_j with w_s = exp(score_s - m) / s of the lane's head,
// every lane of group 0 (and all others) ending with the wave's sum; alpha (or null) takes w_s,
// the weight before dropout
// (MASK: 0 no mask, 1 a mask, -1 the pointer tested per slot)
template <int GL, bool ONE, int MASK>
__device__ __forceinline__ float4 slot_gather_loop(const float *__restrict__ P, int ld_p, int d,
                                                   const int *__restrict__ idx,
                                                   const float *__restrict__ v, int K,
                                                   const HeadLane<GL, ONE> &hl, float ui,
                                                   float slope, int b, int e, float m, float s,
                                                   float *alpha, const GatDrop &dr) {
  constexpr int NB = kWave / GL;
  float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll 2
  for (int k = b + hl.q; k < e; k += NB) {
    const int j = idx[k];
    const long long eh = (long long)k * K + hl.hd;
    const float w = expf(leaky(ui + v[(long long)j * K + hl.hd], slope) - m) / s;
    if (alpha && hl.lead) alpha[eh] = w;
    axpy4(acc, (MASK < 0 ? dr.mask != nullptr : MASK > 0) ? w * drop_factor(dr, eh) : w,
          row4(P + (long long)j * ld_p, hl.c0, d, hl.c0 < d));
  }
  return across_groups4<GL>(acc);
}

// (ONE: the null-mask test stands outside the slot loop -- inside it the d = 128 forward measured
// 9 % slower than without the test; the many-head kernels keep one loop body, two of them cost
// a wave of occupancy there)
template <int GL, bool ONE>
__device__ __forceinline__ float4 slot_gather(const float *__restrict__ P, int ld_p, int d,
                                              const int *__restrict__ idx,
                                              const float *__restrict__ v, int K,
                                              const HeadLane<GL, ONE> &hl, float ui, float slope,
                                              int b, int e, float m, float s, float *alpha,
                                              const GatDrop &dr) {
  if constexpr (!ONE)
    return slot_gather_loop<GL, ONE, -1>(P, ld_p, d, idx, v, K, hl, ui, slope, b, e, m, s, alpha,
                                         dr);
  else
    return dr.mask ? slot_gather_loop<GL, ONE, 1>(P, ld_p, d, idx, v, K, hl, ui, slope, b, e, m, s,
                                                  alpha, dr)
                   : slot_gather_loop<GL, ONE, 0>(P, ld_p, d, idx, v, K, hl, ui, slope, b, e, m, s,
                                                  alpha, dr);
}
}  // namespace

// u[i][h] = P_i[h] . a_dst[h], v[i][h] = P_i[h] . a_src[h]: one row per group of GL lanes
template <int GL, bool ONE>
__global__ __launch_bounds__(kItemThreads) void k_gat_scores(
    const float *__restrict__ P, int ld_p, int n, int d, int K, int hlanes,
    const float *__restrict__ a_dst, const float *__restrict__ a_src, float *__restrict__ u,
    float *__restrict__ v) {
  constexpr int RPB = kItemThreads / GL;
  if constexpr (ONE) K = 1;  // (the [..][K] indices fold to the one-head ones at compile time)
  const HeadLane<GL, ONE> hl(threadIdx.x % kWave, d, K, hlanes);
  const int grp = threadIdx.x / GL, c0 = hl.c0;
  const float4 ad = cols4(a_dst, c0, d), as = cols4(a_src, c0, d);
  for (long long base = (long long)blockIdx.x * RPB; base < n; base += (long long)gridDim.x * RPB) {
    const long long r = base + grp;
    const bool live = r < n;
    const float4 p = row4(P + r * ld_p, c0, d, live && c0 < d);
    const float su = head_sum<GL, ONE>(dot4(p, ad), hlanes);
    const float sv = head_sum<GL, ONE>(dot4(p, as), hlanes);
    if (live && hl.lead) {
      u[r * K + hl.hd] = su;
      v[r * K + hl.hd] = sv;
    }
  }
}

// items [0, n): the rows of at most kGatSeg slots, whole; items [n, n + n_row_segs): the long
// rows' segments, which leave {max, sum, unnormalised partial row} in row_ws
template <int GL, bool ONE>
__global__ __launch_bounds__(kItemThreads) void k_gat_fwd(
    const GatPattern g, const float *__restrict__ P, int ld_p, const float *__restrict__ u,
    const float *__restrict__ v, float slope, float *__restrict__ Z, int ld_z, int d, int K,
    int hlanes, float *__restrict__ alpha, const GatDrop dr) {
  const int lane = threadIdx.x % kWave;
  if constexpr (ONE) K = 1;  // (the [..][K] indices fold to the one-head ones at compile time)
  const HeadLane<GL, ONE> hl(lane, d, K, hlanes);
  const int c0 = hl.c0;
  const long long items = (long long)g.n + g.n_row_segs;
  for (long long it = first_item(); it < items; it += item_stride()) {
    if (it < g.n) {
      const int i = (int)it, b = g.indptr[i], e = g.indptr[i + 1];
      if (e - b > kGatSeg) continue;
      float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (e > b) {
        const float ui = u[(long long)i * K + hl.hd];
        float m, s;
        slot_stats<GL, ONE>(g.indices, v, K, hl.hd, ui, slope, b, e, lane, &m, &s);
        z = slot_gather<GL, ONE>(P, ld_p, d, g.indices, v, K, hl, ui, slope, b, e, m, s, alpha, dr);
      }
      if (lane < GL && c0 < d) *reinterpret_cast<float4 *>(Z + (long long)i * ld_z + c0) = z;
    } else {
      const long long t = it - g.n;
      const int4 sg = g.row_segs[t];
      const float ui = u[(long long)sg.x * K + hl.hd];
      float m, s;
      slot_stats<GL, ONE>(g.indices, v, K, hl.hd, ui, slope, sg.y, sg.z, lane, &m, &s);
      const float4 z = slot_gather<GL, ONE>(P, ld_p, d, g.indices, v, K, hl, ui, slope, sg.y, sg.z,
                                            m, 1.0f, nullptr, dr);
      float *ws = g.row_ws + t * kGatWsStride;
      if (lane < GL && hl.lead) {
        ws[hl.hd] = m;
        ws[kGatMaxHeads + hl.hd] = s;
      }
      if (lane < GL && c0 < d) *reinterpret_cast<float4 *>(ws + 2 * kGatMaxHeads + c0) = z;
    }
  }
}

// one wave per segment of a long row: the row's max and sum from its segments in order, the
// segment's alpha, and (the row's first segment) Z
template <int GL, bool ONE>
__global__ __launch_bounds__(kItemThreads) void k_gat_fwd_merge(
    const GatPattern g, const float *__restrict__ u, const float *__restrict__ v, float slope,
    float *__restrict__ Z, int ld_z, int d, int K, int hlanes, float *__restrict__ alpha) {
  constexpr int NB = kWave / GL;
  const int lane = threadIdx.x % kWave;
  if constexpr (ONE) K = 1;  // (the [..][K] indices fold to the one-head ones at compile time)
  const HeadLane<GL, ONE> hl(lane, d, K, hlanes);
  const int c0 = hl.c0;
  for (long long t = first_item(); t < g.n_row_segs; t += item_stride()) {
    const int4 sg = g.row_segs[t];
    const int i = sg.x, first = sg.w;
    const int nseg = (g.indptr[i + 1] - g.indptr[i] + kGatSeg - 1) / kGatSeg;
    const float *ws = g.row_ws + (long long)first * kGatWsStride + hl.hd;
    float m = -INFINITY;
    for (int k = 0; k < nseg; k++) m = fmaxf(m, ws[(long long)k * kGatWsStride]);
    float s = 0.0f;
    for (int k = 0; k < nseg; k++)
      s += ws[(long long)k * kGatWsStride + kGatMaxHeads] *
           expf(ws[(long long)k * kGatWsStride] - m);
    if (alpha) {
      const float ui = u[(long long)i * K + hl.hd];
      if constexpr (ONE) {
        for (int k = sg.y + lane; k < sg.z; k += kWave)
          alpha[k] = expf(leaky(ui + v[g.indices[k]], slope) - m) / s;
      } else {
        for (int k = sg.y + hl.q; k < sg.z; k += NB)
          if (hl.lead)
            alpha[(long long)k * K + hl.hd] =
                expf(leaky(ui + v[(long long)g.indices[k] * K + hl.hd], slope) - m) / s;
      }
    }
    if (t == first && lane < GL && c0 < d) {
      float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      for (int k = 0; k < nseg; k++) {
        const float *w = ws + (long long)k * kGatWsStride;
        axpy4(z, expf(w[0] - m),
              *reinterpret_cast<const float4 *>(w - hl.hd + 2 * kGatMaxHeads + c0));
      }
      z.x /= s;
      z.y /= s;
      z.z /= s;
      z.w /= s;
      *reinterpret_cast<float4 *>(Z + (long long)i * ld_z + c0) = z;
    }
  }
}

// backward row pass: dx_s^h = alpha_s^h (m'_s^h G_i[h] . P_j[h] - G_i[h] . Z_i[h])
// leaky'(u_i^h + v_j^h) for every slot of the item (items as in k_gat_fwd; a long row's segments
// need no merge)
template <int GL, bool ONE>
__global__ __launch_bounds__(kItemThreads) void k_gat_bwd_rows(
    const GatPattern g, const float *__restrict__ P, int ld_p, const float *__restrict__ u,
    const float *__restrict__ v, float slope, const float *__restrict__ alpha,
    const float *__restrict__ Z, int ld_z, const float *__restrict__ G, int ld_g, int d, int K,
    int hlanes, const GatDrop dr, float *__restrict__ dx) {
  constexpr int NB = kWave / GL;
  const int lane = threadIdx.x % kWave;
  if constexpr (ONE) K = 1;  // (the [..][K] indices fold to the one-head ones at compile time)
  const HeadLane<GL, ONE> hl(lane, d, K, hlanes);
  const int c0 = hl.c0;
  const long long items = (long long)g.n + g.n_row_segs;
  for (long long it = first_item(); it < items; it += item_stride()) {
    int i, b, e;
    if (it < g.n) {
      i = (int)it;
      b = g.indptr[i];
      e = g.indptr[i + 1];
      if (e - b > kGatSeg) continue;
    } else {
      const int4 sg = g.row_segs[it - g.n];
      i = sg.x;
      b = sg.y;
      e = sg.z;
    }
    if (e <= b) continue;
    const float4 gi = row4(G + (long long)i * ld_g, c0, d, c0 < d);
    const float4 zi = row4(Z + (long long)i * ld_z, c0, d, c0 < d);
    const float c = head_sum<GL, ONE>(dot4(gi, zi), hlanes), ui = u[(long long)i * K + hl.hd];
    // (the same trip count for every group: the head sums run under uniform control flow)
    for (int k0 = b; k0 < e; k0 += NB) {
      const int k = k0 + hl.q;
      const bool on = k < e;
      const int j = on ? g.indices[k] : i;
      float t = head_sum<GL, ONE>(
          dot4(gi, row4(P + (long long)j * ld_p, c0, d, on && c0 < d)), hlanes);
      if (on && hl.lead) {
        const long long eh = (long long)k * K + hl.hd;
        if (dr.mask) t = drop_factor(dr, eh) * t;
        dx[eh] = alpha[eh] * (t - c) * (ui + v[(long long)j * K + hl.hd] > 0.0f ? 1.0f : slope);
      }
    }
  }
}

namespace {
// one item of the column pass: slots [b, e) of the transposed index; acc = sum alpha_s^h m'_s^h
// G_row[h], dv^h = sum dx_s^h, both over the groups (every lane ends with the wave's sums)
template <int GL, bool ONE>
__device__ __forceinline__ float4 col_gather(const GatPattern &g, const float *__restrict__ alpha,
                                             const float *__restrict__ dx,
                                             const float *__restrict__ G, int ld_g, int d, int K,
                                             const HeadLane<GL, ONE> &hl, const GatDrop &dr, int b,
                                             int e, float *dv_out) {
  constexpr int NB = kWave / GL;
  float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float dv = 0.0f;
#pragma unroll 2
  for (int o = b + hl.q; o < e; o += NB) {
    const int r = g.csc_row[o];
    const long long eh = (long long)g.csc_pos[o] * K + hl.hd;
    axpy4(acc, dr.mask ? alpha[eh] * drop_factor(dr, eh) : alpha[eh],
          row4(G + (long long)r * ld_g, hl.c0, d, hl.c0 < d));
    dv += dx[eh];
  }
  *dv_out = across_groups<GL>(dv);
  return across_groups4<GL>(acc);
}

// the final write of column j: du_j^h from row j's dx (ONE: one slot per lane, then the wave),
// then dP_j = acc + du_j a_dst + dv_j a_src
template <int GL, bool ONE>
__device__ __forceinline__ void col_finish(const GatPattern &g, int j, float4 acc, float dv,
                                           const float *__restrict__ dx,
                                           const float *__restrict__ a_dst,
                                           const float *__restrict__ a_src, int d, int K,
                                           const HeadLane<GL, ONE> &hl, float *__restrict__ dP,
                                           int ld_dp, float *__restrict__ du_out,
                                           float *__restrict__ dv_out, int lane) {
  constexpr int NB = kWave / GL;
  const int c0 = hl.c0;
  float du = 0.0f;
  if constexpr (ONE) {
    for (int k = g.indptr[j] + lane; k < g.indptr[j + 1]; k += kWave) du += dx[k];
    du = wave_sum(du);
  } else {
    for (int k = g.indptr[j] + hl.q; k < g.indptr[j + 1]; k += NB) du += dx[(long long)k * K + hl.hd];
    du = across_groups<GL>(du);
  }
  if (lane < GL && hl.lead) {
    du_out[(long long)j * K + hl.hd] = du;
    dv_out[(long long)j * K + hl.hd] = dv;
  }
  if (lane < GL && c0 < d) {
    const float4 ad = cols4(a_dst, c0, d), as = cols4(a_src, c0, d);
    float4 o;
    o.x = (acc.x + du * ad.x) + dv * as.x;
    o.y = (acc.y + du * ad.y) + dv * as.y;
    o.z = (acc.z + du * ad.z) + dv * as.z;
    o.w = (acc.w + du * ad.w) + dv * as.w;
    *reinterpret_cast<float4 *>(dP + (long long)j * ld_dp + c0) = o;
  }
}
}  // namespace

// items [0, n): the columns of at most kGatSeg incoming slots, whole; items [n, n + n_col_segs):
// the long columns' segments, which leave {dv, partial row} in col_ws
template <int GL, bool ONE>
__global__ __launch_bounds__(kItemThreads) void k_gat_bwd_cols(
    const GatPattern g, const float *__restrict__ alpha, const float *__restrict__ dx,
    const float *__restrict__ G, int ld_g, const float *__restrict__ a_dst,
    const float *__restrict__ a_src, int d, int K, int hlanes, const GatDrop dr,
    float *__restrict__ dP, int ld_dp, float *__restrict__ du, float *__restrict__ dv,
    float *__restrict__ col_ws) {
  const int lane = threadIdx.x % kWave;
  if constexpr (ONE) K = 1;  // (the [..][K] indices fold to the one-head ones at compile time)
  const HeadLane<GL, ONE> hl(lane, d, K, hlanes);
  const int c0 = hl.c0;
  const long long items = (long long)g.n + g.n_col_segs;
  for (long long it = first_item(); it < items; it += item_stride()) {
    if (it < g.n) {
      const int j = (int)it, b = g.csc_ptr[j], e = g.csc_ptr[j + 1];
      if (e - b > kGatSeg) continue;
      float dvj;
      const float4 acc = col_gather<GL, ONE>(g, alpha, dx, G, ld_g, d, K, hl, dr, b, e, &dvj);
      col_finish<GL, ONE>(g, j, acc, dvj, dx, a_dst, a_src, d, K, hl, dP, ld_dp, du, dv, lane);
    } else {
      const long long t = it - g.n;
      const int4 sg = g.col_segs[t];
      float dvj;
      const float4 acc =
          col_gather<GL, ONE>(g, alpha, dx, G, ld_g, d, K, hl, dr, sg.y, sg.z, &dvj);
      float *ws = col_ws + t * kGatWsStride;
      if (lane < GL && hl.lead) ws[hl.hd] = dvj;
      if (lane < GL && c0 < d) *reinterpret_cast<float4 *>(ws + 2 * kGatMaxHeads + c0) = acc;
    }
  }
}

// one wave per long column: its segments' partials in segment order, then the final write
template <int GL, bool ONE>
__global__ __launch_bounds__(kItemThreads) void k_gat_bwd_colmerge(
    const GatPattern g, const float *__restrict__ dx, const float *__restrict__ a_dst,
    const float *__restrict__ a_src, int d, int K, int hlanes, float *__restrict__ dP, int ld_dp,
    float *__restrict__ du, float *__restrict__ dv, const float *__restrict__ col_ws) {
  const int lane = threadIdx.x % kWave;
  if constexpr (ONE) K = 1;  // (the [..][K] indices fold to the one-head ones at compile time)
  const HeadLane<GL, ONE> hl(lane, d, K, hlanes);
  const int c0 = hl.c0;
  for (long long t = first_item(); t < g.n_long_cols; t += item_stride()) {
    const int j = g.long_cols[t].x, first = g.long_cols[t].y;
    const int nseg = (g.csc_ptr[j + 1] - g.csc_ptr[j] + kGatSeg - 1) / kGatSeg;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float dvj = 0.0f;
    for (int k = 0; k < nseg; k++) {
      const float *w = col_ws + (long long)(first + k) * kGatWsStride;
      dvj += w[hl.hd];
      if (c0 < d) {
        const float4 p = *reinterpret_cast<const float4 *>(w + 2 * kGatMaxHeads + c0);
        acc.x += p.x;
        acc.y += p.y;
        acc.z += p.z;
        acc.w += p.w;
      }
    }
    col_finish<GL, ONE>(g, j, acc, dvj, dx, a_dst, a_src, d, K, hl, dP, ld_dp, du, dv, lane);
  }
}

// this workgroup's rows of sum du_i^h P_i[h] and sum dv_i^h P_i[h] (a lane's own head of du, dv
// [n][K]): per lane group in row order, then the groups in group order (LDS), into partial
// [block][2][ldp].  (No ONE form: at K = 1 the head index is 0 and nothing else depends on it.)
template <int GL>
__global__ __launch_bounds__(kItemThreads) void k_gat_da(
    const float *__restrict__ P, int ld_p, int n, int d, int K, int hlanes,
    const float *__restrict__ du, const float *__restrict__ dv, float *__restrict__ partial,
    int ldp) {
  constexpr int RPB = kItemThreads / GL;
  constexpr int W = GL * 4;
  __shared__ __align__(16) float sh[RPB * 2 * W];
  const int li = threadIdx.x % GL, grp = threadIdx.x / GL, c0 = 4 * li;
  const int hd = min(li / hlanes, K - 1);
  float4 ad = make_float4(0.0f, 0.0f, 0.0f, 0.0f), as = ad;
  for (long long r = (long long)blockIdx.x * RPB + grp; r < n; r += (long long)gridDim.x * RPB) {
    const float4 p = row4(P + r * ld_p, c0, d, c0 < d);
    axpy4(ad, du[r * K + hd], p);
    axpy4(as, dv[r * K + hd], p);
  }
  *reinterpret_cast<float4 *>(&sh[(grp * 2 + 0) * W + c0]) = ad;
  *reinterpret_cast<float4 *>(&sh[(grp * 2 + 1) * W + c0]) = as;
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * W; i += kItemThreads) {
    const int c = i % W;
    if (c >= ldp) continue;
    float s = 0.0f;
    for (int q = 0; q < RPB; q++) s += sh[q * 2 * W + i];
    partial[((long long)blockIdx.x * 2 + i / W) * ldp + c] = s;
  }
}

// da[k][c] = the nb partials [2][ldp] summed in block order
__global__ __launch_bounds__(kItemThreads) void k_gat_da_reduce(const float *__restrict__ partial,
                                                                int nb, int ldp, int d,
                                                                float *__restrict__ da) {
  const int i = blockIdx.x * kItemThreads + threadIdx.x;
  if (i >= 2 * ldp) return;
  const int c = i % ldp;
  if (c >= d) return;
  float s = 0.0f;
#pragma unroll 8
  for (int b = 0; b < nb; b++) s += partial[(long long)b * 2 * ldp + i];
  da[(i / ldp) * d + c] = s;
}

static int gat_da_blocks(int n, int d) {
  return (int)std::max<long long>(
      1, std::min<long long>(ceil_div(n, kItemThreads / item_gl(d)), kGatDaBlocks));
}

// KERNEL<GL, ONE>: ONE where `heads` in scope is 1
#define GAT_DISPATCH_ONE(KERNEL, ONE, grid, s, ...)                                               \
  do {                                                                                            \
    switch (item_gl(d)) {                                                                         \
      case 1: PGCN_LAUNCH((KERNEL<1, ONE>), grid, dim3(kItemThreads), 0, s, __VA_ARGS__); break;   \
      case 2: PGCN_LAUNCH((KERNEL<2, ONE>), grid, dim3(kItemThreads), 0, s, __VA_ARGS__); break;   \
      case 4: PGCN_LAUNCH((KERNEL<4, ONE>), grid, dim3(kItemThreads), 0, s, __VA_ARGS__); break;   \
      case 8: PGCN_LAUNCH((KERNEL<8, ONE>), grid, dim3(kItemThreads), 0, s, __VA_ARGS__); break;   \
      case 16: PGCN_LAUNCH((KERNEL<16, ONE>), grid, dim3(kItemThreads), 0, s, __VA_ARGS__); break; \
      default: PGCN_LAUNCH((KERNEL<32, ONE>), grid, dim3(kItemThreads), 0, s, __VA_ARGS__); break; \
    }                                                                                             \
  } while (0)
#define GAT_DISPATCH(KERNEL, grid, s, ...)                    \
  do {                                                        \
    if (heads > 1)                                            \
      GAT_DISPATCH_ONE(KERNEL, false, grid, s, __VA_ARGS__);  \
    else                                                      \
      GAT_DISPATCH_ONE(KERNEL, true, grid, s, __VA_ARGS__);   \
  } while (0)

bool gat_heads_ok(int d, int heads) {
  if (d < 1 || d > kGatMaxWidth || heads < 1) return false;
  if (heads == 1) return true;
  if (d % heads != 0) return false;
  const int dh = d / heads;
  return dh >= 4 && dh <= kGatMaxWidth && (dh & (dh - 1)) == 0;
}

// lanes per head: dh / 4 (one head: the whole group)
static int gat_head_lanes(int d, int heads) { return heads > 1 ? d / heads / 4 : item_gl(d); }

void launch_gat_scores(const float *P, int ld_p, int n, int d, int heads, const float *a_dst,
                       const float *a_src, float *u, float *v, hipStream_t s) {
  PGCN_CHECK(gat_heads_ok(d, heads) && n >= 0, PGCN_E_INVALID,
             "gat_scores: 1 <= d <= 128, heads dividing d into widths of 4 .. 128 (a power of two)");
  if (n == 0) return;
  const dim3 grid((unsigned)std::min<long long>(ceil_div(n, kItemThreads / item_gl(d)),
                                                kItemMaxBlocks));
  GAT_DISPATCH(k_gat_scores, grid, s, P, ld_p, n, d, heads, gat_head_lanes(d, heads), a_dst, a_src,
               u, v);
}

void launch_gat_fwd(const GatPattern &g, const float *P, int ld_p, const float *u, const float *v,
                    float slope, float *Z, int ld_z, int d, int heads, const uint64_t *drop_mask,
                    long long drop_base, float drop_scale, float *alpha, hipStream_t s) {
  PGCN_CHECK(gat_heads_ok(d, heads) && g.n >= 0, PGCN_E_INVALID,
             "gat_fwd: 1 <= d <= 128, heads dividing d into widths of 4 .. 128 (a power of two)");
  if (g.n == 0) return;
  note_path(KP_GAT_FWD);
  if (heads > 1) note_path(KP_GAT_HEADS);
  const int hl = gat_head_lanes(d, heads);
  const GatDrop dr{drop_mask, drop_base, drop_scale};
  GAT_DISPATCH(k_gat_fwd, item_grid((long long)g.n + g.n_row_segs), s, g, P, ld_p, u, v, slope, Z,
               ld_z, d, heads, hl, alpha, dr);
  if (g.n_row_segs > 0)
    GAT_DISPATCH(k_gat_fwd_merge, item_grid(g.n_row_segs), s, g, u, v, slope, Z, ld_z, d, heads, hl,
                 alpha);
}

namespace {
struct GatBwdWs {
  size_t dx, du, dv, col_ws, part, floats;
};
size_t up4(size_t x) { return (x + 3) / 4 * 4; }
GatBwdWs gat_bwd_layout(const GatPattern &g, int d, int heads) {
  GatBwdWs w;
  w.dx = 0;
  w.du = w.dx + up4((size_t)g.nnz * heads);
  w.dv = w.du + up4((size_t)g.n * heads);
  w.col_ws = w.dv + up4((size_t)g.n * heads);
  w.part = w.col_ws + (size_t)g.n_col_segs * kGatWsStride;
  w.floats = w.part + (size_t)gat_da_blocks(g.n, d) * 2 * (size_t)((d + 3) / 4 * 4);
  return w;
}
}  // namespace

size_t gat_bwd_workspace(const GatPattern &g, int d, int heads) {
  if (g.n <= 0 || !gat_heads_ok(d, heads)) return 0;
  return gat_bwd_layout(g, d, heads).floats * sizeof(float);
}

void launch_gat_bwd(const GatPattern &g, const float *P, int ld_p, const float *u, const float *v,
                    float slope, const float *alpha, const float *Z, int ld_z, const float *G,
                    int ld_g, const float *a_dst, const float *a_src, float *dP, int ld_dp, int d,
                    int heads, const uint64_t *drop_mask, long long drop_base, float drop_scale,
                    float *da, void *workspace, hipStream_t s) {
  PGCN_CHECK(gat_heads_ok(d, heads) && g.n >= 0, PGCN_E_INVALID,
             "gat_bwd: 1 <= d <= 128, heads dividing d into widths of 4 .. 128 (a power of two)");
  if (g.n == 0) return;
  note_path(KP_GAT_BWD);
  if (heads > 1) note_path(KP_GAT_HEADS);
  const GatBwdWs w = gat_bwd_layout(g, d, heads);
  float *ws = static_cast<float *>(workspace);
  float *dx = ws + w.dx, *du = ws + w.du, *dv = ws + w.dv, *col_ws = ws + w.col_ws;
  float *partial = ws + w.part;
  const int hl = gat_head_lanes(d, heads);
  const GatDrop dr{drop_mask, drop_base, drop_scale};
  GAT_DISPATCH(k_gat_bwd_rows, item_grid((long long)g.n + g.n_row_segs), s, g, P, ld_p, u, v, slope,
               alpha, Z, ld_z, G, ld_g, d, heads, hl, dr, dx);
  GAT_DISPATCH(k_gat_bwd_cols, item_grid((long long)g.n + g.n_col_segs), s, g, alpha, dx, G, ld_g,
               a_dst, a_src, d, heads, hl, dr, dP, ld_dp, du, dv, col_ws);
  if (g.n_long_cols > 0)
    GAT_DISPATCH(k_gat_bwd_colmerge, item_grid(g.n_long_cols), s, g, dx, a_dst, a_src, d, heads, hl,
                 dP, ld_dp, du, dv, col_ws);
  const int nb = gat_da_blocks(g.n, d), ldp = (d + 3) / 4 * 4;
  ITEM_DISPATCH(k_gat_da, dim3((unsigned)nb), s, P, ld_p, g.n, d, heads, hl, du, dv, partial, ldp);
  PGCN_LAUNCH(k_gat_da_reduce, dim3((unsigned)ceil_div(2 * ldp, kItemThreads)), dim3(kItemThreads),
              0, s, partial, nb, ldp, d, da);
}

}  // namespace pgcn
