// parallel-gcn_amd/csrc/k_link.hip -- link prediction's dot-product decoder over a node variable,
// for gfx950 (the reference has no pair-level model): scores_e = H[src_e] . H[dst_e] for a list of
// node pairs, and the backward dH_i = sum over the pairs (e, o) that touch node i of g_e H[o],
// without float atomics.
//
// Layout: slot_items.hpp's, shared with k_gat.hip and k_sage.hip.
//   forward: GL lanes per pair, 64 / GL pairs per wave; lane li multiplies the float4s at column
//   4 li of the two rows and adds the four products left to right, and the lanes of a group meet in
//   xor butterflies over the offsets 1 .. GL / 2.
//   backward: one wave per node over its incidence entries (LinkIndex: {pair, other endpoint} in
//   ascending pair order); group q takes entries q, q + 64 / GL, ..., each lane adding g_e times
//   its float4 of H[other], and the groups meet in across_groups.  The chain of an entry is
//   inc_pair -> G[e] and inc_other -> H row: the loop is unrolled by two, so the index loads of the
//   next entry are issued before the rows of this one are consumed.
// Nodes with more than kGatSeg entries go through the index's segment list: each segment is a wave
// of its own in the same launch and leaves its partial row in the index's workspace; a second
// launch adds a node's partials in segment order.  Every order depends on the pair list and d
// only: two calls give the same bits.
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"
#include "slot_items.hpp"

#pragma clang fp contract(off)

namespace pgcn {

// item w: the pairs w * (64 / GL) .. + 64 / GL - 1
template <int GL>
__global__ __launch_bounds__(kItemThreads) void k_link_score_fwd(
    const int *__restrict__ src, const int *__restrict__ dst, long long n_pairs,
    const float *__restrict__ H, int ld_h, int d, float *__restrict__ scores, int ld_s) {
  constexpr int NB = kWave / GL;
  const int lane = threadIdx.x % kWave, q = lane / GL, c0 = 4 * (lane % GL);
  const long long items = (n_pairs + NB - 1) / NB;
  for (long long it = first_item(); it < items; it += item_stride()) {
    const long long e = it * NB + q;
    const bool live = e < n_pairs;
    float s = 0.0f;
    if (live && c0 < d) {
      const float4 a = row4(H + (long long)src[e] * ld_h, c0, d, true);
      const float4 b = row4(H + (long long)dst[e] * ld_h, c0, d, true);
      s = a.x * b.x;
      s += a.y * b.y;
      s += a.z * b.z;
      s += a.w * b.w;
    }
#pragma unroll
    for (int off = 1; off < GL; off <<= 1) s += __shfl_xor(s, off, 64);
    if (live && c0 == 0)
      *reinterpret_cast<float4 *>(scores + e * ld_s) = make_float4(s, 0.0f, 0.0f, 0.0f);
  }
}

namespace {
// entries [b, e) of the incidence index: sum of G[pair][0] * H[other] over the groups (every lane
// ends with the wave's sums)
template <int GL>
__device__ __forceinline__ float4 entries_sum(const LinkIndex &l, const float *__restrict__ H,
                                              int ld_h, int d, const float *__restrict__ G,
                                              int ld_g, int b, int e, int lane) {
  constexpr int NB = kWave / GL;
  const int q = lane / GL, c0 = 4 * (lane % GL);
  float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (c0 < d) {
#pragma unroll 2
    for (int k = b + q; k < e; k += NB) {
      const int p = l.inc_pair[k], o = l.inc_other[k];
      const float g = G[(long long)p * ld_g];
      const float4 h = row4(H + (long long)o * ld_h, c0, d, true);
      acc.x += g * h.x;
      acc.y += g * h.y;
      acc.z += g * h.z;
      acc.w += g * h.w;
    }
  }
  acc.x = across_groups<GL>(acc.x);
  acc.y = across_groups<GL>(acc.y);
  acc.z = across_groups<GL>(acc.z);
  acc.w = across_groups<GL>(acc.w);
  return acc;
}

// the float4 at column c0 of a row of width d: zero from column d on, whatever the sums hold there
__device__ __forceinline__ void store_row4(float *p, int c0, int d, float4 v) {
  if (c0 + 1 >= d) v.y = 0.0f;
  if (c0 + 2 >= d) v.z = 0.0f;
  if (c0 + 3 >= d) v.w = 0.0f;
  *reinterpret_cast<float4 *>(p + c0) = v;
}
}  // namespace

// items [0, n): the nodes of at most kGatSeg entries, whole (none: a zero row); items [n, n +
// n_segs): the long nodes' segments, which leave their partial rows in l.ws
template <int GL>
__global__ __launch_bounds__(kItemThreads) void k_link_score_bwd(
    const LinkIndex l, const float *__restrict__ H, int ld_h, int d, const float *__restrict__ G,
    int ld_g, float *__restrict__ dH, int ld_dh) {
  const int lane = threadIdx.x % kWave, c0 = 4 * (lane % GL);
  const long long items = (long long)l.n + l.n_segs;
  for (long long it = first_item(); it < items; it += item_stride()) {
    if (it < l.n) {
      const int i = (int)it, b = l.inc_ptr[i], e = l.inc_ptr[i + 1];
      if (e - b > kGatSeg) continue;
      const float4 acc = entries_sum<GL>(l, H, ld_h, d, G, ld_g, b, e, lane);
      if (lane < GL && c0 < d) store_row4(dH + (long long)i * ld_dh, c0, d, acc);
    } else {
      const long long t = it - l.n;
      const int4 sg = l.segs[t];
      const float4 acc = entries_sum<GL>(l, H, ld_h, d, G, ld_g, sg.y, sg.z, lane);
      if (lane < GL && c0 < d)
        *reinterpret_cast<float4 *>(l.ws + t * kLinkWsStride + c0) = acc;
    }
  }
}

// one wave per long node: its segments' partials in segment order
template <int GL>
__global__ __launch_bounds__(kItemThreads) void k_link_score_bwd_merge(const LinkIndex l, int d,
                                                                       float *__restrict__ dH,
                                                                       int ld_dh) {
  const int lane = threadIdx.x % kWave, c0 = 4 * (lane % GL);
  for (long long t = first_item(); t < l.n_long; t += item_stride()) {
    if (lane >= GL || c0 >= d) continue;
    const int i = l.longs[t].x, first = l.longs[t].y;
    const int nseg = (l.inc_ptr[i + 1] - l.inc_ptr[i] + kGatSeg - 1) / kGatSeg;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int k = 0; k < nseg; k++) {
      const float4 p =
          *reinterpret_cast<const float4 *>(l.ws + (long long)(first + k) * kLinkWsStride + c0);
      acc.x += p.x;
      acc.y += p.y;
      acc.z += p.z;
      acc.w += p.w;
    }
    store_row4(dH + (long long)i * ld_dh, c0, d, acc);
  }
}

void launch_link_score_fwd(const LinkIndex &l, const float *H, int ld_h, int d, float *scores,
                           int ld_s, hipStream_t s) {
  PGCN_CHECK(d >= 1 && d <= kLinkMaxWidth && l.n >= 0 && l.n_pairs >= 0, PGCN_E_INVALID,
             "link_score_fwd: 1 <= d <= 128");
  if (l.n_pairs == 0) return;
  note_path(KP_LINK_FWD);
  const long long items = ceil_div(l.n_pairs, (long long)(kWave / item_gl(d)));
  ITEM_DISPATCH(k_link_score_fwd, item_grid(items), s, l.src, l.dst, l.n_pairs, H, ld_h, d, scores,
                ld_s);
}

void launch_link_score_bwd(const LinkIndex &l, const float *H, int ld_h, int d, const float *G,
                           int ld_g, float *dH, int ld_dh, hipStream_t s) {
  PGCN_CHECK(d >= 1 && d <= kLinkMaxWidth && l.n >= 0 && l.n_pairs >= 0, PGCN_E_INVALID,
             "link_score_bwd: 1 <= d <= 128");
  if (l.n_pairs == 0 || l.n == 0) return;
  note_path(KP_LINK_BWD);
  ITEM_DISPATCH(k_link_score_bwd, item_grid((long long)l.n + l.n_segs), s, l, H, ld_h, d, G, ld_g,
                dH, ld_dh);
  if (l.n_long > 0) ITEM_DISPATCH(k_link_score_bwd_merge, item_grid(l.n_long), s, l, d, dH, ld_dh);
}

}  // namespace pgcn
