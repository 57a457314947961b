// parallel-gcn_amd/csrc/k_sage.hip -- GraphSAGE's max aggregator over the CSR slots of a square
// pattern, for gfx950 (the reference has no such module): out_i[c] = add_i[c] + max over row i's
// slots of in_j[c] with the winning slot recorded, and the backward that routes every gradient
// element to the one slot that won, without float atomics.  (The mean aggregator is a GraphSum
// with values 1 / len_i: DevGraph on other scales, no kernel here.)
//
// Layout: slot_items.hpp's, shared with k_gat.hip.  One wave per work item -- a row (forward) or
// a column of the transposed index (backward) -- cut into 64 / GL neighbour groups of GL lanes;
// group q takes slots q, q + 64 / GL, ... of the item in CSR order.
//   forward: a lane keeps {value, slot} per component; a candidate replaces the incumbent only
//   when strictly greater, so the lowest slot of equal values stays.  The groups meet in xor
//   butterflies over the lane offsets GL .. 32 under "greater value, else lower slot", which is
//   associative and commutative: the result does not depend on how slots were dealt to groups.
//   backward: a lane loads the int4 of arg_i and the float4 of G_i of every slot (i, j) into its
//   column j, keeps the components whose arg is that slot, and the groups are summed by
//   butterflies.
// Items longer than kGatSeg slots go through the graph's segment lists (DevGraph::gat_pattern):
// each segment is a wave of its own in the same launch and leaves its partial in the graph's
// workspace (SageWs); a second launch merges an item's segments in segment order by the same
// rule (forward) or sums them in order (backward).  Every order depends on the pattern and d
// only: two calls give the same bits.
#include <algorithm>
#include <climits>

#include "common.hpp"
#include "kernels.hpp"
#include "slot_items.hpp"

#pragma clang fp contract(off)

namespace pgcn {

namespace {
// a lane's running maxima: empty = {-inf, INT_MAX}
struct Best4 {
  float4 v;
  int4 s;
};

__device__ __forceinline__ Best4 best_empty() {
  Best4 b;
  b.v = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
  b.s = make_int4(INT_MAX, INT_MAX, INT_MAX, INT_MAX);
  return b;
}

// a later slot of the same lane: strictly greater only
__device__ __forceinline__ void take_next(float &v, int &s, float ov, int os) {
  if (ov > v) {
    v = ov;
    s = os;
  }
}

// another group's or segment's winner: greater value, else lower slot
__device__ __forceinline__ void take_other(float &v, int &s, float ov, int os) {
  if (ov > v || (ov == v && os < s)) {
    v = ov;
    s = os;
  }
}

template <int GL>
__device__ __forceinline__ void across_groups_best(float &v, int &s) {
#pragma unroll
  for (int off = GL; off < 64; off <<= 1) {
    const float ov = __shfl_xor(v, off, 64);
    const int os = __shfl_xor(s, off, 64);
    take_other(v, s, ov, os);
  }
}

// the winners of slots [b, e) of the index list: every lane of group 0 (and all others) ends
// with the wave's
template <int GL>
__device__ __forceinline__ Best4 slot_max(const float *__restrict__ in, int ld_in, int d,
                                          const int *__restrict__ idx, int b, int e, int lane) {
  constexpr int NB = kWave / GL;
  const int q = lane / GL, c0 = 4 * (lane % GL);
  Best4 w = best_empty();
#pragma unroll 2
  for (int k = b + q; k < e; k += NB) {
    const float4 p = row4(in + (long long)idx[k] * ld_in, c0, d, c0 < d);
    take_next(w.v.x, w.s.x, p.x, k);
    take_next(w.v.y, w.s.y, p.y, k);
    take_next(w.v.z, w.s.z, p.z, k);
    take_next(w.v.w, w.s.w, p.w, k);
  }
  across_groups_best<GL>(w.v.x, w.s.x);
  across_groups_best<GL>(w.v.y, w.s.y);
  across_groups_best<GL>(w.v.z, w.s.z);
  across_groups_best<GL>(w.v.w, w.s.w);
  return w;
}

// the final write of row i by the lane of column c0: out = add + max (one add; the maximum
// itself without `add`), arg = the slot; an empty row: out = add (or 0), arg = -1; columns from
// d on: 0 and -1
__device__ __forceinline__ void row_finish(const Best4 &w, bool empty, int i, int c0, int d,
                                           const float *__restrict__ add, int ld_add,
                                           float *__restrict__ out, int ld_out,
                                           int *__restrict__ arg, int ld_arg) {
  float4 o = empty ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : w.v;
  int4 a = empty ? make_int4(-1, -1, -1, -1) : w.s;
  if (add) {
    const float4 r = row4(add + (long long)i * ld_add, c0, d, true);
    if (empty) {
      o = r;
    } else {
      o.x = r.x + o.x;
      o.y = r.y + o.y;
      o.z = r.z + o.z;
      o.w = r.w + o.w;
    }
  }
  if (c0 + 1 >= d) o.y = 0.0f, a.y = -1;
  if (c0 + 2 >= d) o.z = 0.0f, a.z = -1;
  if (c0 + 3 >= d) o.w = 0.0f, a.w = -1;
  *reinterpret_cast<float4 *>(out + (long long)i * ld_out + c0) = o;
  if (arg) *reinterpret_cast<int4 *>(arg + (long long)i * ld_arg + c0) = a;
}
}  // namespace

// items [0, n): the rows of at most kGatSeg slots, whole; items [n, n + n_row_segs): the long
// rows' segments, which leave their winners in ws.row_val / ws.row_arg
template <int GL>
__global__ __launch_bounds__(kItemThreads) void k_agg_max_fwd(
    const GatPattern g, const SageWs ws, const float *__restrict__ in, int ld_in, int d,
    const float *__restrict__ add, int ld_add, float *__restrict__ out, int ld_out,
    int *__restrict__ arg, int ld_arg) {
  const int lane = threadIdx.x % kWave, c0 = 4 * (lane % GL);
  const long long items = (long long)g.n + g.n_row_segs;
  for (long long it = first_item(); it < items; it += item_stride()) {
    if (it < g.n) {
      const int i = (int)it, b = g.indptr[i], e = g.indptr[i + 1];
      if (e - b > kGatSeg) continue;
      const Best4 w = slot_max<GL>(in, ld_in, d, g.indices, b, e, lane);
      if (lane < GL && c0 < d) row_finish(w, e <= b, i, c0, d, add, ld_add, out, ld_out, arg, ld_arg);
    } else {
      const long long t = it - g.n;
      const int4 sg = g.row_segs[t];
      const Best4 w = slot_max<GL>(in, ld_in, d, g.indices, sg.y, sg.z, lane);
      if (lane < GL && c0 < d) {
        *reinterpret_cast<float4 *>(ws.row_val + t * kSageWsStride + c0) = w.v;
        *reinterpret_cast<int4 *>(ws.row_arg + t * kSageWsStride + c0) = w.s;
      }
    }
  }
}

// one wave per long row (the wave of its first segment): its segments' winners in segment
// order, then the final write
template <int GL>
__global__ __launch_bounds__(kItemThreads) void k_agg_max_fwd_merge(
    const GatPattern g, const SageWs ws, int d, const float *__restrict__ add, int ld_add,
    float *__restrict__ out, int ld_out, int *__restrict__ arg, int ld_arg) {
  const int lane = threadIdx.x % kWave, c0 = 4 * (lane % GL);
  for (long long t = first_item(); t < g.n_row_segs; t += item_stride()) {
    const int4 sg = g.row_segs[t];
    if (t != sg.w || lane >= GL || c0 >= d) continue;
    const int i = sg.x;
    const int nseg = (g.indptr[i + 1] - g.indptr[i] + kGatSeg - 1) / kGatSeg;
    Best4 w = best_empty();
    for (int k = 0; k < nseg; k++) {
      const float4 v = *reinterpret_cast<const float4 *>(ws.row_val + (t + k) * kSageWsStride + c0);
      const int4 s = *reinterpret_cast<const int4 *>(ws.row_arg + (t + k) * kSageWsStride + c0);
      take_other(w.v.x, w.s.x, v.x, s.x);
      take_other(w.v.y, w.s.y, v.y, s.y);
      take_other(w.v.z, w.s.z, v.z, s.z);
      take_other(w.v.w, w.s.w, v.w, s.w);
    }
    row_finish(w, false, i, c0, d, add, ld_add, out, ld_out, arg, ld_arg);
  }
}

namespace {
// slots [b, e) of the transposed index: the sum of the G_i components whose arg is the slot,
// over the groups (every lane ends with the wave's sums)
template <int GL>
__device__ __forceinline__ float4 col_select(const GatPattern &g, const float *__restrict__ G,
                                             int ld_g, const int *__restrict__ arg, int ld_arg,
                                             int d, int b, int e, int lane) {
  constexpr int NB = kWave / GL;
  const int q = lane / GL, c0 = 4 * (lane % GL);
  float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (c0 < d) {
#pragma unroll 2
    for (int o = b + q; o < e; o += NB) {
      const int r = g.csc_row[o], k = g.csc_pos[o];
      const int4 a = *reinterpret_cast<const int4 *>(arg + (long long)r * ld_arg + c0);
      const float4 gv = row4(G + (long long)r * ld_g, c0, d, true);
      if (a.x == k) acc.x += gv.x;
      if (a.y == k) acc.y += gv.y;
      if (a.z == k) acc.z += gv.z;
      if (a.w == k) acc.w += gv.w;
    }
  }
  acc.x = across_groups<GL>(acc.x);
  acc.y = across_groups<GL>(acc.y);
  acc.z = across_groups<GL>(acc.z);
  acc.w = across_groups<GL>(acc.w);
  return acc;  // (columns from d on: G read as zero there, whatever arg's padding names)
}
}  // namespace

// items [0, n): the columns of at most kGatSeg incoming slots, whole; items [n, n + n_col_segs):
// the long columns' segments, which leave their partial rows in ws.col_ws
template <int GL>
__global__ __launch_bounds__(kItemThreads) void k_agg_max_bwd(
    const GatPattern g, const SageWs ws, const float *__restrict__ G, int ld_g,
    const int *__restrict__ arg, int ld_arg, int d, float *__restrict__ din, int ld_din) {
  const int lane = threadIdx.x % kWave, c0 = 4 * (lane % GL);
  const long long items = (long long)g.n + g.n_col_segs;
  for (long long it = first_item(); it < items; it += item_stride()) {
    if (it < g.n) {
      const int j = (int)it, b = g.csc_ptr[j], e = g.csc_ptr[j + 1];
      if (e - b > kGatSeg) continue;
      const float4 acc = col_select<GL>(g, G, ld_g, arg, ld_arg, d, b, e, lane);
      if (lane < GL && c0 < d) *reinterpret_cast<float4 *>(din + (long long)j * ld_din + c0) = acc;
    } else {
      const long long t = it - g.n;
      const int4 sg = g.col_segs[t];
      const float4 acc = col_select<GL>(g, G, ld_g, arg, ld_arg, d, sg.y, sg.z, lane);
      if (lane < GL && c0 < d)
        *reinterpret_cast<float4 *>(ws.col_ws + t * kSageWsStride + c0) = acc;
    }
  }
}

// one wave per long column: its segments' partials in segment order
template <int GL>
__global__ __launch_bounds__(kItemThreads) void k_agg_max_bwd_merge(const GatPattern g,
                                                                    const SageWs ws, int d,
                                                                    float *__restrict__ din,
                                                                    int ld_din) {
  const int lane = threadIdx.x % kWave, c0 = 4 * (lane % GL);
  for (long long t = first_item(); t < g.n_long_cols; t += item_stride()) {
    if (lane >= GL || c0 >= d) continue;
    const int j = g.long_cols[t].x, first = g.long_cols[t].y;
    const int nseg = (g.csc_ptr[j + 1] - g.csc_ptr[j] + kGatSeg - 1) / kGatSeg;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int k = 0; k < nseg; k++) {
      const float4 p =
          *reinterpret_cast<const float4 *>(ws.col_ws + (long long)(first + k) * kSageWsStride + c0);
      acc.x += p.x;
      acc.y += p.y;
      acc.z += p.z;
      acc.w += p.w;
    }
    *reinterpret_cast<float4 *>(din + (long long)j * ld_din + c0) = acc;
  }
}

template <bool ADD>
__global__ __launch_bounds__(kItemThreads) void k_copy_cols(const float *__restrict__ src,
                                                            int ld_src, float *__restrict__ dst,
                                                            int ld_dst, long long total, int cols) {
  for (long long e = (long long)blockIdx.x * kItemThreads + threadIdx.x; e < total;
       e += (long long)gridDim.x * kItemThreads) {
    const long long r = e / cols;
    const int c = (int)(e - r * cols);
    const float v = src[r * ld_src + c];
    float *o = dst + r * ld_dst + c;
    *o = ADD ? *o + v : v;
  }
}

void launch_agg_max_fwd(const GatPattern &g, const SageWs &ws, const float *in, int ld_in, int d,
                        const float *add, int ld_add, float *out, int ld_out, int *arg,
                        int ld_arg, hipStream_t s) {
  PGCN_CHECK(d >= 1 && d <= kSageMaxWidth && g.n >= 0 && g.nnz <= INT_MAX, PGCN_E_INVALID,
             "agg_max_fwd: 1 <= d <= 128, nnz within an int");
  if (g.n == 0) return;
  ITEM_DISPATCH(k_agg_max_fwd, item_grid((long long)g.n + g.n_row_segs), s, g, ws, in, ld_in, d,
                add, ld_add, out, ld_out, arg, ld_arg);
  if (g.n_row_segs > 0)
    ITEM_DISPATCH(k_agg_max_fwd_merge, item_grid(g.n_row_segs), s, g, ws, d, add, ld_add, out,
                  ld_out, arg, ld_arg);
}

void launch_agg_max_bwd(const GatPattern &g, const SageWs &ws, const float *G, int ld_g,
                        const int *arg, int ld_arg, int d, float *din, int ld_din, hipStream_t s) {
  PGCN_CHECK(d >= 1 && d <= kSageMaxWidth && g.n >= 0 && g.nnz <= INT_MAX, PGCN_E_INVALID,
             "agg_max_bwd: 1 <= d <= 128, nnz within an int");
  if (g.n == 0) return;
  ITEM_DISPATCH(k_agg_max_bwd, item_grid((long long)g.n + g.n_col_segs), s, g, ws, G, ld_g, arg,
                ld_arg, d, din, ld_din);
  if (g.n_long_cols > 0)
    ITEM_DISPATCH(k_agg_max_bwd_merge, item_grid(g.n_long_cols), s, g, ws, d, din, ld_din);
}

void launch_copy_cols(const float *src, int ld_src, float *dst, int ld_dst, int n, int cols,
                      bool add, hipStream_t s) {
  PGCN_CHECK(n >= 0 && cols >= 1 && ld_src >= cols && ld_dst >= cols, PGCN_E_INVALID,
             "copy_cols: strides");
  if (n == 0) return;
  const long long total = (long long)n * cols;
  const dim3 grid((unsigned)std::min<long long>(ceil_div(total, kItemThreads), kItemMaxBlocks));
  if (add)
    PGCN_LAUNCH(k_copy_cols<true>, grid, dim3(kItemThreads), 0, s, src, ld_src, dst, ld_dst, total,
                cols);
  else
    PGCN_LAUNCH(k_copy_cols<false>, grid, dim3(kItemThreads), 0, s, src, ld_src, dst, ld_dst, total,
                cols);
}

}  // namespace pgcn
