// parallel-gcn_amd/csrc/k_nbr.hip -- GraphSAGE neighbour sampling for gfx950 (the reference has no
// such module): the per-epoch draw of at most K = fanout slots of every row of a square CSR
// pattern, the transposed index of the sampled pattern rebuilt on the device behind it, and the
// mean / max aggregation over the fixed-stride sampled pattern with its backward.  No float
// atomics; every order is a function of the arguments only; nothing allocates or syncs.
//
// The draw (k_nbr_draw<G>), a group of G = pow2ceil(K) lanes per row, 64 / G rows per wave.  Row i
// has L slots.  L <= K: the row keeps all of them in order, cnt_i = L.  L > K: Floyd's algorithm
// gives a uniform K-subset of [0, L) without a rejection loop.  All arithmetic modulo 2^64 (numpy
// uint64 gives the same bits), mix = k_neg.hip's splitmix64 finaliser, GAMMA = 0x9E3779B97F4A7C15:
//     k     = mix(seed + GAMMA * (round + 1))
//     key_i = mix(k + GAMMA * (i + 1))
//     for t = 0 .. K - 1:  m = L - K + t
//                          r = ((mix(key_i + GAMMA * (t + 1)) >> 32) * (m + 1)) >> 32
//                          pick_t = r unless r is among pick_0 .. pick_{t-1}, else m
//   Lane t of the group hashes its own r_t up front (the K hashes run in parallel); step t then
//   broadcasts r_t, the lanes below t compare it with their settled picks, and one wave ballot cut
//   to the group's bits decides whether lane t keeps r_t or takes m_t (never picked before: every
//   earlier pick is below it).  The ascending order is a rank count: lane t's position is the
//   number of the group's picks below its own (K broadcasts).  The lane then stores the global
//   slot b_i + pick and its neighbour at position i K + rank, and -1 at the positions from cnt_i
//   on; beside them it feeds the sort: the entry {node = the neighbour, or n for a padding
//   position; key = i K + position}.
//
// The transposed index.  launch_sort_by_node (k_neg.hip's stable LSD radix sort, the same
// kernels) sorts the n K entries by node in link_sort_passes(n + 1) passes; the padding entries,
// node n, end behind every real one, and equal nodes keep their key order = ascending (row,
// position).  k_nbr_finish (a lane per sorted entry) turns the key into {row = key / K, slot =
// slot[key]}, launch_index_ptr finds t_ptr by binary search, launch_index_segments writes the
// segment records of the lists above kGatSeg entries, padded to their capacities.
//
// The forward (k_nbr_agg_fwd<GL, MODE>), GL = item_gl(d) lanes per row -- lane li holds the
// float4 at column 4 li -- and 64 / GL rows per wave.  Per chunk of GL entries the group loads GL
// neighbour ids (and slots, for the max) with one coalesced load, lane li entry c + li, and hands
// them round by width-GL broadcasts; a lane gathers kNbrFlight rows' float4s before it folds them
// in, so that many gathers are in flight.  Every lane walks the row's entries in stored order:
// the mean is the sequential fp32 sum p = 0 .. cnt - 1, times one 1.0f / (float)cnt, plus add;
// the max keeps {value, slot} under "strictly greater", so the lowest slot of equal values wins.
//
// The backward (k_nbr_agg_bwd<GL, MODE>), slot_items.hpp's layout: a wave per node j or per
// kGatSeg-entry segment of a long list, cut into 64 / GL groups; group q takes entries q, q + 64 /
// GL, ... of the list, the groups meet in xor butterflies.  A segment leaves its partial row in
// ws, k_nbr_bwd_merge adds a long node's partials in segment order.
#include <algorithm>
#include <climits>

#include "common.hpp"
#include "kernels.hpp"
#include "slot_items.hpp"

#pragma clang fp contract(off)

namespace pgcn {

namespace {
constexpr int kNbrThreads = 256;
constexpr int kNbrFlight = 4;  // gathers a lane of the forward keeps in flight

__device__ __forceinline__ unsigned long long nbr_mix(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
constexpr unsigned long long kGamma = 0x9E3779B97F4A7C15ull;
}  // namespace

template <int G>
__global__ __launch_bounds__(kNbrThreads) void k_nbr_draw(const NbrSample p,
                                                          unsigned long long seed,
                                                          unsigned long long round) {
  const int K = p.fanout, t = threadIdx.x % G, lane = threadIdx.x % kWave;
  const long long row = ((long long)blockIdx.x * kNbrThreads + threadIdx.x) / G;
  const bool live = row < p.n;
  const int i = live ? (int)row : p.n - 1;
  const int b = p.indptr[i], L = p.indptr[i + 1] - b;
  const bool sampled = L > K;
  const int cnt = sampled ? K : L;
  const unsigned long long k = nbr_mix(seed + kGamma * (round + 1ull));
  const unsigned long long key = nbr_mix(k + kGamma * ((unsigned long long)i + 1ull));
  const unsigned long long h = nbr_mix(key + kGamma * ((unsigned long long)t + 1ull));
  const int m = L - K + t;  // (used only when sampled and t < K: then 0 < m < L)
  int pick = sampled && t < K ? (int)(((h >> 32) * (unsigned long long)(m + 1)) >> 32) : t;
  const unsigned long long gmask = G == 64 ? ~0ull : ((1ull << (G % 64)) - 1ull);
  const int gshift = lane & ~(G - 1);
  for (int u = 1; u < K; u++) {  // lanes below u are settled; lane u still holds r_u
    const int ru = __shfl(pick, u, G);
    const unsigned long long hit = (__ballot(t < u && pick == ru) >> gshift) & gmask;
    if (t == u && sampled && hit) pick = m;
  }
  int rank = 0;
  for (int u = 0; u < K; u++) {
    const int pu = __shfl(pick, u, G);
    rank += (u < cnt && pu < pick) ? 1 : 0;
  }
  if (!live || t >= K) return;
  const bool kept = t < cnt;  // (then pick < L)
  const long long at = (long long)i * K + (kept ? rank : t);
  const int j = kept ? p.indices[b + pick] : -1;
  p.slot[at] = kept ? b + pick : -1;
  p.nbr[at] = j;
  p.nodes[1][at] = kept ? j : p.n;
  p.keys[1][at] = (unsigned)at;
  if (t == 0) p.cnt[i] = cnt;
}

// a lane per sorted entry o: its row and slot (-1 for the padding entries behind t_ptr[n])
__global__ __launch_bounds__(kNbrThreads) void k_nbr_finish(const NbrSample p,
                                                            const int *__restrict__ nodes,
                                                            const unsigned *__restrict__ keys,
                                                            int total) {
  const long long g = (long long)blockIdx.x * kNbrThreads + threadIdx.x;
  if (g >= total) return;
  const bool real = nodes[g] < p.n;
  const unsigned key = keys[g];
  p.t_row[g] = real ? (int)(key / (unsigned)p.fanout) : -1;
  p.t_slot[g] = real ? p.slot[key] : -1;
}

namespace {
// the final write of row i by the lane of column c0 (k_sage.hip's row_finish): out = add + v,
// arg = the slot; an empty row: out = add (or 0), arg = -1; columns from d on: 0 and -1
__device__ __forceinline__ void nbr_row_finish(float4 o, int4 a, bool empty, int i, int c0, int d,
                                               const float *__restrict__ add, int ld_add,
                                               float *__restrict__ out, int ld_out,
                                               int *__restrict__ arg, int ld_arg) {
  if (empty) {
    o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    a = make_int4(-1, -1, -1, -1);
  }
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

__device__ __forceinline__ void nbr_take(float &v, int &s, float ov, int os, bool on) {
  if (on && ov > v) {
    v = ov;
    s = os;
  }
}
}  // namespace

// item w: rows w (64 / GL) .. of the sampled pattern, one lane group each
template <int GL, int MODE>
__global__ __launch_bounds__(kItemThreads) void k_nbr_agg_fwd(
    const NbrSample p, const float *__restrict__ in, int ld_in, int d,
    const float *__restrict__ add, int ld_add, float *__restrict__ out, int ld_out,
    int *__restrict__ arg, int ld_arg) {
  constexpr int RW = kWave / GL;                            // rows per wave
  constexpr int U = GL < kNbrFlight ? GL : kNbrFlight;      // entries per step
  const int lane = threadIdx.x % kWave, li = lane % GL, c0 = 4 * li, K = p.fanout;
  const bool col = c0 < d;
  const long long items = ((long long)p.n + RW - 1) / RW;
  for (long long w = first_item(); w < items; w += item_stride()) {
    const long long row = w * RW + lane / GL;
    const bool live = row < p.n;
    const int i = live ? (int)row : p.n - 1;
    const int cnt = live ? p.cnt[i] : 0;
    int cmax = cnt;  // the wave's longest row: every lane runs the broadcasts of every step
#pragma unroll
    for (int off = GL; off < kWave; off <<= 1) cmax = max(cmax, __shfl_xor(cmax, off, kWave));
    float4 acc = MODE == kNbrMax ? make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY)
                                 : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int4 win = make_int4(INT_MAX, INT_MAX, INT_MAX, INT_MAX);
    for (int c = 0; c < cmax; c += GL) {
      const long long e = (long long)i * K + min(c + li, K - 1);
      const int my_n = p.nbr[e], my_s = MODE == kNbrMax ? p.slot[e] : 0;
      for (int u0 = 0; u0 < GL && c + u0 < cmax; u0 += U) {
        float4 v[U];
        int sl[U];
        bool on[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
          const int j = __shfl(my_n, u0 + u, GL);
          sl[u] = __shfl(my_s, u0 + u, GL);
          on[u] = c + u0 + u < cnt;
          v[u] = row4(in + (long long)(on[u] ? j : 0) * ld_in, c0, d, on[u] && col);
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
          if (MODE == kNbrMax) {
            nbr_take(acc.x, win.x, v[u].x, sl[u], on[u]);
            nbr_take(acc.y, win.y, v[u].y, sl[u], on[u]);
            nbr_take(acc.z, win.z, v[u].z, sl[u], on[u]);
            nbr_take(acc.w, win.w, v[u].w, sl[u], on[u]);
          } else {  // (an entry that is off adds +0, and a sum that starts at +0 is never -0)
            acc.x += v[u].x;
            acc.y += v[u].y;
            acc.z += v[u].z;
            acc.w += v[u].w;
          }
        }
      }
    }
    if (!live || !col) continue;
    if (MODE == kNbrMean) {
      const float inv = 1.0f / (float)max(cnt, 1);
      acc.x *= inv;
      acc.y *= inv;
      acc.z *= inv;
      acc.w *= inv;
    }
    nbr_row_finish(acc, win, cnt == 0, i, c0, d, add, ld_add, out, ld_out,
                   MODE == kNbrMax ? arg : nullptr, ld_arg);
  }
}

namespace {
// entries [b, e) of the transposed index: their contributions summed over the groups (every lane
// ends with the wave's sums)
template <int GL, int MODE>
__device__ __forceinline__ float4 nbr_col_sum(const NbrSample &p, const float *__restrict__ G,
                                              int ld_g, const int *__restrict__ arg, int ld_arg,
                                              int d, int b, int e, int lane) {
  constexpr int NB = kWave / GL;
  const int q = lane / GL, c0 = 4 * (lane % GL);
  float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (c0 < d) {
#pragma unroll 2
    for (int o = b + q; o < e; o += NB) {
      const int r = p.t_row[o];
      const float4 gv = row4(G + (long long)r * ld_g, c0, d, true);
      if (MODE == kNbrMax) {
        const int k = p.t_slot[o];
        const int4 a = *reinterpret_cast<const int4 *>(arg + (long long)r * ld_arg + c0);
        if (a.x == k) acc.x += gv.x;
        if (a.y == k) acc.y += gv.y;
        if (a.z == k) acc.z += gv.z;
        if (a.w == k) acc.w += gv.w;
      } else {
        const float inv = 1.0f / (float)p.cnt[r];
        acc.x += gv.x * inv;
        acc.y += gv.y * inv;
        acc.z += gv.z * inv;
        acc.w += gv.w * inv;
      }
    }
  }
  acc.x = across_groups<GL>(acc.x);
  acc.y = across_groups<GL>(acc.y);
  acc.z = across_groups<GL>(acc.z);
  acc.w = across_groups<GL>(acc.w);
  return acc;
}
}  // namespace

// items [0, n): the nodes whose lists hold at most kGatSeg entries, whole; items [n, n +
// seg_cap): the segment records (the padding ones are empty ranges: zero partials)
template <int GL, int MODE>
__global__ __launch_bounds__(kItemThreads) void k_nbr_agg_bwd(
    const NbrSample p, const float *__restrict__ G, int ld_g, const int *__restrict__ arg,
    int ld_arg, int d, float *__restrict__ din, int ld_din) {
  const int lane = threadIdx.x % kWave, c0 = 4 * (lane % GL);
  const long long items = (long long)p.n + p.seg_cap;
  for (long long it = first_item(); it < items; it += item_stride()) {
    if (it < p.n) {
      const int j = (int)it, b = p.t_ptr[j], e = p.t_ptr[j + 1];
      if (e - b > kGatSeg) continue;
      const float4 acc = nbr_col_sum<GL, MODE>(p, G, ld_g, arg, ld_arg, d, b, e, lane);
      if (lane < GL && c0 < d) store_row4(din + (long long)j * ld_din, c0, d, acc);
    } else {
      const long long t = it - p.n;
      const int4 sg = p.segs[t];
      const float4 acc = nbr_col_sum<GL, MODE>(p, G, ld_g, arg, ld_arg, d, sg.y, sg.z, lane);
      if (lane < GL && c0 < d)
        *reinterpret_cast<float4 *>(p.ws + t * kSageWsStride + c0) = acc;
    }
  }
}

// one wave per long-node record: its segments' partials in segment order (a padding record
// rewrites node 0's row with the bits it has: k_neg.hip's header)
template <int GL>
__global__ __launch_bounds__(kItemThreads) void k_nbr_bwd_merge(const NbrSample p, int d,
                                                                float *__restrict__ din,
                                                                int ld_din) {
  const int lane = threadIdx.x % kWave, c0 = 4 * (lane % GL);
  for (long long t = first_item(); t < p.long_cap; t += item_stride()) {
    if (lane >= GL || c0 >= d) continue;
    const int j = p.longs[t].x, first = p.longs[t].y;
    const int nseg = (p.t_ptr[j + 1] - p.t_ptr[j] + kGatSeg - 1) / kGatSeg;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int k = 0; k < nseg && first + k < p.seg_cap; k++) {
      const float4 v =
          *reinterpret_cast<const float4 *>(p.ws + (long long)(first + k) * kSageWsStride + c0);
      acc.x += v.x;
      acc.y += v.y;
      acc.z += v.z;
      acc.w += v.w;
    }
    store_row4(din + (long long)j * ld_din, c0, d, acc);
  }
}

namespace {
void check_nbr(const NbrSample &p, int mode, int d, const char *what) {
  PGCN_CHECK(p.n >= 0 && p.fanout >= 1 && p.fanout <= kNbrMaxFanout &&
                 (long long)p.n * p.fanout <= INT_MAX,
             PGCN_E_INVALID, what);
  PGCN_CHECK((mode == kNbrMean || mode == kNbrMax) && d >= 1 && d <= kSageMaxWidth,
             PGCN_E_INVALID, what);
}
}  // namespace

#define NBR_DRAW_CASE(GG)                                                                     \
  case GG:                                                                                    \
    PGCN_LAUNCH(k_nbr_draw<GG>, dim3((unsigned)ceil_div((long long)p.n * GG, kNbrThreads)),   \
                dim3(kNbrThreads), 0, s, p, seed, round);                                     \
    break

void launch_nbr_draw(const NbrSample &p, unsigned long long seed, unsigned long long round,
                     hipStream_t s) {
  check_nbr(p, kNbrMean, 1, "nbr_draw: 1 <= fanout <= 64, n * fanout within an int");
  if (p.n == 0) return;
  note_path(KP_NBR_DRAW);
  int G = 1;
  while (G < p.fanout) G <<= 1;
  switch (G) {
    NBR_DRAW_CASE(1);
    NBR_DRAW_CASE(2);
    NBR_DRAW_CASE(4);
    NBR_DRAW_CASE(8);
    NBR_DRAW_CASE(16);
    NBR_DRAW_CASE(32);
    default:
      NBR_DRAW_CASE(64);
  }
  const int total = p.n * p.fanout;
  const int at = launch_sort_by_node(total, p.n + 1, p.nodes, p.keys, p.hist, s);
  PGCN_LAUNCH(k_nbr_finish, dim3((unsigned)ceil_div(total, kNbrThreads)), dim3(kNbrThreads), 0, s,
              p, p.nodes[at], p.keys[at], total);
  launch_index_ptr(p.nodes[at], total, p.n, p.t_ptr, s);
  if (p.long_cap)
    launch_index_segments(p.t_ptr, p.n, p.marks, p.segs, p.seg_cap, p.longs, p.long_cap, s);
}
#undef NBR_DRAW_CASE

// KERNEL<GL, mode> for the width `d` and the `mode` in scope
#define NBR_DISPATCH(KERNEL, grid, s, ...)                                \
  do {                                                                    \
    if (mode == kNbrMax) {                                                \
      auto KMAX = [&](auto gl) {                                          \
        PGCN_LAUNCH((KERNEL<decltype(gl)::value, kNbrMax>), grid,         \
                    dim3(kItemThreads), 0, s, __VA_ARGS__);               \
      };                                                                  \
      nbr_for_gl(d, KMAX);                                                \
    } else {                                                              \
      auto KMEAN = [&](auto gl) {                                         \
        PGCN_LAUNCH((KERNEL<decltype(gl)::value, kNbrMean>), grid,        \
                    dim3(kItemThreads), 0, s, __VA_ARGS__);               \
      };                                                                  \
      nbr_for_gl(d, KMEAN);                                               \
    }                                                                     \
  } while (0)

namespace {
template <typename F>
void nbr_for_gl(int d, F &&f) {
  switch (item_gl(d)) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    default: f(std::integral_constant<int, 32>{}); break;
  }
}
}  // namespace

void launch_nbr_agg_fwd(const NbrSample &p, int mode, const float *in, int ld_in, int d,
                        const float *add, int ld_add, float *out, int ld_out, int *arg, int ld_arg,
                        hipStream_t s) {
  check_nbr(p, mode, d, "nbr_agg_fwd: mode 1 or 2, 1 <= d <= 128, 1 <= fanout <= 64");
  if (p.n == 0) return;
  note_path(KP_NBR_FWD);
  const dim3 grid = item_grid(ceil_div((long long)p.n, kWave / item_gl(d)));
  NBR_DISPATCH(k_nbr_agg_fwd, grid, s, p, in, ld_in, d, add, ld_add, out, ld_out, arg, ld_arg);
}

void launch_nbr_agg_bwd(const NbrSample &p, int mode, const float *G, int ld_g, const int *arg,
                        int ld_arg, int d, float *din, int ld_din, hipStream_t s) {
  check_nbr(p, mode, d, "nbr_agg_bwd: mode 1 or 2, 1 <= d <= 128, 1 <= fanout <= 64");
  if (p.n == 0) return;
  note_path(KP_NBR_BWD);
  const dim3 grid = item_grid((long long)p.n + p.seg_cap);
  NBR_DISPATCH(k_nbr_agg_bwd, grid, s, p, G, ld_g, arg, ld_arg, d, din, ld_din);
  if (p.long_cap > 0)
    ITEM_DISPATCH(k_nbr_bwd_merge, item_grid(p.long_cap), s, p, d, din, ld_din);
}
#undef NBR_DISPATCH

}  // namespace pgcn
