// parallel-gcn_amd/csrc/k_neg.hip -- per-epoch negative sampling for link training, on the device,
// for gfx950 (the reference has no pair-level model): the draw of fresh negative endpoints and the
// rebuild of a pair list's incidence index (LinkIndex, kernels.hpp) after its dst column changed.
// Integer work only; every result is a function of the inputs, never of a grid size or of the
// order in which workgroups run.  256-thread workgroups, loads from clamped addresses, vector
// stores, unsigned LDS atomics for counts only.
//
// The draw (k_neg_sample), one lane per draw e < m:
//   the anchor s = src[e] has the strictly ascending exclusion row x[0 .. L) (s itself included);
//   with free = n - L the lane takes r in [0, free) and returns the r-th node NOT in the row: the
//   smallest j in [0, L] with x[j] - j > r (x[L] = infinity), found by binary search, gives r + j.
//   No rejection loop: exact, uniform over the free nodes, one pass over log2(L) row entries.
//   The random word, all arithmetic modulo 2^64 (numpy uint64 gives the same bits):
//     mix(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
//             z = (z ^ (z >> 27)) * 0x94D049BB133111EB
//             return z ^ (z >> 31)                                   (splitmix64's finaliser)
//     k = mix(seed + 0x9E3779B97F4A7C15 * (round + 1))
//     h = mix(k    + 0x9E3779B97F4A7C15 * (e + 1))
//     r = ((h >> 32) * free) >> 32
//
// The rebuild (launch_links_rebuild).  The 2 E' role entries of the E' selected pairs are (node,
// key = 2 e + role), role 0 the src end, generated in ascending key order straight from the pair
// arrays by the first pass's loads.  A stable LSD radix sort by node -- 8-bit digits,
// link_sort_passes(n) passes, ping-pong buffers -- leaves every node's entries in ascending key
// order, which is the order build_incidence defines (ascending pair, src role first): no per-list
// sort, and the length of a list never matters.  Per pass:
//   k_sort_hist    a workgroup per kSortTile-entry tile: digit counts in LDS -> hist[digit][tile]
//   k_scan_rows    a workgroup per digit: the exclusive scan of its row of tile counts, in strips
//                  of 256 (coalesced) with a carry, and the row's total
//   k_sort_scatter scans the 256 row totals in LDS (the digits' first slots), then walks the tile
//                  again in kSortItems strips of 256: a wave finds the lanes of its own digit with
//                  8 ballots (match-any), the waves' per-digit counts meet in LDS in wave order, a
//                  running per-digit cursor carries over the strips: rank = cursor + earlier waves
//                  + earlier lanes, so equal digits keep their input order.
// Then k_inc_finish (a lane per sorted entry) writes inc_pair / inc_other, k_inc_ptr (a lane per
// node) finds ptr[i] as the first sorted entry of a node >= i by binary search -- no lane ever
// fills a gap serially -- and, only when a list can exceed kGatSeg at all, three launches build the
// segment records of gat_segments on the device: k_seg_mark (per 256 nodes the segment and
// long-node counts), k_scan_rows over the two count rows, k_seg_write (records in node order, then
// the padding below).
//
// The backward kernels take n_segs and n_long by value, and a rebuild never tells the host what it
// found.  A rebuildable index therefore always carries its capacity: with N2 = 2 E' entries at
// most long_cap = N2 / (kGatSeg + 1) nodes are long and they have at most ceil(N2 / kGatSeg) +
// long_cap segments; seg_cap is that plus one.  Behind the S real segment and NL real long records
// the padding is harmless by construction: a padding segment is the empty range {0, 0, 0, 0} (a
// zero partial row), a padding long record names node 0 -- its real record {0, 0} when node 0 is
// long, else {0, S} with segment S = node 0's whole list, so the merge rewrites the row the main
// launch already wrote with the same bits (0 + x, and a sum that starts at +0 is never -0).
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"

namespace pgcn {

namespace {
constexpr int kNegThreads = 256;
constexpr int kNegWaves = kNegThreads / kWave;
constexpr int kSortItems = kSortTile / kNegThreads;
static_assert(kSortTile % kNegThreads == 0, "a tile is whole strips");

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ int clamp_node(int v, int n) { return min(max(v, 0), n - 1); }

// exclusive prefix of v over the workgroup's 256 threads (lds: kNegWaves ints); *total: their sum
__device__ __forceinline__ int block_excl(int v, int *lds, int *total) {
  const int lane = threadIdx.x % kWave, w = threadIdx.x / kWave;
  int inc = v;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const int u = __shfl_up(inc, off, kWave);
    if (lane >= off) inc += u;
  }
  if (lane == kWave - 1) lds[w] = inc;
  __syncthreads();
  int base = 0, sum = 0;
#pragma unroll
  for (int k = 0; k < kNegWaves; k++) {
    if (k < w) base += lds[k];
    sum += lds[k];
  }
  *total = sum;
  __syncthreads();
  return base + inc - v;
}

// where a pass reads its entries: the pair arrays (the first pass) or the previous pass's output
struct SortIn {
  const int *sel, *src, *dst;  // first pass
  const int *nodes;            // later passes
  const unsigned *keys;
  int n;
};

template <bool FIRST>
__device__ __forceinline__ void load_entry(const SortIn &in, int k, int *node, unsigned *key) {
  if (FIRST) {
    const int e = in.sel[k >> 1], role = k & 1;
    *key = 2u * (unsigned)e + (unsigned)role;
    *node = clamp_node(role ? in.dst[e] : in.src[e], in.n);
  } else {
    *node = in.nodes[k];
    *key = in.keys[k];
  }
}
}  // namespace

__global__ __launch_bounds__(kNegThreads) void k_neg_sample(
    const int *__restrict__ src, long long m, int n, const long long *__restrict__ excl_ptr,
    const int *__restrict__ excl_idx, unsigned long long seed, unsigned long long round,
    int *__restrict__ dst) {
  const long long e = (long long)blockIdx.x * kNegThreads + threadIdx.x;
  const bool on = e < m;
  const int s = clamp_node(src[on ? e : m - 1], n);
  const long long b = excl_ptr[s];
  const int L = (int)(excl_ptr[s + 1] - b);
  const unsigned long long freen = (unsigned long long)(n - L);
  const unsigned long long k = mix64(seed + 0x9E3779B97F4A7C15ull * (round + 1ull));
  const unsigned long long h = mix64(k + 0x9E3779B97F4A7C15ull * ((unsigned long long)e + 1ull));
  const int r = (int)(((h >> 32) * freen) >> 32);
  const int *__restrict__ x = excl_idx + b;
  int lo = 0, hi = L;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (x[mid] - mid <= r) lo = mid + 1;
    else hi = mid;
  }
  if (on) dst[e] = r + lo;
}

template <bool FIRST>
__global__ __launch_bounds__(kNegThreads) void k_sort_hist(const SortIn in, int total, int shift,
                                                            unsigned *__restrict__ hist, int W) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * kSortTile;
#pragma unroll
  for (int c = 0; c < kSortItems; c++) {
    const long long k = base + c * kNegThreads + threadIdx.x;  // may pass INT_MAX in the last tile
    int node;
    unsigned key;
    load_entry<FIRST>(in, (int)(k < total ? k : total - 1), &node, &key);
    if (k < total) atomicAdd(&h[(node >> shift) & 255], 1u);
  }
  __syncthreads();
  hist[(long long)threadIdx.x * W + blockIdx.x] = h[threadIdx.x];
}

// a workgroup per row of a [rows][W]: the row's exclusive scan in place, strips of 256 with a
// carry, and its total in a[rows * W + row]
__global__ __launch_bounds__(kNegThreads) void k_scan_rows(unsigned *__restrict__ a, int W) {
  __shared__ int lds[kNegWaves];
  unsigned *__restrict__ row = a + (long long)blockIdx.x * W;
  unsigned carry = 0;
  for (int base = 0; base < W; base += kNegThreads) {
    const int i = base + threadIdx.x;
    const unsigned v = i < W ? row[min(i, W - 1)] : 0u;
    int sum;
    const int ex = block_excl((int)v, lds, &sum);
    if (i < W) row[i] = carry + (unsigned)ex;
    carry += (unsigned)sum;
  }
  if (threadIdx.x == 0) a[(long long)gridDim.x * W + blockIdx.x] = carry;
}

template <bool FIRST>
__global__ __launch_bounds__(kNegThreads) void k_sort_scatter(
    const SortIn in, int total, int shift, const unsigned *__restrict__ hist, int W,
    int *__restrict__ out_nodes, unsigned *__restrict__ out_keys) {
  __shared__ unsigned cur[256];              // the next output slot of every digit
  __shared__ unsigned wcnt[kNegWaves][256];  // this strip's entries per wave and digit
  __shared__ int lds[kNegWaves];
  const int t = threadIdx.x, lane = t % kWave, w = t / kWave;
  int all;  // digit t's first slot: the digits before it, then this digit's earlier tiles
  cur[t] = (unsigned)block_excl((int)hist[256LL * W + t], lds, &all) +
           hist[(long long)t * W + blockIdx.x];
#pragma unroll
  for (int k = 0; k < kNegWaves; k++) wcnt[k][t] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * kSortTile;
  for (int c = 0; c < kSortItems; c++) {
    const long long k = base + c * kNegThreads + t;  // may pass INT_MAX in the last tile
    const bool on = k < total;
    int node;
    unsigned key;
    load_entry<FIRST>(in, (int)(on ? k : total - 1), &node, &key);
    const int g = (node >> shift) & 255;
    unsigned long long same = __ballot(on);  // the live lanes of this wave with digit g
#pragma unroll
    for (int bit = 0; bit < 8; bit++) {
      const bool set = (g >> bit) & 1;
      const unsigned long long bal = __ballot(on && set);
      same &= set ? bal : ~bal;
    }
    const int rank = __popcll(same & ((1ull << lane) - 1ull));
    if (on && rank == 0) wcnt[w][g] = (unsigned)__popcll(same);
    __syncthreads();
    if (on) {
      unsigned o = cur[g] + (unsigned)rank;
      for (int k2 = 0; k2 < w; k2++) o += wcnt[k2][g];
      if (o < (unsigned)total) {
        out_nodes[o] = node;
        out_keys[o] = key;
      }
    }
    __syncthreads();
    unsigned add = 0;
#pragma unroll
    for (int k2 = 0; k2 < kNegWaves; k2++) {
      add += wcnt[k2][t];
      wcnt[k2][t] = 0;
    }
    cur[t] += add;
    __syncthreads();
  }
}

// a lane per sorted entry k: the pair and its other endpoint
__global__ __launch_bounds__(kNegThreads) void k_inc_finish(
    const unsigned *__restrict__ keys, int total, int n, const int *__restrict__ src,
    const int *__restrict__ dst, int *__restrict__ pair, int *__restrict__ other) {
  const long long g = (long long)blockIdx.x * kNegThreads + threadIdx.x;
  const bool on = g < total;
  const int k = on ? (int)g : total - 1;
  const unsigned key = keys[k];
  const int e = (int)(key >> 1);
  const int o = clamp_node((key & 1u) ? src[e] : dst[e], n);
  if (!on) return;
  pair[k] = e;
  other[k] = o;
}

// a lane per i in [0, n]: ptr[i] = the first sorted entry whose node is >= i (total: none)
__global__ __launch_bounds__(kNegThreads) void k_inc_ptr(const int *__restrict__ nodes, int total,
                                                          int n, int *__restrict__ ptr) {
  const long long g = (long long)blockIdx.x * kNegThreads + threadIdx.x;
  if (g > n) return;
  const int i = (int)g;
  int lo = 0, hi = total;
  while (lo < hi) {
    const int mid = (int)(((long long)lo + hi) >> 1);
    if (nodes[mid] < i) lo = mid + 1;
    else hi = mid;
  }
  ptr[i] = lo;
}

namespace {
__device__ __forceinline__ void seg_counts(const int *__restrict__ ptr, int n, int i, int *b,
                                           int *len, int *nseg) {
  const int ic = min(i, n - 1);
  *b = ptr[ic];
  *len = i < n ? ptr[ic + 1] - *b : 0;
  *nseg = *len > kGatSeg ? (*len + kGatSeg - 1) / kGatSeg : 0;
}
}  // namespace

// marks[b] = the segments of nodes 256 b .. 256 b + 255, marks[B + b] = their long nodes (the
// row scan leaves the two totals in marks[2 B], marks[2 B + 1])
__global__ __launch_bounds__(kNegThreads) void k_seg_mark(const int *__restrict__ ptr, int n,
                                                           unsigned *__restrict__ marks, int B) {
  __shared__ unsigned sum[2];
  if (threadIdx.x < 2) sum[threadIdx.x] = 0;
  __syncthreads();
  int b, len, nseg;
  seg_counts(ptr, n, blockIdx.x * kNegThreads + threadIdx.x, &b, &len, &nseg);
  if (nseg) {
    atomicAdd(&sum[0], (unsigned)nseg);
    atomicAdd(&sum[1], 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    marks[blockIdx.x] = sum[0];
    marks[B + blockIdx.x] = sum[1];
  }
}

// workgroups [0, B): the records of their 256 nodes, at the scanned offsets; every thread g of the
// grid: the padding records g (see the header) -- disjoint from the real ones, so no order matters
__global__ __launch_bounds__(kNegThreads) void k_seg_write(
    const int *__restrict__ ptr, int n, const unsigned *__restrict__ marks, int B,
    int4 *__restrict__ segs, int seg_cap, int2 *__restrict__ longs, int long_cap) {
  __shared__ int lds[kNegWaves];
  const int S = (int)marks[2 * B], NL = (int)marks[2 * B + 1];
  if ((int)blockIdx.x < B) {
    int b, len, nseg;
    const int i = blockIdx.x * kNegThreads + threadIdx.x;
    seg_counts(ptr, n, i, &b, &len, &nseg);
    int all;
    const int first = (int)marks[blockIdx.x] + block_excl(nseg, lds, &all);
    const int at = (int)marks[B + blockIdx.x] + block_excl(nseg ? 1 : 0, lds, &all);
    if (nseg && at < long_cap && first + nseg <= seg_cap) {
      longs[at] = make_int2(i, first);
      for (int j = 0; j < nseg; j++)
        segs[first + j] =
            make_int4(i, b + j * kGatSeg, min(b + (j + 1) * kGatSeg, b + len), first);
    }
  }
  const long long g = (long long)blockIdx.x * kNegThreads + threadIdx.x;
  const int p0 = ptr[0], p1 = ptr[1];
  const bool long0 = p1 - p0 > kGatSeg;
  if (g >= NL && g < long_cap) longs[g] = make_int2(0, long0 ? 0 : S);
  if (g >= S && g < seg_cap)
    segs[g] = g == S && !long0 ? make_int4(0, p0, p1, S) : make_int4(0, 0, 0, 0);
}

int link_sort_passes(int n) {
  int bits = 0;
  while (bits < 31 && ((long long)1 << bits) < n) bits++;  // bits(n - 1)
  return std::max(1, (bits + 7) / 8);  // n == 1 still takes one pass: the first pass generates
}

void launch_neg_sample(const int *src, long long m, int n, const long long *excl_ptr,
                       const int *excl_idx, unsigned long long seed, unsigned long long round,
                       int *dst, hipStream_t s) {
  if (m == 0) return;
  PGCN_LAUNCH(k_neg_sample, dim3((unsigned)ceil_div(m, kNegThreads)), dim3(kNegThreads), 0, s, src,
              m, n, excl_ptr, excl_idx, seed, round, dst);
}

int links_rebuild_stages(const LinkBuild &b) {
  if (b.total == 0) return 0;
  return 3 * link_sort_passes(b.n) + 1 + (b.long_cap ? 1 : 0);
}

void launch_links_rebuild(const LinkBuild &b, hipStream_t s, hipEvent_t *stage_end) {
  if (b.total == 0) return;  // ptr stays all zero
  const dim3 tiles((unsigned)b.tiles), thr(kNegThreads);
  const int passes = link_sort_passes(b.n);
  auto stage = [&] {
    if (stage_end) PGCN_HIP(hipEventRecord(*stage_end++, s));
  };
  SortIn in{b.sel, b.src, b.dst, nullptr, nullptr, b.n};
  for (int p = 0; p < passes; p++) {
    const int shift = 8 * p, to = p & 1;
    if (p == 0) {
      PGCN_LAUNCH(k_sort_hist<true>, tiles, thr, 0, s, in, b.total, shift, b.hist, b.tiles);
    } else {
      PGCN_LAUNCH(k_sort_hist<false>, tiles, thr, 0, s, in, b.total, shift, b.hist, b.tiles);
    }
    stage();
    PGCN_LAUNCH(k_scan_rows, dim3(256), thr, 0, s, b.hist, b.tiles);
    stage();
    if (p == 0) {
      PGCN_LAUNCH(k_sort_scatter<true>, tiles, thr, 0, s, in, b.total, shift, b.hist, b.tiles,
                  b.nodes[to], b.keys[to]);
    } else {
      PGCN_LAUNCH(k_sort_scatter<false>, tiles, thr, 0, s, in, b.total, shift, b.hist, b.tiles,
                  b.nodes[to], b.keys[to]);
    }
    stage();
    in.nodes = b.nodes[to];
    in.keys = b.keys[to];
  }
  PGCN_LAUNCH(k_inc_finish, dim3((unsigned)ceil_div(b.total, kNegThreads)), thr, 0, s, in.keys,
              b.total, b.n, b.src, b.dst, b.pair, b.other);
  PGCN_LAUNCH(k_inc_ptr, dim3((unsigned)ceil_div((long long)b.n + 1, kNegThreads)), thr, 0, s,
              in.nodes, b.total, b.n, b.ptr);
  stage();
  if (b.long_cap == 0) return;  // no list can exceed kGatSeg
  launch_index_segments(b.ptr, b.n, b.marks, b.segs, b.seg_cap, b.longs, b.long_cap, s);
  stage();
}

void launch_index_segments(const int *ptr, int n, unsigned *marks, int4 *segs, int seg_cap,
                           int2 *longs, int long_cap, hipStream_t s) {
  const dim3 thr(kNegThreads);
  const int B = (int)ceil_div(n, kNegThreads);
  PGCN_LAUNCH(k_seg_mark, dim3((unsigned)B), thr, 0, s, ptr, n, marks, B);
  PGCN_LAUNCH(k_scan_rows, dim3(2), thr, 0, s, marks, B);
  const long long cover = std::max<long long>(n, std::max(seg_cap, long_cap));
  PGCN_LAUNCH(k_seg_write, dim3((unsigned)ceil_div(cover, kNegThreads)), thr, 0, s, ptr, n, marks,
              B, segs, seg_cap, longs, long_cap);
}

int launch_sort_by_node(int total, int n_ids, int *const nodes[2], unsigned *const keys[2],
                        unsigned *hist, hipStream_t s) {
  const int tiles = (int)ceil_div(total, kSortTile), passes = link_sort_passes(n_ids);
  const dim3 grid((unsigned)tiles), thr(kNegThreads);
  SortIn in{nullptr, nullptr, nullptr, nodes[1], keys[1], n_ids};
  for (int p = 0; p < passes; p++) {
    const int shift = 8 * p, to = p & 1;
    PGCN_LAUNCH(k_sort_hist<false>, grid, thr, 0, s, in, total, shift, hist, tiles);
    PGCN_LAUNCH(k_scan_rows, dim3(256), thr, 0, s, hist, tiles);
    PGCN_LAUNCH(k_sort_scatter<false>, grid, thr, 0, s, in, total, shift, hist, tiles, nodes[to],
                keys[to]);
    in.nodes = nodes[to];
    in.keys = keys[to];
  }
  return (passes - 1) & 1;
}

void launch_index_ptr(const int *nodes, int total, int n, int *ptr, hipStream_t s) {
  PGCN_LAUNCH(k_inc_ptr, dim3((unsigned)ceil_div((long long)n + 1, kNegThreads)),
              dim3(kNegThreads), 0, s, nodes, total, n, ptr);
}

}  // namespace pgcn
