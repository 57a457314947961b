// parallel-gcn_amd/csrc/k_topk.hip -- link prediction's 1-vs-all retrieval for gfx950 (the
// reference has no pair-level model): for every query (anchor a, exclude list X) the k candidates
// v in [0, n) \ X with the highest rank score r(a, v) (k_rank.hip's fmaf chain, which the f32 MFMA
// computes bit for bit), ties to the lower index, without ever storing the [Q][n] score matrix.
//
// A selection key is 64 bits, ordered(score) << 32 | ~v: ordered() maps a float (its zero
// canonicalised to +0 first) to an unsigned that compares as the float does, so a greater key is a
// candidate that precedes.  Keys of distinct candidates are distinct; 0 is "no entry".
//
//   k_topk_sweep<NV, E>: k_rank_sweep's workgroup, tiles, staging and MFMA loop (rank_sweep.hpp).
//       A wave owns its 32 queries over its split's candidate range, so everything per query is
//       wave-private: a threshold tau (-inf until the query has held k entries, then the k-th best
//       score as of the last prune; +inf for a row beyond Q, which then never passes) and an append
//       buffer of cap = 64 E keys in the handle's workspace, one per (query, split).  The epilogue
//       tests acc > tau (strict: within a split v ascends, so a later candidate that ties the k-th
//       loses) and ballots per accumulator register; a zero ballot costs one scalar branch.
//       Otherwise the passing lanes drop v >= n and append their keys at the positions the ballot's
//       prefix counts give.  After a tile, a query whose count exceeds cap - 64 (a tile adds at most
//       64) is pruned: the wave takes the buffer's keys (64 E of them, E per lane), drops the new
//       ones found in X by binary search (all lanes at once: X never costs the appends a lookup),
//       sorts (a bitonic network over shuffles), keeps the k best and refreshes tau.
//       Every query is pruned once more at the end of the range, which leaves k keys in descending
//       order (0 where the split had fewer candidates) at the front of its buffer.
//   k_topk_merge<E>: a wave per query folds the splits' k keys, one split at a time, into its k
//       best by the same sort, and writes idx / score with the padding (-1, -inf).
// Two launches whatever the data.  No atomics; every step is a function of the inputs alone, so two
// calls give the same bits.
#include <algorithm>
#include <climits>

#include "common.hpp"
#include "kernels.hpp"
#include "rank_sweep.hpp"

#pragma clang fp contract(off)

namespace pgcn {

namespace {
typedef unsigned long long u64;

__device__ __forceinline__ u64 topk_key(float s, int v) {
  s = s + 0.0f;  // -0 -> +0: the key must not see a zero's sign
  const unsigned b = __float_as_uint(s);
  const unsigned o = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((u64)o << 32) | (u64)(~(unsigned)v);
}
__device__ __forceinline__ float topk_key_score(u64 key) {
  const unsigned o = (unsigned)(key >> 32);
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// lanes of one wave exchange data through memory: what was stored before is visible after
__device__ __forceinline__ void wave_mem_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// the wave's 64 E keys, element i = 64 e + lane in key[e], into descending order of i
template <int E>
__device__ __forceinline__ void wave_sort_desc(u64 (&key)[E], int lane) {
#pragma unroll
  for (int k2 = 2; k2 <= 64 * E; k2 <<= 1) {
#pragma unroll
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      if (j >= 64) {  // partners are registers of one lane; the block's direction is e's alone
        const int je = j / 64;
#pragma unroll
        for (int e = 0; e < E; e++) {
          if (e & je) continue;
          const bool desc = ((64 * e) & k2) == 0;
          const u64 a = key[e], b = key[e | je];
          const u64 hi = a > b ? a : b, lo = a > b ? b : a;
          key[e] = desc ? hi : lo;
          key[e | je] = desc ? lo : hi;
        }
      } else {
#pragma unroll
        for (int e = 0; e < E; e++) {
          const u64 other = __shfl_xor(key[e], j, 64);
          const bool desc = ((64 * e + lane) & k2) == 0, lower = (lane & j) == 0;
          const u64 hi = key[e] > other ? key[e] : other, lo = key[e] > other ? other : key[e];
          key[e] = (desc == lower) ? hi : lo;
        }
      }
    }
  }
}

// element i of the sorted keys, i wave-uniform
template <int E>
__device__ __forceinline__ u64 wave_key_at(const u64 (&key)[E], int i) {
  u64 mine = key[0];
#pragma unroll
  for (int e = 1; e < E; e++) mine = (i >> 6) == e ? key[e] : mine;
  return __shfl(mine, i & 63, 64);
}

// is v in the ascending list idx[lo .. hi)
__device__ __forceinline__ bool list_holds(const int *__restrict__ idx, long long lo, long long hi,
                                           int v) {
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    const int x = idx[mid];
    if (x == v) return true;
    if (x < v) lo = mid + 1;
    else hi = mid;
  }
  return false;
}

// the whole wave: buf[0 .. count), of which the entries from `clean` on have not met the exclude
// list idx[lo .. hi) yet -> the k best of the candidates among them in descending order at
// buf[0 .. k), 0 behind the last; returns how many those are (at most k) and in *tau the k-th best
// score, -inf when there are fewer than k
template <int E>
__device__ __forceinline__ int wave_prune(u64 *buf, int count, int clean, int k, int lane,
                                          const int *__restrict__ idx, long long lo, long long hi,
                                          float *tau) {
  u64 key[E];
  int valid = 0;
#pragma unroll
  for (int e = 0; e < E; e++) {
    const int i = 64 * e + lane;
    key[e] = i < count ? buf[i] : 0ull;
    if (i >= clean && i < count && list_holds(idx, lo, hi, (int)~(unsigned)key[e])) key[e] = 0ull;
    valid += __popcll(__ballot(key[e] != 0ull));
  }
  wave_sort_desc<E>(key, lane);
#pragma unroll
  for (int e = 0; e < E; e++)
    if (64 * e + lane < k) buf[64 * e + lane] = key[e];
  *tau = valid >= k ? topk_key_score(wave_key_at<E>(key, k - 1)) : -INFINITY;
  return min(valid, k);
}
}  // namespace

// NV: as k_rank_sweep.  E: keys per lane of a prune, the append buffers hold cap = 64 E >= k + 64
template <int NV, int E>
__global__ __launch_bounds__(kRankThreads) void k_topk_sweep(
    const int *__restrict__ anchor, const long long *__restrict__ xptr,
    const int *__restrict__ xidx, int Q, int n, int k, const float *__restrict__ H, int ld_h, int d,
    int tiles, int tiles_per_split, u64 *__restrict__ ws) {
  using L = SweepLds<NV>;
  constexpr int S = L::S, HD = L::HD, CAP = 64 * E;
  __shared__ float lds[L::kFloats];
  __shared__ float tau_s[kRankTQ];
  __shared__ int cnt_s[kRankTQ], clean_s[kRankTQ];
  float *As = lds, *Bs = lds + kRankTQ * S;

  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const int half = lane >> 5, col = lane & 31;
  const int q0 = blockIdx.x * kRankTQ;
  const int t_begin = blockIdx.y * tiles_per_split;
  const int t_end = min(tiles, t_begin + tiles_per_split);
  if (t_begin >= t_end) return;
  const int splits = gridDim.y;

  sweep_gather_anchors<NV>(As, anchor, q0, Q, H, ld_h, d, n, tid);
  float4 stage[NV];
  sweep_load_tile<NV>(stage, H, ld_h, d, n, t_begin, tid);
  sweep_store_tile<NV>(Bs, stage, tid);

  // per accumulator register (a query row per lane half): the threshold and the buffer's count
  float th[16];
  int cnt[16];
#pragma unroll
  for (int r = 0; r < 16; r++) {
    th[r] = q0 + 32 * wave + sweep_row(r, half) < Q ? -INFINITY : INFINITY;
    cnt[r] = 0;
  }
  const unsigned below = (1u << col) - 1u;
  if (tid < kRankTQ) clean_s[tid] = 0;
  __syncthreads();

  const int groups = (d + 7) / 8;
  const float *a_row = As + (32 * wave + col) * S + half * HD;
  for (int t = t_begin; t < t_end; t++) {
    const int cur = (t - t_begin) & 1;
    const bool more = t + 1 < t_end;
    if (more) sweep_load_tile<NV>(stage, H, ld_h, d, n, t + 1, tid);
    const float *b_row = Bs + cur * (kRankTC * S) + col * S + half * HD;
    f32x16 acc0, acc1;
    sweep_mfma<S>(a_row, b_row, groups, acc0, acc1);
    const int v0 = t * kRankTC + col, v1 = v0 + 32;
    int most = 0;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      bool p0 = acc0[r] > th[r], p1 = acc1[r] > th[r];
      if (__ballot(p0 || p1) == 0ull) continue;
      // (th = +inf beyond Q: a passing lane's query exists)
      const int q = q0 + 32 * wave + sweep_row(r, half);
      p0 = p0 && v0 < n;
      p1 = p1 && v1 < n;
      const unsigned m0 = (unsigned)(__ballot(p0) >> (32 * half));
      const unsigned m1 = (unsigned)(__ballot(p1) >> (32 * half));
      const int c0 = __popc(m0);
      // (cnt <= CAP - 64 before a tile, a tile adds at most 64: every position is below CAP)
      u64 *buf = ws + ((long long)q * splits + blockIdx.y) * CAP;
      if (p0) buf[cnt[r] + __popc(m0 & below)] = topk_key(acc0[r], v0);
      if (p1) buf[cnt[r] + c0 + __popc(m1 & below)] = topk_key(acc1[r], v1);
      cnt[r] += c0 + __popc(m1);
      most = max(most, cnt[r]);
    }
    const bool last = !more;
    if (last || __ballot(most > CAP - 64) != 0ull) {
      // the wave's queries that are due, one after the other
      if (col == 0) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
          tau_s[32 * wave + sweep_row(r, half)] = th[r];
          cnt_s[32 * wave + sweep_row(r, half)] = cnt[r];
        }
      }
      wave_mem_sync();
      for (int row = 0; row < 32; row++) {
        const int q = q0 + 32 * wave + row;
        const int c = cnt_s[32 * wave + row];
        if (q >= Q || !(last || c > CAP - 64)) continue;
        const long long lo = xptr ? xptr[q] : 0, hi = xptr ? xptr[q + 1] : 0;
        float tau;
        const int kept = wave_prune<E>(ws + ((long long)q * splits + blockIdx.y) * CAP, c,
                                       clean_s[32 * wave + row], k, lane, xidx, lo, hi, &tau);
        if (lane == 0) {
          tau_s[32 * wave + row] = tau;
          cnt_s[32 * wave + row] = kept;
          clean_s[32 * wave + row] = kept;
        }
      }
      wave_mem_sync();
#pragma unroll
      for (int r = 0; r < 16; r++) {
        th[r] = tau_s[32 * wave + sweep_row(r, half)];
        cnt[r] = cnt_s[32 * wave + sweep_row(r, half)];
      }
    }
    if (more) sweep_store_tile<NV>(Bs + (cur ^ 1) * (kRankTC * S), stage, tid);
    __syncthreads();
  }
}

// a wave per query: the k best of its splits' k keys, then idx / score with the padding
template <int E>
__global__ __launch_bounds__(kRankThreads) void k_topk_merge(const u64 *__restrict__ ws, int Q,
                                                             int splits, int k,
                                                             int *__restrict__ idx,
                                                             float *__restrict__ score) {
  constexpr int CAP = 64 * E, HALF = E / 2;
  const int lane = threadIdx.x % kWave;
  const int q = blockIdx.x * (kRankThreads / kWave) + threadIdx.x / kWave;
  if (q >= Q) return;
  u64 key[E];
#pragma unroll
  for (int e = 0; e < E; e++) key[e] = 0ull;
  for (int s = 0; s < splits; s++) {
    const u64 *buf = ws + ((long long)q * splits + s) * CAP;
    // (the running best sits sorted in the elements below 64 HALF >= k; the split's keys go behind)
#pragma unroll
    for (int e = 0; e < HALF; e++)
      key[HALF + e] = 64 * e + lane < k ? buf[64 * e + lane] : 0ull;
    wave_sort_desc<E>(key, lane);
  }
#pragma unroll
  for (int e = 0; e < HALF; e++) {
    const int i = 64 * e + lane;
    if (i < k) {
      const u64 x = key[e];
      idx[(long long)q * k + i] = x ? (int)~(unsigned)x : -1;
      score[(long long)q * k + i] = x ? topk_key_score(x) : -INFINITY;
    }
  }
}

int topk_splits(long long Q, int n) {
  const int q = (int)std::min<long long>(std::max<long long>(Q, 1), INT_MAX);
  const long long tiles = ceil_div(std::max(n, 1), kRankTC);
  // rank_splits' ranges of ceil(tiles / splits) tiles; the splits that hold a tile
  return (int)ceil_div(tiles, ceil_div(tiles, rank_splits(q, n)));
}

int topk_cap(int k) { return k <= 64 ? 128 : 256; }

long long topk_workspace_bytes(long long Q, int n, int k) {
  return Q * topk_splits(Q, n) * topk_cap(k) * (long long)sizeof(u64);
}

void launch_link_topk(const TopKQueries &q, const float *H, int ld_h, int d, int *idx, float *score,
                      hipStream_t s) {
  PGCN_CHECK(d >= 1 && d <= kLinkMaxWidth && q.n >= 1 && q.n_queries >= 0 && q.k >= 1 &&
                 q.k <= kTopKMax,
             PGCN_E_INVALID, "link_topk: 1 <= d <= 128, 1 <= k <= 128");
  if (q.n_queries == 0) return;
  const int Q = q.n_queries;
  const int tiles = (int)ceil_div(q.n, kRankTC), splits = topk_splits(Q, q.n);
  const int tps = (int)ceil_div(tiles, splits);
  // (every split of the grid holds a tile: the merge reads all of them)
  PGCN_CHECK(q.splits == splits && (int)ceil_div(tiles, tps) == splits && q.ws, PGCN_E_INVALID,
             "link_topk: the handle's workspace does not fit its queries");
  const dim3 grid((unsigned)ceil_div(Q, kRankTQ), (unsigned)q.splits);
  u64 *ws = reinterpret_cast<u64 *>(q.ws);
  note_path(KP_TOPK_SWEEP);
#define TOPK_SWEEP_E(NV, E)                                                                    \
  PGCN_LAUNCH((k_topk_sweep<NV, E>), grid, dim3(kRankThreads), 0, s, q.anchor, q.exclude_ptr, \
              q.exclude_idx, Q, q.n, q.k, H, ld_h, d, tiles, tps, ws)
#define TOPK_SWEEP(NV)                \
  do {                                \
    if (q.k <= 64) TOPK_SWEEP_E(NV, 2); \
    else TOPK_SWEEP_E(NV, 4);         \
  } while (0)
  PGCN_SWEEP_BY_WIDTH(d, TOPK_SWEEP);
#undef TOPK_SWEEP
#undef TOPK_SWEEP_E
  note_path(KP_TOPK_MERGE);
  const dim3 mgrid((unsigned)ceil_div(Q, kRankThreads / kWave));
  if (q.k <= 64)
    PGCN_LAUNCH((k_topk_merge<2>), mgrid, dim3(kRankThreads), 0, s, ws, Q, q.splits, q.k, idx, score);
  else
    PGCN_LAUNCH((k_topk_merge<4>), mgrid, dim3(kRankThreads), 0, s, ws, Q, q.splits, q.k, idx, score);
}

}  // namespace pgcn
