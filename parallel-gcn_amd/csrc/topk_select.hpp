// parallel-gcn_amd/csrc/topk_select.hpp -- the selection machinery the 1-vs-all top-K sweeps share
// (k_topk.hip under the dot product, k_topk_mlp.hip under the Hadamard-MLP decoder): the 64-bit
// selection key, a wave's bitonic sort over shuffles, the exclude-list lookup, the prune of one
// append buffer by a whole wave, and the merge kernel that folds a query's lists into idx / score.
//
// A selection key is ordered(score) << 32 | ~v: ordered() maps a float (its zero canonicalised to
// +0 first) to an unsigned that compares as the float does, so a greater key is a candidate that
// precedes.  Keys of distinct candidates are distinct; 0 is "no entry".
// Device code only; include after common.hpp, kernels.hpp and rank_sweep.hpp.
#pragma once

#include "common.hpp"
#include "kernels.hpp"
#include "rank_sweep.hpp"

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

// a wave per query: the k best of its `lists` lists' k keys (list s of query q at
// ws + (q lists + s) 64 E, sorted, 0 behind the last), then idx / score with the padding
template <int E>
__global__ __launch_bounds__(kRankThreads) void k_topk_merge(const u64 *__restrict__ ws, int Q,
                                                             int lists, int k,
                                                             int *__restrict__ idx,
                                                             float *__restrict__ score) {
  constexpr int CAP = 64 * E, HALF = E / 2;
  const int lane = threadIdx.x % kWave;
  const int q = blockIdx.x * (kRankThreads / kWave) + threadIdx.x / kWave;
  if (q >= Q) return;
  u64 key[E];
#pragma unroll
  for (int e = 0; e < E; e++) key[e] = 0ull;
  for (int s = 0; s < lists; s++) {
    const u64 *buf = ws + ((long long)q * lists + s) * CAP;
    // (the running best sits sorted in the elements below 64 HALF >= k; the list's keys go behind)
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

// keys per append buffer: 128 for k <= 64, 256 above
constexpr int topk_cap_of(int k) { return k <= 64 ? 128 : 256; }
}  // namespace
}  // namespace pgcn
