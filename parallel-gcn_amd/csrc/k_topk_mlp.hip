// parallel-gcn_amd/csrc/k_topk_mlp.hip -- link prediction's 1-vs-all retrieval under the
// Hadamard-MLP decoder for gfx950 (the reference has no pair-level model): for every query (anchor
// a, exclude list X) the k candidates v in [0, n) \ X with the highest decoder score of the pair
// (a, v) -- k_topk.hip's answer for k_link_mlp.hip's score, bit for bit -- ties to the lower index,
// without the [Q][n] score matrix and without the Q n explicit pairs the pair forward would need.
//
//   k_topk_mlp_sweep<ND, UT, E>: k_rank_mlp_sweep's workgroup, LDS image, staging and per-query
//       MFMA loop and epilogue (rank_mlp_sweep.hpp: the same code, not a copy): 4 waves own 64
//       queries and a range of 64-candidate chunks; wave w owns candidate block cb = w & 1 of every
//       chunk (candidate = lane & 31) and the queries qh + 2 qi, qh = w >> 1, of the block.  That
//       sweep hands over ONE query's 32 scores at a time, the same in both lane halves, so the
//       selecting epilogue is not the dot sweep's (16 registers x 32 queries at once): the query is
//       wave-uniform, and so is everything decided about it.
//       Selection state is per (query, split, cb) and therefore wave-private -- no atomics, nothing
//       crosses waves: a threshold tau (-inf until a prune has seen k candidates, then the k-th
//       best score as of the last prune), the count of the append buffer and the count that has met
//       the exclude list, in 1.5 KiB of LDS at [32 wave + qi] (written by lane 0, read as a
//       broadcast; no register is held across the MFMA loop for them), and an append buffer of
//       cap = 64 E keys in the handle's workspace, list 2 split + cb of the query.
//       Per query: pass = s > tau && v < n (strict: within a list v ascends, so a later candidate
//       that ties the k-th loses), one ballot, its low 32 bits.  Zero is the common case: one
//       scalar branch.  Otherwise lanes 0 .. 31 append topk_key(s, v) at count + popc(mask & below).
//       A query adds at most 32 keys per chunk, so it is pruned right there when count > cap - 32,
//       by the whole wave (topk_select.hpp's wave_prune: exclude-list binary search on the entries
//       appended since the last prune, bitonic sort, the k best written back, tau refreshed from
//       candidates only); the accumulators are dead by then.  In the range's last chunk every
//       query of every wave is pruned, whatever its block saw, so every list the merge reads holds
//       its k keys in descending order, 0 behind the last.
//   k_topk_merge<E> (topk_select.hpp), unchanged: a wave per query folds its 2 x splits lists.
// Two launches whatever the data.  Every step is a function of the inputs alone: two calls give the
// same bits.
#include <algorithm>
#include <climits>

#include "common.hpp"
#include "kernels.hpp"
#include "rank_sweep.hpp"
#include "link_mlp_tile.hpp"
#include "rank_mlp_sweep.hpp"
#include "topk_select.hpp"

#pragma clang fp contract(off)

namespace pgcn {

// ND, UT: as k_rank_mlp_sweep.  E: keys per lane of a prune, the append buffers hold
// cap = 64 E >= k + 32
template <int ND, int UT, int E>
__global__ __launch_bounds__(kMlpThreads) void k_topk_mlp_sweep(
    const int *__restrict__ anchor, const long long *__restrict__ xptr,
    const int *__restrict__ xidx, int Q, int n, int k, const float *__restrict__ H, int ld_h, int d,
    const float *__restrict__ P, int ld_p, int h, int chunks, int chunks_per_split,
    u64 *__restrict__ ws) {
  using L = MlpLds<ND, UT>;
  constexpr int CAP = 64 * E, kSlots = 2 * kRankMlpTQ;  // a slot per (query, cb): [32 wave + qi]
  __shared__ __attribute__((aligned(16))) float lds[L::kFwdFloats + kRankMlpTQ * L::S];
  __shared__ float tau_s[kSlots];
  __shared__ int cnt_s[kSlots], clean_s[kSlots];
  float *As = lds + L::kFwdFloats, *Cs = lds + L::oZ;
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const int half = lane >> 5, col = lane & 31, cb = wave & 1, qh = wave >> 1;
  const int q0 = blockIdx.x * kRankMlpTQ;
  const int c_begin = blockIdx.y * chunks_per_split;
  const int c_end = min(chunks, c_begin + chunks_per_split);
  if (c_begin >= c_end) return;  // (never: the host counts the splits that hold a chunk)
  const int lists = 2 * gridDim.y;

  mlp_stage_params<ND, UT>(lds, P, ld_p, d, h, tid);
  const float b2 = P[(long long)(d + 2) * ld_p];
  float4 stage[L::NG];
  rank_mlp_gather_anchors<ND, UT>(As, stage, anchor, q0, Q, H, ld_h, d, n, tid);
  if (tid < kSlots) {
    tau_s[tid] = -INFINITY;
    cnt_s[tid] = 0;
    clean_s[tid] = 0;
  }
  const int nq = min(kRankMlpTQ, Q - q0);  // the block's queries
  rank_mlp_load_chunk<ND, UT>(stage, H, ld_h, d, n, c_begin, tid);

  const int groups = (d + 7) / 8;
  const float *c_row = Cs + (cb * 32 + col) * L::S + half * L::HD;
  const float *w_row = lds + L::oW1 + col * L::S + half * L::HD;
  const unsigned below = (1u << col) - 1u;
  for (int c = c_begin; c < c_end; c++) {
    rank_mlp_store_rows<ND, UT>(Cs, stage, tid);
    __syncthreads();
    const bool last = c + 1 == c_end;
    if (!last) rank_mlp_load_chunk<ND, UT>(stage, H, ld_h, d, n, c + 1, tid);
    const int v = c * kRankMlpTC + cb * 32 + col;
    for (int qi = 0; qh + 2 * qi < nq; qi++) {
      const int qs = qh + 2 * qi, slot = 32 * wave + qi;
      const float *a_row = As + qs * L::S + half * L::HD;
      const float s = rank_mlp_query_score<ND, UT>(lds, a_row, c_row, w_row, groups, b2, half);
      const bool pass = s > tau_s[slot] && v < n;
      // (both lane halves hold every candidate: the ballot's low 32 lanes are the block)
      const unsigned m = (unsigned)__ballot(pass);
      if (m == 0u && !last) continue;
      const int q = q0 + qs;
      u64 *buf = ws + ((long long)q * lists + 2 * blockIdx.y + cb) * CAP;
      int count = cnt_s[slot];
      // (count <= CAP - 32 before a chunk, a chunk adds at most 32: every position is below CAP)
      if (pass && half == 0) buf[count + __popc(m & below)] = topk_key(s, v);
      count += __popc(m);
      if (last || count > CAP - 32) {
        wave_mem_sync();
        const long long lo = xptr ? xptr[q] : 0, hi = xptr ? xptr[q + 1] : 0;
        float tau;
        const int kept = wave_prune<E>(buf, count, clean_s[slot], k, lane, xidx, lo, hi, &tau);
        if (lane == 0) {
          tau_s[slot] = tau;
          cnt_s[slot] = kept;
          clean_s[slot] = kept;
        }
      } else if (lane == 0) {
        cnt_s[slot] = count;
      }
      wave_mem_sync();
    }
    __syncthreads();
  }
}

int topk_mlp_splits(long long Q, int n) {
  const int q = (int)std::min<long long>(std::max<long long>(Q, 1), INT_MAX);
  const long long chunks = ceil_div(std::max(n, 1), kRankMlpTC);
  // rank_mlp_splits' ranges of ceil(chunks / splits) chunks; the splits that hold a chunk
  return (int)ceil_div(chunks, ceil_div(chunks, rank_mlp_splits(q, n)));
}

long long topk_mlp_workspace_bytes(long long Q, int n, int k) {
  return Q * topk_mlp_splits(Q, n) * 2 * topk_cap(k) * (long long)sizeof(u64);
}

void launch_link_topk_mlp(const TopKQueries &q, const float *H, int ld_h, int d, const float *P,
                          int ld_p, int h, int *idx, float *score, hipStream_t s) {
  PGCN_CHECK(d >= 1 && d <= kLinkMaxWidth && h >= 1 && h <= kLinkMlpMaxHidden && q.n >= 1 &&
                 q.n_queries >= 0 && q.k >= 1 && q.k <= kTopKMax,
             PGCN_E_INVALID, "link_topk_mlp: 1 <= d <= 128, 1 <= h <= 128, 1 <= k <= 128");
  PGCN_CHECK(q.mlp, PGCN_E_INVALID,
             "link_topk_mlp: the handle's workspace was sized for the dot sweep "
             "(pgcn_topk_queries_create_mlp)");
  if (q.n_queries == 0) return;
  const int Q = q.n_queries;
  const int chunks = (int)ceil_div(q.n, kRankMlpTC), splits = topk_mlp_splits(Q, q.n);
  const int cps = (int)ceil_div(chunks, splits);
  // (every split of the grid holds a chunk: the merge reads all of them)
  PGCN_CHECK(q.splits == splits && (int)ceil_div(chunks, cps) == splits && q.ws, PGCN_E_INVALID,
             "link_topk_mlp: the handle's workspace does not fit its queries");
  const dim3 grid((unsigned)ceil_div(Q, kRankMlpTQ), (unsigned)splits);
  u64 *ws = reinterpret_cast<u64 *>(q.ws);
  note_path(KP_TOPK_MLP_SWEEP);
#define TOPK_MLP_SWEEP(ND, UT)                                                                    \
  do {                                                                                            \
    if (q.k <= 64)                                                                                \
      PGCN_LAUNCH((k_topk_mlp_sweep<ND, UT, 2>), grid, dim3(kMlpThreads), 0, s, q.anchor,         \
                  q.exclude_ptr, q.exclude_idx, Q, q.n, q.k, H, ld_h, d, P, ld_p, h, chunks, cps, \
                  ws);                                                                            \
    else                                                                                          \
      PGCN_LAUNCH((k_topk_mlp_sweep<ND, UT, 4>), grid, dim3(kMlpThreads), 0, s, q.anchor,         \
                  q.exclude_ptr, q.exclude_idx, Q, q.n, q.k, H, ld_h, d, P, ld_p, h, chunks, cps, \
                  ws);                                                                            \
  } while (0)
  MLP_BY_SHAPE(d, h, TOPK_MLP_SWEEP);
#undef TOPK_MLP_SWEEP
  note_path(KP_TOPK_MLP_MERGE);
  const dim3 mgrid((unsigned)ceil_div(Q, kRankThreads / kWave));
  if (q.k <= 64)
    PGCN_LAUNCH((k_topk_merge<2>), mgrid, dim3(kRankThreads), 0, s, ws, Q, 2 * splits, q.k, idx,
                score);
  else
    PGCN_LAUNCH((k_topk_merge<4>), mgrid, dim3(kRankThreads), 0, s, ws, Q, 2 * splits, q.k, idx,
                score);
}

}  // namespace pgcn
