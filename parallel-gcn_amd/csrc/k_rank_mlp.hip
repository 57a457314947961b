// parallel-gcn_amd/csrc/k_rank_mlp.hip -- link prediction's 1-vs-all ranking under the Hadamard-MLP
// decoder for gfx950 (the reference has no pair-level model): for every query (anchor a, target t)
// the number of candidates v in [0, n) whose decoder score is above, and the number whose score is
// exactly, the score of (a, t) -- k_rank.hip's counts, for k_link_mlp.hip's score -- without the
// [Q][n] score matrix and without the Q n explicit pairs the pair forward would need.
//
// The score is the forward's, bit for bit: z[i] = H[a][i] * H[v][i] (one rounded product), pre[u]
// accumulated on v_mfma_f32_32x32x2_f32 from zero with i ascending to round_up8(d), then
// link_mlp_tile.hpp's epilogue in its one order.  The ReLU keeps the score from being folded onto
// the nodes, so every (query, candidate) pair pays the [d] x [d][h] contraction.
//
//   thresholds: launch_link_mlp_fwd itself on the pair view (anchor, target) of the query set, into
//       the handle's [Q][4] scratch; k_rank_mlp_zero clears the counts.
//   k_rank_mlp_sweep<ND, UT>: a workgroup of 4 waves owns kRankMlpTQ = 64 queries and a range of
//       kRankMlpTC = 64-candidate chunks (grid: query blocks x candidate splits).  LDS holds, for the
//       workgroup's whole life, the forward's image -- W1^T in the split layout, b1, w2 -- with the
//       candidate chunk where the forward keeps its z tile, and the block's anchor rows behind it;
//       thresholds and targets sit in the image's G / partials words.  Wave w owns the chunk's
//       candidate block w & 1 (candidate = lane & 31) and the queries (w >> 1), (w >> 1) + 2, ...
//       of the block.  Per query it forms the MFMA's B operand on the fly -- a v_mul of an anchor
//       float4 (a broadcast read) and its candidate float4 -- and runs ALL UT unit tiles, so the sum
//       over units never leaves the wave: accumulators acc[uh][q] are the forward's wave uh, tile
//       uh + 2 q; the two lane sums take mlp_lane_sum, each its __shfl_xor(32), then
//       red[0] + red[1], then + b2 as mlp_tile_score has them.  No z buffer, no LDS write and no
//       barrier per query; two barriers per chunk (the next chunk's rows are loaded into registers
//       under this chunk's MFMAs).  Both lane halves then hold the candidate's score: compared with
//       the threshold, v >= n and v == t_e masked, two ballots; lane l of the wave keeps the count
//       of the wave's l-th query (lanes 0 .. 31 greater, 32 .. 63 equal) in ONE register, and at
//       the end of the range adds it to the query's word (unsigned integer atomics: order-free).
//   k_rank_mlp_filter<ND, UT>: the (anchor, filter entry) pairs in 64-pair tiles through the
//       forward's own tile code (z staged in LDS, mlp_pre, mlp_lane_sum, mlp_tile_score); an entry
//       the sweep counted leaves its query's counts (integer atomics).
// Every count is an integer sum: two calls give the same bits.
// The staging and a query's score (the MFMA loop and the epilogue) live in rank_mlp_sweep.hpp, shared
// with k_topk_mlp.hip.
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"
#include "rank_sweep.hpp"
#include "link_mlp_tile.hpp"
#include "rank_mlp_sweep.hpp"

#pragma clang fp contract(off)

namespace pgcn {
__global__ __launch_bounds__(kMlpThreads) void k_rank_mlp_zero(unsigned *__restrict__ a,
                                                               unsigned *__restrict__ b, int Q) {
  for (int e = blockIdx.x * kMlpThreads + threadIdx.x; e < Q; e += gridDim.x * kMlpThreads)
    a[e] = b[e] = 0u;
}

template <int ND, int UT>
__global__ __launch_bounds__(kMlpThreads) void k_rank_mlp_sweep(
    const int *__restrict__ anchor, const int *__restrict__ target, const float *__restrict__ thr,
    int Q, int n, const float *__restrict__ H, int ld_h, int d, const float *__restrict__ P,
    int ld_p, int h, int chunks, int chunks_per_split, unsigned *__restrict__ greater,
    unsigned *__restrict__ equal) {
  using L = MlpLds<ND, UT>;
  __shared__ __attribute__((aligned(16))) float lds[L::kFwdFloats + kRankMlpTQ * L::S];
  float *As = lds + L::kFwdFloats, *Cs = lds + L::oZ;
  int *tgs = reinterpret_cast<int *>(lds + L::oRed);
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const int half = lane >> 5, col = lane & 31, cb = wave & 1, qh = wave >> 1;
  const int q0 = blockIdx.x * kRankMlpTQ;
  const int c_begin = blockIdx.y * chunks_per_split;
  const int c_end = min(chunks, c_begin + chunks_per_split);
  if (c_begin >= c_end) return;

  mlp_stage_params<ND, UT>(lds, P, ld_p, d, h, tid);
  const float b2 = P[(long long)(d + 2) * ld_p];
  float4 stage[L::NG];
  // the block's anchor rows (zero rows from Q on), thresholds and targets, once
  rank_mlp_gather_anchors<ND, UT>(As, stage, anchor, q0, Q, H, ld_h, d, n, tid);
  if (tid < kRankMlpTQ) {
    const int q = q0 + tid;
    lds[L::oG + tid] = q < Q ? thr[4 * (long long)q] : 0.0f;
    tgs[tid] = q < Q ? target[q] : -1;
  }
  const int nq = min(kRankMlpTQ, Q - q0);  // the block's queries
  rank_mlp_load_chunk<ND, UT>(stage, H, ld_h, d, n, c_begin, tid);

  const int groups = (d + 7) / 8;
  const float *c_row = Cs + (cb * 32 + col) * L::S + half * L::HD;
  const float *w_row = lds + L::oW1 + col * L::S + half * L::HD;
  unsigned cnt = 0u;  // of query q0 + qh + 2 col: greater (half 0) / equal (half 1)
  for (int c = c_begin; c < c_end; c++) {
    rank_mlp_store_rows<ND, UT>(Cs, stage, tid);
    __syncthreads();
    if (c + 1 < c_end) rank_mlp_load_chunk<ND, UT>(stage, H, ld_h, d, n, c + 1, tid);
    const int v = c * kRankMlpTC + cb * 32 + col;
    for (int qi = 0; qh + 2 * qi < nq; qi++) {
      const int qs = qh + 2 * qi;
      const float *a_row = As + qs * L::S + half * L::HD;
      const float s = rank_mlp_query_score<ND, UT>(lds, a_row, c_row, w_row, groups, b2, half);
      const float th = lds[L::oG + qs];
      const bool ok = v < n && v != tgs[qs];
      const unsigned long long bg = __ballot(ok && s > th), be = __ballot(ok && s == th);
      // (both lane halves hold every candidate: its low 32 lanes are the block)
      const unsigned add = (unsigned)__popc((unsigned)(half ? be : bg));
      cnt += col == qi ? add : 0u;
    }
    __syncthreads();
  }
  const int q = q0 + qh + 2 * col;
  if (q < Q && cnt) atomicAdd((half ? equal : greater) + q, cnt);
}

// the pair (anchor of query e, F_e's entry) for every filter entry p in [0, F): its forward score
// through the forward's tile code; what the sweep counted for it leaves the counts
template <int ND, int UT>
__global__ __launch_bounds__(kMlpThreads) void k_rank_mlp_filter(
    const int *__restrict__ anchor, const float *__restrict__ thr,
    const long long *__restrict__ fptr, const int *__restrict__ fidx, int Q, long long F, int n,
    const float *__restrict__ H, int ld_h, int d, const float *__restrict__ P, int ld_p, int h,
    unsigned *__restrict__ greater, unsigned *__restrict__ equal) {
  using L = MlpLds<ND, UT>;
  __shared__ __attribute__((aligned(16))) float lds[L::kFwdFloats];
  int *qe = reinterpret_cast<int *>(lds + L::oG);  // the query of the tile's pair
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const long long tiles = (F + kLinkMlpTile - 1) / kLinkMlpTile;
  const int groups = (d + 7) / 8;

  mlp_stage_params<ND, UT>(lds, P, ld_p, d, h, tid);
  const float b2 = P[(long long)(d + 2) * ld_p];
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const long long p = t * kLinkMlpTile + tid;
    if (tid < kLinkMlpTile) {
      // the last e with fptr[e] <= p (fptr[0] = 0, fptr[Q] = F > p)
      const long long pc = min(p, F - 1);
      int lo = 0, hi = Q;
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (fptr[mid] <= pc) lo = mid; else hi = mid;
      }
      qe[tid] = lo;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < L::NG; i++) {
      const int idx = i * kMlpThreads + tid, row = idx / L::CPR, ch = idx % L::CPR;
      const long long pr = t * kLinkMlpTile + row;
      const float4 a = load_chunk(H, ld_h, d, n, anchor[qe[row]], ch);
      const float4 b = load_chunk(H, ld_h, d, n, fidx[min(pr, F - 1)], ch);
      const float4 z = make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
      put_split<L::HD>(lds + L::oZ + row * L::S, ch,
                       pr < F ? z : make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    }
    __syncthreads();
    f32x16 acc[L::NQ];
    mlp_pre<ND, UT>(lds, groups, wave, lane, acc);
    const float v = mlp_tile_score<ND, UT>(lds, mlp_lane_sum<ND, UT>(lds, acc, wave >> 1, lane >> 5),
                                           b2, wave, lane, tid);
    if (tid < kLinkMlpTile && p < F) {
      const int e = qe[tid];
      const float th = thr[4 * (long long)e];
      if (v > th) atomicSub(greater + e, 1u);
      if (v == th) atomicSub(equal + e, 1u);
    }
  }
}

int rank_mlp_splits(int Q, int n) {
  const long long qb = ceil_div(std::max(Q, 1), kRankMlpTQ);
  const long long chunks = ceil_div(std::max(n, 1), kRankMlpTC);
  return (int)std::max<long long>(1, std::min(ceil_div(chunks, 8), ceil_div(4 * kCUs, qb)));
}

void launch_link_rank_mlp(const RankQueries &q, const float *H, int ld_h, int d, const float *P,
                          int ld_p, int h, unsigned *greater, unsigned *equal, hipStream_t s) {
  PGCN_CHECK(d >= 1 && d <= kLinkMaxWidth && h >= 1 && h <= kLinkMlpMaxHidden && q.n >= 1 &&
                 q.n_queries >= 0,
             PGCN_E_INVALID, "link_rank_mlp: 1 <= d <= 128, 1 <= h <= 128");
  if (q.n_queries == 0) return;
  const int Q = q.n_queries;
  // the thresholds: the forward on the pairs (a_e, t_e), {score, 0, 0, 0} per query
  LinkIndex view;
  view.n = q.n;
  view.n_pairs = Q;
  view.src = q.anchor;
  view.dst = q.target;
  launch_link_mlp_fwd(view, H, ld_h, d, P, ld_p, h, q.thr, 4, s);
  const unsigned zgrid = (unsigned)std::min<long long>(ceil_div(Q, kMlpThreads), 4 * kCUs);
  PGCN_LAUNCH(k_rank_mlp_zero, dim3(zgrid), dim3(kMlpThreads), 0, s, greater, equal, Q);

  const int chunks = (int)ceil_div(q.n, kRankMlpTC), splits = rank_mlp_splits(Q, q.n);
  const int cps = (int)ceil_div(chunks, splits);
  const dim3 grid((unsigned)ceil_div(Q, kRankMlpTQ), (unsigned)ceil_div(chunks, cps));
  note_path(KP_RANK_MLP_SWEEP);
#define RANK_MLP_SWEEP(ND, UT)                                                                   \
  PGCN_LAUNCH((k_rank_mlp_sweep<ND, UT>), grid, dim3(kMlpThreads), 0, s, q.anchor, q.target, q.thr, \
              Q, q.n, H, ld_h, d, P, ld_p, h, chunks, cps, greater, equal)
  MLP_BY_SHAPE(d, h, RANK_MLP_SWEEP);
#undef RANK_MLP_SWEEP
  if (q.filter_ptr && q.n_filter > 0) {
    note_path(KP_RANK_MLP_FILTER);
    const long long F = q.n_filter;
    const unsigned fgrid =
        (unsigned)std::min<long long>(ceil_div(F, kLinkMlpTile), (long long)2 * kCUs);
#define RANK_MLP_FILTER(ND, UT)                                                                  \
  PGCN_LAUNCH((k_rank_mlp_filter<ND, UT>), dim3(fgrid), dim3(kMlpThreads), 0, s, q.anchor, q.thr, \
              q.filter_ptr, q.filter_idx, Q, F, q.n, H, ld_h, d, P, ld_p, h, greater, equal)
    MLP_BY_SHAPE(d, h, RANK_MLP_FILTER);
#undef RANK_MLP_FILTER
  }
}

}  // namespace pgcn
