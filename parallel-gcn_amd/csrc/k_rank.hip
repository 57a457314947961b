// parallel-gcn_amd/csrc/k_rank.hip -- link prediction's 1-vs-all ranking for gfx950 (the reference
// has no pair-level model): for every query (anchor a, target t) the number of candidates v in
// [0, n) that score above, and the number that score exactly, the target's score -- the counts MRR
// and Hits@K are made of -- without ever storing the [Q][n] score matrix.
//
// The rank score is a k-ordered fp32 fused chain, r(a, v) = s_d with s_0 = 0 and
// s_{c+1} = fmaf(H[a][c], H[v][c], s_c).  This is NOT k_link.hip's order (float4 partials met in
// xor butterflies): a chain is what v_mfma_f32_32x32x2_f32 computes bit for bit, so the sweep's
// MFMA tiles, the thresholds and the filter correction (plain __fmaf_rn loops) agree exactly and
// scores are compared with > and ==.  Columns >= d are staged as zeros, never multiplied from
// memory: fmaf(0, 0, s) = s up to the sign of a zero, which no comparison sees.
//
//   k_rank_scores: a lane per pair, the chain as written above; also the thresholds
//       r(a_e, t_e) of a rank call, which then zeroes the query's two counts in the same pass.
//   k_rank_sweep<NV>: a workgroup of 4 waves owns kRankTQ = 128 queries and a range of
//       kRankTC = 64-candidate tiles (grid: query blocks x candidate splits).  The anchors' rows are
//       gathered once into LDS; candidate rows H[v0 .. v0 + 64) stream through two LDS buffers
//       (float4 loads of tile t + 1 issued before the MFMAs of tile t, written after them: one
//       barrier per tile).  Wave w multiplies its 32 queries with the tile's 64 candidates: two
//       32 x 32 accumulators from zero, k ascending.  An LDS row keeps the even columns in its first
//       half and the odd ones in its second, so the lane half that feeds k = 2 s + h reads four
//       k-steps with one ds_read_b128.  The epilogue compares every accumulator element with its
//       query row's threshold into per-lane counters, masking v >= n and v == t_e in the
//       tiles that hold either (one wave-uniform test per tile).  An accumulator register is one
//       query row per lane half: at the end of its range the wave sums each counter over the 32
//       lanes of a half and adds it to the query's counts (unsigned integer atomics: order-free).
//   k_rank_filter: a wave per query walks the filter list F_e, each lane the chain of one entry,
//       and takes what the sweep counted for it out of the two counts.
// Every count is an integer sum: two calls give the same bits.
// The chain, the staging and the MFMA loop live in rank_sweep.hpp, shared with k_topk.hip.
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"
#include "rank_sweep.hpp"

#pragma clang fp contract(off)

namespace pgcn {

__global__ __launch_bounds__(kRankThreads) void k_rank_scores(
    const int *__restrict__ src, const int *__restrict__ dst, long long m,
    const float *__restrict__ H, int ld_h, int d, float *__restrict__ scores,
    unsigned *__restrict__ zero0, unsigned *__restrict__ zero1) {
  const long long stride = (long long)gridDim.x * kRankThreads;
  for (long long e = (long long)blockIdx.x * kRankThreads + threadIdx.x; e < m; e += stride) {
    scores[e] = chain_score(H + (long long)src[e] * ld_h, H + (long long)dst[e] * ld_h, d);
    if (zero0) {
      zero0[e] = 0u;
      zero1[e] = 0u;
    }
  }
}

// NV: float4s a thread stages per candidate tile; LDS rows hold W = 16 NV >= round_up8(d) columns
template <int NV>
__global__ __launch_bounds__(kRankThreads) void k_rank_sweep(
    const int *__restrict__ anchor, const int *__restrict__ target, const float *__restrict__ thr,
    int Q, int n, const float *__restrict__ H, int ld_h, int d, int tiles, int tiles_per_split,
    unsigned *__restrict__ greater, unsigned *__restrict__ equal) {
  using L = SweepLds<NV>;
  constexpr int S = L::S, HD = L::HD;
  __shared__ float lds[L::kFloats];
  float *As = lds, *Bs = lds + kRankTQ * S;

  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const int half = lane >> 5, col = lane & 31;
  const int q0 = blockIdx.x * kRankTQ;
  const int t_begin = blockIdx.y * tiles_per_split;
  const int t_end = min(tiles, t_begin + tiles_per_split);
  if (t_begin >= t_end) return;

  // the anchors' rows, once
  sweep_gather_anchors<NV>(As, anchor, q0, Q, H, ld_h, d, n, tid);
  float4 stage[NV];
  sweep_load_tile<NV>(stage, H, ld_h, d, n, t_begin, tid);
  sweep_store_tile<NV>(Bs, stage, tid);

  // accumulator register r of this lane is query row (r & 3) + 8 (r >> 2) + 4 half of the wave's 32
  float th[16];
  int tg[16];
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int q = q0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * half;
    th[r] = q < Q ? thr[q] : 0.0f;
    tg[r] = q < Q ? target[q] : -1;
  }
  // the target of query row lane & 31: a tile that holds none of the wave's targets and no
  // candidate >= n takes the epilogue without masks
  const int my_q = q0 + 32 * wave + col, my_t = my_q < Q ? target[my_q] : -1;
  unsigned cg[16], ce[16];
#pragma unroll
  for (int r = 0; r < 16; r++) cg[r] = ce[r] = 0u;
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
    const bool masked = (t + 1) * kRankTC > n ||
                        __ballot((unsigned)(my_t - t * kRankTC) < (unsigned)kRankTC) != 0ull;
    if (!masked) {
#pragma unroll
      for (int r = 0; r < 16; r++) {
        cg[r] += (acc0[r] > th[r] ? 1u : 0u) + (acc1[r] > th[r] ? 1u : 0u);
        ce[r] += (acc0[r] == th[r] ? 1u : 0u) + (acc1[r] == th[r] ? 1u : 0u);
      }
    } else {
      const bool in0 = v0 < n, in1 = v1 < n;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const bool ok0 = in0 && v0 != tg[r], ok1 = in1 && v1 != tg[r];
        cg[r] += (ok0 && acc0[r] > th[r] ? 1u : 0u) + (ok1 && acc1[r] > th[r] ? 1u : 0u);
        ce[r] += (ok0 && acc0[r] == th[r] ? 1u : 0u) + (ok1 && acc1[r] == th[r] ? 1u : 0u);
      }
    }
    if (more) sweep_store_tile<NV>(Bs + (cur ^ 1) * (kRankTC * S), stage, tid);
    __syncthreads();
  }

  // a register's counts meet over the 32 lanes of its half (one query row)
#pragma unroll
  for (int r = 0; r < 16; r++) {
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) {
      cg[r] += __shfl_xor(cg[r], off, 64);
      ce[r] += __shfl_xor(ce[r], off, 64);
    }
  }
  if (col == 0) {
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int q = q0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * half;
      if (q < Q) {
        if (cg[r]) atomicAdd(greater + q, cg[r]);
        if (ce[r]) atomicAdd(equal + q, ce[r]);
      }
    }
  }
}

// a wave per query: what the sweep counted for the entries of its filter list leaves the counts
__global__ __launch_bounds__(kRankThreads) void k_rank_filter(
    const int *__restrict__ anchor, const float *__restrict__ thr,
    const long long *__restrict__ fptr, const int *__restrict__ fidx, int Q,
    const float *__restrict__ H, int ld_h, int d, unsigned *__restrict__ greater,
    unsigned *__restrict__ equal) {
  const int lane = threadIdx.x % kWave;
  const long long stride = (long long)gridDim.x * (kRankThreads / kWave);
  for (long long e = ((long long)blockIdx.x * kRankThreads + threadIdx.x) / kWave; e < Q;
       e += stride) {
    const long long b = fptr[e], en = fptr[e + 1];
    if (b == en) continue;
    const float *a = H + (long long)anchor[e] * ld_h;
    const float t = thr[e];
    unsigned cg = 0u, ce = 0u;
    for (long long k = b + lane; k < en; k += kWave) {
      const float s = chain_score(a, H + (long long)fidx[k] * ld_h, d);
      cg += s > t ? 1u : 0u;
      ce += s == t ? 1u : 0u;
    }
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      cg += __shfl_xor(cg, off, 64);
      ce += __shfl_xor(ce, off, 64);
    }
    if (lane == 0) {
      greater[e] -= cg;
      equal[e] -= ce;
    }
  }
}

int rank_splits(int Q, int n) {
  const long long qb = ceil_div(std::max(Q, 1), kRankTQ), tiles = ceil_div(std::max(n, 1), kRankTC);
  return (int)std::max<long long>(1, std::min(ceil_div(tiles, 8), ceil_div(4 * kCUs, qb)));
}

void launch_rank_scores(const int *src, const int *dst, long long m, const float *H, int ld_h,
                        int d, float *scores, unsigned *zero0, unsigned *zero1, hipStream_t s) {
  PGCN_CHECK(d >= 1 && d <= kLinkMaxWidth && m >= 0, PGCN_E_INVALID,
             "link_rank_scores: 1 <= d <= 128");
  if (m == 0) return;
  const unsigned grid =
      (unsigned)std::min<long long>(ceil_div(m, kRankThreads), (long long)32 * kCUs);
  PGCN_LAUNCH(k_rank_scores, dim3(grid), dim3(kRankThreads), 0, s, src, dst, m, H, ld_h, d, scores,
              zero0, zero1);
}

void launch_link_rank(const RankQueries &q, const float *H, int ld_h, int d, unsigned *greater,
                      unsigned *equal, hipStream_t s) {
  PGCN_CHECK(d >= 1 && d <= kLinkMaxWidth && q.n >= 1 && q.n_queries >= 0, PGCN_E_INVALID,
             "link_rank: 1 <= d <= 128");
  if (q.n_queries == 0) return;
  const int Q = q.n_queries;
  launch_rank_scores(q.anchor, q.target, Q, H, ld_h, d, q.thr, greater, equal, s);
  const int tiles = (int)ceil_div(q.n, kRankTC), splits = rank_splits(Q, q.n);
  const int tps = (int)ceil_div(tiles, splits);
  const dim3 grid((unsigned)ceil_div(Q, kRankTQ), (unsigned)ceil_div(tiles, tps));
  note_path(KP_RANK_SWEEP);
#define RANK_SWEEP(NV)                                                                        \
  PGCN_LAUNCH((k_rank_sweep<NV>), grid, dim3(kRankThreads), 0, s, q.anchor, q.target, q.thr, Q, \
              q.n, H, ld_h, d, tiles, tps, greater, equal)
  PGCN_SWEEP_BY_WIDTH(d, RANK_SWEEP);
#undef RANK_SWEEP
  if (q.filter_ptr) {
    note_path(KP_RANK_FILTER);
    const unsigned fgrid = (unsigned)std::min<long long>(
        ceil_div(Q, kRankThreads / kWave), (long long)32 * kCUs);
    PGCN_LAUNCH(k_rank_filter, dim3(fgrid), dim3(kRankThreads), 0, s, q.anchor, q.thr,
                q.filter_ptr, q.filter_idx, Q, H, ld_h, d, greater, equal);
  }
}

}  // namespace pgcn
