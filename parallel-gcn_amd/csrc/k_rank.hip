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
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace pgcn {

namespace {
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kRankThreads = 256;

// r(a, v) over d columns of two rows (16-byte aligned, readable up to round_up4(d))
__device__ __forceinline__ float chain_score(const float *__restrict__ a,
                                             const float *__restrict__ b, int d) {
  float s = 0.0f;
  int c = 0;
  for (; c + 4 <= d; c += 4) {
    const float4 x = *reinterpret_cast<const float4 *>(a + c);
    const float4 y = *reinterpret_cast<const float4 *>(b + c);
    s = __fmaf_rn(x.x, y.x, s);
    s = __fmaf_rn(x.y, y.y, s);
    s = __fmaf_rn(x.z, y.z, s);
    s = __fmaf_rn(x.w, y.w, s);
  }
  if (c < d) {
    const float4 x = *reinterpret_cast<const float4 *>(a + c);
    const float4 y = *reinterpret_cast<const float4 *>(b + c);
    s = __fmaf_rn(x.x, y.x, s);
    if (c + 1 < d) s = __fmaf_rn(x.y, y.y, s);
    if (c + 2 < d) s = __fmaf_rn(x.z, y.z, s);
  }
  return s;
}
}  // namespace

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

namespace {
// the float4 at columns 4 ch .. 4 ch + 3 into a split row: even columns at [0, HD), odd at [HD, 2 HD)
template <int HD>
__device__ __forceinline__ void put_split(float *row, int ch, float4 v) {
  *reinterpret_cast<float2 *>(row + 2 * ch) = make_float2(v.x, v.z);
  *reinterpret_cast<float2 *>(row + HD + 2 * ch) = make_float2(v.y, v.w);
}

// the float4 at chunk ch of row `node` of H (always loaded, from a clamped address), zero where
// the row or the column does not exist
__device__ __forceinline__ float4 load_chunk(const float *__restrict__ H, int ld_h, int d, int n,
                                             int node, int ch) {
  const int c0 = 4 * ch, last = ((d + 3) / 4 - 1) * 4;
  const float4 r = *reinterpret_cast<const float4 *>(H + (long long)min(node, n - 1) * ld_h +
                                                     min(c0, last));
  const bool row_on = node < n;
  float4 v;
  v.x = row_on && c0 < d ? r.x : 0.0f;
  v.y = row_on && c0 + 1 < d ? r.y : 0.0f;
  v.z = row_on && c0 + 2 < d ? r.z : 0.0f;
  v.w = row_on && c0 + 3 < d ? r.w : 0.0f;
  return v;
}
}  // namespace

// NV: float4s a thread stages per candidate tile; LDS rows hold W = 16 NV >= round_up8(d) columns
template <int NV>
__global__ __launch_bounds__(kRankThreads) void k_rank_sweep(
    const int *__restrict__ anchor, const int *__restrict__ target, const float *__restrict__ thr,
    int Q, int n, const float *__restrict__ H, int ld_h, int d, int tiles, int tiles_per_split,
    unsigned *__restrict__ greater, unsigned *__restrict__ equal) {
  constexpr int W = 16 * NV, S = W + 4, HD = W / 2, CPR = 4 * NV;
  __shared__ float lds[(kRankTQ + 2 * kRankTC) * S];
  float *As = lds, *Bs = lds + kRankTQ * S;

  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const int half = lane >> 5, col = lane & 31;
  const int q0 = blockIdx.x * kRankTQ;
  const int t_begin = blockIdx.y * tiles_per_split;
  const int t_end = min(tiles, t_begin + tiles_per_split);
  if (t_begin >= t_end) return;

  // the anchors' rows, once
#pragma unroll
  for (int i = 0; i < 2 * NV; i++) {
    const int idx = i * kRankThreads + tid, row = idx / CPR, ch = idx % CPR, q = q0 + row;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (q < Q) v = load_chunk(H, ld_h, d, n, anchor[q], ch);
    put_split<HD>(As + row * S, ch, v);
  }
  float4 stage[NV];
#pragma unroll
  for (int i = 0; i < NV; i++) {
    const int idx = i * kRankThreads + tid;
    stage[i] = load_chunk(H, ld_h, d, n, t_begin * kRankTC + idx / CPR, idx % CPR);
  }
#pragma unroll
  for (int i = 0; i < NV; i++) {
    const int idx = i * kRankThreads + tid;
    put_split<HD>(Bs + (idx / CPR) * S, idx % CPR, stage[i]);
  }

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
    if (more) {
#pragma unroll
      for (int i = 0; i < NV; i++) {
        const int idx = i * kRankThreads + tid;
        stage[i] = load_chunk(H, ld_h, d, n, (t + 1) * kRankTC + idx / CPR, idx % CPR);
      }
    }
    const float *b_row = Bs + cur * (kRankTC * S) + col * S + half * HD;
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; r++) acc0[r] = acc1[r] = 0.0f;
    for (int j = 0; j < groups; j++) {
      const float4 a = *reinterpret_cast<const float4 *>(a_row + 4 * j);
      const float4 b0 = *reinterpret_cast<const float4 *>(b_row + 4 * j);
      const float4 b1 = *reinterpret_cast<const float4 *>(b_row + 32 * S + 4 * j);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0.x, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b1.x, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b0.y, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1.y, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b0.z, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b1.z, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b0.w, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b1.w, acc1, 0, 0, 0);
    }
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
    if (more) {
      float *nxt = Bs + (cur ^ 1) * (kRankTC * S);
#pragma unroll
      for (int i = 0; i < NV; i++) {
        const int idx = i * kRankThreads + tid;
        put_split<HD>(nxt + (idx / CPR) * S, idx % CPR, stage[i]);
      }
    }
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
  if (d <= 16) RANK_SWEEP(1);
  else if (d <= 32) RANK_SWEEP(2);
  else if (d <= 64) RANK_SWEEP(4);
  else RANK_SWEEP(8);
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
