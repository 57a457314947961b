// parallel-gcn_amd/csrc/k_link_mlp.hip -- link prediction's Hadamard-MLP decoder for gfx950 (the
// reference has no pair-level model): with z_e = H[src_e] o H[dst_e] over d columns and the packed
// parameter tensor P [d + 3][ld_p] (rows 0 .. d - 1: W1 [d][h], row d: b1, row d + 1: w2, row
// d + 2: {b2, 0, ...}),
//   pre_e[u] = b1[u] + sum_i z_e[i] W1[i][u],   score_e = b2 + sum_u w2[u] max(pre_e[u], 0),
// and its backward, without an [E][h] array in HBM, without float atomics, every order a function
// of (pair list, d, h) only.
//
// Both pair kernels are persistent workgroups of 256 threads that keep W1 transposed in LDS for
// their whole life -- row u holds W1[.][u], even i in the row's first half and odd i in its second
// (rank_sweep.hpp's put_split layout), so the lane half that feeds k = 2 s + half of
// v_mfma_f32_32x32x2_f32 reads four k-steps with one ds_read_b128 -- and walk the 64-pair tiles
// grid-stride.  A tile's rows are gathered with float4 loads from clamped addresses (no branch
// around a load), multiplied in registers and stored split into the z buffer; the loads of the
// workgroup's next tile are issued before this tile's MFMAs and written after them.
//
//   pre (mlp_pre, shared by forward and backward): hidden units on the MFMA's row side
//   (A = W1^T, B = z^T), so accumulator register r of a lane is unit sweep_row(r, half) of a
//   32-unit tile and ONE pair, lane & 31, of a 32-pair block.  Wave w owns pair block w & 1 and
//   the unit tiles (w >> 1), (w >> 1) + 2.
//   forward: w2[u] * max(acc + b1[u], 0) summed inside the lane over its registers and unit tiles
//   in a fixed order; one exchange across the lane halves, one add across the two waves of a pair
//   block (through LDS), + b2.  ONE launch.
//   backward, launch 1 (pairs): pre again, dhid[e][u] = G_e w2[u] [pre > 0] staged split in LDS;
//   dz = dhid W1^T ([tile][d], A = W1 read column-wise from the same LDS image, B = dhid^T) to the
//   workspace as [E][round_up4(d)]; dW1 += z^T dhid with the [d][h] accumulators resident in
//   registers over the workgroup's whole pair range (wave w owns the 32 x 32 blocks of row tiles
//   (w & 1), + 2 and unit tiles (w >> 1), + 2); db1, dw2 per lane, db2 per lane of wave 0.  At its
//   end a workgroup writes one P-shaped partial block.
//   launch 2 (reduce): the workgroups' partials added in workgroup order into dP, padding zeroed.
//   launch 3 (nodes): k_link.hip's backward over the incidence index with a vector coefficient,
//   dH[i] = sum over node i's entries of dz[pair] o H[other]; the long lists through the index's
//   segment records and the merge launch of k_link.hip (launch 4).
// One LDS image per (ND, UT) = (row width class 32 / 64 / 128, unit tiles 1 / 2 / 4); at
// d = h = 128: W1 66 KiB + z 33 KiB (+ dhid 33 KiB in the backward) + 2 KiB.
// The LDS image, mlp_pre and the forward's epilogue live in link_mlp_tile.hpp, shared with
// k_rank_mlp.hip.
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"
#include "rank_sweep.hpp"
#include "link_mlp_tile.hpp"
#include "slot_items.hpp"

#pragma clang fp contract(off)

namespace pgcn {
namespace {
// tile t: z = H[src] o H[dst] of its pairs into registers (clamped addresses, zero beyond the pair
// list and beyond column d), and G[e][0] of pair t * tile + tid (threads below the tile size)
template <int ND, int UT>
__device__ __forceinline__ void mlp_load_tile(float4 *stage, float &g,
                                              const LinkIndex &l, const float *__restrict__ H,
                                              int ld_h, int d, const float *__restrict__ G,
                                              int ld_g, long long t, int tid) {
  using L = MlpLds<ND, UT>;
  const int last = ((d + 3) / 4 - 1) * 4;
#pragma unroll
  for (int i = 0; i < L::NG; i++) {
    const int idx = i * kMlpThreads + tid, row = idx / L::CPR, c0 = 4 * (idx % L::CPR);
    const long long e = t * kLinkMlpTile + row, ec = min(e, l.n_pairs - 1);
    const int cc = min(c0, last);
    const float4 a = *reinterpret_cast<const float4 *>(H + (long long)l.src[ec] * ld_h + cc);
    const float4 b = *reinterpret_cast<const float4 *>(H + (long long)l.dst[ec] * ld_h + cc);
    const bool on = e < l.n_pairs;
    float4 v;
    v.x = on && c0 < d ? a.x * b.x : 0.0f;
    v.y = on && c0 + 1 < d ? a.y * b.y : 0.0f;
    v.z = on && c0 + 2 < d ? a.z * b.z : 0.0f;
    v.w = on && c0 + 3 < d ? a.w * b.w : 0.0f;
    stage[i] = v;
  }
  if (G) {
    const long long e = t * kLinkMlpTile + tid;
    const float r = G[min(e, l.n_pairs - 1) * ld_g];
    g = tid < kLinkMlpTile && e < l.n_pairs ? r : 0.0f;
  }
}
template <int ND, int UT>
__device__ __forceinline__ void mlp_store_tile(float *lds,
                                               const float4 *stage, int tid) {
  using L = MlpLds<ND, UT>;
#pragma unroll
  for (int i = 0; i < L::NG; i++) {
    const int idx = i * kMlpThreads + tid;
    put_split<L::HD>(lds + L::oZ + (idx / L::CPR) * L::S, idx % L::CPR, stage[i]);
  }
}
}  // namespace

template <int ND, int UT>
__global__ __launch_bounds__(kMlpThreads) void k_link_mlp_fwd(
    const LinkIndex l, const float *__restrict__ H, int ld_h, int d, const float *__restrict__ P,
    int ld_p, int h, float *__restrict__ scores, int ld_s) {
  using L = MlpLds<ND, UT>;
  __shared__ __attribute__((aligned(16))) float lds[L::kFwdFloats];
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const long long tiles = (l.n_pairs + kLinkMlpTile - 1) / kLinkMlpTile;
  const int groups = (d + 7) / 8;

  mlp_stage_params<ND, UT>(lds, P, ld_p, d, h, tid);
  const float b2 = P[(long long)(d + 2) * ld_p];
  float4 stage[L::NG];
  float g_unused = 0.0f;
  long long t = blockIdx.x;
  mlp_load_tile<ND, UT>(stage, g_unused, l, H, ld_h, d, nullptr, 0, t, tid);
  for (; t < tiles; t += gridDim.x) {
    mlp_store_tile<ND, UT>(lds, stage, tid);
    __syncthreads();
    if (t + gridDim.x < tiles)
      mlp_load_tile<ND, UT>(stage, g_unused, l, H, ld_h, d, nullptr, 0, t + gridDim.x, tid);
    f32x16 acc[L::NQ];
    mlp_pre<ND, UT>(lds, groups, wave, lane, acc);
    const float v = mlp_tile_score<ND, UT>(lds, mlp_lane_sum<ND, UT>(lds, acc, wave >> 1, lane >> 5),
                                           b2, wave, lane, tid);
    const long long e = t * kLinkMlpTile + tid;
    if (tid < kLinkMlpTile && e < l.n_pairs) {
      *reinterpret_cast<float4 *>(scores + e * ld_s) = make_float4(v, 0.0f, 0.0f, 0.0f);
    }
  }
}

// part: one [d + 3][lp] block per workgroup (the elements u < h of rows 0 .. d + 1, and [d + 2][0])
template <int ND, int UT>
__global__ __launch_bounds__(kMlpThreads) void k_link_mlp_bwd_pairs(
    const LinkIndex l, const float *__restrict__ H, int ld_h, int d, const float *__restrict__ P,
    int ld_p, int h, const float *__restrict__ G, int ld_g, float *__restrict__ dz, int ld_z,
    float *__restrict__ part, int lp) {
  using L = MlpLds<ND, UT>;
  __shared__ __attribute__((aligned(16))) float lds[L::kBwdFloats];
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const int half = lane >> 5, col = lane & 31, pb = wave & 1, uh = wave >> 1;
  const long long tiles = (l.n_pairs + kLinkMlpTile - 1) / kLinkMlpTile;
  const int groups = (d + 7) / 8, groups_u = (h + 7) / 8;
  float *ds = lds + L::oD;

  mlp_stage_params<ND, UT>(lds, P, ld_p, d, h, tid);
  f32x16 dw[L::NI][L::NQ];
  float b1a[L::NQ][16], w2a[L::NQ][16];
#pragma unroll
  for (int q = 0; q < L::NQ; q++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      b1a[q][r] = w2a[q][r] = 0.0f;
#pragma unroll
      for (int qi = 0; qi < L::NI; qi++) dw[qi][q][r] = 0.0f;
    }
  float gsum = 0.0f;

  float4 stage[L::NG];
  float g = 0.0f;
  long long t = blockIdx.x;
  mlp_load_tile<ND, UT>(stage, g, l, H, ld_h, d, G, ld_g, t, tid);
  for (; t < tiles; t += gridDim.x) {
    mlp_store_tile<ND, UT>(lds, stage, tid);
    if (tid < kLinkMlpTile) {
      lds[L::oG + tid] = g;
      gsum = gsum + g;
    }
    __syncthreads();
    if (t + gridDim.x < tiles)
      mlp_load_tile<ND, UT>(stage, g, l, H, ld_h, d, G, ld_g, t + gridDim.x, tid);

    // pre, then dhid into LDS (split rows over the units) and the lane's db1 / dw2 terms
    {
      f32x16 acc[L::NQ];
      mlp_pre<ND, UT>(lds, groups, wave, lane, acc);
      const float gp = lds[L::oG + pb * 32 + col];
#pragma unroll
      for (int q = 0; q < L::NQ; q++) {
        const int ut = uh + 2 * q;
        if (ut < UT) {
#pragma unroll
          for (int g4 = 0; g4 < 4; g4++) {
            const int u0 = 32 * ut + 8 * g4 + 4 * half;
            const float4 b1v = *reinterpret_cast<const float4 *>(lds + L::oB1 + u0);
            const float4 w2v = *reinterpret_cast<const float4 *>(lds + L::oW2 + u0);
            float dv[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
              const int r = 4 * g4 + k;
              const float pre = acc[q][r] + f4at(b1v, k);
              const float hid = fmaxf(pre, 0.0f);
              const float gh = gp * hid;
              w2a[q][r] = w2a[q][r] + gh;
              const float gw = gp * f4at(w2v, k);
              dv[k] = pre > 0.0f ? gw : 0.0f;
              b1a[q][r] = b1a[q][r] + dv[k];
            }
            put_split<L::HDU>(ds + (pb * 32 + col) * L::SU, u0 / 4,
                              make_float4(dv[0], dv[1], dv[2], dv[3]));
          }
        }
      }
    }
    __syncthreads();

    // dz[pair][i] = sum_u W1[i][u] dhid[pair][u], u ascending: pair block pb, row tiles uh, uh + 2
    {
      const float *b_row = ds + (pb * 32 + col) * L::SU + half * L::HDU;
      const long long e = t * kLinkMlpTile + pb * 32 + col;
#pragma unroll
      for (int qi = 0; qi < L::NI; qi++) {
        const int it = uh + 2 * qi;
        if (it < L::IT) {
          f32x16 acc;
#pragma unroll
          for (int r = 0; r < 16; r++) acc[r] = 0.0f;
          const float *a_col = lds + L::oW1 + half * L::S + split_pos<L::HD>(32 * it + col);
          for (int j = 0; j < groups_u; j++) {
            const float4 b = *reinterpret_cast<const float4 *>(b_row + 4 * j);
            const float *a = a_col + 8 * j * L::S;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * L::S], b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * L::S], b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[6 * L::S], b.w, acc, 0, 0, 0);
          }
          if (e < l.n_pairs) {
#pragma unroll
            for (int g4 = 0; g4 < 4; g4++) {
              const int i0 = 32 * it + 8 * g4 + 4 * half;
              if (i0 < ld_z)
                *reinterpret_cast<float4 *>(dz + e * ld_z + i0) = make_float4(
                    acc[4 * g4], acc[4 * g4 + 1], acc[4 * g4 + 2], acc[4 * g4 + 3]);
            }
          }
        }
      }
    }

    // dW1[i][u] += sum over the tile's pairs of z[pair][i] dhid[pair][u], pairs ascending
    {
      const int ib = wave & 1;
      for (int s2 = 0; s2 < kLinkMlpTile / 2; s2++) {
        const int p = 2 * s2 + half;
        float a[L::NI], b[L::NQ];
#pragma unroll
        for (int qi = 0; qi < L::NI; qi++) {
          const int it = ib + 2 * qi;
          a[qi] = it < L::IT ? lds[L::oZ + p * L::S + split_pos<L::HD>(32 * it + col)] : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < L::NQ; q++) {
          const int ut = uh + 2 * q;
          b[q] = ut < UT ? ds[p * L::SU + split_pos<L::HDU>(32 * ut + col)] : 0.0f;
        }
#pragma unroll
        for (int qi = 0; qi < L::NI; qi++)
#pragma unroll
          for (int q = 0; q < L::NQ; q++)
            if (ib + 2 * qi < L::IT && uh + 2 * q < UT)
              dw[qi][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[qi], b[q], dw[qi][q], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // this workgroup's partial block
  float *mine = part + (long long)blockIdx.x * (d + 3) * lp;
#pragma unroll
  for (int qi = 0; qi < L::NI; qi++)
#pragma unroll
    for (int q = 0; q < L::NQ; q++) {
      const int it = (wave & 1) + 2 * qi, ut = uh + 2 * q;
      if (it < L::IT && ut < UT) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int i = 32 * it + sweep_row(r, half), u = 32 * ut + col;
          if (i < d && u < h) mine[(long long)i * lp + u] = dw[qi][q][r];
        }
      }
    }
  // db1 / dw2: a register's terms meet over the 32 lanes of its half (the pairs of a block), the
  // two pair blocks through LDS ([pb][WU] of each, in the dhid buffer: the loop ended on a barrier)
#pragma unroll
  for (int q = 0; q < L::NQ; q++) {
    const int ut = uh + 2 * q;
    if (ut < UT) {
#pragma unroll
      for (int r = 0; r < 16; r++) {
        float vb = b1a[q][r], vw = w2a[q][r];
#pragma unroll
        for (int off = 1; off < 32; off <<= 1) {
          vb = vb + __shfl_xor(vb, off, 64);
          vw = vw + __shfl_xor(vw, off, 64);
        }
        if (col == 0) {
          const int u = 32 * ut + sweep_row(r, half);
          ds[pb * L::WU + u] = vb;
          ds[(2 + pb) * L::WU + u] = vw;
        }
      }
    }
  }
  if (wave == 0) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) gsum = gsum + __shfl_xor(gsum, off, 64);
    if (lane == 0) mine[(long long)(d + 2) * lp] = gsum;
  }
  __syncthreads();
  if (tid < h) {
    mine[(long long)d * lp + tid] = ds[tid] + ds[L::WU + tid];
    mine[(long long)(d + 1) * lp + tid] = ds[2 * L::WU + tid] + ds[3 * L::WU + tid];
  }
}

// dP = the partial blocks in workgroup order; zero where P holds padding
__global__ __launch_bounds__(kMlpThreads) void k_link_mlp_reduce(const float *__restrict__ part,
                                                                 int lp, int blocks, int d, int h,
                                                                 float *__restrict__ dP,
                                                                 int ld_dp) {
  const int total = (d + 3) * ld_dp;
  for (int idx = blockIdx.x * kMlpThreads + threadIdx.x; idx < total;
       idx += gridDim.x * kMlpThreads) {
    const int row = idx / ld_dp, c = idx % ld_dp;
    float s = 0.0f;
    if (c < h && (row < d + 2 || c == 0)) {
      const float *p = part + (long long)row * lp + c;
      for (int b = 0; b < blocks; b++) s = s + p[(long long)b * (d + 3) * lp];
    }
    dP[idx] = s;
  }
}

namespace {
// entries [b, e) of the incidence index: sum of dz[pair] o H[other] over the groups (every lane
// ends with the wave's sums)
template <int GL>
__device__ __forceinline__ float4 mlp_entries_sum(const LinkIndex &l, const float *__restrict__ H,
                                                  int ld_h, int d, const float *__restrict__ dz,
                                                  int ld_z, int b, int e, int lane) {
  constexpr int NB = kWave / GL;
  const int q = lane / GL, c0 = 4 * (lane % GL);
  float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (c0 < d) {
#pragma unroll 2
    for (int k = b + q; k < e; k += NB) {
      const int p = l.inc_pair[k], o = l.inc_other[k];
      const float4 g = *reinterpret_cast<const float4 *>(dz + (long long)p * ld_z + c0);
      const float4 x = row4(H + (long long)o * ld_h, c0, d, true);
      acc.x += g.x * x.x;
      acc.y += g.y * x.y;
      acc.z += g.z * x.z;
      acc.w += g.w * x.w;
    }
  }
  acc.x = across_groups<GL>(acc.x);
  acc.y = across_groups<GL>(acc.y);
  acc.z = across_groups<GL>(acc.z);
  acc.w = across_groups<GL>(acc.w);
  return acc;
}
}  // namespace

// k_link_score_bwd's items: the nodes of at most kGatSeg entries whole, then the long nodes'
// segments, which leave their partial rows in l.ws
template <int GL>
__global__ __launch_bounds__(kItemThreads) void k_link_mlp_bwd_nodes(
    const LinkIndex l, const float *__restrict__ H, int ld_h, int d, const float *__restrict__ dz,
    int ld_z, float *__restrict__ dH, int ld_dh) {
  const int lane = threadIdx.x % kWave, c0 = 4 * (lane % GL);
  const long long items = (long long)l.n + l.n_segs;
  for (long long it = first_item(); it < items; it += item_stride()) {
    if (it < l.n) {
      const int i = (int)it, b = l.inc_ptr[i], e = l.inc_ptr[i + 1];
      if (e - b > kGatSeg) continue;
      const float4 acc = mlp_entries_sum<GL>(l, H, ld_h, d, dz, ld_z, b, e, lane);
      if (lane < GL && c0 < d) store_row4(dH + (long long)i * ld_dh, c0, d, acc);
    } else {
      const long long t = it - l.n;
      const int4 sg = l.segs[t];
      const float4 acc = mlp_entries_sum<GL>(l, H, ld_h, d, dz, ld_z, sg.y, sg.z, lane);
      if (lane < GL && c0 < d)
        *reinterpret_cast<float4 *>(l.ws + t * kLinkWsStride + c0) = acc;
    }
  }
}

namespace {
long long mlp_lds_bytes(int d, int h, bool bwd) {
  const long long S = mlp_nd(d) + 4, WU = 32 * mlp_ut(h);
  return 4 * ((WU + kLinkMlpTile) * S + 2 * WU + 3 * kLinkMlpTile +
              (bwd ? kLinkMlpTile * (WU + 4) : 0));
}
// persistent workgroups of a pair kernel: as many as a CU's LDS holds (4 at most forward, 2
// backward, whose registers allow no more), never more than tiles -- a function of (E, d, h) only
int mlp_blocks(long long n_pairs, int d, int h, bool bwd) {
  const long long per_cu =
      std::max<long long>(1, std::min<long long>(bwd ? 2 : 4, kMlpLdsBudget / mlp_lds_bytes(d, h, bwd)));
  return (int)std::max<long long>(
      1, std::min<long long>(ceil_div(n_pairs, kLinkMlpTile), per_cu * kCUs));
}
void check_mlp_dims(const LinkIndex &l, int d, int h) {
  PGCN_CHECK(d >= 1 && d <= kLinkMaxWidth && h >= 1 && h <= kLinkMlpMaxHidden && l.n >= 0 &&
                 l.n_pairs >= 0,
             PGCN_E_INVALID, "link_mlp: 1 <= d <= 128, 1 <= h <= 128");
}

}  // namespace

long long link_mlp_workspace_bytes(const LinkIndex &l, int d, int h) {
  const long long ld_z = (d + 3) / 4 * 4, lp = (h + 3) / 4 * 4;
  return 4 * (l.n_pairs * ld_z + (long long)mlp_blocks(l.n_pairs, d, h, true) * (d + 3) * lp +
              (long long)l.n_segs * kLinkWsStride);
}

void launch_link_mlp_fwd(const LinkIndex &l, const float *H, int ld_h, int d, const float *P,
                         int ld_p, int h, float *scores, int ld_s, hipStream_t s) {
  check_mlp_dims(l, d, h);
  if (l.n_pairs == 0) return;
  note_path(KP_LINK_MLP_FWD);
  const dim3 grid((unsigned)mlp_blocks(l.n_pairs, d, h, false));
#define MLP_FWD(ND, UT)                                                                      \
  PGCN_LAUNCH((k_link_mlp_fwd<ND, UT>), grid, dim3(kMlpThreads), 0, s, l, H, ld_h, d, P, ld_p, h, \
              scores, ld_s)
  MLP_BY_SHAPE(d, h, MLP_FWD);
#undef MLP_FWD
}

void launch_link_mlp_bwd(const LinkIndex &l, const float *H, int ld_h, int d, const float *P,
                         int ld_p, int h, const float *G, int ld_g, float *dH, int ld_dh,
                         float *dP, int ld_dp, void *ws, long long ws_bytes, hipStream_t s) {
  check_mlp_dims(l, d, h);
  PGCN_CHECK(ws_bytes >= link_mlp_workspace_bytes(l, d, h), PGCN_E_INVALID,
             "link_mlp_bwd: the workspace is smaller than pgcn_link_mlp_workspace");
  if (l.n_pairs == 0 || l.n == 0) return;
  note_path(KP_LINK_MLP_BWD);
  const int ld_z = (d + 3) / 4 * 4, lp = (h + 3) / 4 * 4;
  const int blocks = mlp_blocks(l.n_pairs, d, h, true);
  float *dz = static_cast<float *>(ws);
  float *part = dz + l.n_pairs * ld_z;
  LinkIndex lw = l;  // the segments' partial rows go to the caller's workspace
  lw.ws = part + (long long)blocks * (d + 3) * lp;
#define MLP_BWD(ND, UT)                                                                          \
  PGCN_LAUNCH((k_link_mlp_bwd_pairs<ND, UT>), dim3((unsigned)blocks), dim3(kMlpThreads), 0, s, l, \
              H, ld_h, d, P, ld_p, h, G, ld_g, dz, ld_z, part, lp)
  MLP_BY_SHAPE(d, h, MLP_BWD);
#undef MLP_BWD
  const unsigned rgrid = (unsigned)ceil_div((long long)(d + 3) * ld_dp, kMlpThreads);
  PGCN_LAUNCH(k_link_mlp_reduce, dim3(rgrid), dim3(kMlpThreads), 0, s, part, lp, blocks, d, h, dP,
              ld_dp);
  ITEM_DISPATCH(k_link_mlp_bwd_nodes, item_grid((long long)l.n + l.n_segs), s, lw, H, ld_h, d, dz,
                ld_z, dH, ld_dh);
  launch_link_bwd_merge(lw, d, dH, ld_dh, s);
}

}  // namespace pgcn
