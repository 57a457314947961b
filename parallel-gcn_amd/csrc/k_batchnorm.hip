// parallel-gcn_amd/csrc/k_batchnorm.hip -- BatchNorm over the rows of a node variable, for gfx950:
// per column c over all n rows  mean_c, var_c (biased), rstd_c = 1 / sqrtf(var_c + eps),
// y = gamma_c * (x - mean_c) * rstd_c + beta_c, and its backward.  (The reference has no such
// module.)  The statistics are the pass's own, in training and in eval: no running averages.
//
// Lane layout (every kernel but the two small reducing ones): LayerNorm's -- a row per group of
// GL lanes inside a wave, NV float4 per lane, the lane's float4 k at column 4 * (lane + GL * k),
// so a group's loads are contiguous.  G = 256 / GL groups per workgroup.
//   d <= 16: GL 4 | <= 64: 16 | <= 128: 32 | <= 256: 64 | <= 512: 64 x 2 | <= 1024: 64 x 4
//
// Forward, three launches.
// (1) k_batchnorm_stats: one read of x.  A workgroup takes tiles of R = G * 16 / NV consecutive
//     rows, grid-stride, and holds a tile in registers: group g holds rows g, G + g, 2 G + g, ...
//     of the tile (one load instruction covers G consecutive rows), 16 float4 = 64 VGPRs per
//     lane whatever the width.  A lane sums its rows in that order -- as differences from the
//     tile's first row, the pivot, which are exact where a column's mean dwarfs its spread -- the
//     groups' sums meet in LDS and every lane adds them in group order: the tile's column means
//     = pivot + sum / count.  From the resident copy
//     the lanes then take the CENTRED second moment M2 = sum (x - tile mean)^2, met the same way
//     -- never E[x^2] - mean^2.  Columns [d, ld) read as zero.  The tile's record goes to the
//     workspace: {count, 0, 0, 0, mean[w4], M2[w4]}, w4 = round_up4(d).
// (2) k_batchnorm_merge: the records combined in tile order with the pairwise update
//       delta = mean_b - mean_a;  mean = mean_a + delta * n_b / (n_a + n_b)
//       M2 = M2_a + M2_b + delta^2 * n_a * n_b / (n_a + n_b)
//     (the means as differences from tile 0's, added back at the end) in two levels -- slot q of a workgroup merges tiles [q spg, (q + 1) spg), then slot 0 merges
//     the slots in order -- and stats [2][w4] = {mean, rstd} written.  spg is the smallest
//     multiple of 16 with spg * min(spg, 64) >= tiles: spg^2 >= tiles up to 4,096 tiles, and 64
//     slots of longer chains beyond (the LDS holds 64 slots).
// (3) k_batchnorm_apply: a row per lane group, the column constants in registers; xhat kept for
//     a training call; the final write goes through gs_epilogue (mode 1) as k_layernorm_fwd's
//     does, the tail's loads issued before the arithmetic.  In place is safe: an element is read
//     and written by the same lane.
// Backward, three launches: k_batchnorm_bwd_partial sums dy * xhat and dy over each workgroup's
// rows (per group in row order, the groups in group order through LDS) into partial [2][ldp];
// k_batchnorm_bwd_reduce sums the partials in block order in two levels and writes dgamma /
// dbeta; k_batchnorm_bwd_dx is elementwise.  Grids depend on (n, d) only and nothing is atomic:
// every result is bit-reproducible.
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace pgcn {

namespace {
constexpr int kBnThreads = 256;
constexpr int kBnTileF4 = 16;  // float4s of the resident tile per lane (64 VGPRs)
constexpr int kBnRecHead = 4;  // a record's floats before its mean: {count, 0, 0, 0}
constexpr int kBnStatBlocks = 8 * kCUs;
constexpr int kBnRowBlocks = 8 * kCUs;  // apply, dx
constexpr int kBnBwdBlocks = 1024;      // partials: two levels of <= 32

// the float4 at columns c0 .. c0 + 3 of a row of logical width d: columns >= d read as zero
// (the padding may hold anything)
__device__ __forceinline__ float4 load_row4(const float *p, int c0, int d, bool on) {
  float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (on) {
    v = *reinterpret_cast<const float4 *>(p + c0);
    if (c0 + 1 >= d) v.y = 0.0f;
    if (c0 + 2 >= d) v.z = 0.0f;
    if (c0 + 3 >= d) v.w = 0.0f;
  }
  return v;
}

__device__ __forceinline__ float4 load_cols4(const float *p, int c0, int d) {
  float4 v;
  v.x = c0 < d ? p[c0] : 0.0f;
  v.y = c0 + 1 < d ? p[c0 + 1] : 0.0f;
  v.z = c0 + 2 < d ? p[c0 + 2] : 0.0f;
  v.w = c0 + 3 < d ? p[c0 + 3] : 0.0f;
  return v;
}

__device__ __forceinline__ float4 add4(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

// (n_a, mean_a, M2_a) <- the pair merged with (n_b, mean_b, M2_b); n_a, n_b >= 1
__device__ __forceinline__ void bn_merge(float &na, float &ma, float &qa, float nb, float mb,
                                         float qb) {
  const float tot = na + nb, w = nb / tot, delta = mb - ma;
  ma = ma + delta * w;
  qa = (qa + qb) + (delta * delta) * (na * w);
  na = tot;
}
}  // namespace

template <int GL, int NV>
__global__ __launch_bounds__(kBnThreads) void k_batchnorm_stats(const float *__restrict__ x,
                                                                int ld_x, int n, int d, int w4,
                                                                float *__restrict__ rec) {
  constexpr int G = kBnThreads / GL;
  constexpr int RG = kBnTileF4 / NV;  // rows of a tile per group
  constexpr int R = G * RG;
  constexpr int W = GL * NV * 4;
  __shared__ __align__(16) float sh[G * W];
  const int lane = threadIdx.x % GL, grp = threadIdx.x / GL;
  const int tiles = (int)(((long long)n + R - 1) / R);
  const int stride = kBnRecHead + 2 * w4;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const long long base = (long long)t * R;
    const int cnt = (int)min((long long)R, (long long)n - base);
    // the sums run on x - pivot, the pivot being the tile's first row: with a column mean far
    // from zero the differences are exact and small, so the tile mean = pivot + sum / count is
    // within one rounding of the true one (a plain sum of 1,024 values near 200 is not)
    float4 v[RG][NV], s[NV], pv[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) {
      const int c0 = 4 * (lane + GL * k);
      s[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      pv[k] = load_row4(x + base * ld_x, c0, d, c0 < d);
    }
#pragma unroll
    for (int i = 0; i < RG; i++) {
      const int ri = i * G + grp;
#pragma unroll
      for (int k = 0; k < NV; k++) {
        const int c0 = 4 * (lane + GL * k);
        v[i][k] = load_row4(x + (base + ri) * ld_x, c0, d, ri < cnt && c0 < d);
        s[k].x += ri < cnt ? v[i][k].x - pv[k].x : 0.0f;
        s[k].y += ri < cnt ? v[i][k].y - pv[k].y : 0.0f;
        s[k].z += ri < cnt ? v[i][k].z - pv[k].z : 0.0f;
        s[k].w += ri < cnt ? v[i][k].w - pv[k].w : 0.0f;
      }
    }
#pragma unroll
    for (int k = 0; k < NV; k++)
      *reinterpret_cast<float4 *>(&sh[grp * W + 4 * (lane + GL * k)]) = s[k];
    __syncthreads();
    const float fc = (float)cnt;
    float4 mean[NV], q[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) {
      const int c0 = 4 * (lane + GL * k);
      float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      for (int g = 0; g < G; g++) a = add4(a, *reinterpret_cast<const float4 *>(&sh[g * W + c0]));
      mean[k] = make_float4(pv[k].x + a.x / fc, pv[k].y + a.y / fc, pv[k].z + a.z / fc,
                            pv[k].w + a.w / fc);
      q[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < RG; i++) {
      const bool live = i * G + grp < cnt;
#pragma unroll
      for (int k = 0; k < NV; k++) {
        // (a column >= d holds zeros and a zero mean: it adds nothing)
        const float ex = v[i][k].x - mean[k].x, ey = v[i][k].y - mean[k].y;
        const float ez = v[i][k].z - mean[k].z, ew = v[i][k].w - mean[k].w;
        q[k].x += live ? ex * ex : 0.0f;
        q[k].y += live ? ey * ey : 0.0f;
        q[k].z += live ? ez * ez : 0.0f;
        q[k].w += live ? ew * ew : 0.0f;
      }
    }
#pragma unroll
    for (int k = 0; k < NV; k++)
      *reinterpret_cast<float4 *>(&sh[grp * W + 4 * (lane + GL * k)]) = q[k];
    __syncthreads();
    if (grp == 0) {
      float *r = rec + (long long)t * stride;
      if (lane == 0) *reinterpret_cast<float4 *>(r) = make_float4(fc, 0.0f, 0.0f, 0.0f);
#pragma unroll
      for (int k = 0; k < NV; k++) {
        const int c0 = 4 * (lane + GL * k);
        if (c0 >= w4) continue;
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int g = 0; g < G; g++) a = add4(a, *reinterpret_cast<const float4 *>(&sh[g * W + c0]));
        *reinterpret_cast<float4 *>(r + kBnRecHead + c0) = mean[k];
        *reinterpret_cast<float4 *>(r + kBnRecHead + w4 + c0) = a;
      }
    }
    __syncthreads();  // (the next tile's sums overwrite sh)
  }
}

// stats [2][w4] = {mean, rstd} from the tile records, merged in tile order: slot q of this
// workgroup merges tiles [q spg, (q + 1) spg), slot 0 then merges the slots in order.  16 columns
// per workgroup (the merges are chains of dependent updates: many short chains side by side, as
// k_layernorm_reduce)
constexpr int kBnMrgEl = 16, kBnMrgSlots = 64;
__global__ __launch_bounds__(kBnMrgEl *kBnMrgSlots) void k_batchnorm_merge(
    const float *__restrict__ rec, int tiles, int spg, int w4, float eps,
    float *__restrict__ stats) {
  __shared__ float shn[kBnMrgSlots][kBnMrgEl], shm[kBnMrgSlots][kBnMrgEl],
      shq[kBnMrgSlots][kBnMrgEl];
  const int el = threadIdx.x % kBnMrgEl, q = threadIdx.x / kBnMrgEl;
  const int c = blockIdx.x * kBnMrgEl + el;
  const int n_groups = (tiles + spg - 1) / spg;  // <= kBnMrgSlots (bn_merge_spg)
  const int stride = kBnRecHead + 2 * w4;
  if (c < w4 && q < n_groups) {
    const int lo = q * spg, hi = min(tiles, lo + spg);
    // (the means travel as differences from tile 0's: the update is shift-invariant, and the
    // roundings of small differences do not add up to an ulp of a mean far from zero)
    const float pivot = rec[kBnRecHead + c];
    const float *r = rec + (long long)lo * stride;
    float na = r[0], ma = r[kBnRecHead + c] - pivot, qa = r[kBnRecHead + w4 + c];
#pragma unroll 4
    for (int t = lo + 1; t < hi; t++) {
      r += stride;
      bn_merge(na, ma, qa, r[0], r[kBnRecHead + c] - pivot, r[kBnRecHead + w4 + c]);
    }
    shn[q][el] = na;
    shm[q][el] = ma;
    shq[q][el] = qa;
  }
  __syncthreads();
  if (q != 0 || c >= w4) return;
  float na = shn[0][el], ma = shm[0][el], qa = shq[0][el];
  for (int g = 1; g < n_groups; g++) bn_merge(na, ma, qa, shn[g][el], shm[g][el], shq[g][el]);
  stats[c] = rec[kBnRecHead + c] + ma;
  stats[w4 + c] = 1.0f / sqrtf(qa / na + eps);
}

template <int GL, int NV>
__global__ __launch_bounds__(kBnThreads) void k_batchnorm_apply(
    const float *x, int ld_x, float *y, int ld_y, int n, int d, const float *__restrict__ gamma,
    const float *__restrict__ beta, const float *__restrict__ stats, int w4, float *xhat,
    int ld_xhat, const GsEpilogue e) {
  constexpr int RPB = kBnThreads / GL;
  const int lane = threadIdx.x % GL, grp = threadIdx.x / GL;
  float4 ga[NV], be[NV], mu[NV], rs[NV];
#pragma unroll
  for (int k = 0; k < NV; k++) {
    const int c0 = 4 * (lane + GL * k);
    ga[k] = load_cols4(gamma, c0, d);
    be[k] = load_cols4(beta, c0, d);
    mu[k] = load_cols4(stats, c0, d);
    rs[k] = load_cols4(stats + w4, c0, d);
  }
  for (long long base = (long long)blockIdx.x * RPB; base < n; base += (long long)gridDim.x * RPB) {
    const long long r = base + grp;
    const bool live = r < n;
    float4 v[NV];
    GsEpiIn in[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) {
      const int c0 = 4 * (lane + GL * k);
      const bool on = live && c0 < d;
      v[k] = load_row4(x + r * ld_x, c0, d, on);
      if (on) gs_epi_load(in[k], r, c0, e);  // before the arithmetic (gs_epilogue.hpp)
    }
#pragma unroll
    for (int k = 0; k < NV; k++) {
      const int c0 = 4 * (lane + GL * k);
      if (!(live && c0 < d)) continue;
      // (columns >= d: x, mean, rstd, gamma and beta all read as zero -- the padding is zero)
      const float4 h = make_float4((v[k].x - mu[k].x) * rs[k].x, (v[k].y - mu[k].y) * rs[k].y,
                                   (v[k].z - mu[k].z) * rs[k].z, (v[k].w - mu[k].w) * rs[k].w);
      if (xhat) *reinterpret_cast<float4 *>(xhat + r * ld_xhat + c0) = h;
      float4 a = make_float4(ga[k].x * h.x + be[k].x, ga[k].y * h.y + be[k].y,
                             ga[k].z * h.z + be[k].z, ga[k].w * h.w + be[k].w);
      gs_epilogue(a, r, c0, e, in[k]);
      *reinterpret_cast<float4 *>(y + r * ld_y + c0) = a;
    }
  }
}

template <int GL, int NV>
__global__ __launch_bounds__(kBnThreads) void k_batchnorm_bwd_partial(
    const float *__restrict__ dy, int ld_dy, const float *__restrict__ xhat, int ld_xhat, int n,
    int d, float *__restrict__ partial, int ldp) {
  constexpr int RPB = kBnThreads / GL;
  constexpr int W = GL * NV * 4;
  __shared__ __align__(16) float sh[RPB * 2 * W];
  const int lane = threadIdx.x % GL, grp = threadIdx.x / GL;
  float4 ag[NV], ab[NV];
#pragma unroll
  for (int k = 0; k < NV; k++) {
    ag[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    ab[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  for (long long base = (long long)blockIdx.x * RPB; base < n; base += (long long)gridDim.x * RPB) {
    const long long r = base + grp;
#pragma unroll
    for (int k = 0; k < NV; k++) {
      const int c0 = 4 * (lane + GL * k);
      const bool on = r < n && c0 < d;
      const float4 t = load_row4(dy + r * ld_dy, c0, d, on);
      const float4 h = load_row4(xhat + r * ld_xhat, c0, d, on);
      ag[k].x += t.x * h.x;
      ag[k].y += t.y * h.y;
      ag[k].z += t.z * h.z;
      ag[k].w += t.w * h.w;
      ab[k] = add4(ab[k], t);
    }
  }
  // this workgroup's column sums: its groups in group order
#pragma unroll
  for (int k = 0; k < NV; k++) {
    const int c0 = 4 * (lane + GL * k);
    *reinterpret_cast<float4 *>(&sh[(grp * 2 + 0) * W + c0]) = ag[k];
    *reinterpret_cast<float4 *>(&sh[(grp * 2 + 1) * W + c0]) = ab[k];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * W; i += kBnThreads) {
    const int c = i % W;
    if (c >= ldp) continue;
    float s = 0.0f;
    for (int q = 0; q < RPB; q++) s += sh[q * 2 * W + i];
    partial[((long long)blockIdx.x * 2 + i / W) * ldp + c] = s;
  }
}

// dgamma / dbeta = the nb partials [2][ldp] summed in block order: groups of spg blocks first
// (slot q sums group q; <= 32 groups of <= 32), then the groups in order
constexpr int kBnRedEl = 16, kBnRedSlots = 32;
__global__ __launch_bounds__(kBnRedEl *kBnRedSlots) void k_batchnorm_bwd_reduce(
    const float *__restrict__ partial, int nb, int spg, int ldp, int d, float *__restrict__ dgamma,
    float *__restrict__ dbeta) {
  __shared__ float sh[kBnRedSlots][kBnRedEl];
  const int el = threadIdx.x % kBnRedEl, q = threadIdx.x / kBnRedEl;
  const int i = blockIdx.x * kBnRedEl + el;
  const int n_groups = (nb + spg - 1) / spg;
  if (i < 2 * ldp && q < n_groups) {
    float s = 0.0f;
    const int hi = min(nb, (q + 1) * spg);
#pragma unroll 8
    for (int b = q * spg; b < hi; b++) s += partial[(long long)b * 2 * ldp + i];
    sh[q][el] = s;
  }
  __syncthreads();
  if (q != 0 || i >= 2 * ldp) return;
  float s = 0.0f;
  for (int g = 0; g < n_groups; g++) s += sh[g][el];
  const int c = i % ldp;
  if (c < d) (i < ldp ? dgamma : dbeta)[c] = s;
}

template <int GL, int NV>
__global__ __launch_bounds__(kBnThreads) void k_batchnorm_bwd_dx(
    const float *dy, int ld_dy, const float *__restrict__ xhat, int ld_xhat,
    const float *__restrict__ stats, int w4, const float *__restrict__ gamma,
    const float *__restrict__ dgamma, const float *__restrict__ dbeta, int n, int d, float *dx,
    int ld_dx) {
  constexpr int RPB = kBnThreads / GL;
  const int lane = threadIdx.x % GL, grp = threadIdx.x / GL;
  const float fn = (float)n;
  float4 co[NV], mg[NV], mb[NV];  // gamma * rstd, dgamma / n, dbeta / n (zero from column d on)
#pragma unroll
  for (int k = 0; k < NV; k++) {
    const int c0 = 4 * (lane + GL * k);
    const float4 ga = load_cols4(gamma, c0, d), rs = load_cols4(stats + w4, c0, d);
    const float4 g = load_cols4(dgamma, c0, d), b = load_cols4(dbeta, c0, d);
    co[k] = make_float4(ga.x * rs.x, ga.y * rs.y, ga.z * rs.z, ga.w * rs.w);
    mg[k] = make_float4(g.x / fn, g.y / fn, g.z / fn, g.w / fn);
    mb[k] = make_float4(b.x / fn, b.y / fn, b.z / fn, b.w / fn);
  }
  for (long long base = (long long)blockIdx.x * RPB; base < n; base += (long long)gridDim.x * RPB) {
    const long long r = base + grp;
#pragma unroll
    for (int k = 0; k < NV; k++) {
      const int c0 = 4 * (lane + GL * k);
      if (!(r < n && c0 < d)) continue;
      const float4 t = load_row4(dy + r * ld_dy, c0, d, true);
      const float4 h = load_row4(xhat + r * ld_xhat, c0, d, true);
      float4 o;  // (columns >= d: every factor reads as zero)
      o.x = co[k].x * ((t.x - mb[k].x) - h.x * mg[k].x);
      o.y = co[k].y * ((t.y - mb[k].y) - h.y * mg[k].y);
      o.z = co[k].z * ((t.z - mb[k].z) - h.z * mg[k].z);
      o.w = co[k].w * ((t.w - mb[k].w) - h.w * mg[k].w);
      *reinterpret_cast<float4 *>(dx + r * ld_dx + c0) = o;
    }
  }
}

static int bn_group_lanes(int d) {
  const int d4 = (d + 3) / 4;
  return d4 <= 4 ? 4 : d4 <= 16 ? 16 : d4 <= 32 ? 32 : 64;
}

static int bn_rows_per_block(int d) { return kBnThreads / bn_group_lanes(d); }

int batchnorm_tile_rows(int d) {
  const int d4 = (d + 3) / 4;
  const int nv = d4 <= 64 ? 1 : d4 <= 128 ? 2 : 4;
  return bn_rows_per_block(d) * (kBnTileF4 / nv);
}

static int bn_tiles(int n, int d) { return (int)ceil_div(n, batchnorm_tile_rows(d)); }

static int bn_bwd_blocks(int n, int d) {
  return (int)std::min<long long>(ceil_div(n, bn_rows_per_block(d)), kBnBwdBlocks);
}

#define BN_DISPATCH(KERNEL, grid, s, ...)                                                  \
  do {                                                                                     \
    const int d4_ = (d + 3) / 4;                                                           \
    if (d4_ <= 4) PGCN_LAUNCH((KERNEL<4, 1>), grid, dim3(kBnThreads), 0, s, __VA_ARGS__);   \
    else if (d4_ <= 16) PGCN_LAUNCH((KERNEL<16, 1>), grid, dim3(kBnThreads), 0, s, __VA_ARGS__); \
    else if (d4_ <= 32) PGCN_LAUNCH((KERNEL<32, 1>), grid, dim3(kBnThreads), 0, s, __VA_ARGS__); \
    else if (d4_ <= 64) PGCN_LAUNCH((KERNEL<64, 1>), grid, dim3(kBnThreads), 0, s, __VA_ARGS__); \
    else if (d4_ <= 128) PGCN_LAUNCH((KERNEL<64, 2>), grid, dim3(kBnThreads), 0, s, __VA_ARGS__); \
    else PGCN_LAUNCH((KERNEL<64, 4>), grid, dim3(kBnThreads), 0, s, __VA_ARGS__);          \
  } while (0)

size_t batchnorm_fwd_workspace(int n, int d) {
  if (n <= 0 || d <= 0) return 0;
  return (size_t)bn_tiles(n, d) * (size_t)(kBnRecHead + 2 * ((d + 3) / 4 * 4)) * sizeof(float);
}

void launch_batchnorm_fwd(const float *x, int ld_x, float *y, int ld_y, int n, int d,
                          const float *gamma, const float *beta, float eps, float *xhat,
                          int ld_xhat, float *stats, void *workspace, const GsEpilogue *epi,
                          hipStream_t s) {
  PGCN_CHECK(d >= 1 && d <= kBatchNormMaxWidth && n >= 0, PGCN_E_INVALID,
             "batchnorm_fwd: 1 <= d <= 1024");
  if (n == 0) return;
  const GsEpilogue e = epi ? *epi : GsEpilogue{};
  const int tiles = bn_tiles(n, d), w4 = (d + 3) / 4 * 4;
  float *rec = static_cast<float *>(workspace);
  const dim3 sgrid((unsigned)std::min(tiles, kBnStatBlocks));
  BN_DISPATCH(k_batchnorm_stats, sgrid, s, x, ld_x, n, d, w4, rec);
  int spg = 16;  // tiles per slot: spg^2 >= tiles while 64 slots hold them, longer chains beyond
  while ((long long)spg * std::min(spg, kBnMrgSlots) < tiles) spg += 16;
  PGCN_LAUNCH(k_batchnorm_merge, dim3((unsigned)ceil_div(w4, kBnMrgEl)),
              dim3(kBnMrgEl * kBnMrgSlots), 0, s, rec, tiles, spg, w4, eps, stats);
  const dim3 grid((unsigned)std::min<long long>(ceil_div(n, bn_rows_per_block(d)), kBnRowBlocks));
  BN_DISPATCH(k_batchnorm_apply, grid, s, x, ld_x, y, ld_y, n, d, gamma, beta, stats, w4, xhat,
              ld_xhat, e);
}

size_t batchnorm_bwd_workspace(int n, int d) {
  if (n <= 0 || d <= 0) return 0;
  return (size_t)bn_bwd_blocks(n, d) * 2 * (size_t)((d + 3) / 4 * 4) * sizeof(float);
}

void launch_batchnorm_bwd(const float *dy, int ld_dy, const float *xhat, int ld_xhat,
                          const float *stats, const float *gamma, int n, int d, float *dx,
                          int ld_dx, float *dgamma, float *dbeta, void *workspace, hipStream_t s) {
  PGCN_CHECK(d >= 1 && d <= kBatchNormMaxWidth && n >= 0, PGCN_E_INVALID,
             "batchnorm_bwd: 1 <= d <= 1024");
  if (n == 0) return;
  const int nb = bn_bwd_blocks(n, d), ldp = (d + 3) / 4 * 4;
  float *partial = static_cast<float *>(workspace);
  const dim3 pgrid((unsigned)nb);
  BN_DISPATCH(k_batchnorm_bwd_partial, pgrid, s, dy, ld_dy, xhat, ld_xhat, n, d, partial, ldp);
  int spg = 16;  // ~sqrt(nb) partials per group in each level
  while (spg * spg < nb) spg += 16;
  PGCN_LAUNCH(k_batchnorm_bwd_reduce, dim3((unsigned)ceil_div(2 * ldp, kBnRedEl)),
              dim3(kBnRedEl * kBnRedSlots), 0, s, partial, nb, spg, ldp, d, dgamma, dbeta);
  const dim3 grid((unsigned)std::min<long long>(ceil_div(n, bn_rows_per_block(d)), kBnRowBlocks));
  BN_DISPATCH(k_batchnorm_bwd_dx, grid, s, dy, ld_dy, xhat, ld_xhat, stats, ldp, gamma, dgamma,
              dbeta, n, d, dx, ld_dx);
}

}  // namespace pgcn
