// parallel-gcn_amd/csrc/k_layernorm.hip -- LayerNorm over the columns of a node variable, for
// gfx950: y = gamma * (x - mean) * rstd + beta per row, and its backward with the column sums
// of the scale / shift gradients.  (The reference has no such module.)
//
// Layout (both kernels): one row per group of GL lanes inside a wave, NV float4 per lane, the
// lane's float4 k at column 4 * (lane + GL * k) -- a group's loads are contiguous.  The row
// stays in registers; the row sums are xor butterflies inside the group (every lane ends with
// the same bits), so there is no LDS round trip at any width up to 1,024.
//   d <= 16: GL 4 | <= 64: 16 | <= 128: 32 | <= 256: 64 | <= 512: 64 x 2 | <= 1024: 64 x 4
// Forward: two passes over the registers (mean, then sum (x - mean)^2), never E[x^2] - mean^2.
// The final write goes through gs_epilogue (mode 1): the ReLU, residual add and hidden Dropout
// behind the LayerNorm run here with the roundings of their own kernels.
// Backward: dx in place is allowed (a row is read whole before it is written).  Each workgroup
// sums dy * xhat and dy over its rows in row order per lane group, then over its groups in
// group order (LDS), into its partial [2][ldp]; k_layernorm_reduce sums the partials in block
// order in two levels of about sqrt(blocks) (the grouping of launch_tn_reduce_blocks).  Grids
// depend on (n, d) only: bit-reproducible, no float atomics.
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace pgcn {

namespace {
constexpr int kLnThreads = 256;
constexpr int kLnFwdBlocks = 8 * kCUs;
constexpr int kLnBwdBlocks = 1024;  // partials: two levels of <= 32

template <int GL>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int off = GL / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

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

__device__ __forceinline__ float4 load_cols4(const float *p, int c0, int d, float fill) {
  float4 v;
  v.x = c0 < d ? p[c0] : fill;
  v.y = c0 + 1 < d ? p[c0 + 1] : fill;
  v.z = c0 + 2 < d ? p[c0 + 2] : fill;
  v.w = c0 + 3 < d ? p[c0 + 3] : fill;
  return v;
}
}  // namespace

template <int GL, int NV>
__global__ __launch_bounds__(kLnThreads) void k_layernorm_fwd(
    const float *x, int ld_x, float *y, int ld_y, int n, int d, const float *__restrict__ gamma,
    const float *__restrict__ beta, float eps, float *xhat, int ld_xhat, float *rstd,
    const GsEpilogue e) {
  constexpr int RPB = kLnThreads / GL;
  const int lane = threadIdx.x % GL, grp = threadIdx.x / GL;
  float4 ga[NV], be[NV];
#pragma unroll
  for (int k = 0; k < NV; k++) {
    const int c0 = 4 * (lane + GL * k);
    ga[k] = load_cols4(gamma, c0, d, 0.0f);
    be[k] = load_cols4(beta, c0, d, 0.0f);
  }
  const float fd = (float)d;
  for (long long base = (long long)blockIdx.x * RPB; base < n; base += (long long)gridDim.x * RPB) {
    const long long r = base + grp;
    const bool live = r < n;
    float4 v[NV];
    GsEpiIn in[NV];
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < NV; k++) {
      const int c0 = 4 * (lane + GL * k);
      const bool on = live && c0 < d;
      v[k] = load_row4(x + r * ld_x, c0, d, on);
      if (on) gs_epi_load(in[k], r, c0, e);  // before the reductions (gs_epilogue.hpp)
      s += (v[k].x + v[k].y) + (v[k].z + v[k].w);
    }
    const float mean = group_sum<GL>(s) / fd;
    float q = 0.0f;
#pragma unroll
    for (int k = 0; k < NV; k++) {
      const int c0 = 4 * (lane + GL * k);
      v[k].x = c0 < d ? v[k].x - mean : 0.0f;
      v[k].y = c0 + 1 < d ? v[k].y - mean : 0.0f;
      v[k].z = c0 + 2 < d ? v[k].z - mean : 0.0f;
      v[k].w = c0 + 3 < d ? v[k].w - mean : 0.0f;
      q += (v[k].x * v[k].x + v[k].y * v[k].y) + (v[k].z * v[k].z + v[k].w * v[k].w);
    }
    const float rs = 1.0f / sqrtf(group_sum<GL>(q) / fd + eps);
    if (rstd && live && lane == 0) rstd[r] = rs;
#pragma unroll
    for (int k = 0; k < NV; k++) {
      const int c0 = 4 * (lane + GL * k);
      if (!(live && c0 < d)) continue;
      const float4 h = make_float4(v[k].x * rs, v[k].y * rs, v[k].z * rs, v[k].w * rs);
      if (xhat) *reinterpret_cast<float4 *>(xhat + r * ld_xhat + c0) = h;
      // (columns >= d: gamma and beta read as zero, so the padding is written as zero)
      float4 a = make_float4(ga[k].x * h.x + be[k].x, ga[k].y * h.y + be[k].y,
                             ga[k].z * h.z + be[k].z, ga[k].w * h.w + be[k].w);
      gs_epilogue(a, r, c0, e, in[k]);
      *reinterpret_cast<float4 *>(y + r * ld_y + c0) = a;
    }
  }
}

template <int GL, int NV>
__global__ __launch_bounds__(kLnThreads) void k_layernorm_bwd(
    const float *dy, int ld_dy, const float *xhat, int ld_xhat, const float *__restrict__ rstd,
    const float *__restrict__ gamma, int n, int d, float *dx, int ld_dx,
    float *__restrict__ partial, int ldp) {
  constexpr int RPB = kLnThreads / GL;
  constexpr int W = GL * NV * 4;
  __shared__ __align__(16) float sh[RPB * 2 * W];
  const int lane = threadIdx.x % GL, grp = threadIdx.x / GL;
  float4 ga[NV], ag[NV], ab[NV];
#pragma unroll
  for (int k = 0; k < NV; k++) {
    ga[k] = load_cols4(gamma, 4 * (lane + GL * k), d, 0.0f);
    ag[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    ab[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  const float fd = (float)d;
  for (long long base = (long long)blockIdx.x * RPB; base < n; base += (long long)gridDim.x * RPB) {
    const long long r = base + grp;
    const bool live = r < n;
    float4 g[NV], h[NV];
    float s1 = 0.0f, s2 = 0.0f;
    const float rs = live ? rstd[r] : 0.0f;
#pragma unroll
    for (int k = 0; k < NV; k++) {
      const int c0 = 4 * (lane + GL * k);
      const bool on = live && c0 < d;
      const float4 t = load_row4(dy + r * ld_dy, c0, d, on);
      h[k] = load_row4(xhat + r * ld_xhat, c0, d, on);
      ag[k].x += t.x * h[k].x;
      ag[k].y += t.y * h[k].y;
      ag[k].z += t.z * h[k].z;
      ag[k].w += t.w * h[k].w;
      ab[k].x += t.x;
      ab[k].y += t.y;
      ab[k].z += t.z;
      ab[k].w += t.w;
      g[k] = make_float4(t.x * ga[k].x, t.y * ga[k].y, t.z * ga[k].z, t.w * ga[k].w);
      s1 += (g[k].x + g[k].y) + (g[k].z + g[k].w);
      s2 += (g[k].x * h[k].x + g[k].y * h[k].y) + (g[k].z * h[k].z + g[k].w * h[k].w);
    }
    const float m1 = group_sum<GL>(s1) / fd, m2 = group_sum<GL>(s2) / fd;
#pragma unroll
    for (int k = 0; k < NV; k++) {
      const int c0 = 4 * (lane + GL * k);
      if (!(live && c0 < d)) continue;
      float4 o;
      o.x = rs * ((g[k].x - m1) - h[k].x * m2);
      o.y = c0 + 1 < d ? rs * ((g[k].y - m1) - h[k].y * m2) : 0.0f;
      o.z = c0 + 2 < d ? rs * ((g[k].z - m1) - h[k].z * m2) : 0.0f;
      o.w = c0 + 3 < d ? rs * ((g[k].w - m1) - h[k].w * m2) : 0.0f;
      *reinterpret_cast<float4 *>(dx + r * ld_dx + c0) = o;
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
  for (int i = threadIdx.x; i < 2 * W; i += kLnThreads) {
    const int c = i % W;
    if (c >= ldp) continue;
    float s = 0.0f;
    for (int q = 0; q < RPB; q++) s += sh[q * 2 * W + i];
    partial[((long long)blockIdx.x * 2 + i / W) * ldp + c] = s;
  }
}

// out[k][c] = the nb partials [2][ldp] summed in block order: groups of spg blocks first (slot q
// of this workgroup sums group q, <= 32 groups of <= 32), then the groups in order.  16 elements
// per workgroup: the sums are chains of dependent adds, so the launch's time is its longest
// chain's loads -- many short chains side by side
constexpr int kLnRedEl = 16, kLnRedSlots = 32;
__global__ __launch_bounds__(kLnRedEl * kLnRedSlots) void k_layernorm_reduce(
    const float *__restrict__ partial, int nb, int spg, int ldp, int d, float *__restrict__ dgamma,
    float *__restrict__ dbeta) {
  __shared__ float sh[kLnRedSlots][kLnRedEl];
  const int el = threadIdx.x % kLnRedEl, q = threadIdx.x / kLnRedEl;
  const int i = blockIdx.x * kLnRedEl + el;
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

static int ln_rows_per_block(int d) {
  const int d4 = (d + 3) / 4;
  const int gl = d4 <= 4 ? 4 : d4 <= 16 ? 16 : d4 <= 32 ? 32 : 64;
  return kLnThreads / gl;
}

static int ln_bwd_blocks(int n, int d) {
  return (int)std::min<long long>(ceil_div(n, ln_rows_per_block(d)), kLnBwdBlocks);
}

#define LN_DISPATCH(KERNEL, grid, s, ...)                                                  \
  do {                                                                                     \
    const int d4_ = (d + 3) / 4;                                                           \
    if (d4_ <= 4) PGCN_LAUNCH((KERNEL<4, 1>), grid, dim3(kLnThreads), 0, s, __VA_ARGS__);   \
    else if (d4_ <= 16) PGCN_LAUNCH((KERNEL<16, 1>), grid, dim3(kLnThreads), 0, s, __VA_ARGS__); \
    else if (d4_ <= 32) PGCN_LAUNCH((KERNEL<32, 1>), grid, dim3(kLnThreads), 0, s, __VA_ARGS__); \
    else if (d4_ <= 64) PGCN_LAUNCH((KERNEL<64, 1>), grid, dim3(kLnThreads), 0, s, __VA_ARGS__); \
    else if (d4_ <= 128) PGCN_LAUNCH((KERNEL<64, 2>), grid, dim3(kLnThreads), 0, s, __VA_ARGS__); \
    else PGCN_LAUNCH((KERNEL<64, 4>), grid, dim3(kLnThreads), 0, s, __VA_ARGS__);          \
  } while (0)

void launch_layernorm_fwd(const float *x, int ld_x, float *y, int ld_y, int n, int d,
                          const float *gamma, const float *beta, float eps, float *xhat,
                          int ld_xhat, float *rstd, const GsEpilogue *epi, hipStream_t s) {
  PGCN_CHECK(d >= 1 && d <= kLayerNormMaxWidth && n >= 0, PGCN_E_INVALID,
             "layernorm_fwd: 1 <= d <= 1024");
  if (n == 0) return;
  const GsEpilogue e = epi ? *epi : GsEpilogue{};
  const dim3 grid((unsigned)std::min<long long>(ceil_div(n, ln_rows_per_block(d)), kLnFwdBlocks));
  LN_DISPATCH(k_layernorm_fwd, grid, s, x, ld_x, y, ld_y, n, d, gamma, beta, eps, xhat, ld_xhat,
              rstd, e);
}

size_t layernorm_bwd_workspace(int n, int d) {
  if (n <= 0 || d <= 0) return 0;
  return (size_t)ln_bwd_blocks(n, d) * 2 * (size_t)((d + 3) / 4 * 4) * sizeof(float);
}

void launch_layernorm_bwd(const float *dy, int ld_dy, const float *xhat, int ld_xhat,
                          const float *rstd, const float *gamma, int n, int d, float *dx, int ld_dx,
                          float *dgamma, float *dbeta, void *workspace, hipStream_t s) {
  PGCN_CHECK(d >= 1 && d <= kLayerNormMaxWidth && n >= 0, PGCN_E_INVALID,
             "layernorm_bwd: 1 <= d <= 1024");
  if (n == 0) return;
  const int nb = ln_bwd_blocks(n, d), ldp = (d + 3) / 4 * 4;
  float *partial = static_cast<float *>(workspace);
  const dim3 grid((unsigned)nb);
  LN_DISPATCH(k_layernorm_bwd, grid, s, dy, ld_dy, xhat, ld_xhat, rstd, gamma, n, d, dx, ld_dx,
              partial, ldp);
  int spg = 16;  // ~sqrt(nb) partials per group in each level (blocks_plan, k_gemm.hip)
  while (spg * spg < nb) spg += 16;
  PGCN_LAUNCH(k_layernorm_reduce, dim3((unsigned)ceil_div(2 * ldp, kLnRedEl)),
              dim3(kLnRedEl * kLnRedSlots), 0, s, partial, nb, spg, ldp, d, dgamma, dbeta);
}

}  // namespace pgcn
