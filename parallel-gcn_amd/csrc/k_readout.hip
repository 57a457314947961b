// parallel-gcn_amd/csrc/k_readout.hip -- graph-level readout for gfx950 (the reference has no
// such module): a segmented sum / mean / max over each graph's rows of a node variable, and its
// backward, without float atomics.  Graphs are contiguous row ranges graph_ptr[g] ..
// graph_ptr[g + 1]; the adjacency pattern is not looked at.
//
// Layout: slot_items.hpp's wave, shared with k_sage.hip.  A wave is cut into 64 / GL row groups
// of GL lanes, lane li of a group holding the float4 at column 4 * li of its row; group q takes
// rows b + q, b + q + 64 / GL, ... of its row list in order and the groups meet in xor
// butterflies over the lane offsets GL .. 32.  The max keeps {value, row} per component under
// "greater value, else lower row" (k_sage.hip's rule: associative and commutative, -0.0 == +0.0),
// so the lowest row of equal values wins however the rows were dealt.
//   ranges of at most kReadoutChunk rows: one wave per range, four ranges per workgroup step
//   (k_readout_fwd: the whole forward when no range is longer).
//   longer ranges are cut where the row index is a multiple of kReadoutChunk, so a piece has at
//   most kReadoutChunk rows and the 256-thread workgroup of row block k = [k T, (k + 1) T) meets
//   at most two long ranges: the one holding its first row and the one holding its last
//   (anything strictly inside the block is short).  k_readout_pieces reduces those pieces, four
//   waves on a quarter of the block each, combined in wave order through LDS, into workspace
//   slot 2 k (first row's range) or 2 k + 1; k_readout_combine then reduces a long range's
//   slots in piece order with the same wave code and writes the final row.
// Every order depends on graph_ptr and d only: two calls give the same bits.
#include <algorithm>
#include <climits>

#include "common.hpp"
#include "kernels.hpp"
#include "slot_items.hpp"

#pragma clang fp contract(off)

namespace pgcn {

namespace {
constexpr int kT = kReadoutChunk;
constexpr int kQuarter = kT / kItemWaves;

// a lane's running result: the sums (s unused), or the maxima with their rows
struct Acc4 {
  float4 v;
  int4 s;
};

template <bool MAX>
__device__ __forceinline__ Acc4 acc_empty() {
  Acc4 a;
  const float e = MAX ? -INFINITY : 0.0f;
  a.v = make_float4(e, e, e, e);
  a.s = make_int4(INT_MAX, INT_MAX, INT_MAX, INT_MAX);
  return a;
}

// greater value, else lower row
__device__ __forceinline__ void take_best(float &v, int &s, float ov, int os) {
  if (ov > v || (ov == v && os < s)) {
    v = ov;
    s = os;
  }
}

template <bool MAX>
__device__ __forceinline__ void acc_take(Acc4 &a, const float4 &p, const int4 &s) {
  if (MAX) {
    take_best(a.v.x, a.s.x, p.x, s.x);
    take_best(a.v.y, a.s.y, p.y, s.y);
    take_best(a.v.z, a.s.z, p.z, s.z);
    take_best(a.v.w, a.s.w, p.w, s.w);
  } else {
    a.v.x += p.x;
    a.v.y += p.y;
    a.v.z += p.z;
    a.v.w += p.w;
  }
}

template <int GL, bool MAX>
__device__ __forceinline__ void across(float &v, int &s) {
#pragma unroll
  for (int off = GL; off < 64; off <<= 1) {
    const float ov = __shfl_xor(v, off, 64);
    if (MAX) {
      const int os = __shfl_xor(s, off, 64);
      take_best(v, s, ov, os);
    } else {
      v += ov;
    }
  }
}

// items [b, e) of a row list through load(k, value, rows): every lane ends with the wave's result
template <int GL, bool MAX, class Load>
__device__ __forceinline__ Acc4 wave_reduce(int b, int e, int lane, const Load &load) {
  constexpr int NB = kWave / GL;
  Acc4 w = acc_empty<MAX>();
#pragma unroll 4
  for (int k = b + lane / GL; k < e; k += NB) {
    float4 p;
    int4 s;
    load(k, p, s);
    acc_take<MAX>(w, p, s);
  }
  across<GL, MAX>(w.v.x, w.s.x);
  across<GL, MAX>(w.v.y, w.s.y);
  across<GL, MAX>(w.v.z, w.s.z);
  across<GL, MAX>(w.v.w, w.s.w);
  return w;
}

// items [b, e) by the workgroup: wave w takes [b + w per, b + (w + 1) per), the waves' results
// meet in wave order; lanes < GL of wave 0 return the result
template <int GL, bool MAX, class Load>
__device__ __forceinline__ Acc4 block_reduce(int b, int e, int per, const Load &load, Acc4 *lds) {
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int wb = (int)std::min<long long>(e, (long long)b + (long long)wave * per);
  const int we = (int)std::min<long long>(e, (long long)wb + per);
  const Acc4 w = wave_reduce<GL, MAX>(wb, we, lane, load);
  __syncthreads();  // (the previous call's reads of lds)
  if (lane < GL) lds[wave * 32 + lane] = w;
  __syncthreads();
  Acc4 r = acc_empty<MAX>();
  if (wave == 0 && lane < GL) {
    r = lds[lane];
    for (int k = 1; k < kItemWaves; k++) acc_take<MAX>(r, lds[k * 32 + lane].v, lds[k * 32 + lane].s);
  }
  return r;
}

// rows of `in`: the value with columns from d on zero, the row id itself
struct RowLoad {
  const float *in;
  int ld, d, c0;
  __device__ __forceinline__ void operator()(int k, float4 &p, int4 &s) const {
    p = row4(in + (long long)k * ld, c0, d, c0 < d);
    s = make_int4(k, k, k, k);
  }
};

// the workspace slots of one long range: piece p of the range is slot 2 (k0 + p), or 2 k0 + 1
// for a first piece that does not start its row block (the rows are read for the max only)
template <bool MAX>
struct SlotLoad {
  const float *val;
  const int *arg;
  int k0, odd_first, c0, d;
  __device__ __forceinline__ void operator()(int p, float4 &v, int4 &s) const {
    const long long slot = 2LL * (k0 + p) + (p == 0 ? odd_first : 0);
    v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    s = make_int4(INT_MAX, INT_MAX, INT_MAX, INT_MAX);
    if (c0 < d) {
      v = *reinterpret_cast<const float4 *>(val + slot * kReadoutWsStride + c0);
      if (MAX) s = *reinterpret_cast<const int4 *>(arg + slot * kReadoutWsStride + c0);
    }
  }
};

// the final write of range g (len rows) by the lane of column c0: the sum, the sum times one
// 1 / len, or the maxima and their rows; an empty range: 0 and -1; columns from d on: 0 and -1
template <bool MAX>
__device__ __forceinline__ void range_finish(const Acc4 &w, int len, int mode, int g, int c0, int d,
                                             float *__restrict__ out, int ld_out,
                                             int *__restrict__ arg, int ld_arg) {
  float4 o = w.v;
  int4 a = MAX ? w.s : make_int4(-1, -1, -1, -1);
  if (len <= 0) {
    o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    a = make_int4(-1, -1, -1, -1);
  } else if (mode == kReadoutMean) {
    const float inv = 1.0f / (float)len;
    o.x *= inv;
    o.y *= inv;
    o.z *= inv;
    o.w *= inv;
  }
  if (c0 + 1 >= d) o.y = 0.0f, a.y = -1;
  if (c0 + 2 >= d) o.z = 0.0f, a.z = -1;
  if (c0 + 3 >= d) o.w = 0.0f, a.w = -1;
  *reinterpret_cast<float4 *>(out + (long long)g * ld_out + c0) = o;
  if (arg) *reinterpret_cast<int4 *>(arg + (long long)g * ld_arg + c0) = a;
}

// the range holding row r: the last g with graph_ptr[g] <= r (graph_ptr[G] = n > r)
__device__ __forceinline__ int range_of(const int *__restrict__ graph_ptr, int G, int r) {
  int lo = 0, hi = G;  // graph_ptr[lo] <= r < graph_ptr[hi]
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (graph_ptr[mid] <= r) lo = mid;
    else hi = mid;
  }
  return lo;
}
}  // namespace

// one wave per range; chunked: the ranges longer than kReadoutChunk are left to the two kernels
// below
template <int GL, bool MAX>
__global__ __launch_bounds__(kItemThreads) void k_readout_fwd(
    const float *__restrict__ in, int ld_in, const int *__restrict__ graph_ptr, int G, int n, int d,
    int mode, int chunked, float *__restrict__ out, int ld_out, int *__restrict__ arg, int ld_arg) {
  const int lane = threadIdx.x % kWave, c0 = 4 * (lane % GL);
  const RowLoad load{in, ld_in, d, c0};
  for (long long it = first_item(); it < G; it += item_stride()) {
    const int g = (int)it;
    const int b = std::max(graph_ptr[g], 0), e = std::min(graph_ptr[g + 1], n);
    if (chunked && e - b > kT) continue;
    const Acc4 w = wave_reduce<GL, MAX>(b, e, lane, load);
    if (lane < GL && c0 < d) range_finish<MAX>(w, e - b, mode, g, c0, d, out, ld_out, arg, ld_arg);
  }
}

// one workgroup per row block k: the pieces of the (at most two) long ranges that meet it
template <int GL, bool MAX>
__global__ __launch_bounds__(kItemThreads) void k_readout_pieces(
    const float *__restrict__ in, int ld_in, const int *__restrict__ graph_ptr, int G, int n, int d,
    float *__restrict__ ws_val, int *__restrict__ ws_arg) {
  __shared__ Acc4 lds[kItemWaves * 32];
  const int lane = threadIdx.x % kWave, c0 = 4 * (lane % GL);
  const RowLoad load{in, ld_in, d, c0};
  const int blocks = (int)(((long long)n + kT - 1) / kT);
  for (int k = blockIdx.x; k < blocks; k += gridDim.x) {
    const int r0 = k * kT, r1 = (int)std::min<long long>(n, (long long)r0 + kT);
    const int gf = range_of(graph_ptr, G, r0), gl = range_of(graph_ptr, G, r1 - 1);
    for (int which = 0; which < 2; which++) {  // (uniform over the workgroup)
      if (which == 1 && gl == gf) break;
      const int g = which ? gl : gf;
      const int s = graph_ptr[g], e = graph_ptr[g + 1];
      if (e - s <= kT) continue;
      const Acc4 w = block_reduce<GL, MAX>(std::max(s, r0), std::min(e, r1), kQuarter, load, lds);
      if (threadIdx.x < GL && c0 < d) {
        const long long slot = 2LL * k + which;
        *reinterpret_cast<float4 *>(ws_val + slot * kReadoutWsStride + c0) = w.v;
        if (MAX) *reinterpret_cast<int4 *>(ws_arg + slot * kReadoutWsStride + c0) = w.s;
      }
    }
  }
}

// one workgroup per long range: its pieces in order, then the final write
template <int GL, bool MAX>
__global__ __launch_bounds__(kItemThreads) void k_readout_combine(
    const int *__restrict__ graph_ptr, int G, int n, int d, int mode,
    const float *__restrict__ ws_val, const int *__restrict__ ws_arg, float *__restrict__ out,
    int ld_out, int *__restrict__ arg, int ld_arg) {
  __shared__ Acc4 lds[kItemWaves * 32];
  const int lane = threadIdx.x % kWave, c0 = 4 * (lane % GL);
  for (int g = blockIdx.x; g < G; g += gridDim.x) {
    const int s = std::max(graph_ptr[g], 0), e = std::min(graph_ptr[g + 1], n);
    if (e - s <= kT) continue;  // (uniform)
    const int k0 = s / kT, k1 = (e - 1) / kT, pieces = k1 - k0 + 1;
    const SlotLoad<MAX> load{ws_val, ws_arg, k0, s > k0 * kT ? 1 : 0, c0, d};
    const Acc4 w = block_reduce<GL, MAX>(0, pieces, (pieces + kItemWaves - 1) / kItemWaves, load, lds);
    if (threadIdx.x < GL && c0 < d)
      range_finish<MAX>(w, e - s, mode, g, c0, d, out, ld_out, arg, ld_arg);
  }
}

// din_i = the gradient row of i's range: as it is (sum), times one 1 / len (mean), or its
// components whose recorded row is i (max); a float4 per thread, every row of din written
__global__ __launch_bounds__(kItemThreads) void k_readout_bwd(
    const float *__restrict__ Gout, int ld_g, const int *__restrict__ graph_ptr,
    const int *__restrict__ node_graph, const int *__restrict__ arg, int ld_arg, int G,
    long long total, int d4, int d, int mode, float *__restrict__ din, int ld_din) {
  for (long long t = (long long)blockIdx.x * kItemThreads + threadIdx.x; t < total;
       t += (long long)gridDim.x * kItemThreads) {
    const long long i = t / d4;
    const int c0 = 4 * (int)(t - i * d4);
    const int g = node_graph[i];
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (g >= 0 && g < G) {
      v = row4(Gout + (long long)g * ld_g, c0, d, true);
      if (mode == kReadoutMean) {
        const float inv = 1.0f / (float)(graph_ptr[g + 1] - graph_ptr[g]);
        v.x *= inv;
        v.y *= inv;
        v.z *= inv;
        v.w *= inv;
      } else if (mode == kReadoutMax) {
        const int4 a = *reinterpret_cast<const int4 *>(arg + (long long)g * ld_arg + c0);
        if (a.x != i) v.x = 0.0f;
        if (a.y != i) v.y = 0.0f;
        if (a.z != i) v.z = 0.0f;
        if (a.w != i) v.w = 0.0f;
      }
    }
    *reinterpret_cast<float4 *>(din + i * ld_din + c0) = v;
  }
}

size_t readout_workspace(int n) {
  const size_t slots = 2 * (size_t)ceil_div(std::max(n, 0), kT);
  return slots * kReadoutWsStride * (sizeof(float) + sizeof(int));
}

#define READOUT_DISPATCH(KERNEL, grid, s, ...)                                               \
  do {                                                                                       \
    switch (item_gl(d) * (mode == kReadoutMax ? -1 : 1)) {                                   \
      case 1: PGCN_LAUNCH((KERNEL<1, false>), grid, dim3(kItemThreads), 0, s, __VA_ARGS__); break;   \
      case 2: PGCN_LAUNCH((KERNEL<2, false>), grid, dim3(kItemThreads), 0, s, __VA_ARGS__); break;   \
      case 4: PGCN_LAUNCH((KERNEL<4, false>), grid, dim3(kItemThreads), 0, s, __VA_ARGS__); break;   \
      case 8: PGCN_LAUNCH((KERNEL<8, false>), grid, dim3(kItemThreads), 0, s, __VA_ARGS__); break;   \
      case 16: PGCN_LAUNCH((KERNEL<16, false>), grid, dim3(kItemThreads), 0, s, __VA_ARGS__); break; \
      case 32: PGCN_LAUNCH((KERNEL<32, false>), grid, dim3(kItemThreads), 0, s, __VA_ARGS__); break; \
      case -1: PGCN_LAUNCH((KERNEL<1, true>), grid, dim3(kItemThreads), 0, s, __VA_ARGS__); break;   \
      case -2: PGCN_LAUNCH((KERNEL<2, true>), grid, dim3(kItemThreads), 0, s, __VA_ARGS__); break;   \
      case -4: PGCN_LAUNCH((KERNEL<4, true>), grid, dim3(kItemThreads), 0, s, __VA_ARGS__); break;   \
      case -8: PGCN_LAUNCH((KERNEL<8, true>), grid, dim3(kItemThreads), 0, s, __VA_ARGS__); break;   \
      case -16: PGCN_LAUNCH((KERNEL<16, true>), grid, dim3(kItemThreads), 0, s, __VA_ARGS__); break; \
      default: PGCN_LAUNCH((KERNEL<32, true>), grid, dim3(kItemThreads), 0, s, __VA_ARGS__); break;  \
    }                                                                                        \
  } while (0)

void launch_readout_fwd(const float *in, int ld_in, const int *graph_ptr, int G, int n, int d,
                        int mode, int max_len, float *out, int ld_out, int *arg, int ld_arg,
                        void *workspace, hipStream_t s) {
  PGCN_CHECK(d >= 1 && d <= kReadoutMaxWidth && G >= 0 && n >= 0 && mode >= kReadoutSum &&
                 mode <= kReadoutMax && max_len >= 0 && (max_len <= kT || workspace),
             PGCN_E_INVALID, "readout_fwd: 1 <= d <= 128, mode 1..3, a workspace for long ranges");
  if (G == 0) return;
  const int chunked = max_len > kT && n > kT;
  READOUT_DISPATCH(k_readout_fwd, item_grid(G), s, in, ld_in, graph_ptr, G, n, d, mode, chunked, out,
                   ld_out, arg, ld_arg);
  if (!chunked) return;
  const long long blocks = ceil_div(n, kT);
  float *ws_val = static_cast<float *>(workspace);
  int *ws_arg = reinterpret_cast<int *>(ws_val + 2 * blocks * kReadoutWsStride);
  const dim3 gp((unsigned)std::min<long long>(blocks, kItemMaxBlocks));
  READOUT_DISPATCH(k_readout_pieces, gp, s, in, ld_in, graph_ptr, G, n, d, ws_val, ws_arg);
  // (at most n / kReadoutChunk ranges are long; the others' workgroups leave at once)
  const dim3 gc((unsigned)std::min<long long>(G, kItemMaxBlocks));
  READOUT_DISPATCH(k_readout_combine, gc, s, graph_ptr, G, n, d, mode, ws_val, ws_arg, out, ld_out,
                   arg, ld_arg);
}

void launch_readout_bwd(const float *Gout, int ld_g, const int *graph_ptr, const int *node_graph,
                        const int *arg, int ld_arg, int G, int n, int d, int mode, float *din,
                        int ld_din, hipStream_t s) {
  PGCN_CHECK(d >= 1 && d <= kReadoutMaxWidth && G >= 0 && n >= 0 && mode >= kReadoutSum &&
                 mode <= kReadoutMax && (mode != kReadoutMax || arg),
             PGCN_E_INVALID, "readout_bwd: 1 <= d <= 128, mode 1..3, arg for the max");
  if (n == 0) return;
  const int d4 = (d + 3) / 4;
  const long long total = (long long)n * d4;
  const dim3 grid((unsigned)std::min<long long>(ceil_div(total, kItemThreads), kItemMaxBlocks));
  PGCN_LAUNCH(k_readout_bwd, grid, dim3(kItemThreads), 0, s, Gout, ld_g, graph_ptr, node_graph, arg,
              ld_arg, G, total, d4, d, mode, din, ld_din);
}

}  // namespace pgcn
