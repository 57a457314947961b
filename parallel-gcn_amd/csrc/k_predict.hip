// parallel-gcn_amd/csrc/k_predict.hip -- per-row prediction from logits (class, confidence,
// softmax row) and the confusion matrix of predictions against labels, for gfx950.
//
// New with the engine's inference interface (the reference prints one test accuracy and
// keeps nothing per node).  The softmax is built from the loss kernel's pieces
// (k_elementwise.hip xent_tile): the same max shift, exp_nonpos, summation order and div_rn.
// One step is added: the shift z - max rounds (up to 2^-20 absolute for gaps of 16..32, i.e. 16
// units of 2^-24 relative on a small probability), which the loss tolerates and a reported
// probability should not, so the shift's rounding error is recovered exactly (TwoSum) and
// applied to the exponential.  A probability is then within (c + 3) 2^-24 relative of the
// exact softmax of the given logits, and within those few units of the loss kernel's own.
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"
#include "softmax_parts.hpp"

#pragma clang fp contract(off)

namespace pgcn {

constexpr int PT = 4 * kPredictRows;  // threads: a lane quad per row, 16 rows per wave
typedef float floatx4p __attribute__((ext_vector_type(4)));

// exp(z - mx) for z <= mx: exp_nonpos of the rounded difference d, times 1 + err, where err =
// (z - mx) - d exactly (TwoSum; |err| <= ulp(d) / 2 <= 2^-18 wherever the exponential is not 0)
__device__ __forceinline__ float shifted_exp(float z, float mx) {
  const float d = z - mx;
  const float bp = d - z, ap = d - bp;
  const float err = (z - ap) + (-mx - bp);
  const float e = exp_nonpos(d);
  return e == 0.0f ? 0.0f : fmaf(e, err, e);
}

// tile row stride for cp = round_up4(c) columns: a multiple of 4 with S / 4 odd (the quads'
// walks down a wave's 16 rows hit distinct banks)
__host__ __device__ inline int predict_stride(int cp) { return (cp / 4) % 2 ? cp : cp + 4; }

// A block of kPredictRows = 64 rows, 4 waves, each wave alone on its 16 rows (no block
// barrier).  The wave's rows come in as 16-byte pieces of their first cp columns (one
// contiguous run when ld == cp) into its part of an LDS tile [64][S]; lane q of a row's quad
// takes classes q, q + 4, ... as in xent_tile.  Argmax: each lane keeps its first maximum,
// the quad combines by (value, lower index).  Probabilities replace the logits in the tile and
// leave as 16-byte pieces.  Columns >= c are never used (select, not arithmetic).
// NP > 0 (c <= 48): the 16-byte pieces per lane of a wave's 16 rows (16 * cp / 4 <= 64 * NP),
// all loaded before the first goes to LDS (one HBM latency per wave, as xent_tile's copy);
// NP = 0: wider rows, a plain loop (eight pieces held at once took 216 VGPRs)
template <int NP>
__global__ __launch_bounds__(PT) void k_predict_rows(const float *__restrict__ logits, int ld,
                                                     int n, int c, int *__restrict__ cls,
                                                     float *__restrict__ conf,
                                                     float *__restrict__ probs, int ld_probs) {
  extern __shared__ float smem[];
  const int cp = (c + 3) & ~3, c4 = cp >> 2, S = predict_stride(cp);
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
  const long long row0 = (long long)blockIdx.x * kPredictRows, wrow0 = row0 + 16 * wv;
  const int rows = (int)min((long long)kPredictRows, (long long)n - row0);
  const int wrows = max(0, min(16, rows - 16 * wv));  // this wave's rows
  float *L = smem + wv * 16 * S;
  // piece p of the wave = row p / c4, float4 p % c4 (24-bit multiply-shift: exact, p < 512)
  const int pieces = wrows * c4;
  const unsigned magic = (1u << 20) / (unsigned)c4 + 1u;
  if constexpr (NP == 0) {
    for (int p = ln; p < pieces; p += 64) {
      const int r = (int)(__umul24((unsigned)p, magic) >> 20), j = 4 * (p - r * c4);
      *reinterpret_cast<floatx4p *>(L + r * S + j) =
          *reinterpret_cast<const floatx4p *>(logits + (wrow0 + r) * (long long)ld + j);
    }
  }
  floatx4p in[NP > 0 ? NP : 1];
#pragma unroll
  for (int u = 0; u < NP; u++) {
    const int p = ln + 64 * u;
    if (p < pieces) {
      const int r = (int)(__umul24((unsigned)p, magic) >> 20), j = 4 * (p - r * c4);
      in[u] = *reinterpret_cast<const floatx4p *>(logits + (wrow0 + r) * (long long)ld + j);
    }
  }
#pragma unroll
  for (int u = 0; u < NP; u++) {
    const int p = ln + 64 * u;
    if (p < pieces) {
      const int r = (int)(__umul24((unsigned)p, magic) >> 20), j = 4 * (p - r * c4);
      *reinterpret_cast<floatx4p *>(L + r * S + j) = in[u];
    }
  }
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
  const int rq = ln >> 2, q = ln & 3;
  float *l = L + rq * S;
  const bool live = rq < wrows;
  constexpr int NV = 12;
  const bool regs = c <= 4 * NV;
  float v[NV];
  // the lane's first maximum over its classes (ascending, strict >)
  float best = -INFINITY;
  int arg = 0x7fffffff;
  if (live) {
    if (regs) {
#pragma unroll
      for (int k = 0; k < NV; k++) {
        const int j = q + 4 * k;
        v[k] = j < c ? l[j] : -1e30f;
        if (j < c && (v[k] > best || arg == 0x7fffffff)) {
          best = v[k];
          arg = j;
        }
      }
    } else {
      for (int j = q; j < c; j += 4) {
        const float x = l[j];
        if (x > best || arg == 0x7fffffff) {
          best = x;
          arg = j;
        }
      }
    }
  }
  // the quad's maximum and its lowest index (all four lanes end with the same pair)
#pragma unroll
  for (int m = 1; m <= 2; m <<= 1) {
    const float ob = __shfl_xor(best, m, 64);
    const int oa = __shfl_xor(arg, m, 64);
    if (oa != 0x7fffffff && (arg == 0x7fffffff || ob > best || (ob == best && oa < arg))) {
      best = ob;
      arg = oa;
    }
  }
  // exp-sum in xent_tile's order: the lane's classes ascending, then (s0 + s1) + (s2 + s3)
  float s = 0.0f;
  if (live) {
    if (regs) {
#pragma unroll
      for (int k = 0; k < NV; k++) {
        if (q + 4 * k < c) {
          v[k] = shifted_exp(v[k], best);
          s += v[k];
        }
      }
    } else {
      for (int j = q; j < c; j += 4) {
        const float e = shifted_exp(l[j], best);
        l[j] = e;  // (the lane's own cells)
        s += e;
      }
    }
  }
  s += __shfl_xor(s, 1, 64);
  const float se = s + __shfl_xor(s, 2, 64);
  const float rse = 1.0f / se;
  if (live && q == 0) {
    if (cls) cls[wrow0 + rq] = arg;
    if (conf) conf[wrow0 + rq] = div_rn(1.0f, se, rse);  // shifted_exp = 1 at the maximum
  }
  if (!probs) return;  // uniform
  if (live) {
    if (regs) {
#pragma unroll
      for (int k = 0; k < NV; k++) {
        const int j = q + 4 * k;
        if (j < c) l[j] = div_rn(v[k], se, rse);
      }
    } else {
      for (int j = q; j < c; j += 4) l[j] = div_rn(l[j], se, rse);
    }
    for (int j = c + q; j < cp; j += 4) l[j] = 0.0f;
  }
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
  for (int p = ln; p < pieces; p += 64) {
    const int r = (int)(__umul24((unsigned)p, magic) >> 20), j = 4 * (p - r * c4);
    *reinterpret_cast<float4 *>(probs + (wrow0 + r) * (long long)ld_probs + j) =
        *reinterpret_cast<const float4 *>(L + r * S + j);
  }
}

// counts[t * c + p] += rows with truth t >= 0 predicted p: each workgroup counts its rows in an
// LDS copy of the table (integer LDS atomics), then adds its non-zero cells to global memory
// (integer atomics: the sums do not depend on the order)
__global__ __launch_bounds__(256) void k_confusion(const int *__restrict__ cls,
                                                   const int *__restrict__ truth, int n, int c,
                                                   unsigned int *__restrict__ counts) {
  extern __shared__ unsigned int tab[];
  const int cells = c * c;
  for (int i = threadIdx.x; i < cells; i += 256) tab[i] = 0u;
  __syncthreads();
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (long long)gridDim.x * 256) {
    const int t = truth[i], p = cls[i];
    if (t >= 0 && t < c && p >= 0 && p < c) atomicAdd(&tab[t * c + p], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < cells; i += 256) {
    const unsigned int v = tab[i];
    if (v) atomicAdd(&counts[i], v);
  }
}

void launch_predict_rows(const float *logits, int ld, int n, int c, int *cls, float *conf,
                         float *probs, int ld_probs, hipStream_t s) {
  PGCN_CHECK(logits && n >= 0 && c >= 1 && c <= kPredictMaxClasses && ld % 4 == 0 && ld >= c,
             PGCN_E_INVALID, "predict_rows: 1 <= c <= 128, ld a multiple of 4 and >= c");
  PGCN_CHECK(!probs || (ld_probs % 4 == 0 && ld_probs >= c), PGCN_E_INVALID,
             "predict_rows: ld_probs a multiple of 4 and >= c");
  if (n == 0 || (!cls && !conf && !probs)) return;
  const size_t lds = (size_t)kPredictRows * predict_stride((c + 3) & ~3) * sizeof(float);
  const dim3 grid((unsigned)ceil_div(n, kPredictRows));
  if (c <= 48)  // 16 rows x 12 pieces = 3 per lane
    PGCN_LAUNCH(k_predict_rows<3>, grid, dim3(PT), lds, s, logits, ld, n, c, cls, conf, probs,
                ld_probs);
  else
    PGCN_LAUNCH(k_predict_rows<0>, grid, dim3(PT), lds, s, logits, ld, n, c, cls, conf, probs,
                ld_probs);
}

void launch_confusion(const int *cls, const int *truth, int n, int c, unsigned int *counts,
                      hipStream_t s) {
  PGCN_CHECK(counts && n >= 0 && c >= 1 && c <= kPredictMaxClasses && (n == 0 || (cls && truth)),
             PGCN_E_INVALID, "confusion: 1 <= c <= 128");
  const size_t lds = (size_t)c * c * sizeof(unsigned int);  // 64 KB at c = 128
  PGCN_HIP(hipMemsetAsync(counts, 0, lds, s));
  if (n == 0) return;
  // 8 rows per thread, at most two workgroups per CU (each flushes up to c * c cells)
  const unsigned blocks = (unsigned)std::min<long long>(ceil_div(n, 256 * 8), 2 * kCUs);
  PGCN_LAUNCH(k_confusion, dim3(blocks), dim3(256), lds, s, cls, truth, n, c, counts);
}

}  // namespace pgcn
