// parallel-gcn_amd/csrc/k_multilabel.hip -- multi-label node classification for gfx950: the
// per-class sigmoid with binary cross-entropy on logits (loss, gradient, Hamming errors), the
// per-row thresholded prediction, and the per-class tp / fp / fn counts behind micro / macro F1.
//
// New with the multi-label engine (the reference trains one class per node).  Labels are a bit
// matrix label_bits[n][words] (bit j % 32 of word j / 32: node i has class j); a row is labelled
// iff truth[i] >= 0, the single-label convention, so the split machinery keyed on it is shared.
// The loss has the cross-entropy kernel's contract: kXentRows rows per workgroup, per-block
// {loss sum, wrong} partials reduced by k_reduce_scalars, the gradient divided by `count`
// (labelled rows of the split x classes, known on the host).  Unlike it, the logits are never
// written.  All three kernels are element-wise: a row's float4s lie on adjacent lanes, and
// nothing goes through LDS but the four waves' sums.  The loss kernel's time is its arithmetic
// per element (an exponential, a log1p series, up to three quotients), not its bytes: DESIGN.md
// §3 "Multi-label loss" has the measurements.
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"
#include "softmax_parts.hpp"

#pragma clang fp contract(off)

namespace pgcn {

#ifndef PGCN_XENT_ROWS
#define PGCN_XENT_ROWS 64
#endif
constexpr int MR = PGCN_XENT_ROWS;  // rows per block (xent_blocks' rows: the partials' layout)
constexpr int MT = 4 * MR;          // 4 waves, wave w on rows MR / 4 * w ...
constexpr int MWR = MR / 4;         // rows per wave
typedef float floatx4m __attribute__((ext_vector_type(4)));

// log1p(e) for 0 <= e <= 1 as 2 atanh(s), s = e / (2 + e) <= 1/3: the odd series through s^15
// (the first dropped term is below 1.4e-9 of the sum), Horner in s^2.  Within 4 units of 2^-24
// relative of log1p for every normal e (a float32 restatement against float64 over 2.4 M values:
// 3.8), and e itself for e -> 0.  The device library's log1pf took about 200 instructions per
// element here and made the kernel VALU-bound.
__device__ __forceinline__ float log1p_unit(float e) {
  const float d = 2.0f + e;
  const float s = div_rn(e, d, __builtin_amdgcn_rcpf(d)), s2 = s * s;
  float p = 0x1.111112p-4f;              // 1/15
  p = fmaf(p, s2, 0x1.3b13b2p-4f);       // 1/13
  p = fmaf(p, s2, 0x1.745d18p-4f);       // 1/11
  p = fmaf(p, s2, 0x1.c71c72p-4f);       // 1/9
  p = fmaf(p, s2, 0x1.24924ap-3f);       // 1/7
  p = fmaf(p, s2, 0x1.99999ap-3f);       // 1/5
  p = fmaf(p, s2, 0x1.555556p-2f);       // 1/3
  p = fmaf(p, s2, 1.0f);
  return (2.0f * s) * p;
}

// One element: x the logit, y its target bit.  e = exp(-|x|) <= 1, so neither sign overflows:
//   loss    = max(x, 0) - x y + log1p(e)                                  (log1p_unit)
//   sigmoid = (x >= 0 ? 1 : e) / (1 + e),  sigmoid - 1 = -(x >= 0 ? e : 1) / (1 + e)
// (the y = 1 gradient from the second form: no cancelling subtraction).  Returns sigmoid - y
// (TRAIN; an eval call skips the quotient).  The reciprocal of 1 + e in [1, 2] is the hardware's
// (1 ulp): div_rn's correction step then leaves the quotient within an ulp.
template <bool TRAIN>
__device__ __forceinline__ float bce_elem(float x, bool y, float *loss, int *wrong) {
  const float e = exp_nonpos(-fabsf(x));
  *loss += (fmaxf(x, 0.0f) - (y ? x : 0.0f)) + log1p_unit(e);
  *wrong += ((x > 0.0f) != y) ? 1 : 0;
  if constexpr (!TRAIN) return 0.0f;
  const float den = 1.0f + e, rden = __builtin_amdgcn_rcpf(den);
  const bool pos = x >= 0.0f;
  const float num = y ? (pos ? -e : -1.0f) : (pos ? 1.0f : e);
  return div_rn(num, den, rden);
}

// The float4 piece of columns [4 j, 4 j + 4) of one labelled row: word = the label word holding
// those columns' bits.  Columns >= c contribute nothing and get a zero gradient (selects: their
// logits may be NaN).
template <bool TRAIN>
__device__ __forceinline__ floatx4m bce_piece(floatx4m x, unsigned word, int j, int c, float count,
                                              float rcount, float *loss, int *wrong) {
  floatx4m g;
  const unsigned bits = word >> ((4 * j) & 31);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    float l = 0.0f;
    int w = 0;
    const float d = bce_elem<TRAIN>(x[k], (bits >> k) & 1u, &l, &w);
    const bool in = 4 * j + k < c;
    if (in) {
      *loss += l;
      *wrong += w;
    }
    g[k] = TRAIN && in ? div_rn(d, count, rcount) : 0.0f;
  }
  return g;
}

// NP > 0: a wave's MWR rows of ld4 float4s fit NP pieces per lane (MWR * ld4 <= 64 NP), all
// loaded before the first is used (one HBM latency per wave); NP = 0: any ld, a plain loop.
// Piece p of a wave = row p / ld4, float4 p % ld4: a row's float4s on adjacent lanes.
// A piece's logits, label word and truth are loaded together (no load waits for another; an
// unlabelled row's logits are read and dropped: the n c floats of the kernel's byte count).
// TRAIN: the gradient is computed and written; an eval call computes the loss terms only.
template <int NP, bool TRAIN>
__global__ __launch_bounds__(MT) void k_bce_fwd(const float *__restrict__ logits, int ld,
                                                float *__restrict__ grad,
                                                const int *__restrict__ truth,
                                                const uint32_t *__restrict__ label_bits, int words,
                                                int n, int c, int count,
                                                float *__restrict__ partials) {
  __shared__ float red[2 * (MT / 64)];
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
  const int ld4 = ld >> 2, c4 = (c + 3) >> 2;
  const long long wrow0 = (long long)blockIdx.x * MR + (long long)MWR * wv;
  const int wrows = (int)max(0LL, min((long long)MWR, (long long)n - wrow0));
  const int pieces = wrows * ld4;
  const float fcount = (float)count, rcount = 1.0f / fcount;
  float loss = 0.0f;
  int wrong = 0;
  if constexpr (NP > 0) {
    floatx4m x[NP];
    unsigned word[NP];
    int row[NP], col[NP];
    bool use[NP];
#pragma unroll
    for (int u = 0; u < NP; u++) {
      const int p = ln + 64 * u;
      row[u] = p / ld4;
      col[u] = p - row[u] * ld4;
      use[u] = false;
      x[u] = floatx4m{0.0f, 0.0f, 0.0f, 0.0f};
      word[u] = 0u;
      if (p < pieces && col[u] < c4) {
        const long long i = wrow0 + row[u];
        use[u] = truth[i] >= 0;
        x[u] = *reinterpret_cast<const floatx4m *>(logits + i * (long long)ld + 4 * col[u]);
        word[u] = label_bits[i * (long long)words + ((4 * col[u]) >> 5)];
      }
    }
#pragma unroll
    for (int u = 0; u < NP; u++) {
      const int p = ln + 64 * u;
      floatx4m g = {0.0f, 0.0f, 0.0f, 0.0f};
      if (use[u]) g = bce_piece<TRAIN>(x[u], word[u], col[u], c, fcount, rcount, &loss, &wrong);
      if (TRAIN && p < pieces)
        *reinterpret_cast<floatx4m *>(grad + (wrow0 + row[u]) * (long long)ld + 4 * col[u]) = g;
    }
  } else {
    for (int p = ln; p < pieces; p += 64) {
      const int r = p / ld4, j = p - r * ld4;
      const long long i = wrow0 + r;
      floatx4m g = {0.0f, 0.0f, 0.0f, 0.0f};
      if (j < c4) {
        const int t = truth[i];
        const floatx4m x = *reinterpret_cast<const floatx4m *>(logits + i * (long long)ld + 4 * j);
        const unsigned word = label_bits[i * (long long)words + ((4 * j) >> 5)];
        if (t >= 0) g = bce_piece<TRAIN>(x, word, j, c, fcount, rcount, &loss, &wrong);
      }
      if (TRAIN) *reinterpret_cast<floatx4m *>(grad + i * (long long)ld + 4 * j) = g;
    }
  }
  // the wave's sums: a fixed xor tree (every lane ends with the same bits), then the waves in
  // wave order
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    loss += __shfl_xor(loss, m, 64);
    wrong += __shfl_xor(wrong, m, 64);
  }
  if (ln == 0) {
    red[2 * wv] = loss;
    red[2 * wv + 1] = (float)wrong;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float ls = red[0], ws = red[1];
#pragma unroll
    for (int w2 = 1; w2 < MT / 64; w2++) {
      ls += red[2 * w2];
      ws += red[2 * w2 + 1];
    }
    partials[2 * blockIdx.x] = ls;
    partials[2 * blockIdx.x + 1] = ws;
  }
}

// bits[i][w] bit j = logits[i][32 w + j] > 0 (columns >= c: zero); probs (optional): the sigmoid
// row, zero in columns [c, round_up4(c)).  A lane per float4 of cp = round_up4(c) columns, a
// row's float4s on adjacent lanes; the row's words are put together by the lanes that own a
// word's first float4 from their neighbours' nibbles (shuffles inside the wave: rows do not
// straddle waves, 8 lanes per word).
__global__ __launch_bounds__(256) void k_predict_multilabel(const float *__restrict__ logits,
                                                            int ld, int n, int c,
                                                            uint32_t *__restrict__ bits, int words,
                                                            float *__restrict__ probs,
                                                            int ld_probs) {
  // 32 lanes per row (c <= 128: 32 float4s), two rows per wave
  const int ln = threadIdx.x & 63, half = ln >> 5, j = ln & 31;
  const long long i = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 2 + half;
  const int c4 = (c + 3) >> 2;
  const bool live = i < n && j < c4;
  floatx4m x = {0.0f, 0.0f, 0.0f, 0.0f};
  if (live) x = *reinterpret_cast<const floatx4m *>(logits + i * (long long)ld + 4 * j);
  unsigned nib = 0u;
  floatx4m s = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const bool in = live && 4 * j + k < c;
    const float v = in ? x[k] : 0.0f;  // (padding may hold NaN)
    if (in && v > 0.0f) nib |= 1u << k;
    const float e = exp_nonpos(-fabsf(v));
    const float den = 1.0f + e;
    s[k] = in ? div_rn(v >= 0.0f ? 1.0f : e, den, 1.0f / den) : 0.0f;
  }
  // word w of the row = nibbles of lanes 8 w .. 8 w + 7 (of this half)
  unsigned word = nib << (4 * (j & 7));
#pragma unroll
  for (int m = 1; m < 8; m <<= 1) word |= __shfl_xor(word, m, 64);
  if (i < n && (j & 7) == 0 && (j >> 3) < words) bits[i * (long long)words + (j >> 3)] = word;
  if (probs && live) *reinterpret_cast<floatx4m *>(probs + i * (long long)ld_probs + 4 * j) = s;
}

// counts[0][j] tp, counts[1][j] fp, counts[2][j] fn of class j over the rows with truth >= 0:
// each workgroup counts its rows in LDS (integer atomics), then adds its non-zero cells to
// global memory (integer atomics: the sums do not depend on the order)
__global__ __launch_bounds__(256) void k_multilabel_counts(const uint32_t *__restrict__ pred,
                                                           const uint32_t *__restrict__ label,
                                                           const int *__restrict__ truth, int n,
                                                           int c, int words,
                                                           unsigned int *__restrict__ counts) {
  __shared__ unsigned int tab[3 * kPredictMaxClasses];
  for (int k = threadIdx.x; k < 3 * c; k += 256) tab[k] = 0u;
  __syncthreads();
  // one (row, word) per thread step
  const long long total = (long long)n * words;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total;
       t += (long long)gridDim.x * 256) {
    const long long i = t / words;
    const int w = (int)(t - i * words);
    if (truth[i] < 0) continue;
    const int left = c - 32 * w;
    const unsigned valid = left >= 32 ? 0xffffffffu : ((1u << left) - 1u);
    const unsigned p = pred[t] & valid, y = label[t] & valid;
    unsigned tp = p & y, fp = p & ~y, fn = ~p & y;
    while (tp) {
      const int b = __builtin_ctz(tp);
      tp &= tp - 1;
      atomicAdd(&tab[32 * w + b], 1u);
    }
    while (fp) {
      const int b = __builtin_ctz(fp);
      fp &= fp - 1;
      atomicAdd(&tab[c + 32 * w + b], 1u);
    }
    while (fn) {
      const int b = __builtin_ctz(fn);
      fn &= fn - 1;
      atomicAdd(&tab[2 * c + 32 * w + b], 1u);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < 3 * c; k += 256) {
    const unsigned int v = tab[k];
    if (v) atomicAdd(&counts[k], v);
  }
}

void check_bce_args(int ld, int words, int n, int c, int count) {
  PGCN_CHECK(c >= 1 && c <= kPredictMaxClasses, PGCN_E_INVALID, "bce: 1 <= classes <= 128");
  PGCN_CHECK(ld >= c && ld % 4 == 0, PGCN_E_INVALID, "bce: ld a multiple of 4 and >= classes");
  PGCN_CHECK(words == (c + 31) / 32, PGCN_E_INVALID, "bce: words = ceil(classes / 32)");
  PGCN_CHECK(count >= 1 && n >= 0, PGCN_E_INVALID, "bce: count >= 1, n >= 0");
}

void launch_bce_fwd(const float *logits, int ld, float *grad, const int *truth,
                    const uint32_t *label_bits, int words, int n, int c, int count, int training,
                    float *partials, hipStream_t s) {
  check_bce_args(ld, words, n, c, count);
  if (n == 0) return;
  PGCN_CHECK(logits && truth && label_bits && partials && (!training || grad), PGCN_E_INVALID,
             "bce: null argument");
  const dim3 grid((unsigned)xent_blocks(n));
  PGCN_CHECK((long long)grid.x * MR >= n && (long long)(grid.x - 1) * MR < n, PGCN_E_INVALID,
             "bce: the block rows differ from xent_blocks'");
#define BCE(NP, TRAIN)                                                                     \
  PGCN_LAUNCH((k_bce_fwd<NP, TRAIN>), grid, dim3(MT), 0, s, logits, ld, grad, truth, label_bits, \
              words, n, c, count, partials)
#define BCE_NP(TRAIN)                   \
  do {                                  \
    if (per_wave <= 64) BCE(1, TRAIN);  \
    else if (per_wave <= 128) BCE(2, TRAIN); \
    else if (per_wave <= 192) BCE(3, TRAIN); \
    else BCE(0, TRAIN);                 \
  } while (0)
  const int per_wave = MWR * (ld / 4);
  if (training) BCE_NP(true);
  else BCE_NP(false);
#undef BCE_NP
#undef BCE
}

void check_predict_multilabel_args(int ld, int n, int c, int words, bool probs, int ld_probs) {
  PGCN_CHECK(n >= 0 && c >= 1 && c <= kPredictMaxClasses && ld % 4 == 0 && ld >= c,
             PGCN_E_INVALID, "predict_multilabel: 1 <= c <= 128, ld a multiple of 4 and >= c");
  PGCN_CHECK(words == (c + 31) / 32, PGCN_E_INVALID, "predict_multilabel: words = ceil(c / 32)");
  PGCN_CHECK(!probs || (ld_probs % 4 == 0 && ld_probs >= c), PGCN_E_INVALID,
             "predict_multilabel: ld_probs a multiple of 4 and >= c");
}

void launch_predict_multilabel(const float *logits, int ld, int n, int c, uint32_t *bits,
                               int words, float *probs, int ld_probs, hipStream_t s) {
  check_predict_multilabel_args(ld, n, c, words, probs != nullptr, ld_probs);
  if (n == 0) return;
  PGCN_CHECK(logits && bits, PGCN_E_INVALID, "predict_multilabel: null argument");
  PGCN_LAUNCH(k_predict_multilabel, dim3((unsigned)ceil_div(n, 8)), dim3(256), 0, s, logits, ld,
              n, c, bits, words, probs, ld_probs);
}

void check_multilabel_counts_args(int n, int c, int words) {
  PGCN_CHECK(n >= 0 && c >= 1 && c <= kPredictMaxClasses && words == (c + 31) / 32,
             PGCN_E_INVALID, "multilabel_counts: 1 <= c <= 128, words = ceil(c / 32)");
}

void launch_multilabel_counts(const uint32_t *pred_bits, const uint32_t *label_bits,
                              const int *truth, int n, int c, int words, unsigned int *counts,
                              hipStream_t s) {
  check_multilabel_counts_args(n, c, words);
  PGCN_CHECK(counts && (n == 0 || (pred_bits && label_bits && truth)), PGCN_E_INVALID,
             "multilabel_counts: null argument");
  PGCN_HIP(hipMemsetAsync(counts, 0, (size_t)3 * c * sizeof(unsigned int), s));
  if (n == 0) return;
  const long long total = (long long)n * words;
  const unsigned blocks = (unsigned)std::min<long long>(ceil_div(total, 256 * 8), 2 * kCUs);
  PGCN_LAUNCH(k_multilabel_counts, dim3(blocks), dim3(256), 0, s, pred_bits, label_bits, truth, n,
              c, words, counts);
}

}  // namespace pgcn
