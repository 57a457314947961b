// parallel-gcn_amd/csrc/softmax_parts.hpp -- the loss kernel's softmax pieces (device code),
// shared by k_elementwise.hip (xent_tile) and k_predict.hip (which adds an exact correction of
// the max shift's rounding, see there).
#pragma once
#include <hip/hip_runtime.h>

namespace pgcn {

// expf for x <= 0 (a max-shifted logit): the device library's expf sequence without its
// overflow select, which cannot fire there -- the same operations in the same order, so the
// same bits (tests: the loss kernel against the oracle; `test_exp_nonpos_matches_expf`)
__device__ __forceinline__ float exp_nonpos(float x) {
  const float l2e = 0x1.715476p+0f, l2e_lo = 0x1.4ae0bep-26f;
  const float ph = x * l2e;
  const float e = __builtin_rintf(ph);
  const float pl = fmaf(x, l2e_lo, fmaf(x, l2e, -ph));
  const float r = __builtin_ldexpf(__builtin_amdgcn_exp2f((ph - e) + pl), (int)e);
  return x < -0x1.9d1da0p+6f ? 0.0f : r;
}

// a / b rounded to nearest from rb = RN(1 / b) (Markstein: q within an ulp, the residual exact
// by fma, one correction step): the IEEE quotient's bits for normal operands and results.
// The residual r = a - q b is exact only while its lowest bit (ulp(q) ulp(b) = 2^(e_q - 46))
// is representable, i.e. q >= 2^-103: below 2^-100 (r03's form missed bits for quotients up to
// 3e-38, the advisor's case) the loss kernel takes the IEEE division itself;
// tests/test_gpu_kernels.py test_div_rn_matches_ieee checks the bits over dense a (subnormals
// included) and b in [1, 128]
__device__ __forceinline__ float div_rn(float a, float b, float rb) {
  const float q = a * rb;
  if (__builtin_expect(fabsf(q) < 0x1p-100f, 0)) return a / b;
  const float r = fmaf(-q, b, a);
  return fmaf(r, rb, q);
}

}  // namespace pgcn
