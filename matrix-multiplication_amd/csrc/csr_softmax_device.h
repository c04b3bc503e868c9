// Device-side pieces shared by the units that walk CSR rows in the softmax's order (csr_softmax.hip: the row softmax;
// csr_attention.hip: the fused attention row kernels).  Not installed.  Everything here has internal linkage (an
// anonymous namespace per including unit).  The including unit sets `#pragma clang fp contract(off)` BEFORE including this
// file: no expression below may be contracted.
#ifndef MI_CSR_SOFTMAX_DEVICE_H_
#define MI_CSR_SOFTMAX_DEVICE_H_

#include "lowp_device.h"

namespace {

// the xor tree over the lanes of a group of G (d = G/2 … 1); every lane ends with the result
template <int G>
__device__ __forceinline__ float tree_sum(float v) {
#pragma unroll
  for (int d = G / 2; d >= 1; d >>= 1) v = v + __shfl_xor(v, d);
  return v;
}
template <int G>
__device__ __forceinline__ float tree_max(float v) {
#pragma unroll
  for (int d = G / 2; d >= 1; d >>= 1) v = __builtin_fmaxf(v, __shfl_xor(v, d));
  return v;
}
// the tree's steps d = 32 … G on the NA = 64 / G chains a lane holds (chain index l + G·k ↔ acc[k])
template <int NA>
__device__ __forceinline__ float fold_chains(float (&acc)[NA]) {
#pragma unroll
  for (int h = NA / 2; h >= 1; h >>= 1)
#pragma unroll
    for (int k = 0; k < h; ++k) acc[k] = acc[k] + acc[k + h];
  return acc[0];
}

// exp(t − m) without the rounding of the subtraction: t − m = hi + lo exactly (two-sum), exp(hi + lo) = E + E·lo with
// E = expf(hi) up to lo² ≤ 2⁻³⁸.  (Rounding t − m alone costs half an ulp OF THE DIFFERENCE — 1.9e-6 relative in e at a
// spread of 32 … 64 — which is sixteen times the exponential's own error.)  A non-finite difference has no low part:
// −inf gives 0, NaN stays NaN.
__device__ __forceinline__ float exp_shifted(float t, float m) {
  const float hi = t - m;
  const float bb = hi - t;
  const float lo = (t - (hi - bb)) + (-m - bb);
  const float e = expf(hi);
  return __builtin_isfinite(hi) ? __builtin_fmaf(e, lo, e) : e;
}

// (start, length) of global row g of a batch of M-row items; offsets [batch, M + 1] with global bases
__device__ __forceinline__ void row_span(const int32_t* __restrict__ rowptr, long g, int M, long rows, int& start, int& len) {
  start = 0;
  len = 0;
  if (g < rows) {
    const long item = g / M, at = g + item;  // item·(M + 1) + (g − item·M)
    start = rowptr[at];
    len = rowptr[at + 1] - start;
    if (len < 0) len = 0;
  }
}

}  // namespace

#endif  // MI_CSR_SOFTMAX_DEVICE_H_
