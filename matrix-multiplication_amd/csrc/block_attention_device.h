// Device-side pieces shared by the three block-sparse attention units — block_attention.hip (forward and backward over
// workgroup tiles staged in LDS), block_attention_decode.hip (one wave per list entry, k fragments straight from global
// memory) and block_attention_prefill.hip (the forward's tiles fed through the KV cache's addressing, §3.27) — said once
// (DESIGN.md §3.24): the block size, the transposed image of a walk block, the scores of a walk block staged in LDS (the
// training and the prefill walks'), a score-shaped tile as the B operand of the product that sums over the walk rows, that
// product, and the reductions over a row's four lanes.  The decode unit's `score` from registers, the walkers and the Args
// stay with their units.  Not installed.
// Everything here has internal linkage (an anonymous namespace per including unit).
#ifndef MI_BLOCK_ATTENTION_DEVICE_H_
#define MI_BLOCK_ATTENTION_DEVICE_H_

#include "mfma_device.h"

namespace {

constexpr int kB = 64;       // rows of a block: the kernels' tile on both sides
constexpr int kTStr = kStr;  // row stride of a transposed image [D][64 + 8] in elements
static_assert(kB == kTileK, "a transposed image row is one staged k-tile");

// acc[f][r] = ⟨walk row 16f + 4lg + r, own row li⟩ over d, from the row image R [64][D + 8] of the walk block in LDS
template <class T, int D>
__device__ __forceinline__ void score(f32x4 (&acc)[4], const unsigned short* R, const uint4 (&own)[D / 32], int li, int lg) {
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < D / 32; ++s) {
      const uint4 a = *reinterpret_cast<const uint4*>(R + (16 * f + li) * (D + 8) + 32 * s + 8 * lg);
      acc[f] = mfma<T>(a, own[s], acc[f]);
    }
  }
}

// a score-shaped tile narrowed to T as the B operand of the two k-steps over the walk rows
template <class T>
__device__ __forceinline__ void pack_tile(uint4 (&b)[2], const f32x4 (&x)[4]) {
#pragma unroll
  for (int s = 0; s < 2; ++s)
    b[s] = uint4{pack2<T>(x[2 * s][0], x[2 * s][1]), pack2<T>(x[2 * s][2], x[2 * s][3]), pack2<T>(x[2 * s + 1][0], x[2 * s + 1][1]),
                 pack2<T>(x[2 * s + 1][2], x[2 * s + 1][3])};
}

// out[fd][r] += Σ over the walk rows of Tt[d = 16fd + 4lg + r][walk row] · b[walk row][own row li]
template <class T, int D>
__device__ __forceinline__ void accumulate(f32x4 (&out)[D / 16], const unsigned short* Tt, const uint4 (&b)[2], int li, int lg) {
#pragma unroll
  for (int fd = 0; fd < D / 16; ++fd)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const unsigned short* p = Tt + (16 * fd + li) * kTStr + 32 * s + 4 * lg;
      const uint2 lo = *reinterpret_cast<const uint2*>(p), hi = *reinterpret_cast<const uint2*>(p + 16);
      out[fd] = mfma<T>(uint4{lo.x, lo.y, hi.x, hi.y}, b[s], out[fd]);
    }
}

__device__ __forceinline__ float group_max(float x) {  // over the four lanes li, li + 16, li + 32, li + 48
  x = fmaxf(x, __shfl_xor(x, 16));
  return fmaxf(x, __shfl_xor(x, 32));
}
__device__ __forceinline__ float group_sum(float x) {
  x = x + __shfl_xor(x, 16);
  return x + __shfl_xor(x, 32);
}

}  // namespace

#endif  // MI_BLOCK_ATTENTION_DEVICE_H_
