// Device-side pieces shared by the six bfloat16 / float16 units on the matrix cores — gemm_lowp.hip, bsr_mm.hip and
// bsr_linear.hip (through bsr_device.h), block_attention.hip, block_attention_decode.hip and block_attention_prefill.hip
// (through block_attention_device.h) — said once: the wrapper round v_mfma_f32_16x16x32_{bf16,f16}, the element
// of an 8-element piece, the row stride of a staged k-tile and the transposing store of a rows-contiguous operand.  The
// element types are lowp_device.h's.  load8 and the wave's MFMA loop are NOT here: sharing them changed kernels (§3.24).
// Not installed.  Everything here has internal linkage (an anonymous namespace per including unit).
#ifndef MI_MFMA_DEVICE_H_
#define MI_MFMA_DEVICE_H_

#include "lowp_device.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// one 16 × 16 × 32 step: lane (li, lg) gives the k-values 8lg … + 7 of row li of each operand
template <class T>
__device__ __forceinline__ f32x4 mfma(uint4 a, uint4 b, f32x4 c);
template <>
__device__ __forceinline__ f32x4 mfma<Bf16>(uint4 a, uint4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
template <>
__device__ __forceinline__ f32x4 mfma<F16>(uint4 a, uint4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

constexpr int kTileK = 64;  // k per staged LDS tile (two MFMA k-steps)
// LDS row stride of a staged tile in elements.  The 144-byte row puts the 16 rows a fragment read touches on 16 different
// 16-byte bank slots.
constexpr int kStr = kTileK + 8;

// element i of a piece of 8
__device__ __forceinline__ unsigned half_of(uint4 v, int i) {
  const unsigned w = (i >> 1) == 0 ? v.x : (i >> 1) == 1 ? v.y : (i >> 1) == 2 ? v.z : v.w;
  return (i & 1) ? (w >> 16) : (w & 0xffffu);
}

// The staging store of an operand stored rows-contiguous (element (r, k) at P[k·ld + r]): unit u holds 4 k-rows × 8 rows,
// v[q] the 8 rows 8(u / 16) … + 7 at k = 4(u % 16) + q, and writes them transposed as eight 8-byte pieces of the image
// S [rows][kStr].  The 16 k-quads of a row group go to 16 consecutive lanes: a wave's 8-byte LDS writes of one transposed
// row then fall on 32 different 8-byte bank slots (2-way, the least 512 bytes allow) — with the row groups on consecutive
// lanes instead, rows 8 apart sit 1152 ≡ 128 (mod 256) bytes apart and the writes were 8-way.
__device__ __forceinline__ void store_rc(unsigned short* S, const uint4 (&v)[4], int u) {
  const int r = (u >> 4) * 8, kk = (u & 15) * 4;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint2 w = {half_of(v[0], i) | (half_of(v[1], i) << 16), half_of(v[2], i) | (half_of(v[3], i) << 16)};
    *reinterpret_cast<uint2*>(S + (r + i) * kStr + kk) = w;
  }
}

}  // namespace

#endif  // MI_MFMA_DEVICE_H_
