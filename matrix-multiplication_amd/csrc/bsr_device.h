// Device-side pieces shared by the block-sparse translation units on the matrix cores (bsr_mm.hip: A·b and the sampled
// product; bsr_linear.hip: x·Wᵀ and the weight gradient): the staging of a 64 × 64 value block and of a rows-contiguous tile
// through registers into LDS images [rows][kStr], the 32-row × (FN·16)-column wave tile and its fragment-pair store.  The
// MFMA wrapper, half_of, the row stride kStr and the transposing store are mfma_device.h's, which gemm_lowp.hip and the
// attention units share.  Not installed.  Everything here has internal linkage (an anonymous namespace
// per including unit).
#ifndef MI_BSR_DEVICE_H_
#define MI_BSR_DEVICE_H_

#include "mfma_device.h"

namespace {

constexpr int kB = 64;  // rows and columns of a block: the k-tile of every kernel here
static_assert(kB == kTileK, "a block is one staged k-tile");

__device__ __forceinline__ uint4 pack8(const unsigned short (&e)[8]) {
  return uint4{e[0] | ((unsigned)e[1] << 16), e[2] | ((unsigned)e[3] << 16), e[4] | ((unsigned)e[5] << 16),
               e[6] | ((unsigned)e[7] << 16)};
}

// 8 contiguous elements p[0 … 7], of which the first `avail` exist (zeros for the rest; nothing read when avail ≤ 0).
// (gemm_lowp.hip has this function with pack8 written out: each unit's kernels change with the other's form, §3.24.)
template <bool VEC>
__device__ __forceinline__ uint4 load8(const uint16_t* p, int avail) {
  if (VEC && avail >= 8) return *reinterpret_cast<const uint4*>(p);
  unsigned short e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) e[j] = j < avail ? p[j] : (unsigned short)0;
  return pack8(e);
}

// A 64 × 64 value block, k contiguous as stored (element (r, k) at P[64r + k]): 512 pieces of 8, two per thread.
struct BlockKC {
  uint4 lo, hi;  // pieces tid and tid + 256 (two members, not an array: they stay in registers)
  __device__ __forceinline__ void load(const uint16_t* P, int tid) {
    lo = *reinterpret_cast<const uint4*>(P + (long)tid * 8);
    hi = *reinterpret_cast<const uint4*>(P + (long)(tid + 256) * 8);
  }
  __device__ __forceinline__ void store(unsigned short* S, int tid) const {
    *reinterpret_cast<uint4*>(S + (tid >> 3) * kStr + (tid & 7) * 8) = lo;
    *reinterpret_cast<uint4*>(S + ((tid >> 3) + 32) * kStr + (tid & 7) * 8) = hi;
  }
};

// R output-side rows × 64 values of k of an operand stored rows-contiguous (element (r, k) at P[k·ld + r]): 2R units of
// 4 k-rows × 8 rows, one per thread, transposed in registers into 8-byte LDS writes (store_rc).
template <int R>
struct TileRC {
  uint4 v[4];
  template <bool VEC>
  __device__ __forceinline__ void load(const uint16_t* P, long ld, int row0, int rows, int tid) {
    const int r = row0 + (tid >> 4) * 8, kk = (tid & 15) * 4;
    const int avail = tid < 2 * R ? rows - r : 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = load8<VEC>(P + (long)(kk + q) * ld + r, avail);
  }
  __device__ __forceinline__ void store(unsigned short* S, int tid) const {
    if (tid < 2 * R) store_rc(S, v, tid);
  }
};

// The 2 × FN accumulators of a wave over one staged 64-deep k-tile: As [64][kStr] the output rows, Bs [BN][kStr] the
// output columns.  Fragment pair j/2: row li of fragment j holds column 32(j/2) + 8(li/4) + 4(j%2) + li%4 of the wave's
// tile, so that a lane ends with eight adjacent columns of one row.  (gemm_lowp_kernel and bsr_linear_kernel have this
// loop written out, FM × FN: called from there, with FM a parameter, it changed their kernels, §3.24.)
template <class T, int FN>
__device__ __forceinline__ void tile_mfma(f32x4 (&acc)[2][FN], const unsigned short* As, const unsigned short* Bs, int wm, int wn,
                                          int li, int lg) {
#pragma unroll
  for (int ks = 0; ks < kB / 32; ++ks) {
    const int kofs = ks * 32 + 8 * lg;
    uint4 af[2], bf[FN];
#pragma unroll
    for (int i = 0; i < 2; ++i) af[i] = *reinterpret_cast<const uint4*>(As + (wm * 32 + i * 16 + li) * kStr + kofs);
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int c = wn * (FN * 16) + (j >> 1) * 32 + 8 * (li >> 2) + 4 * (j & 1) + (li & 3);
      bf[j] = *reinterpret_cast<const uint4*>(Bs + c * kStr + kofs);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] = mfma<T>(bf[j], af[i], acc[i][j]);
  }
}

// lane (li, lg) holds row li of each 16-row fragment and columns 8·lg … 8·lg + 7 of each fragment pair
template <class T, int FN, bool VEC>
__device__ __forceinline__ void store_acc(const f32x4 (&acc)[2][FN], uint16_t* C, long ldc, int n0, int n, int wm, int wn, int li,
                                          int lg) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = wm * 32 + i * 16 + li;
#pragma unroll
    for (int p = 0; p < FN / 2; ++p) {
      const int c = n0 + wn * (FN * 16) + p * 32 + 8 * lg;
      const f32x4 x = acc[i][2 * p], y = acc[i][2 * p + 1];
      uint16_t* dst = C + (long)r * ldc + c;
      if (VEC && c + 8 <= n) {
        *reinterpret_cast<uint4*>(dst) =
            uint4{pack2<T>(x[0], x[1]), pack2<T>(x[2], x[3]), pack2<T>(y[0], y[1]), pack2<T>(y[2], y[3])};
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (c + e < n) dst[e] = T::down(x[e]);
          if (c + 4 + e < n) dst[4 + e] = T::down(y[e]);
        }
      }
    }
  }
}

}  // namespace

#endif  // MI_BSR_DEVICE_H_
