// Softmax over the stored entries of every CSR row (torch.sparse.softmax(A, dim = -1) on a CSR tensor; DGL / PyG: "edge
// softmax") and its backward — gfx950.  Contract: include/mi_spmm.h, "CSR row softmax"; design: DESIGN.md §3.12.
//
// One kernel family, three forms of serving a row, ONE summation order:
//   register form   a group of G lanes (16, 32 or 64, picked from nnz / rows: a shape-only rule) owns a row of at most
//                   8·G entries: read once (entry p by lane p mod G), kept in registers, written once;
//   LDS form        a longer row of at most kLdsEntries is served by the whole workgroup (256 threads) after its groups'
//                   short rows: read once into LDS, written once from it;
//   streaming form  a row beyond that goes through the same workgroup in chunks of the LDS buffer: one pass for the
//                   maximum, one for the sum (chunk by chunk through LDS), one that recomputes and writes — three reads,
//                   one write, no workspace, no second launch, any length (hub rows of 10⁶ entries included).
// The columns are never read.  No atomics, no read-back, no host synchronisation: graph-capturable.
//
// THE ORDER (the bits of a row depend on its entries and `scale` alone — not on G, the form, the neighbours, the batch):
//   forward   t_p = fl(scale · x_p)   (one fp32 multiply, never fused into the subtraction)
//             m   = max_p t_p          (exact; NaN entries do not take part in it)
//             e_p = E + E·lo, E = expf(hi), hi + lo = t_p − m exactly (two-sum; the accurate exponential; a non-finite
//                   hi has no low part)
//             chain c (0 ≤ c < 64) starts at +0 and adds the e_p with p ≡ c (mod 64) in increasing p;
//             the 64 chains are combined by the xor tree: for d = 32, 16, 8, 4, 2, 1: c_i ← c_i + c_(i xor d)  → s
//             y_p = fl(e_p · fl(1 / s))
//   backward  chain c starts at +0 and takes fmaf(dy_p, y_p, ·) for p ≡ c (mod 64) in increasing p; the same tree → d
//             dx_p = fl(scale · fl(y_p · fl(dy_p − d)))
// A group of G lanes holds chains l, l + G, l + 2G, … in lane l (64 / G accumulators), so the tree's first steps
// (d ≥ G) are adds inside a lane and the rest are lane exchanges: every G reproduces the order.  The workgroup forms
// leave the sum to their first wave (G = 64), fed from LDS; everything else in them is element-wise.
// Padding adds +0 (or fmaf(0, 0, ·)) to a chain, which changes no bit: a chain is never −0.
// Special values follow the arithmetic: −inf → 0; a NaN or +inf entry, or a row of only −inf, → NaN in the whole row.
// bfloat16 / float16: entries widened exactly, all of the above in fp32, one rounding at the store.
#include "lowp_device.h"

#pragma clang fp contract(off)

#include "csr_softmax_device.h"

namespace {

constexpr int kBlock = 256;        // threads of a workgroup
constexpr int kRegs = 8;           // entries per lane of the register form
constexpr int kLdsEntries = 4096;  // floats of the workgroup forms' buffer (16 KiB: does not limit the register form's occupancy)

// the maximum over the workgroup of one value per thread (red: 4 floats of LDS)
__device__ __forceinline__ float block_max(float v, float* red) {
  v = tree_max<64>(v);
  __syncthreads();  // red may still be read from the previous use
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return __builtin_fmaxf(__builtin_fmaxf(red[0], red[1]), __builtin_fmaxf(red[2], red[3]));
}


// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <class E>
__device__ void softmax_row_block(const typename E::S* x, typename E::S* y, int L, float scale, float* lds, float* red, unsigned z) {
  const int tid = threadIdx.x;
  const bool one = L <= kLdsEntries;
  float m = -__builtin_inff();
  for (int p = tid; p < L; p += kBlock) {
    const float t = __fmul_rn(scale, E::up(x[p]));
    if (one) lds[p] = t;
    m = __builtin_fmaxf(m, t);
  }
  m = block_max(m, red);
  float acc = 0.f;  // chain `tid` of the first wave
  for (int c0 = 0; c0 < L; c0 += kLdsEntries) {
    const int n = min(kLdsEntries, L - c0);
    if (!one) __syncthreads();  // the previous chunk has been summed
    for (int p = tid; p < n; p += kBlock) lds[p] = exp_shifted(one ? lds[p] : __fmul_rn(scale, E::up(x[c0 + p])), m);
    __syncthreads();
    if (tid < 64)
      for (int p = tid; p < n; p += 64) acc = acc + lds[p];  // kLdsEntries % 64 == 0: p ≡ c0 + p (mod 64)
  }
  if (tid < 64) {
    acc = tree_sum<64>(acc);
    if (tid == 0) red[4] = acc;
  }
  __syncthreads();
  const float inv = 1.0f / red[4];
  if (one) {
    for (int p = tid; p < L; p += kBlock) y[p] = E::down(lds[p] * inv, z);
  } else {
    for (int p = tid; p < L; p += kBlock) y[p] = E::down(exp_shifted(__fmul_rn(scale, E::up(x[p])), m) * inv, z);
  }
  __syncthreads();  // lds and red are free again
}

template <class E, int G>
__global__ __launch_bounds__(kBlock) void csr_softmax_kernel(const int32_t* __restrict__ rowptr, int M, long rows,
                                                             const typename E::S* x, float scale, typename E::S* y) {
  constexpr int NA = 64 / G, RPB = kBlock / G;
  const unsigned z = (unsigned)(M >> 31);  // 0 (M ≥ 1), opaque to the compiler: see down()
  __shared__ float lds[kLdsEntries];
  __shared__ float red[8];
  __shared__ int big_start[RPB], big_len[RPB];
  const int lane = threadIdx.x & (G - 1), grp = threadIdx.x / G;
  int start, L;
  row_span(rowptr, (long)blockIdx.x * RPB + grp, M, rows, start, L);
  const bool big = L > G * kRegs;
  if (lane == 0) {
    big_start[grp] = start;
    big_len[grp] = big ? L : 0;
  }
  if (!big && L > 0) {
    const typename E::S* xr = x + start;
    typename E::S* yr = y + start;
    float t[kRegs];
    float m = -__builtin_inff();
#pragma unroll
    for (int j = 0; j < kRegs; ++j) {
      const int p = lane + j * G;
      t[j] = p < L ? __fmul_rn(scale, E::up(xr[p])) : -__builtin_inff();
      m = __builtin_fmaxf(m, t[j]);
    }
    m = tree_max<G>(m);
    float acc[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = 0.f;
#pragma unroll
    for (int j = 0; j < kRegs; ++j) {
      t[j] = lane + j * G < L ? exp_shifted(t[j], m) : 0.f;
      acc[j % NA] = acc[j % NA] + t[j];
    }
    const float inv = 1.0f / tree_sum<G>(fold_chains<NA>(acc));
#pragma unroll
    for (int j = 0; j < kRegs; ++j) {
      const int p = lane + j * G;
      if (p < L) yr[p] = E::down(t[j] * inv, z);
    }
  }
  if (!__syncthreads_or(big)) return;
  for (int r = 0; r < RPB; ++r)
    if (big_len[r] > 0) softmax_row_block<E>(x + big_start[r], y + big_start[r], big_len[r], scale, lds, red, z);
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
template <class E>
__device__ void softmax_bwd_row_block(const typename E::S* y, const typename E::S* dy, typename E::S* dx, int L, float scale,
                                      float* lds, float* red, unsigned z) {
  constexpr int kHalf = kLdsEntries / 2;  // y in lds[0, kHalf), dy in lds[kHalf, 2·kHalf); kHalf % 64 == 0
  const int tid = threadIdx.x;
  const bool one = L <= kHalf;
  float acc = 0.f;
  for (int c0 = 0; c0 < L; c0 += kHalf) {
    const int n = min(kHalf, L - c0);
    if (!one) __syncthreads();
    for (int p = tid; p < n; p += kBlock) {
      lds[p] = E::up(y[c0 + p]);
      lds[kHalf + p] = E::up(dy[c0 + p]);
    }
    __syncthreads();
    if (tid < 64)
      for (int p = tid; p < n; p += 64) acc = __builtin_fmaf(lds[kHalf + p], lds[p], acc);
  }
  if (tid < 64) {
    acc = tree_sum<64>(acc);
    if (tid == 0) red[4] = acc;
  }
  __syncthreads();
  const float d = red[4];
  if (one) {
    for (int p = tid; p < L; p += kBlock) dx[p] = E::down(scale * (lds[p] * (lds[kHalf + p] - d)), z);
  } else {
    for (int p = tid; p < L; p += kBlock) dx[p] = E::down(scale * (E::up(y[p]) * (E::up(dy[p]) - d)), z);
  }
  __syncthreads();
}

template <class E, int G>
__global__ __launch_bounds__(kBlock) void csr_softmax_bwd_kernel(const int32_t* __restrict__ rowptr, int M, long rows,
                                                                 const typename E::S* y, const typename E::S* dy, float scale,
                                                                 typename E::S* dx) {
  constexpr int NA = 64 / G, RPB = kBlock / G;
  const unsigned z = (unsigned)(M >> 31);  // 0 (M ≥ 1), opaque to the compiler: see down()
  __shared__ float lds[kLdsEntries];
  __shared__ float red[8];
  __shared__ int big_start[RPB], big_len[RPB];
  const int lane = threadIdx.x & (G - 1), grp = threadIdx.x / G;
  int start, L;
  row_span(rowptr, (long)blockIdx.x * RPB + grp, M, rows, start, L);
  const bool big = L > G * kRegs;
  if (lane == 0) {
    big_start[grp] = start;
    big_len[grp] = big ? L : 0;
  }
  if (!big && L > 0) {
    float yv[kRegs], gv[kRegs];
#pragma unroll
    for (int j = 0; j < kRegs; ++j) {
      const int p = lane + j * G;
      yv[j] = p < L ? E::up(y[start + p]) : 0.f;
      gv[j] = p < L ? E::up(dy[start + p]) : 0.f;
    }
    float acc[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = 0.f;
#pragma unroll
    for (int j = 0; j < kRegs; ++j) acc[j % NA] = __builtin_fmaf(gv[j], yv[j], acc[j % NA]);
    const float d = tree_sum<G>(fold_chains<NA>(acc));
#pragma unroll
    for (int j = 0; j < kRegs; ++j) {
      const int p = lane + j * G;
      if (p < L) dx[start + p] = E::down(scale * (yv[j] * (gv[j] - d)), z);
    }
  }
  if (!__syncthreads_or(big)) return;
  for (int r = 0; r < RPB; ++r)
    if (big_len[r] > 0)
      softmax_bwd_row_block<E>(y + big_start[r], dy + big_start[r], dx + big_start[r], big_len[r], scale, lds, red, z);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// lanes per row from the mean row length (shape only): a group's register form takes rows up to 8·G, so the mean row uses
// two to six of a lane's eight slots
int group_lanes(int64_t nnz, int64_t rows) {
  const int64_t mean = nnz / (rows > 0 ? rows : 1);
  return mean <= 48 ? 16 : mean <= 160 ? 32 : 64;
}

// before any HIP call; MI_OK with *work = false: nothing to do
int validate(int64_t nnz, int32_t batch, int32_t M, bool* work) {
  *work = false;
  if (nnz < 0 || batch < 0 || M < 0) return MI_EINVAL;
  if (nnz > 0x7fffffffLL) return MI_ERANGE;
  if ((int64_t)batch * ((int64_t)M + 1) > 0x7fffffffLL) return MI_ERANGE;
  *work = nnz > 0 && batch > 0 && M > 0;
  return MI_OK;
}

template <class E>
int launch_forward(const int32_t* rowptr, int64_t nnz, int32_t batch, int32_t M, const typename E::S* x, float scale,
                   typename E::S* y, hipStream_t s) {
  const long rows = (long)batch * M;
#define MI_SOFTMAX_FWD(GG)                                                                                                \
  case GG:                                                                                                               \
    hipLaunchKernelGGL((csr_softmax_kernel<E, GG>), dim3((unsigned)((rows + kBlock / GG - 1) / (kBlock / GG))),          \
                       dim3(kBlock), 0, s, rowptr, M, rows, x, scale, y);                                                \
    break;
  switch (group_lanes(nnz, rows)) {
    MI_SOFTMAX_FWD(16)
    MI_SOFTMAX_FWD(32)
    MI_SOFTMAX_FWD(64)
  }
#undef MI_SOFTMAX_FWD
  return mi::check_launch();
}

template <class E>
int launch_backward(const int32_t* rowptr, int64_t nnz, int32_t batch, int32_t M, const typename E::S* y,
                    const typename E::S* dy, float scale, typename E::S* dx, hipStream_t s) {
  const long rows = (long)batch * M;
#define MI_SOFTMAX_BWD(GG)                                                                                                \
  case GG:                                                                                                               \
    hipLaunchKernelGGL((csr_softmax_bwd_kernel<E, GG>), dim3((unsigned)((rows + kBlock / GG - 1) / (kBlock / GG))),      \
                       dim3(kBlock), 0, s, rowptr, M, rows, y, dy, scale, dx);                                           \
    break;
  switch (group_lanes(nnz, rows)) {
    MI_SOFTMAX_BWD(16)
    MI_SOFTMAX_BWD(32)
    MI_SOFTMAX_BWD(64)
  }
#undef MI_SOFTMAX_BWD
  return mi::check_launch();
}

template <class E>
int forward_entry(const int32_t* rowptr, int64_t nnz, int32_t batch, int32_t M, const typename E::S* x, float scale,
                  typename E::S* y, mi_stream_t stream) {
  bool work;
  const int st = validate(nnz, batch, M, &work);
  if (st != MI_OK || !work) return st;
  if (!rowptr || !x || !y) return MI_EINVAL;
  if (sizeof(typename E::S) == 2 && (odd(x) || odd(y))) return MI_EINVAL;
  return launch_forward<E>(rowptr, nnz, batch, M, x, scale, y, static_cast<hipStream_t>(stream));
}

template <class E>
int backward_entry(const int32_t* rowptr, int64_t nnz, int32_t batch, int32_t M, const typename E::S* y,
                   const typename E::S* dy, float scale, typename E::S* dx, mi_stream_t stream) {
  bool work;
  const int st = validate(nnz, batch, M, &work);
  if (st != MI_OK || !work) return st;
  if (!rowptr || !y || !dy || !dx) return MI_EINVAL;
  if (sizeof(typename E::S) == 2 && (odd(y) || odd(dy) || odd(dx))) return MI_EINVAL;
  return launch_backward<E>(rowptr, nnz, batch, M, y, dy, scale, dx, static_cast<hipStream_t>(stream));
}

}  // namespace

extern "C" {

// every form works in place on registers and LDS: no workspace
size_t mi_csr_softmax_workspace_bytes(int64_t, int32_t, int32_t) { return 0; }

int mi_csr_softmax_f32(const int32_t* rowptr, int64_t nnz, int32_t batch, int32_t M, const float* x, float scale, float* y,
                       void*, size_t, mi_stream_t stream) {
  return forward_entry<Fp32>(rowptr, nnz, batch, M, x, scale, y, stream);
}
int mi_csr_softmax_bf16(const int32_t* rowptr, int64_t nnz, int32_t batch, int32_t M, const uint16_t* x, float scale,
                        uint16_t* y, void*, size_t, mi_stream_t stream) {
  return forward_entry<Lowp<Bf16>>(rowptr, nnz, batch, M, x, scale, y, stream);
}
int mi_csr_softmax_f16(const int32_t* rowptr, int64_t nnz, int32_t batch, int32_t M, const uint16_t* x, float scale,
                       uint16_t* y, void*, size_t, mi_stream_t stream) {
  return forward_entry<Lowp<F16>>(rowptr, nnz, batch, M, x, scale, y, stream);
}

int mi_csr_softmax_backward_f32(const int32_t* rowptr, int64_t nnz, int32_t batch, int32_t M, const float* y, const float* dy,
                                float scale, float* dx, void*, size_t, mi_stream_t stream) {
  return backward_entry<Fp32>(rowptr, nnz, batch, M, y, dy, scale, dx, stream);
}
int mi_csr_softmax_backward_bf16(const int32_t* rowptr, int64_t nnz, int32_t batch, int32_t M, const uint16_t* y,
                                 const uint16_t* dy, float scale, uint16_t* dx, void*, size_t, mi_stream_t stream) {
  return backward_entry<Lowp<Bf16>>(rowptr, nnz, batch, M, y, dy, scale, dx, stream);
}
int mi_csr_softmax_backward_f16(const int32_t* rowptr, int64_t nnz, int32_t batch, int32_t M, const uint16_t* y,
                                const uint16_t* dy, float scale, uint16_t* dx, void*, size_t, mi_stream_t stream) {
  return backward_entry<Lowp<F16>>(rowptr, nnz, batch, M, y, dy, scale, dx, stream);
}

}  // extern "C"
