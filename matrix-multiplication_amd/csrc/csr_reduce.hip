// CSR × dense with a max / min / mean reduction over each row's products, and the gradients of max / min, for gfx950
// (MI355X), fp32.  Contract: include/mi_spmm.h (mi_spmm_csr_reduce_f32 and the entries after it); the semantics are those
// of torch.sparse.mm(A, B, reduce=...) (aten::_sparse_mm_reduce_impl), which torch implements for CSR on the CPU only.
//
// amax (amin mirrors it with <): p_e = val[e] · B[col[e], j] (one fp32 multiply).  The result is the sequential scan
// "start at (-inf, nnz), take (p_e, e) iff p_e > cur || isnan(p_e)".  That scan equals an order-independent selection —
// the largest e with a NaN product if there is one, else the smallest e attaining the maximum (-0 == +0 is a tie; the
// output keeps p_arg's sign), else (-inf, nnz) — so a row may be split and its partial results combined (`pick`).
// An empty row gives (+0, nnz).  fmaxf / v_max_f32 drop NaN and do not order ±0: every step is compare-and-select.
//
// The reference's Reducer (src/naive_reducer.cuh) has MIN / MAX branches but its wrapper pins reduce = "sum"
// (src/naive_sparse_mm.cu:119); it would start from lowest() instead of -inf and never select a NaN.  This file follows
// torch instead.
//
// Kernels:
//  * reduce_rows_kernel: G lanes per row (G = 64: one wave, col / val through the scalar unit), W = 4 columns per lane
//    (dword-aligned 16-byte loads; a row's last, partial quad is shifted back over its neighbour — max / min are
//    idempotent, the shared columns are scanned twice and stored twice with the same bits) or W = 1 for N < 4.  U gathers
//    in flight per lane; the batch at a row's end repeats its last entry instead of branching (idempotent again).
//    With a workspace, rows beyond kHubRow entries are skipped and listed (as spmm_device.h's long_list_append does).
//  * reduce_hub_kernel: a listed row cut into S = max(1, len / kHubChunk) chunks, a 16-wave workgroup per chunk and
//    64·W columns, waves combined through LDS; S = 1 writes the result, else a partial (value, arg) row.
//  * rows_divide_kernel: out[i, :] = in[i, :] / count(i), correctly rounded (mean, and its gradient g / count).
//  * reduce_grad_b_kernel: the gradient of max / min for B (below).  No float atomics: every result is one fixed-order
//    chain.
// csr_reduce_device.h owns what this unit shares with csr_reduce_lowp.hip and instantiates here for Fp32: the selection
// steps, the hub-row list, reduce_hub_combine_kernel (the S partials of a row), reduce_grad_val_kernel, the argument
// checks of the four entries, launch_reduce and the launch ladders.  Forms<Fp32> below is this unit's part of the host
// side: the choice of W, and the sum / mean route.
#include "csr_reduce_device.h"
#include "mi_common.h"

namespace {

template <int W>
struct Cols;
template <>
struct Cols<4> {
  typedef f32x4u F;
  typedef i32x4u I;
};
template <>
struct Cols<1> {
  typedef float F;
  typedef int I;
};

template <int W>
__device__ __forceinline__ float& at(typename Cols<W>::F& v, int k) {
  if constexpr (W == 1) return v;
  else return reinterpret_cast<float*>(&v)[k];
}
template <int W>
__device__ __forceinline__ int& at(typename Cols<W>::I& v, int k) {
  if constexpr (W == 1) return v;
  else return reinterpret_cast<int*>(&v)[k];
}

// Scan entries [p, end) of one row for the W columns at Bl (= B + first column).  The batch at the end repeats entry
// end − 1 instead of branching: a repeated (p_e, e) never changes the scan's state.
template <int W, bool MAX>
__device__ __forceinline__ void scan_range(const int* __restrict__ col, const float* __restrict__ val, const float* Bl,
                                           long ldb, int p, int end, typename Cols<W>::F& cur, typename Cols<W>::I& arg) {
  using F = typename Cols<W>::F;
  for (; p < end; p += kU) {
    int c[kU];
    float v[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int q = p + u < end ? p + u : end - 1;
      c[u] = col[q];
      v[u] = val[q];
    }
    F x[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) x[u] = *reinterpret_cast<const F*>(Bl + (long)c[u] * ldb);
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int e = p + u < end ? p + u : end - 1;
#pragma unroll
      for (int k = 0; k < W; ++k) scan<MAX>(v[u] * at<W>(x[u], k), e, at<W>(cur, k), at<W>(arg, k));
    }
  }
}

// First column of lane group position gl in pass c0, or -1 when the lane has no columns there.
template <int W>
__device__ __forceinline__ int lane_column(int c0, int gl, int N) {
  int q = c0 + gl * W;
  if (q >= N) return -1;
  if (W > 1 && q + W > N) q = N - W;  // the last, partial quad: shifted back over its neighbour
  return q;
}

// ---------------------------------------------------------------------------
// G lanes per row, 256 / G rows per workgroup.  grid = ⌈M / (256/G)⌉, block = 256.
// ---------------------------------------------------------------------------
template <int G, int W, bool MAX, bool ARG>
__global__ __launch_bounds__(256) void reduce_rows_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                          const float* __restrict__ val, const float* __restrict__ B,
                                                          float* __restrict__ C, int* __restrict__ argout, int M, int N,
                                                          long ldb, long ldc, long ldarg, int nnz, HubArg hub) {
  using F = typename Cols<W>::F;
  using I = typename Cols<W>::I;
  // (written out in both units: as rows_begin(), or with only the hub test in a function, every rows kernel changed: §3.26)
  long row = ((long)blockIdx.x * 256 + threadIdx.x) / G;
  if constexpr (G == 64) row = __builtin_amdgcn_readfirstlane((int)row);
  const int gl = threadIdx.x % G;
  if (row >= M) return;
  const int p0 = rowptr[row];
  const int end = rowptr[row + 1];
  if (hub.ws != nullptr && end - p0 > kHubRow) {
    if (gl == 0) hub_append(hub, (int)row, end - p0);
    return;
  }
  for (int c0 = 0; c0 < N; c0 += G * W) {
    const int q = lane_column<W>(c0, gl, N);
    if (q < 0) break;
    F cur;
    I arg;
#pragma unroll
    for (int k = 0; k < W; ++k) at<W>(cur, k) = scan_start<MAX>(), at<W>(arg, k) = nnz;
    scan_range<W, MAX>(col, val, B + q, ldb, p0, end, cur, arg);
    if (end == p0) {
#pragma unroll
      for (int k = 0; k < W; ++k) at<W>(cur, k) = 0.f;
    }
    __builtin_nontemporal_store(cur, reinterpret_cast<F*>(C + row * ldc + q));
    if constexpr (ARG) __builtin_nontemporal_store(arg, reinterpret_cast<I*>(argout + row * ldarg + q));
  }
}

// ---------------------------------------------------------------------------
// One chunk of a listed row × 64·W columns.  grid = (cap_s, ⌈N / 64W⌉), block = 1024 (16 waves, each a contiguous
// sixteenth of the chunk), LDS = 16 · 64 · W · 8 bytes.
// ---------------------------------------------------------------------------
template <int W, bool MAX>
__global__ __launch_bounds__(1024) void reduce_hub_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                         const float* __restrict__ val, const float* __restrict__ B,
                                                         float* __restrict__ C, int* __restrict__ argout, int N, long ldb,
                                                         long ldc, long ldarg, int nnz, const int* __restrict__ ws,
                                                         int cap_e, float* __restrict__ part_val,
                                                         int* __restrict__ part_arg) {
  using F = typename Cols<W>::F;
  using I = typename Cols<W>::I;
  __shared__ float s_val[kHubWaves][64 * W];
  __shared__ int s_arg[kHubWaves][64 * W];
  // (slot → wave range and the LDS combine: written out in both units; four forms each changed hub kernels: DESIGN.md §3.26)
  const int slot = blockIdx.x;
  if (slot >= __builtin_amdgcn_readfirstlane(ws[1])) return;
  const int e = ws[4 + 4 * (long)cap_e + slot];
  if (e < 0 || e >= cap_e) return;  // (a rowptr inconsistent with nnz: a slot nobody owns)
  const int* ent = ws + 4 + 4 * (long)e;
  const int row = ent[0], sb = ent[1], S = ent[2], pb = ent[3];
  if (S == 0) return;
  const int g = slot - sb;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int start = rowptr[row];
  const long len = rowptr[row + 1] - start;
  const int lo = start + (int)(len * g / S), hi = start + (int)(len * (g + 1) / S);
  const int wlo = lo + (int)((long)(hi - lo) * wave / kHubWaves), whi = lo + (int)((long)(hi - lo) * (wave + 1) / kHubWaves);
  const int q = lane_column<W>(blockIdx.y * 64 * W, lane, N);
  F cur;
  I arg;
#pragma unroll
  for (int k = 0; k < W; ++k) at<W>(cur, k) = scan_start<MAX>(), at<W>(arg, k) = nnz;
  if (q >= 0) scan_range<W, MAX>(col, val, B + q, ldb, wlo, whi, cur, arg);
#pragma unroll
  for (int k = 0; k < W; ++k) s_val[wave][lane * W + k] = at<W>(cur, k), s_arg[wave][lane * W + k] = at<W>(arg, k);
  __syncthreads();
  if (wave != 0 || q < 0) return;
  for (int w = 1; w < kHubWaves; ++w) {
#pragma unroll
    for (int k = 0; k < W; ++k) pick<MAX>(s_val[w][lane * W + k], s_arg[w][lane * W + k], at<W>(cur, k), at<W>(arg, k));
  }
  if (S == 1) {
    *reinterpret_cast<F*>(C + (long)row * ldc + q) = cur;
    if (argout) *reinterpret_cast<I*>(argout + (long)row * ldarg + q) = arg;
  } else {
    *reinterpret_cast<F*>(part_val + (long)(pb + g) * N + q) = cur;
    *reinterpret_cast<I*>(part_arg + (long)(pb + g) * N + q) = arg;
  }
}

// out[i, j] = in[i, j] / count(i) (correctly rounded); rows without entries are copied.  One wave per row, block = 256.
__global__ __launch_bounds__(256) void rows_divide_kernel(const int* __restrict__ rowptr, int M, int N,
                                                          const float* in, long ldin, float* out, long ldout) {
  const long row = __builtin_amdgcn_readfirstlane((int)(((long)blockIdx.x * 256 + threadIdx.x) >> 6));
  if (row >= M) return;
  const int cnt = rowptr[row + 1] - rowptr[row];
  const float d = (float)cnt;
  for (int j = threadIdx.x & 63; j < N; j += 64) {
    const float x = in[row * ldin + j];
    out[row * ldout + j] = cnt > 0 ? __fdiv_rn(x, d) : x;
  }
}

// ---------------------------------------------------------------------------
// grad_B[k, j] = Σ_{t in row k of Aᵀ} [arg[i, j] == perm[t]] · val[perm[t]] · g[i, j],  i = t_col[t], in Aᵀ order (one fmaf
// chain per element).  G lanes per row of Aᵀ, W columns per lane (the forward's layout; shifted-back quads compute the
// same chain twice).  grid = ⌈K / (256/G)⌉, block = 256.
// ---------------------------------------------------------------------------
template <int G, int W>
__global__ __launch_bounds__(256) void reduce_grad_b_kernel(const int* __restrict__ t_rowptr, const int* __restrict__ t_col,
                                                            const int* __restrict__ perm, const float* __restrict__ val,
                                                            int K, int N, const float* __restrict__ Gm, long ldg,
                                                            const int* __restrict__ argin, long ldarg,
                                                            float* __restrict__ grad_b, long ldgb) {
  using F = typename Cols<W>::F;
  using I = typename Cols<W>::I;
  long row = ((long)blockIdx.x * 256 + threadIdx.x) / G;
  if constexpr (G == 64) row = __builtin_amdgcn_readfirstlane((int)row);
  const int gl = threadIdx.x % G;
  if (row >= K) return;
  const int p0 = t_rowptr[row], end = t_rowptr[row + 1];
  for (int c0 = 0; c0 < N; c0 += G * W) {
    const int q = lane_column<W>(c0, gl, N);
    if (q < 0) break;
    F acc;
#pragma unroll
    for (int k = 0; k < W; ++k) at<W>(acc, k) = 0.f;
    for (int p = p0; p < end; p += kU) {
      int e[kU], i[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int t = p + u < end ? p + u : end - 1;
        e[u] = perm[t];
        i[u] = t_col[t];
      }
      I a[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) a[u] = *reinterpret_cast<const I*>(argin + (long)i[u] * ldarg + q);
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        if (p + u >= end) break;
        const float v = val[e[u]];
#pragma unroll
        for (int k = 0; k < W; ++k)
          if (at<W>(a[u], k) == e[u]) at<W>(acc, k) = __builtin_fmaf(v, Gm[(long)i[u] * ldg + q + k], at<W>(acc, k));
      }
    }
    *reinterpret_cast<F*>(grad_b + row * ldgb + q) = acc;
  }
}

// ---------------------------------------------------------------------------
// host side: the checks, launch_reduce and the ladders are csr_reduce_device.h's; here the choice of W
// ---------------------------------------------------------------------------
template <int W, bool MAX, bool ARG>
int launch_rows(const ReduceCall<float>& c, const HubArg& hub, hipStream_t s) {
  const int G = lanes_for<W>(c.N);
  const dim3 grid((unsigned)(((int64_t)c.M * G + 255) / 256));
#define MI_REDUCE_ROWS(GG)                                                                                                   \
  hipLaunchKernelGGL((reduce_rows_kernel<GG, W, MAX, ARG>), grid, dim3(256), 0, s, c.rowptr, c.col, c.val, c.B, c.C, c.arg, \
                     c.M, c.N, c.ldb, c.ldc, c.ldarg, c.nnz, hub)
  MI_REDUCE_FOR_LANES(G, MI_REDUCE_ROWS)
#undef MI_REDUCE_ROWS
  return mi::check_launch();
}

template <>
struct Forms<Fp32> {
  static int sum_or_mean(const int32_t* rowptr, const int32_t* col, const float* val, int64_t nnz, int32_t M, int32_t K,
                         int32_t N, const float* B, int64_t ldb, float* C, int64_t ldc, int reduce, void* workspace,
                         size_t workspace_bytes, hipStream_t s) {
    int st = mi_spmm_csr_ws_f32(rowptr, col, val, nnz, M, K, N, B, ldb, nullptr, C, ldc, workspace, workspace_bytes,
                                static_cast<mi_stream_t>(s));
    if (st != MI_OK || reduce == MI_REDUCE_SUM) return st;
    return divide(rowptr, M, N, C, ldc, C, ldc, s);
  }

  static int form(const ReduceCall<float>& c) { return c.N >= 4 ? 4 : 1; }  // W

  template <bool MAX>
  static int rows(const ReduceCall<float>& c, int W, const HubArg& hub, hipStream_t s) {
    if (W == 4) return c.arg ? launch_rows<4, MAX, true>(c, hub, s) : launch_rows<4, MAX, false>(c, hub, s);
    return c.arg ? launch_rows<1, MAX, true>(c, hub, s) : launch_rows<1, MAX, false>(c, hub, s);
  }

  template <bool MAX>
  static int hub(const ReduceCall<float>& c, int W, dim3 grid, const int* ws, int cap_e, float* part_val, int* part_arg,
                 hipStream_t s) {
    if (W == 4)
      hipLaunchKernelGGL((reduce_hub_kernel<4, MAX>), grid, dim3(1024), 0, s, c.rowptr, c.col, c.val, c.B, c.C, c.arg, c.N,
                         c.ldb, c.ldc, c.ldarg, c.nnz, ws, cap_e, part_val, part_arg);
    else
      hipLaunchKernelGGL((reduce_hub_kernel<1, MAX>), grid, dim3(1024), 0, s, c.rowptr, c.col, c.val, c.B, c.C, c.arg, c.N,
                         c.ldb, c.ldc, c.ldarg, c.nnz, ws, cap_e, part_val, part_arg);
    return mi::check_launch();
  }

  static int divide(const int32_t* rowptr, int32_t M, int32_t N, const float* in, int64_t ldin, float* out, int64_t ldout,
                    hipStream_t s) {
    hipLaunchKernelGGL(rows_divide_kernel, dim3((unsigned)(((int64_t)M + 3) / 4)), dim3(256), 0, s, rowptr, M, N, in,
                       (long)ldin, out, (long)ldout);
    return mi::check_launch();
  }

  static int grad_b(const int32_t* t_rowptr, const int32_t* t_col, const int32_t* perm, const float* val, int32_t K, int32_t N,
                    const float* G, long ldg, const int32_t* arg, long ldarg, float* grad_b, long ldgb, hipStream_t s) {
    if (N >= 4) {
      const int Gl = lanes_for<4>(N);
      const dim3 grid((unsigned)(((int64_t)K * Gl + 255) / 256));
#define MI_GRAD_B(GG)                                                                                                      \
  hipLaunchKernelGGL((reduce_grad_b_kernel<GG, 4>), grid, dim3(256), 0, s, t_rowptr, t_col, perm, val, K, N, G, ldg, arg, \
                     ldarg, grad_b, ldgb)
      MI_REDUCE_FOR_LANES(Gl, MI_GRAD_B)
#undef MI_GRAD_B
    } else {
      const dim3 grid((unsigned)(((int64_t)K * 4 + 255) / 256));
      hipLaunchKernelGGL((reduce_grad_b_kernel<4, 1>), grid, dim3(256), 0, s, t_rowptr, t_col, perm, val, K, N, G, ldg, arg,
                         ldarg, grad_b, ldgb);
    }
    return mi::check_launch();
  }
};

}  // namespace

extern "C" {

size_t mi_spmm_csr_reduce_workspace_bytes(int64_t nnz, int32_t N) {
  if (nnz <= 0 || N <= 0) return 0;
  const size_t hub = hub_ws_layout(nnz, N).bytes, sum = mi_spmm_csr_workspace_bytes(nnz, N);
  return hub > sum ? hub : sum;
}

int mi_spmm_csr_reduce_f32(const int32_t* rowptr, const int32_t* col, const float* val, int64_t nnz, int32_t M, int32_t K,
                           int32_t N, const float* B, int64_t ldb, float* C, int64_t ldc, int32_t* arg, int64_t ldarg,
                           int reduce, void* workspace, size_t workspace_bytes, mi_stream_t stream) {
  return reduce_entry<Fp32>(rowptr, col, val, nnz, M, K, N, B, ldb, C, ldc, arg, ldarg, reduce, workspace, workspace_bytes,
                            stream);
}

int mi_spmm_rows_divide_f32(const int32_t* rowptr, int32_t M, int32_t N, const float* in, int64_t ldin, float* out,
                            int64_t ldout, mi_stream_t stream) {
  return divide_entry<Fp32>(rowptr, M, N, in, ldin, out, ldout, stream);
}

int mi_spmm_reduce_grad_val_f32(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t M, int32_t K, int32_t N,
                                const float* B, int64_t ldb, const float* G, int64_t ldg, const int32_t* arg,
                                int64_t ldarg, float* grad_val, mi_stream_t stream) {
  return grad_val_entry<Fp32>(rowptr, col, nnz, M, K, N, B, ldb, G, ldg, arg, ldarg, grad_val, stream);
}

int mi_spmm_reduce_grad_b_f32(const int32_t* t_rowptr, const int32_t* t_col, const int32_t* perm, const float* val,
                              int64_t nnz, int32_t M, int32_t K, int32_t N, const float* G, int64_t ldg,
                              const int32_t* arg, int64_t ldarg, float* grad_b, int64_t ldgb, mi_stream_t stream) {
  return grad_b_entry<Fp32>(t_rowptr, t_col, perm, val, nnz, M, K, N, G, ldg, arg, ldarg, grad_b, ldgb, stream);
}

}  // extern "C"
