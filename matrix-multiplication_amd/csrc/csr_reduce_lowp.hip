// CSR × dense with a max / min / mean reduction in bfloat16 and float16, and the gradients of max / min, for gfx950 (MI355X).
// Contract: include/mi_spmm.h (mi_spmm_csr_reduce_bf16 / _f16 and the entries after them): values, B, C and the gradients in
// T ∈ {bf16, fp16}, every product, comparison and sum in fp32 on the exactly widened operands — csr_reduce.hip's arithmetic —
// and ONE narrowing per element, at the store.  arg is the fp32 selection: never a choice among values that only tie after
// narrowing.
//
// sum is mi_spmm_csr_ex_T; mean is the same kernels with the division by the row's entry count in their epilogue
// (csr_lowp.hip, mi::spmm_lowp_mean).  Here:
//  * lowp_reduce_rows_kernel: csr_reduce.hip's reduce_rows_kernel on 2-byte elements.  G lanes per row (G = 64: one wave,
//    col / val wave-uniform), 4 columns per lane: one 8-byte load per gather (VEC: N, ldb, ldc multiples of 4, B and C 8-byte
//    aligned) or four guarded 2-byte loads (any N, leading dimension and 2-byte alignment: odd N, column-offset views).
//    The gathered words stay packed until they are multiplied, so a one-wave row keeps 16 gathers in flight per lane
//    (16 × 512 B per wave at N = 256 — the fp32 kernel's 8 × 1 KiB); the batch at a row's end repeats its last entry.
//  * lowp_reduce_hub_kernel: rows beyond kHubRow entries, listed by the rows kernel — csr_reduce.hip's split, the
//    (value, arg) partials fp32 / int32 in the same workspace layout.
//  * lowp_rows_divide_kernel, lowp_reduce_grad_b_kernel: the fp32 kernels' fixed summation orders, widened on load, rounded
//    once at the store.
// csr_reduce_device.h owns what this unit shares with csr_reduce.hip and instantiates here for Lowp<Bf16> / Lowp<F16>: the
// selection steps, the hub-row list, reduce_hub_combine_kernel, reduce_grad_val_kernel, the argument checks of the four
// entries (with the odd-pointer refusal of 2-byte elements), launch_reduce and the launch ladders.  Forms<Lowp<T>> below is
// this unit's part of the host side: the choice of VEC, and the sum / mean route.
// No float atomics; no host read-back (graph-capturable).
#include "csr_reduce_device.h"
#include "spmm_internal.h"

namespace {

// four consecutive elements as they are stored, two per dword (zeros at and beyond column N in the element form)
template <bool VEC>
__device__ __forceinline__ u32x2 load_raw4(const unsigned short* p, int j, int N) {
  if constexpr (VEC) {
    return *reinterpret_cast<const u32x2*>(p);
  } else {
    const unsigned a = j + 0 < N ? p[0] : 0u, b = j + 1 < N ? p[1] : 0u;
    const unsigned c = j + 2 < N ? p[2] : 0u, d = j + 3 < N ? p[3] : 0u;
    return u32x2{a | (b << 16), c | (d << 16)};
  }
}

template <class T>
__device__ __forceinline__ f32x4 widen4(u32x2 w) {
  return f32x4{T::lo(w.x), T::hi(w.x), T::lo(w.y), T::hi(w.y)};
}

template <bool VEC>
__device__ __forceinline__ void store_arg4(int* p, int j, int N, i32x4u a) {
  if constexpr (VEC) {
    __builtin_nontemporal_store(a, reinterpret_cast<i32x4u*>(p));
  } else {
    if (j + 0 < N) p[0] = a.x;
    if (j + 1 < N) p[1] = a.y;
    if (j + 2 < N) p[2] = a.z;
    if (j + 3 < N) p[3] = a.w;
  }
}

// Scan entries [p, end) of one row for the 4 columns j … j + 3 at Bl (= B + j): csr_reduce.hip's scan_range with U packed
// gathers in flight.  A repeated (p_e, e) never changes the scan's state.
template <class T, bool VEC, bool MAX, int U>
__device__ __forceinline__ void scan_range(const int* __restrict__ col, const unsigned short* __restrict__ val,
                                           const unsigned short* Bl, long ldb, int j, int N, int p, int end, f32x4& cur,
                                           i32x4u& arg) {
  for (; p < end; p += U) {
    int c[U];
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int q = p + u < end ? p + u : end - 1;
      c[u] = col[q];
      v[u] = up<T>(val[q]);
    }
    u32x2 x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) x[u] = load_raw4<VEC>(Bl + (long)c[u] * ldb, j, N);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = p + u < end ? p + u : end - 1;
      const f32x4 b = widen4<T>(x[u]);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float cv = cur[k];
        int ca = arg[k];
        scan<MAX>(v[u] * b[k], e, cv, ca);
        cur[k] = cv, arg[k] = ca;
      }
    }
  }
}

// (the fp32 unit starts its W columns by element: one scan_init for both changed its four hub kernels)
template <bool MAX>
__device__ __forceinline__ void scan_init(f32x4& cur, i32x4u& arg, int nnz) {
  const float s = scan_start<MAX>();
  cur = f32x4{s, s, s, s};
  arg = i32x4u{nnz, nnz, nnz, nnz};
}

// ---------------------------------------------------------------------------
// G lanes per row, 256 / G rows per workgroup, 4 columns per lane, wider rows in passes of 4·G columns.
// grid = ⌈M / (256/G)⌉, block = 256.
// ---------------------------------------------------------------------------
template <class T, int G, bool VEC, bool MAX, bool ARG>
__global__ __launch_bounds__(256) void lowp_reduce_rows_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                               const unsigned short* __restrict__ val,
                                                               const unsigned short* __restrict__ B,
                                                               unsigned short* __restrict__ C, int* __restrict__ argout, int M,
                                                               int N, long ldb, long ldc, long ldarg, int nnz, HubArg hub) {
  constexpr int U = G == 64 && VEC ? 16 : kU;
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
  for (int c0 = 0; c0 < N; c0 += G * 4) {
    const int j = c0 + gl * 4;
    if (j >= N) break;
    f32x4 cur;
    i32x4u arg;
    scan_init<MAX>(cur, arg, nnz);
    scan_range<T, VEC, MAX, U>(col, val, B + j, ldb, j, N, p0, end, cur, arg);
    if (end == p0) cur = f32x4{0.f, 0.f, 0.f, 0.f};
    store4<T, VEC>(C + row * ldc + j, j, N, cur);
    if constexpr (ARG) store_arg4<VEC>(argout + row * ldarg + j, j, N, arg);
  }
}

// ---------------------------------------------------------------------------
// One chunk of a listed row × 256 columns.  grid = (cap_s, ⌈N / 256⌉), block = 1024 (16 waves, each a contiguous sixteenth of
// the chunk), LDS = 16 · 256 · 8 bytes.  S = 1 writes the row (narrowed), else an fp32 / int32 partial row.
// ---------------------------------------------------------------------------
template <class T, bool VEC, bool MAX>
__global__ __launch_bounds__(1024) void lowp_reduce_hub_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                               const unsigned short* __restrict__ val,
                                                               const unsigned short* __restrict__ B,
                                                               unsigned short* __restrict__ C, int* __restrict__ argout, int N,
                                                               long ldb, long ldc, long ldarg, int nnz,
                                                               const int* __restrict__ ws, int cap_e,
                                                               float* __restrict__ part_val, int* __restrict__ part_arg) {
  __shared__ float s_val[kHubWaves][256];
  __shared__ int s_arg[kHubWaves][256];
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
  const int j = blockIdx.y * 256 + lane * 4;
  const bool on = j < N;
  f32x4 cur;
  i32x4u arg;
  scan_init<MAX>(cur, arg, nnz);
  if (on) scan_range<T, VEC, MAX, kU>(col, val, B + j, ldb, j, N, wlo, whi, cur, arg);
#pragma unroll
  for (int k = 0; k < 4; ++k) s_val[wave][lane * 4 + k] = cur[k], s_arg[wave][lane * 4 + k] = arg[k];
  __syncthreads();
  if (wave != 0 || !on) return;
  for (int w = 1; w < kHubWaves; ++w) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float cv = cur[k];
      int ca = arg[k];
      pick<MAX>(s_val[w][lane * 4 + k], s_arg[w][lane * 4 + k], cv, ca);
      cur[k] = cv, arg[k] = ca;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (j + k >= N) break;
    if (S == 1) {
      C[(long)row * ldc + j + k] = T::down(cur[k]);
      if (argout) argout[(long)row * ldarg + j + k] = arg[k];
    } else {
      part_val[(long)(pb + g) * N + j + k] = cur[k];
      part_arg[(long)(pb + g) * N + j + k] = arg[k];
    }
  }
}

// out[i, j] = rne_T(up(in[i, j]) / count(i)) (the fp32 division correctly rounded); rows without entries are copied.
// One wave per row, 4 columns per lane; block = 256.
template <class T, bool VEC>
__global__ __launch_bounds__(256) void lowp_rows_divide_kernel(const int* __restrict__ rowptr, int M, int N,
                                                               const unsigned short* in, long ldin, unsigned short* out,
                                                               long ldout) {
  const long row = __builtin_amdgcn_readfirstlane((int)(((long)blockIdx.x * 256 + threadIdx.x) >> 6));
  if (row >= M) return;
  const int cnt = rowptr[row + 1] - rowptr[row];
  const float d = (float)cnt;
  for (int j = 4 * (threadIdx.x & 63); j < N; j += 256) {
    f32x4 x = load4<T, VEC>(in + row * ldin + j, j, N);
    if (cnt > 0) x = f32x4{__fdiv_rn(x.x, d), __fdiv_rn(x.y, d), __fdiv_rn(x.z, d), __fdiv_rn(x.w, d)};
    store4<T, VEC>(out + row * ldout + j, j, N, x);
  }
}

// ---------------------------------------------------------------------------
// grad_B[k, j] = rne_T(Σ_{t in row k of Aᵀ} [arg[i, j] == perm[t]] · val[perm[t]] · g[i, j]), i = t_col[t], in Aᵀ order: one
// fmaf chain per element (reduce_grad_b_kernel's).  G lanes per row of Aᵀ, 4 columns per lane.  VEC: 16-byte arg loads and
// 8-byte stores (N, ldgb multiples of 4, grad_b 8-byte aligned); else guarded elements.  grid = ⌈K / (256/G)⌉, block = 256.
// ---------------------------------------------------------------------------
template <class T, int G, bool VEC>
__global__ __launch_bounds__(256) void lowp_reduce_grad_b_kernel(const int* __restrict__ t_rowptr, const int* __restrict__ t_col,
                                                                 const int* __restrict__ perm,
                                                                 const unsigned short* __restrict__ val, int K, int N,
                                                                 const unsigned short* __restrict__ Gm, long ldg,
                                                                 const int* __restrict__ argin, long ldarg,
                                                                 unsigned short* __restrict__ grad_b, long ldgb) {
  long row = ((long)blockIdx.x * 256 + threadIdx.x) / G;
  if constexpr (G == 64) row = __builtin_amdgcn_readfirstlane((int)row);
  const int gl = threadIdx.x % G;
  if (row >= K) return;
  const int p0 = t_rowptr[row], end = t_rowptr[row + 1];
  for (int c0 = 0; c0 < N; c0 += G * 4) {
    const int j = c0 + gl * 4;
    if (j >= N) break;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int p = p0; p < end; p += kU) {
      int e[kU], i[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int t = p + u < end ? p + u : end - 1;
        e[u] = perm[t];
        i[u] = t_col[t];
      }
      i32x4u a[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int* src = argin + (long)i[u] * ldarg + j;
        if constexpr (VEC) {
          a[u] = *reinterpret_cast<const i32x4u*>(src);
        } else {  // (no entry index is negative: a column at or beyond N never matches)
          a[u].x = src[0];
          a[u].y = j + 1 < N ? src[1] : -1;
          a[u].z = j + 2 < N ? src[2] : -1;
          a[u].w = j + 3 < N ? src[3] : -1;
        }
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        if (p + u >= end) break;
        const float v = up<T>(val[e[u]]);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (a[u][k] == e[u]) acc[k] = __builtin_fmaf(v, up<T>(Gm[(long)i[u] * ldg + j + k]), acc[k]);
      }
    }
    store4<T, VEC>(grad_b + row * ldgb + j, j, N, acc);
  }
}

// ---------------------------------------------------------------------------
// host side: the checks, launch_reduce and the ladders are csr_reduce_device.h's; here the choice of VEC
// ---------------------------------------------------------------------------
template <class T, bool VEC, bool MAX, bool ARG>
int launch_rows(const ReduceCall<uint16_t>& c, const HubArg& hub, hipStream_t s) {
  const int G = lanes_for<4>(c.N);
  const dim3 grid((unsigned)(((int64_t)c.M * G + 255) / 256));
#define MI_REDUCE_ROWS(GG)                                                                                                  \
  hipLaunchKernelGGL((lowp_reduce_rows_kernel<T, GG, VEC, MAX, ARG>), grid, dim3(256), 0, s, c.rowptr, c.col, c.val, c.B, \
                     c.C, c.arg, c.M, c.N, c.ldb, c.ldc, c.ldarg, c.nnz, hub)
  MI_REDUCE_FOR_LANES(G, MI_REDUCE_ROWS)
#undef MI_REDUCE_ROWS
  return mi::check_launch();
}

template <class T, bool VEC>
int launch_grad_b(const int32_t* t_rowptr, const int32_t* t_col, const int32_t* perm, const uint16_t* val, int32_t K, int32_t N,
                  const uint16_t* G, long ldg, const int32_t* arg, long ldarg, uint16_t* grad_b, long ldgb, hipStream_t s) {
  const int Gl = lanes_for<4>(N);
  const dim3 grid((unsigned)(((int64_t)K * Gl + 255) / 256));
#define MI_GRAD_B(GG)                                                                                                          \
  hipLaunchKernelGGL((lowp_reduce_grad_b_kernel<T, GG, VEC>), grid, dim3(256), 0, s, t_rowptr, t_col, perm, val, K, N, G, ldg, \
                     arg, ldarg, grad_b, ldgb)
  MI_REDUCE_FOR_LANES(Gl, MI_GRAD_B)
#undef MI_GRAD_B
  return mi::check_launch();
}

template <class T>
struct Forms<Lowp<T>> {
  static constexpr bool kBf16 = std::is_same<T, Bf16>::value;

  // NULL workspace: every row is one chain (as the fp32 entry); else the split order of mi_spmm_csr_ex_T
  static int sum_or_mean(const int32_t* rowptr, const int32_t* col, const uint16_t* val, int64_t nnz, int32_t M, int32_t K,
                         int32_t N, const uint16_t* B, int64_t ldb, uint16_t* C, int64_t ldc, int reduce, void* workspace,
                         size_t workspace_bytes, hipStream_t s) {
    const int mode = workspace != nullptr ? MI_LONG_ROWS_SPLIT : MI_LONG_ROWS_NONE;
    if (reduce == MI_REDUCE_SUM)
      return (kBf16 ? mi_spmm_csr_ex_bf16 : mi_spmm_csr_ex_f16)(rowptr, col, val, nnz, M, K, N, B, ldb, C, ldc, mode, workspace,
                                                                workspace_bytes, static_cast<mi_stream_t>(s));
    return mi::spmm_lowp_mean(kBf16, rowptr, col, val, nnz, M, K, N, B, ldb, C, ldc, mode, workspace, workspace_bytes, s);
  }

  // VEC: one 8-byte access per four columns; else guarded elements
  static int form(const ReduceCall<uint16_t>& c) {
    return c.N % 4 == 0 && c.ldb % 4 == 0 && c.ldc % 4 == 0 && aligned8(c.B) && aligned8(c.C);
  }

  template <bool MAX>
  static int rows(const ReduceCall<uint16_t>& c, int vec, const HubArg& hub, hipStream_t s) {
    if (vec) return c.arg ? launch_rows<T, true, MAX, true>(c, hub, s) : launch_rows<T, true, MAX, false>(c, hub, s);
    return c.arg ? launch_rows<T, false, MAX, true>(c, hub, s) : launch_rows<T, false, MAX, false>(c, hub, s);
  }

  template <bool MAX>
  static int hub(const ReduceCall<uint16_t>& c, int vec, dim3 grid, const int* ws, int cap_e, float* part_val, int* part_arg,
                 hipStream_t s) {
    if (vec)
      hipLaunchKernelGGL((lowp_reduce_hub_kernel<T, true, MAX>), grid, dim3(1024), 0, s, c.rowptr, c.col, c.val, c.B, c.C, c.arg,
                         c.N, c.ldb, c.ldc, c.ldarg, c.nnz, ws, cap_e, part_val, part_arg);
    else
      hipLaunchKernelGGL((lowp_reduce_hub_kernel<T, false, MAX>), grid, dim3(1024), 0, s, c.rowptr, c.col, c.val, c.B, c.C, c.arg,
                         c.N, c.ldb, c.ldc, c.ldarg, c.nnz, ws, cap_e, part_val, part_arg);
    return mi::check_launch();
  }

  static int divide(const int32_t* rowptr, int32_t M, int32_t N, const uint16_t* in, int64_t ldin, uint16_t* out, int64_t ldout,
                    hipStream_t s) {
    const dim3 grid((unsigned)(((int64_t)M + 3) / 4));
    if (N % 4 == 0 && ldin % 4 == 0 && ldout % 4 == 0 && aligned8(in) && aligned8(out))
      hipLaunchKernelGGL((lowp_rows_divide_kernel<T, true>), grid, dim3(256), 0, s, rowptr, M, N, in, (long)ldin, out, (long)ldout);
    else
      hipLaunchKernelGGL((lowp_rows_divide_kernel<T, false>), grid, dim3(256), 0, s, rowptr, M, N, in, (long)ldin, out, (long)ldout);
    return mi::check_launch();
  }

  static int grad_b(const int32_t* t_rowptr, const int32_t* t_col, const int32_t* perm, const uint16_t* val, int32_t K, int32_t N,
                    const uint16_t* G, long ldg, const int32_t* arg, long ldarg, uint16_t* grad_b, long ldgb, hipStream_t s) {
    if (N % 4 == 0 && ldgb % 4 == 0 && aligned8(grad_b))
      return launch_grad_b<T, true>(t_rowptr, t_col, perm, val, K, N, G, ldg, arg, ldarg, grad_b, ldgb, s);
    return launch_grad_b<T, false>(t_rowptr, t_col, perm, val, K, N, G, ldg, arg, ldarg, grad_b, ldgb, s);
  }
};

}  // namespace

extern "C" {

int mi_spmm_csr_reduce_bf16(const int32_t* rowptr, const int32_t* col, const uint16_t* val, int64_t nnz, int32_t M, int32_t K,
                            int32_t N, const uint16_t* B, int64_t ldb, uint16_t* C, int64_t ldc, int32_t* arg, int64_t ldarg,
                            int reduce, void* workspace, size_t workspace_bytes, mi_stream_t stream) {
  return reduce_entry<Lowp<Bf16>>(rowptr, col, val, nnz, M, K, N, B, ldb, C, ldc, arg, ldarg, reduce, workspace, workspace_bytes,
                                  stream);
}

int mi_spmm_csr_reduce_f16(const int32_t* rowptr, const int32_t* col, const uint16_t* val, int64_t nnz, int32_t M, int32_t K,
                           int32_t N, const uint16_t* B, int64_t ldb, uint16_t* C, int64_t ldc, int32_t* arg, int64_t ldarg,
                           int reduce, void* workspace, size_t workspace_bytes, mi_stream_t stream) {
  return reduce_entry<Lowp<F16>>(rowptr, col, val, nnz, M, K, N, B, ldb, C, ldc, arg, ldarg, reduce, workspace, workspace_bytes,
                                 stream);
}

int mi_spmm_rows_divide_bf16(const int32_t* rowptr, int32_t M, int32_t N, const uint16_t* in, int64_t ldin, uint16_t* out,
                             int64_t ldout, mi_stream_t stream) {
  return divide_entry<Lowp<Bf16>>(rowptr, M, N, in, ldin, out, ldout, stream);
}

int mi_spmm_rows_divide_f16(const int32_t* rowptr, int32_t M, int32_t N, const uint16_t* in, int64_t ldin, uint16_t* out,
                            int64_t ldout, mi_stream_t stream) {
  return divide_entry<Lowp<F16>>(rowptr, M, N, in, ldin, out, ldout, stream);
}

int mi_spmm_reduce_grad_val_bf16(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t M, int32_t K, int32_t N,
                                 const uint16_t* B, int64_t ldb, const uint16_t* G, int64_t ldg, const int32_t* arg,
                                 int64_t ldarg, uint16_t* grad_val, mi_stream_t stream) {
  return grad_val_entry<Lowp<Bf16>>(rowptr, col, nnz, M, K, N, B, ldb, G, ldg, arg, ldarg, grad_val, stream);
}

int mi_spmm_reduce_grad_val_f16(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t M, int32_t K, int32_t N,
                                const uint16_t* B, int64_t ldb, const uint16_t* G, int64_t ldg, const int32_t* arg,
                                int64_t ldarg, uint16_t* grad_val, mi_stream_t stream) {
  return grad_val_entry<Lowp<F16>>(rowptr, col, nnz, M, K, N, B, ldb, G, ldg, arg, ldarg, grad_val, stream);
}

int mi_spmm_reduce_grad_b_bf16(const int32_t* t_rowptr, const int32_t* t_col, const int32_t* perm, const uint16_t* val,
                               int64_t nnz, int32_t M, int32_t K, int32_t N, const uint16_t* G, int64_t ldg, const int32_t* arg,
                               int64_t ldarg, uint16_t* grad_b, int64_t ldgb, mi_stream_t stream) {
  return grad_b_entry<Lowp<Bf16>>(t_rowptr, t_col, perm, val, nnz, M, K, N, G, ldg, arg, ldarg, grad_b, ldgb, stream);
}

int mi_spmm_reduce_grad_b_f16(const int32_t* t_rowptr, const int32_t* t_col, const int32_t* perm, const uint16_t* val,
                              int64_t nnz, int32_t M, int32_t K, int32_t N, const uint16_t* G, int64_t ldg, const int32_t* arg,
                              int64_t ldarg, uint16_t* grad_b, int64_t ldgb, mi_stream_t stream) {
  return grad_b_entry<Lowp<F16>>(t_rowptr, t_col, perm, val, nnz, M, K, N, G, ldg, arg, ldarg, grad_b, ldgb, stream);
}

}  // extern "C"
