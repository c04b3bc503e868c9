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
//  * lowp_reduce_hub_kernel / lowp_reduce_hub_combine_kernel: rows beyond kHubRow entries, listed by the rows kernel —
//    csr_reduce.hip's split, the (value, arg) partials fp32 / int32 in the same workspace layout.
//  * lowp_rows_divide_kernel, lowp_reduce_grad_val_kernel, lowp_reduce_grad_b_kernel: the fp32 kernels' fixed summation orders,
//    widened on load, rounded once at the store.
// No float atomics; no host read-back (graph-capturable).
#include "csr_reduce_device.h"
#include "lowp_device.h"
#include "spmm_internal.h"

namespace {

typedef int i32x4u __attribute__((ext_vector_type(4), aligned(4)));

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

// The S > 1 rows: partials g = 0 … S−1 combined per column, narrowed.  grid = (cap_e, ⌈N / 256⌉), block = 256.
template <class T, bool MAX>
__global__ __launch_bounds__(256) void lowp_reduce_hub_combine_kernel(unsigned short* __restrict__ C, int* __restrict__ argout,
                                                                      int N, long ldc, long ldarg, const int* __restrict__ ws,
                                                                      const float* __restrict__ part_val,
                                                                      const int* __restrict__ part_arg) {
  const int e = blockIdx.x;
  if (e >= __builtin_amdgcn_readfirstlane(ws[0])) return;
  const int* ent = ws + 4 + 4 * (long)e;
  const int row = ent[0], S = ent[2], pb = ent[3];
  const int j = blockIdx.y * 256 + threadIdx.x;
  if (S <= 1 || j >= N) return;
  float cur = part_val[(long)pb * N + j];
  int arg = part_arg[(long)pb * N + j];
  for (int g = 1; g < S; ++g) pick<MAX>(part_val[(long)(pb + g) * N + j], part_arg[(long)(pb + g) * N + j], cur, arg);
  C[(long)row * ldc + j] = T::down(cur);
  if (argout) argout[(long)row * ldarg + j] = arg;
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
// grad_val[e] = rne_T(Σ_j [arg[i, j] == e] · g[i, j] · B[col[e], j]): reduce_grad_val_kernel's order — lane l keeps columns
// 64t + l of the row's arg and (widened) g in registers (TT chunks; TT = 0: N > 1024, read per entry from the caches), an
// fmaf chain over t ascending, a xor tree (32 … 1) across the wave.  One wave per row, block = 256 (4 rows).
// ---------------------------------------------------------------------------
template <class T, int TT>
__global__ __launch_bounds__(256) void lowp_reduce_grad_val_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                   int M, int N, const unsigned short* __restrict__ B, long ldb,
                                                                   const unsigned short* __restrict__ G, long ldg,
                                                                   const int* __restrict__ argin, long ldarg,
                                                                   unsigned short* __restrict__ grad_val) {
  const long row = __builtin_amdgcn_readfirstlane((int)(((long)blockIdx.x * 256 + threadIdx.x) >> 6));
  if (row >= M) return;
  const int lane = threadIdx.x & 63;
  const int p0 = rowptr[row], end = rowptr[row + 1];
  const unsigned short* Gr = G + row * ldg;
  const int* Ar = argin + row * ldarg;
  constexpr int TR = TT > 0 ? TT : 1;
  float gk[TR];
  int ak[TR];
  if constexpr (TT > 0) {
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      const int j = 64 * t + lane;
      ak[t] = j < N ? Ar[j] : -1;
      gk[t] = j < N ? up<T>(Gr[j]) : 0.f;
    }
  }
  for (int e = p0; e < end; ++e) {
    const unsigned short* Bc = B + (long)col[e] * ldb;
    float acc = 0.f;
    if constexpr (TT > 0) {
#pragma unroll
      for (int t = 0; t < TT; ++t)
        if (ak[t] == e) acc = __builtin_fmaf(gk[t], up<T>(Bc[64 * t + lane]), acc);
    } else {
      for (int j = lane; j < N; j += 64)
        if (Ar[j] == e) acc = __builtin_fmaf(up<T>(Gr[j]), up<T>(Bc[j]), acc);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if (lane == 0) grad_val[e] = T::down(acc);
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
// host side
// ---------------------------------------------------------------------------
inline bool odd(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 1u) != 0; }

template <class T, bool VEC, bool MAX, bool ARG>
int launch_rows(int G, const int32_t* rowptr, const int32_t* col, const uint16_t* val, const uint16_t* B, uint16_t* C,
                int32_t* arg, int32_t M, int32_t N, int64_t ldb, int64_t ldc, int64_t ldarg, int32_t nnz, const HubArg& hub,
                hipStream_t s) {
  const dim3 grid((unsigned)(((int64_t)M * G + 255) / 256));
#define MI_REDUCE_ROWS(GG)                                                                                                   \
  case GG:                                                                                                                  \
    hipLaunchKernelGGL((lowp_reduce_rows_kernel<T, GG, VEC, MAX, ARG>), grid, dim3(256), 0, s, rowptr, col, val, B, C, arg, M, \
                       N, (long)ldb, (long)ldc, (long)ldarg, nnz, hub);                                                     \
    break;
  switch (G) {
    MI_REDUCE_ROWS(1)
    MI_REDUCE_ROWS(2)
    MI_REDUCE_ROWS(4)
    MI_REDUCE_ROWS(8)
    MI_REDUCE_ROWS(16)
    MI_REDUCE_ROWS(32)
    MI_REDUCE_ROWS(64)
    default:
      return MI_EINVAL;
  }
#undef MI_REDUCE_ROWS
  return mi::check_launch();
}

template <class T, bool VEC, bool MAX>
int launch_reduce(const int32_t* rowptr, const int32_t* col, const uint16_t* val, int64_t nnz, int32_t M, int32_t N,
                  const uint16_t* B, int64_t ldb, uint16_t* C, int64_t ldc, int32_t* arg, int64_t ldarg, void* workspace,
                  hipStream_t s) {
  HubArg hub = {nullptr, 0, 0, 0};
  const HubWs hw = hub_ws_layout(nnz, N);
  const bool split = workspace != nullptr && nnz > kHubRow;
  int* ws = static_cast<int*>(workspace);
  if (split) {
    MI_HIP_TRY(hipMemsetAsync(ws, 0, 16, s));
    hub = {ws, (int)hw.cap_e, (int)hw.cap_s, (int)hw.cap_p};
  }
  const int G = lanes_for<4>(N);
  int st = arg ? launch_rows<T, VEC, MAX, true>(G, rowptr, col, val, B, C, arg, M, N, ldb, ldc, ldarg, (int)nnz, hub, s)
               : launch_rows<T, VEC, MAX, false>(G, rowptr, col, val, B, C, arg, M, N, ldb, ldc, ldarg, (int)nnz, hub, s);
  if (st != MI_OK || !split) return st;
  float* part_val = reinterpret_cast<float*>(static_cast<char*>(workspace) + hw.part_val_off);
  int* part_arg = reinterpret_cast<int*>(static_cast<char*>(workspace) + hw.part_arg_off);
  hipLaunchKernelGGL((lowp_reduce_hub_kernel<T, VEC, MAX>), dim3((unsigned)hw.cap_s, (unsigned)((N + 255) / 256)), dim3(1024), 0,
                     s, rowptr, col, val, B, C, arg, N, (long)ldb, (long)ldc, (long)ldarg, (int)nnz, ws, (int)hw.cap_e, part_val,
                     part_arg);
  st = mi::check_launch();
  if (st != MI_OK) return st;
  hipLaunchKernelGGL((lowp_reduce_hub_combine_kernel<T, MAX>), dim3((unsigned)hw.cap_e, (unsigned)((N + 255) / 256)), dim3(256),
                     0, s, C, arg, N, (long)ldc, (long)ldarg, ws, part_val, part_arg);
  return mi::check_launch();
}

template <class T>
int reduce_lowp(bool bf16, const int32_t* rowptr, const int32_t* col, const uint16_t* val, int64_t nnz, int32_t M, int32_t K,
                int32_t N, const uint16_t* B, int64_t ldb, uint16_t* C, int64_t ldc, int32_t* arg, int64_t ldarg, int reduce,
                void* workspace, size_t workspace_bytes, hipStream_t s) {
  // every check before the first HIP call, in the order of mi_spmm_csr_reduce_f32
  if (reduce < MI_REDUCE_SUM || reduce > MI_REDUCE_AMIN) return MI_EINVAL;
  const bool selects = reduce == MI_REDUCE_AMAX || reduce == MI_REDUCE_AMIN;
  if (arg != nullptr && !selects) return MI_EINVAL;
  if (M < 0 || K < 0 || N < 0 || nnz < 0) return MI_EINVAL;
  if (nnz > 0x7fffffffLL) return MI_ERANGE;
  if (M == 0 || N == 0) return MI_OK;
  if (!rowptr || !C || (nnz > 0 && (!col || !val || !B))) return MI_EINVAL;
  if (ldb < N || ldc < N || (arg != nullptr && ldarg < N)) return MI_EINVAL;
  if (odd(val) || odd(B) || odd(C)) return MI_EINVAL;
  if (!selects) {
    // NULL workspace: every row is one chain (as the fp32 entry); else the split order of mi_spmm_csr_ex_T
    const int mode = workspace != nullptr ? MI_LONG_ROWS_SPLIT : MI_LONG_ROWS_NONE;
    if (reduce == MI_REDUCE_SUM)
      return (bf16 ? mi_spmm_csr_ex_bf16 : mi_spmm_csr_ex_f16)(rowptr, col, val, nnz, M, K, N, B, ldb, C, ldc, mode, workspace,
                                                               workspace_bytes, static_cast<mi_stream_t>(s));
    return mi::spmm_lowp_mean(bf16, rowptr, col, val, nnz, M, K, N, B, ldb, C, ldc, mode, workspace, workspace_bytes, s);
  }
  if (workspace != nullptr && nnz > kHubRow) {
    if (workspace_bytes < hub_ws_layout(nnz, N).bytes) return MI_ENOMEM;
    if (!mi::aligned16(workspace)) return MI_EINVAL;
  }
  if (!grid_fits(M, 64)) return MI_ERANGE;
  const bool vec = N % 4 == 0 && ldb % 4 == 0 && ldc % 4 == 0 && aligned8(B) && aligned8(C);
  const bool max = reduce == MI_REDUCE_AMAX;
#define MI_REDUCE_LOWP(VEC_, MAX_) \
  return launch_reduce<T, VEC_, MAX_>(rowptr, col, val, nnz, M, N, B, ldb, C, ldc, arg, ldarg, workspace, s)
  if (vec && max) MI_REDUCE_LOWP(true, true);
  if (vec) MI_REDUCE_LOWP(true, false);
  if (max) MI_REDUCE_LOWP(false, true);
  MI_REDUCE_LOWP(false, false);
#undef MI_REDUCE_LOWP
}

template <class T>
int divide_lowp(const int32_t* rowptr, int32_t M, int32_t N, const uint16_t* in, int64_t ldin, uint16_t* out, int64_t ldout,
                hipStream_t s) {
  if (M < 0 || N < 0) return MI_EINVAL;
  if (M == 0 || N == 0) return MI_OK;
  if (!rowptr || !in || !out || ldin < N || ldout < N) return MI_EINVAL;
  if (odd(in) || odd(out)) return MI_EINVAL;
  const dim3 grid((unsigned)(((int64_t)M + 3) / 4));
  if (N % 4 == 0 && ldin % 4 == 0 && ldout % 4 == 0 && aligned8(in) && aligned8(out))
    hipLaunchKernelGGL((lowp_rows_divide_kernel<T, true>), grid, dim3(256), 0, s, rowptr, M, N, in, (long)ldin, out, (long)ldout);
  else
    hipLaunchKernelGGL((lowp_rows_divide_kernel<T, false>), grid, dim3(256), 0, s, rowptr, M, N, in, (long)ldin, out, (long)ldout);
  return mi::check_launch();
}

template <class T>
int grad_val_lowp(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t M, int32_t K, int32_t N, const uint16_t* B,
                  int64_t ldb, const uint16_t* G, int64_t ldg, const int32_t* arg, int64_t ldarg, uint16_t* grad_val,
                  hipStream_t s) {
  if (M < 0 || K < 0 || N < 0 || nnz < 0) return MI_EINVAL;
  if (nnz > 0x7fffffffLL) return MI_ERANGE;
  if (M == 0 || nnz == 0) return MI_OK;
  if (!rowptr || !col || !grad_val || (N > 0 && (!B || !G || !arg))) return MI_EINVAL;
  if (ldb < N || ldg < N || ldarg < N) return MI_EINVAL;
  if (odd(B) || odd(G) || odd(grad_val)) return MI_EINVAL;
  const dim3 grid((unsigned)(((int64_t)M + 3) / 4));
  const int TT = N <= 64 ? 1 : N <= 128 ? 2 : N <= 256 ? 4 : N <= 512 ? 8 : N <= 1024 ? 16 : 0;
#define MI_GRAD_VAL(TT_)                                                                                                   \
  case TT_:                                                                                                                \
    hipLaunchKernelGGL((lowp_reduce_grad_val_kernel<T, TT_>), grid, dim3(256), 0, s, rowptr, col, M, N, B, (long)ldb, G,   \
                       (long)ldg, arg, (long)ldarg, grad_val);                                                             \
    break;
  switch (TT) {
    MI_GRAD_VAL(0)
    MI_GRAD_VAL(1)
    MI_GRAD_VAL(2)
    MI_GRAD_VAL(4)
    MI_GRAD_VAL(8)
    MI_GRAD_VAL(16)
  }
#undef MI_GRAD_VAL
  return mi::check_launch();
}

template <class T, bool VEC>
int launch_grad_b(const int32_t* t_rowptr, const int32_t* t_col, const int32_t* perm, const uint16_t* val, int32_t K, int32_t N,
                  const uint16_t* G, int64_t ldg, const int32_t* arg, int64_t ldarg, uint16_t* grad_b, int64_t ldgb,
                  hipStream_t s) {
  const int Gl = lanes_for<4>(N);
  const dim3 grid((unsigned)(((int64_t)K * Gl + 255) / 256));
#define MI_GRAD_B(GG)                                                                                                       \
  case GG:                                                                                                                  \
    hipLaunchKernelGGL((lowp_reduce_grad_b_kernel<T, GG, VEC>), grid, dim3(256), 0, s, t_rowptr, t_col, perm, val, K, N, G, \
                       (long)ldg, arg, (long)ldarg, grad_b, (long)ldgb);                                                    \
    break;
  switch (Gl) {
    MI_GRAD_B(1)
    MI_GRAD_B(2)
    MI_GRAD_B(4)
    MI_GRAD_B(8)
    MI_GRAD_B(16)
    MI_GRAD_B(32)
    MI_GRAD_B(64)
  }
#undef MI_GRAD_B
  return mi::check_launch();
}

template <class T>
int grad_b_lowp(const int32_t* t_rowptr, const int32_t* t_col, const int32_t* perm, const uint16_t* val, int64_t nnz, int32_t M,
                int32_t K, int32_t N, const uint16_t* G, int64_t ldg, const int32_t* arg, int64_t ldarg, uint16_t* grad_b,
                int64_t ldgb, hipStream_t s) {
  if (M < 0 || K < 0 || N < 0 || nnz < 0) return MI_EINVAL;
  if (nnz > 0x7fffffffLL) return MI_ERANGE;
  if (K == 0 || N == 0) return MI_OK;
  if (!t_rowptr || !grad_b || (nnz > 0 && (!t_col || !perm || !val || !G || !arg))) return MI_EINVAL;
  if (ldg < N || ldarg < N || ldgb < N) return MI_EINVAL;
  if (odd(val) || odd(G) || odd(grad_b)) return MI_EINVAL;
  if (!grid_fits(K, 64)) return MI_ERANGE;
  if (N % 4 == 0 && ldgb % 4 == 0 && aligned8(grad_b))
    return launch_grad_b<T, true>(t_rowptr, t_col, perm, val, K, N, G, ldg, arg, ldarg, grad_b, ldgb, s);
  return launch_grad_b<T, false>(t_rowptr, t_col, perm, val, K, N, G, ldg, arg, ldarg, grad_b, ldgb, s);
}

}  // namespace

extern "C" {

int mi_spmm_csr_reduce_bf16(const int32_t* rowptr, const int32_t* col, const uint16_t* val, int64_t nnz, int32_t M, int32_t K,
                            int32_t N, const uint16_t* B, int64_t ldb, uint16_t* C, int64_t ldc, int32_t* arg, int64_t ldarg,
                            int reduce, void* workspace, size_t workspace_bytes, mi_stream_t stream) {
  return reduce_lowp<Bf16>(true, rowptr, col, val, nnz, M, K, N, B, ldb, C, ldc, arg, ldarg, reduce, workspace, workspace_bytes,
                           static_cast<hipStream_t>(stream));
}

int mi_spmm_csr_reduce_f16(const int32_t* rowptr, const int32_t* col, const uint16_t* val, int64_t nnz, int32_t M, int32_t K,
                           int32_t N, const uint16_t* B, int64_t ldb, uint16_t* C, int64_t ldc, int32_t* arg, int64_t ldarg,
                           int reduce, void* workspace, size_t workspace_bytes, mi_stream_t stream) {
  return reduce_lowp<F16>(false, rowptr, col, val, nnz, M, K, N, B, ldb, C, ldc, arg, ldarg, reduce, workspace, workspace_bytes,
                          static_cast<hipStream_t>(stream));
}

int mi_spmm_rows_divide_bf16(const int32_t* rowptr, int32_t M, int32_t N, const uint16_t* in, int64_t ldin, uint16_t* out,
                             int64_t ldout, mi_stream_t stream) {
  return divide_lowp<Bf16>(rowptr, M, N, in, ldin, out, ldout, static_cast<hipStream_t>(stream));
}

int mi_spmm_rows_divide_f16(const int32_t* rowptr, int32_t M, int32_t N, const uint16_t* in, int64_t ldin, uint16_t* out,
                            int64_t ldout, mi_stream_t stream) {
  return divide_lowp<F16>(rowptr, M, N, in, ldin, out, ldout, static_cast<hipStream_t>(stream));
}

int mi_spmm_reduce_grad_val_bf16(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t M, int32_t K, int32_t N,
                                 const uint16_t* B, int64_t ldb, const uint16_t* G, int64_t ldg, const int32_t* arg,
                                 int64_t ldarg, uint16_t* grad_val, mi_stream_t stream) {
  return grad_val_lowp<Bf16>(rowptr, col, nnz, M, K, N, B, ldb, G, ldg, arg, ldarg, grad_val, static_cast<hipStream_t>(stream));
}

int mi_spmm_reduce_grad_val_f16(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t M, int32_t K, int32_t N,
                                const uint16_t* B, int64_t ldb, const uint16_t* G, int64_t ldg, const int32_t* arg,
                                int64_t ldarg, uint16_t* grad_val, mi_stream_t stream) {
  return grad_val_lowp<F16>(rowptr, col, nnz, M, K, N, B, ldb, G, ldg, arg, ldarg, grad_val, static_cast<hipStream_t>(stream));
}

int mi_spmm_reduce_grad_b_bf16(const int32_t* t_rowptr, const int32_t* t_col, const int32_t* perm, const uint16_t* val,
                               int64_t nnz, int32_t M, int32_t K, int32_t N, const uint16_t* G, int64_t ldg, const int32_t* arg,
                               int64_t ldarg, uint16_t* grad_b, int64_t ldgb, mi_stream_t stream) {
  return grad_b_lowp<Bf16>(t_rowptr, t_col, perm, val, nnz, M, K, N, G, ldg, arg, ldarg, grad_b, ldgb,
                           static_cast<hipStream_t>(stream));
}

int mi_spmm_reduce_grad_b_f16(const int32_t* t_rowptr, const int32_t* t_col, const int32_t* perm, const uint16_t* val,
                              int64_t nnz, int32_t M, int32_t K, int32_t N, const uint16_t* G, int64_t ldg, const int32_t* arg,
                              int64_t ldarg, uint16_t* grad_b, int64_t ldgb, mi_stream_t stream) {
  return grad_b_lowp<F16>(t_rowptr, t_col, perm, val, nnz, M, K, N, G, ldg, arg, ldarg, grad_b, ldgb,
                          static_cast<hipStream_t>(stream));
}

}  // extern "C"
