// The amax / amin / mean reductions of the CSR product, everything their two translation units share.  csr_reduce.hip
// instantiates it for Fp32, csr_reduce_lowp.hip for Lowp<Bf16> / Lowp<F16> (lowp_device.h's element scheme: E::S, E::up,
// E::down); two units because the build compiles units in parallel.  Here:
//  * the selection steps (scan, pick), the hub-row list and its workspace layout (one layout, fp32 / int32 partials, for
//    every dtype);
//  * the kernels that differ only in the element type: reduce_hub_combine_kernel<E, MAX>, reduce_grad_val_kernel<E, TT>;
//  * the host side, once: the argument checks of the four entries per dtype in one order (reduce_entry, divide_entry,
//    grad_val_entry, grad_b_entry), launch_reduce, and the two launch ladders.
// A unit keeps what depends on its access form — shifted quads W = 4 / 1 in fp32, VEC or guarded 2-byte elements in
// bf16 / fp16 — the rows, hub, divide and grad_B kernels, and hands their launches over as Forms<E>.
// Not installed.  Everything here has internal linkage (an anonymous namespace per including unit).
#ifndef MI_CSR_REDUCE_DEVICE_H_
#define MI_CSR_REDUCE_DEVICE_H_

#include "lowp_device.h"
#include "mi_common.h"

namespace {

constexpr int kHubRow = 8192;     // rows with more entries are split when the caller gave a workspace
constexpr int kHubChunk = 16384;  // entries per workgroup of a split row (S = max(1, len / kHubChunk))
constexpr int kHubWaves = 16;
constexpr int kU = 8;             // gathers in flight per lane

// four columns of a lane at any 4-byte alignment (fp32: a shifted quad; arg: a row of any leading dimension)
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
typedef int i32x4u __attribute__((ext_vector_type(4), aligned(4)));

// One step of the sequential scan.
template <bool MAX>
__device__ __forceinline__ void scan(float p, int e, float& cur, int& arg) {
  const bool take = (MAX ? p > cur : p < cur) || __builtin_isnan(p);
  cur = take ? p : cur;
  arg = take ? e : arg;
}

// (cur, arg) ← the selection over the union of two scans of disjoint entry sets (order-independent).
template <bool MAX>
__device__ __forceinline__ void pick(float v, int a, float& cur, int& arg) {
  const bool vn = __builtin_isnan(v), cn = __builtin_isnan(cur);
  const bool take = vn ? (!cn || a > arg) : (!cn && ((MAX ? v > cur : v < cur) || (v == cur && a < arg)));
  cur = take ? v : cur;
  arg = take ? a : arg;
}

template <bool MAX>
__device__ __forceinline__ float scan_start() {
  return MAX ? -__builtin_inff() : __builtin_inff();
}

// Workspace (ints): [0] rows listed, [1] chunk slots handed out, [2] partial rows handed out, [3] –; cap_e entries of
// {row, slot base, S, partial base}; cap_s slot → entry; then (16-B aligned) cap_p × N floats and cap_p × N ints.
struct HubArg {
  int* ws;  // nullptr: no row is split
  int cap_e, cap_s, cap_p;
};

__device__ __forceinline__ void hub_append(const HubArg& h, int row, int len) {
  int* ws = h.ws;
  const int S = len / kHubChunk < 1 ? 1 : len / kHubChunk;
  const int e = atomicAdd(&ws[0], 1);
  const int sb = atomicAdd(&ws[1], S);
  const int pb = S > 1 ? atomicAdd(&ws[2], S) : 0;
  // the caps hold for any rowptr consistent with nnz; a lying rowptr must not write out of bounds
  if (e >= h.cap_e) return;
  const bool fits = sb + S <= h.cap_s && (S <= 1 || pb + S <= h.cap_p);
  int* ent = ws + 4 + 4 * (long)e;
  ent[0] = row;
  ent[1] = sb;
  ent[2] = fits ? S : 0;
  ent[3] = pb;
  if (!fits) return;
  int* owner = ws + 4 + 4 * (long)h.cap_e;
  for (int g = 0; g < S; ++g) owner[sb + g] = e;
}

// The S > 1 rows: partials g = 0 … S−1 combined per column in order (the order does not matter: `pick` is exact), narrowed
// once.  grid = (cap_e, ⌈N / 256⌉), block = 256.
template <class E, bool MAX>
__global__ __launch_bounds__(256) void reduce_hub_combine_kernel(typename E::S* __restrict__ C, int* __restrict__ argout, int N,
                                                                 long ldc, long ldarg, const int* __restrict__ ws,
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
  C[(long)row * ldc + j] = E::down(cur);
  if (argout) argout[(long)row * ldarg + j] = arg;
}

// ---------------------------------------------------------------------------
// grad_val[e] = down(Σ_j [arg[i, j] == e] · g[i, j] · B[col[e], j]) for the entries e of row i.  One wave per row; lane l
// keeps columns 64t + l of the row's arg and (widened) g in registers (TT chunks; TT = 0: N > 1024, read per entry from
// the caches).  Per entry, a B load only where arg == e, an fmaf chain over t ascending, a xor tree (32 … 1) across the
// wave, one rounding at the store.  No float atomics.  block = 256 (4 rows).
// ---------------------------------------------------------------------------
template <class E, int TT>
__global__ __launch_bounds__(256) void reduce_grad_val_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                              int M, int N, const typename E::S* __restrict__ B, long ldb,
                                                              const typename E::S* __restrict__ G, long ldg,
                                                              const int* __restrict__ argin, long ldarg,
                                                              typename E::S* __restrict__ grad_val) {
  const long row = __builtin_amdgcn_readfirstlane((int)(((long)blockIdx.x * 256 + threadIdx.x) >> 6));
  if (row >= M) return;
  const int lane = threadIdx.x & 63;
  const int p0 = rowptr[row], end = rowptr[row + 1];
  const typename E::S* Gr = G + row * ldg;
  const int* Ar = argin + row * ldarg;
  constexpr int TR = TT > 0 ? TT : 1;
  float gk[TR];
  int ak[TR];
  if constexpr (TT > 0) {
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      const int j = 64 * t + lane;
      ak[t] = j < N ? Ar[j] : -1;
      gk[t] = j < N ? E::up(Gr[j]) : 0.f;
    }
  }
  for (int e = p0; e < end; ++e) {
    const typename E::S* Bc = B + (long)col[e] * ldb;
    float acc = 0.f;
    if constexpr (TT > 0) {
#pragma unroll
      for (int t = 0; t < TT; ++t)
        if (ak[t] == e) acc = __builtin_fmaf(gk[t], E::up(Bc[64 * t + lane]), acc);
    } else {
      for (int j = lane; j < N; j += 64)
        if (Ar[j] == e) acc = __builtin_fmaf(E::up(Gr[j]), E::up(Bc[j]), acc);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if (lane == 0) grad_val[e] = E::down(acc);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct HubWs {
  long cap_e, cap_s, cap_p;
  size_t part_val_off, part_arg_off, bytes;
};
inline HubWs hub_ws_layout(int64_t nnz, int32_t N) {
  HubWs w;
  w.cap_e = nnz / kHubRow + 1;
  w.cap_p = nnz / kHubChunk;
  w.cap_s = w.cap_e + w.cap_p;
  const size_t ints = 4 + 4 * (size_t)w.cap_e + (size_t)w.cap_s;
  w.part_val_off = (ints * sizeof(int) + 15) / 16 * 16;
  w.part_arg_off = w.part_val_off + (size_t)w.cap_p * (size_t)N * sizeof(float);
  w.bytes = w.part_arg_off + (size_t)w.cap_p * (size_t)N * sizeof(int);
  return w;
}

// lanes per row for a width: a power of two with G·W ≥ N, at most a wave
template <int W>
inline int lanes_for(int32_t N) {
  const int need = (N + W - 1) / W;
  return need >= 64 ? 64 : mi::pow2_ceil(need);
}

inline bool grid_fits(int64_t rows, int lanes) { return (rows * lanes + 255) / 256 <= 0x7fffffffLL; }

// The two launch ladders: LAUNCH(v) launches the instantiation for the compile-time v.
#define MI_REDUCE_FOR_LANES(G, LAUNCH) /* lanes per row: lanes_for's values */ \
  switch (G) {                                                                \
    case 1: LAUNCH(1); break;                                                 \
    case 2: LAUNCH(2); break;                                                 \
    case 4: LAUNCH(4); break;                                                 \
    case 8: LAUNCH(8); break;                                                 \
    case 16: LAUNCH(16); break;                                               \
    case 32: LAUNCH(32); break;                                               \
    case 64: LAUNCH(64); break;                                               \
    default: return MI_EINVAL;                                                \
  }
#define MI_REDUCE_FOR_CHUNKS(TT, LAUNCH) /* register chunks of 64 columns; 0: none */ \
  switch (TT) {                                                                      \
    case 0: LAUNCH(0); break;                                                        \
    case 1: LAUNCH(1); break;                                                        \
    case 2: LAUNCH(2); break;                                                        \
    case 4: LAUNCH(4); break;                                                        \
    case 8: LAUNCH(8); break;                                                        \
    case 16: LAUNCH(16); break;                                                      \
  }

// The operands of one amax / amin product, as the rows and hub kernels take them.
template <class S>
struct ReduceCall {
  const int32_t *rowptr, *col;
  const S *val, *B;
  S* C;
  int32_t* arg;
  int32_t M, N;
  long ldb, ldc, ldarg;
  int nnz;
};

// What a unit hands over for its element type: the launches that depend on its access form, and the sum / mean routes
// (different calls per dtype).  Every member returns an MI_* status and is called with checked arguments.
//   static int sum_or_mean(rowptr, col, val, nnz, M, K, N, B, ldb, C, ldc, reduce, workspace, workspace_bytes, s);
//   static int form(const ReduceCall<S>&);              the access form of a call (fp32: W; 16-bit: VEC), chosen once
//   template <bool MAX> static int rows(const ReduceCall<S>&, form, const HubArg&, s);                      the rows kernel
//   template <bool MAX> static int hub(const ReduceCall<S>&, form, grid, ws, cap_e, part_val, part_arg, s);   the hub kernel
//   static int divide(rowptr, M, N, in, ldin, out, ldout, s);
//   static int grad_b(t_rowptr, t_col, perm, val, K, N, G, ldg, arg, ldarg, grad_b, ldgb, s);
template <class E>
struct Forms;

template <class E, bool MAX>
int launch_reduce(const ReduceCall<typename E::S>& c, void* workspace, hipStream_t s) {
  HubArg hub = {nullptr, 0, 0, 0};
  const HubWs hw = hub_ws_layout(c.nnz, c.N);
  const bool split = workspace != nullptr && c.nnz > kHubRow;
  int* ws = static_cast<int*>(workspace);
  if (split) {
    MI_HIP_TRY(hipMemsetAsync(ws, 0, 16, s));
    hub = {ws, (int)hw.cap_e, (int)hw.cap_s, (int)hw.cap_p};
  }
  const int form = Forms<E>::form(c);
  int st = Forms<E>::template rows<MAX>(c, form, hub, s);
  if (st != MI_OK || !split) return st;
  float* part_val = reinterpret_cast<float*>(static_cast<char*>(workspace) + hw.part_val_off);
  int* part_arg = reinterpret_cast<int*>(static_cast<char*>(workspace) + hw.part_arg_off);
  const unsigned blocks = (unsigned)((c.N + 255) / 256);  // 256 columns per workgroup in the hub and the combine kernel
  st = Forms<E>::template hub<MAX>(c, form, dim3((unsigned)hw.cap_s, blocks), ws, (int)hw.cap_e, part_val, part_arg, s);
  if (st != MI_OK) return st;
  hipLaunchKernelGGL((reduce_hub_combine_kernel<E, MAX>), dim3((unsigned)hw.cap_e, blocks), dim3(256), 0, s, c.C, c.arg, c.N,
                     c.ldc, c.ldarg, ws, part_val, part_arg);
  return mi::check_launch();
}

// The four entries: every check before the first HIP call, in one order for every dtype; the `extern "C"` functions of the
// units are wrappers around these.
template <class E>
int reduce_entry(const int32_t* rowptr, const int32_t* col, const typename E::S* val, int64_t nnz, int32_t M, int32_t K,
                 int32_t N, const typename E::S* B, int64_t ldb, typename E::S* C, int64_t ldc, int32_t* arg, int64_t ldarg,
                 int reduce, void* workspace, size_t workspace_bytes, mi_stream_t stream) {
  using S = typename E::S;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (reduce < MI_REDUCE_SUM || reduce > MI_REDUCE_AMIN) return MI_EINVAL;
  const bool selects = reduce == MI_REDUCE_AMAX || reduce == MI_REDUCE_AMIN;
  if (arg != nullptr && !selects) return MI_EINVAL;
  if (M < 0 || K < 0 || N < 0 || nnz < 0) return MI_EINVAL;
  if (nnz > 0x7fffffffLL) return MI_ERANGE;
  if (M == 0 || N == 0) return MI_OK;
  if (!rowptr || !C || (nnz > 0 && (!col || !val || !B))) return MI_EINVAL;
  if (ldb < N || ldc < N || (arg != nullptr && ldarg < N)) return MI_EINVAL;
  if (sizeof(S) == 2 && (odd(val) || odd(B) || odd(C))) return MI_EINVAL;
  if (!selects)
    return Forms<E>::sum_or_mean(rowptr, col, val, nnz, M, K, N, B, ldb, C, ldc, reduce, workspace, workspace_bytes, s);
  if (workspace != nullptr && nnz > kHubRow) {
    if (workspace_bytes < hub_ws_layout(nnz, N).bytes) return MI_ENOMEM;
    if (!mi::aligned16(workspace)) return MI_EINVAL;
  }
  if (!grid_fits(M, 64)) return MI_ERANGE;
  const ReduceCall<S> c = {rowptr, col, val, B, C, arg, M, N, (long)ldb, (long)ldc, (long)ldarg, (int)nnz};
  return reduce == MI_REDUCE_AMAX ? launch_reduce<E, true>(c, workspace, s) : launch_reduce<E, false>(c, workspace, s);
}

template <class E>
int divide_entry(const int32_t* rowptr, int32_t M, int32_t N, const typename E::S* in, int64_t ldin, typename E::S* out,
                 int64_t ldout, mi_stream_t stream) {
  if (M < 0 || N < 0) return MI_EINVAL;
  if (M == 0 || N == 0) return MI_OK;
  if (!rowptr || !in || !out || ldin < N || ldout < N) return MI_EINVAL;
  if (sizeof(typename E::S) == 2 && (odd(in) || odd(out))) return MI_EINVAL;
  return Forms<E>::divide(rowptr, M, N, in, ldin, out, ldout, static_cast<hipStream_t>(stream));
}

template <class E>
int grad_val_entry(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t M, int32_t K, int32_t N,
                   const typename E::S* B, int64_t ldb, const typename E::S* G, int64_t ldg, const int32_t* arg, int64_t ldarg,
                   typename E::S* grad_val, mi_stream_t stream) {
  if (M < 0 || K < 0 || N < 0 || nnz < 0) return MI_EINVAL;
  if (nnz > 0x7fffffffLL) return MI_ERANGE;
  if (M == 0 || nnz == 0) return MI_OK;
  if (!rowptr || !col || !grad_val || (N > 0 && (!B || !G || !arg))) return MI_EINVAL;
  if (ldb < N || ldg < N || ldarg < N) return MI_EINVAL;
  if (sizeof(typename E::S) == 2 && (odd(B) || odd(G) || odd(grad_val))) return MI_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)(((int64_t)M + 3) / 4));
  const int TT = N <= 64 ? 1 : N <= 128 ? 2 : N <= 256 ? 4 : N <= 512 ? 8 : N <= 1024 ? 16 : 0;
#define MI_GRAD_VAL(TT_)                                                                                                    \
  hipLaunchKernelGGL((reduce_grad_val_kernel<E, TT_>), grid, dim3(256), 0, s, rowptr, col, M, N, B, (long)ldb, G, (long)ldg, \
                     arg, (long)ldarg, grad_val)
  MI_REDUCE_FOR_CHUNKS(TT, MI_GRAD_VAL)
#undef MI_GRAD_VAL
  return mi::check_launch();
}

template <class E>
int grad_b_entry(const int32_t* t_rowptr, const int32_t* t_col, const int32_t* perm, const typename E::S* val, int64_t nnz,
                 int32_t M, int32_t K, int32_t N, const typename E::S* G, int64_t ldg, const int32_t* arg, int64_t ldarg,
                 typename E::S* grad_b, int64_t ldgb, mi_stream_t stream) {
  if (M < 0 || K < 0 || N < 0 || nnz < 0) return MI_EINVAL;
  if (nnz > 0x7fffffffLL) return MI_ERANGE;
  if (K == 0 || N == 0) return MI_OK;
  if (!t_rowptr || !grad_b || (nnz > 0 && (!t_col || !perm || !val || !G || !arg))) return MI_EINVAL;
  if (ldg < N || ldarg < N || ldgb < N) return MI_EINVAL;
  if (sizeof(typename E::S) == 2 && (odd(val) || odd(G) || odd(grad_b))) return MI_EINVAL;
  if (!grid_fits(K, 64)) return MI_ERANGE;  // (the 16-bit entries' check; true for every int32 K: DESIGN.md §3.26)
  return Forms<E>::grad_b(t_rowptr, t_col, perm, val, K, N, G, (long)ldg, arg, (long)ldarg, grad_b, (long)ldgb,
                          static_cast<hipStream_t>(stream));
}

}  // namespace

#endif  // MI_CSR_REDUCE_DEVICE_H_
