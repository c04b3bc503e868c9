// Fused sparse attention on a CSR pattern — out = softmax(scale · q·kᵀ on the pattern) · v — and its row-side backward,
// gfx950.  Contract: include/mi_spmm.h, "Fused sparse attention"; design: DESIGN.md §3.13.
//
// ONE launch forward, ONE backward; a 64-lane wave owns a row (four rows per workgroup, no workgroup barrier), and every
// stage of the row keeps the order of the kernel it replaces, so the bits are those of the three-kernel composition
// (mi_sddmm_csr_T → mi_csr_softmax_T → mi_spmm_csr_T and their backward entries):
//   scores   G = pow2_ceil(D / 4) lanes per entry, 64 / G entries per step.  Lane l of a group chains columns 4l … 4l + 3
//            with fmaf from +0 (the chain of lane l of the SDDMM's wave; D ≤ 256: one pass), lanes without columns hold +0,
//            and the group's xor tree G/2 … 1 is the tail of the SDDMM's tree 32 … 1.  The levels 32 … G of that tree only
//            meet lanes without columns: they add +0, which changes a chain in exactly one case (−0, a chain of products
//            that all underflowed, becomes +0) — `+ 0.0f` per skipped level restates it (sddmm_group_kernel does the same).
//            T: the sum is narrowed (rne) and widened again, as the composition stores it.
//   softmax  t_p = fl(scale · s_p) into the wave's LDS slice; the maximum; e_p = exp_shifted(t_p, m); lane c of the wave
//            IS chain c (entries p ≡ c mod 64 in increasing p, from +0), then the xor tree 32 … 1; y_p = fl(e_p · fl(1 / s)),
//            narrowed and widened for T.
//   product  lane j owns output columns j and j + 64: one fmaf chain from +0 over the row's entries in CSR order — the
//            plain chain of mi_spmm_csr_f32 for every row length (the 2-d composition splits rows beyond
//            mi_spmm_long_row_threshold() = 8192 entries; this kernel never does).  Columns and weights travel from a
//            register of 64 entries by readlane; eight gathers of a 4·D-byte row in flight.
//   backward recomputes t_p from q and k and y_p from the row's saved (m, 1/s) — the same expressions, the same bits —,
//            dP_p in the SDDMM order on (dO row, v rows), d by the softmax-backward chains fmaf(dP_p, y_p, ·) and their
//            tree, dS_p = fl(scale · fl(y_p · fl(dP_p − d))), and dq as the CSR-order chain of dS_p · k[col_p, :].  y and dS
//            leave in T in CSR order for the two column-side products (which need the transposed pattern).
// Row lengths: a row of at most kFwdEntries (backward: kBwdEntries) entries is computed once, its values in the wave's
// LDS slice (8 KiB per wave, 32 KiB per workgroup: five workgroups per CU beside 160 KiB of LDS).  A longer row is
// streamed by the same wave in chunks of the slice with recomputation: forward three score passes (maximum, sum,
// product), backward two (d, then dS and dq).  Any length in the one launch; nothing is read back.
// No atomics, no host synchronisation: graph-capturable; the same bits on every run, whatever the neighbours or the batch.
#include "lowp_device.h"

#pragma clang fp contract(off)

#include "csr_softmax_device.h"

namespace {

constexpr int kBlock = 256;         // threads of a workgroup: four independent waves
constexpr int kFwdEntries = 2048;   // floats of a wave's LDS slice, forward (t → e → y)
constexpr int kBwdEntries = 1024;   // backward: two arrays of that many (y, dP → dS); both multiples of 64

// element access of a dense operand: four consecutive columns (16 B / 8 B, aligned), one column, one store; round(f) is
// the value the composition hands from one stage to the next (T: narrowed once, widened exactly)
template <class E>
struct Row;
template <>
struct Row<Fp32> {
  static __device__ __forceinline__ f32x4 quad(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
  static __device__ __forceinline__ float one(const float* p) { return *p; }
  static __device__ __forceinline__ void store(float* p, float v) { *p = v; }
  static __device__ __forceinline__ float round(float f) { return f; }
};
template <class T>
struct Row<Lowp<T>> {
  static __device__ __forceinline__ f32x4 quad(const unsigned short* p) { return load4<T, true>(p, 0, 0); }
  static __device__ __forceinline__ float one(const unsigned short* p) { return up<T>(*p); }
  static __device__ __forceinline__ void store(unsigned short* p, float v) { *p = T::down(v); }
  static __device__ __forceinline__ float round(float f) { return up<T>(T::down(f)); }
};

// LDS written by some lanes of the wave is read by others
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float dot4(f32x4 x, f32x4 y) {
  float acc = 0.f;
  acc = __builtin_fmaf(x.x, y.x, acc);
  acc = __builtin_fmaf(x.y, y.y, acc);
  acc = __builtin_fmaf(x.z, y.z, acc);
  acc = __builtin_fmaf(x.w, y.w, acc);
  return acc;
}

// the SDDMM sum of one entry from the group's partial chains (see the head of the file)
template <int G>
__device__ __forceinline__ float sddmm_tree(float acc) {
#pragma unroll
  for (int w = 32; w >= G; w >>= 1) acc = acc + 0.0f;  // the tree levels whose partner never had columns
  return tree_sum<G>(acc);
}

// The chunk's entries [0, n) (columns colp[0 … n)): t[p] = fl(scale · s_p), s_p = ⟨x, k[col_p, :]⟩ in the SDDMM order,
// and (BWD) dp[p] = ⟨g, v[col_p, :]⟩ likewise.  x, g: this lane's four columns of the q and dO rows (`on`: it has some).
template <class E, int G, bool BWD>
__device__ __forceinline__ void fill_chunk(const int* __restrict__ colp, int n, f32x4 x, f32x4 g, bool on, int lane,
                                           const typename E::S* __restrict__ kitem, long ldk,
                                           const typename E::S* __restrict__ vitem, long ldv, float scale, float* t,
                                           float* dp) {
  constexpr int EPS = 64 / G;        // entries per step
  constexpr int U = G < 4 ? G : 4;   // steps whose gathers are issued together
  const int gl = lane & (G - 1), sub = lane / G;
  const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int b0 = 0; b0 < n; b0 += 64) {
    const int cnt = n - b0 < 64 ? n - b0 : 64;       // wave-uniform
    const int mycol = lane < cnt ? colp[b0 + lane] : 0;  // past the end: row 0 (its sums are never stored)
    for (int i0 = 0; i0 < G && i0 * EPS < cnt; i0 += U) {
      f32x4 yk[U], yv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long c = __shfl(mycol, (i0 + u) * EPS + sub, 64);
        yk[u] = on ? Row<E>::quad(kitem + c * ldk + 4 * gl) : zero;
        if (BWD) yv[u] = on ? Row<E>::quad(vitem + c * ldv + 4 * gl) : zero;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int e = (i0 + u) * EPS + sub;
        const float s = sddmm_tree<G>(on ? dot4(x, yk[u]) : 0.f);
        float d = 0.f;
        if (BWD) d = sddmm_tree<G>(on ? dot4(g, yv[u]) : 0.f);
        if (gl == 0 && e < cnt) {
          t[b0 + e] = __fmul_rn(scale, Row<E>::round(s));
          if (BWD) dp[b0 + e] = Row<E>::round(d);
        }
      }
    }
  }
}

// acc_j ← fmaf(w[p], b[col_p, j], acc_j) over the chunk's entries in order; lane j owns columns j and j + 64
template <class E>
__device__ __forceinline__ void chain_chunk(const int* __restrict__ colp, int n, const float* w,
                                            const typename E::S* __restrict__ bitem, long ldb, int D, int lane, float& a0,
                                            float& a1) {
  const bool on0 = lane < D, on1 = lane + 64 < D;
  for (int b0 = 0; b0 < n; b0 += 64) {
    const int cnt = n - b0 < 64 ? n - b0 : 64;
    const int mycol = lane < cnt ? colp[b0 + lane] : 0;
    const int myw = __float_as_int(lane < cnt ? w[b0 + lane] : 0.f);
#pragma unroll
    for (int i = 0; i < 64; i += 8) {
      if (i < cnt) {
        float x0[8], x1[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const typename E::S* src = bitem + (long)__builtin_amdgcn_readlane(mycol, i + u) * ldb + lane;
          x0[u] = on0 ? Row<E>::one(src) : 0.f;
          x1[u] = on1 ? Row<E>::one(src + 64) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          if (i + u < cnt) {
            const float wv = __int_as_float(__builtin_amdgcn_readlane(myw, i + u));
            a0 = __builtin_fmaf(wv, x0[u], a0);
            a1 = __builtin_fmaf(wv, x1[u], a1);
          }
        }
      }
    }
  }
}

template <class E>
struct Dense {  // a dense operand of the batch: row r of item i at p + i·stride + r·ld
  typename E::S* p;
  long ld, stride;
};

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <class E, int G>
__global__ __launch_bounds__(kBlock) void attention_fwd_kernel(const int32_t* __restrict__ rowptr,
                                                               const int32_t* __restrict__ col, int M, long rows, int D,
                                                               Dense<E> q, Dense<E> k, Dense<E> v, float scale,
                                                               Dense<E> out, float* __restrict__ stats) {
  __shared__ float lds[kBlock / 64][kFwdEntries];
  const unsigned z = (unsigned)(M >> 31);  // 0 (M ≥ 1), opaque to the compiler: see Lowp::down
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, gl = lane & (G - 1);
  const long g = (long)blockIdx.x * (kBlock / 64) + wave;
  if (g >= rows) return;
  const long item = g / M, r = g - item * M;
  int start, L;
  row_span(rowptr, g, M, rows, start, L);
  typename E::S* orow = out.p + item * out.stride + r * out.ld;
  if (L == 0) {  // an empty row: a zero row (the product's chain never starts)
    if (lane < D) Row<E>::store(orow + lane, 0.f);
    if (lane + 64 < D) Row<E>::store(orow + lane + 64, 0.f);
    if (stats != nullptr && lane < 2) stats[2 * g + lane] = 0.f;
    return;
  }
  float* t = lds[wave];
  const bool on = 4 * gl < D;
  const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4 x = on ? Row<E>::quad(q.p + item * q.stride + r * q.ld + 4 * gl) : zero;
  const typename E::S* kitem = k.p + item * k.stride;
  const typename E::S* vitem = v.p + item * v.stride;
  const int* colr = col + start;
  const bool once = L <= kFwdEntries;
  auto fill = [&](int c0, int n) {
    fill_chunk<E, G, false>(colr + c0, n, x, zero, on, lane, kitem, k.ld, nullptr, 0, scale, t, nullptr);
    wave_sync();
  };
  if (once) fill(0, L);
  float m = -__builtin_inff();
  for (int c0 = 0; c0 < L; c0 += kFwdEntries) {
    const int n = min(kFwdEntries, L - c0);
    if (!once) fill(c0, n);
    for (int p = lane; p < n; p += 64) m = __builtin_fmaxf(m, t[p]);
    if (!once) wave_sync();
  }
  m = tree_max<64>(m);
  float acc = 0.f;  // chain `lane`: kFwdEntries % 64 == 0, so p ≡ c0 + p (mod 64)
  for (int c0 = 0; c0 < L; c0 += kFwdEntries) {
    const int n = min(kFwdEntries, L - c0);
    if (!once) fill(c0, n);
    for (int p = lane; p < n; p += 64) {
      const float e = exp_shifted(t[p], m);
      if (once) t[p] = e;
      acc = acc + e;
    }
    if (!once) wave_sync();
  }
  const float inv = 1.0f / tree_sum<64>(acc);
  if (stats != nullptr && lane == 0) {
    stats[2 * g] = m;
    stats[2 * g + 1] = inv;
  }
  float a0 = 0.f, a1 = 0.f;
  for (int c0 = 0; c0 < L; c0 += kFwdEntries) {
    const int n = min(kFwdEntries, L - c0);
    if (!once) fill(c0, n);
    for (int p = lane; p < n; p += 64) t[p] = E::up(E::down((once ? t[p] : exp_shifted(t[p], m)) * inv, z));
    wave_sync();
    chain_chunk<E>(colr + c0, n, t, vitem, v.ld, D, lane, a0, a1);
    if (!once) wave_sync();
  }
  if (lane < D) Row<E>::store(orow + lane, a0);
  if (lane + 64 < D) Row<E>::store(orow + lane + 64, a1);
}

// ---------------------------------------------------------------------------
// backward (row side): dq, and y, dS in CSR order
// ---------------------------------------------------------------------------
template <class E, int G>
__global__ __launch_bounds__(kBlock) void attention_bwd_kernel(const int32_t* __restrict__ rowptr,
                                                               const int32_t* __restrict__ col, int M, long rows, int D,
                                                               Dense<E> q, Dense<E> k, Dense<E> v, Dense<E> dout,
                                                               const float* __restrict__ stats, float scale, Dense<E> dq,
                                                               typename E::S* __restrict__ y_out,
                                                               typename E::S* __restrict__ ds_out) {
  __shared__ float lds[kBlock / 64][2][kBwdEntries];
  const unsigned z = (unsigned)(M >> 31);  // 0 (M ≥ 1), opaque to the compiler: see Lowp::down
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, gl = lane & (G - 1);
  const long g = (long)blockIdx.x * (kBlock / 64) + wave;
  if (g >= rows) return;
  const long item = g / M, r = g - item * M;
  int start, L;
  row_span(rowptr, g, M, rows, start, L);
  typename E::S* dqrow = dq.p + item * dq.stride + r * dq.ld;
  if (L == 0) {
    if (lane < D) Row<E>::store(dqrow + lane, 0.f);
    if (lane + 64 < D) Row<E>::store(dqrow + lane + 64, 0.f);
    return;
  }
  float* yb = lds[wave][0];
  float* pb = lds[wave][1];
  const bool on = 4 * gl < D;
  const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4 x = on ? Row<E>::quad(q.p + item * q.stride + r * q.ld + 4 * gl) : zero;
  const f32x4 go = on ? Row<E>::quad(dout.p + item * dout.stride + r * dout.ld + 4 * gl) : zero;
  const typename E::S* kitem = k.p + item * k.stride;
  const typename E::S* vitem = v.p + item * v.stride;
  const int* colr = col + start;
  const float m = stats[2 * g], inv = stats[2 * g + 1];
  const bool once = L <= kBwdEntries;
  // yb[p] = y_p, pb[p] = dP_p of the chunk
  auto fill = [&](int c0, int n) {
    fill_chunk<E, G, true>(colr + c0, n, x, go, on, lane, kitem, k.ld, vitem, v.ld, scale, yb, pb);
    wave_sync();
    for (int p = lane; p < n; p += 64) yb[p] = E::up(E::down(exp_shifted(yb[p], m) * inv, z));
  };
  float acc = 0.f;  // chain `lane`: kBwdEntries % 64 == 0
  for (int c0 = 0; c0 < L; c0 += kBwdEntries) {
    const int n = min(kBwdEntries, L - c0);
    fill(c0, n);
    for (int p = lane; p < n; p += 64) acc = __builtin_fmaf(pb[p], yb[p], acc);
    if (!once) wave_sync();
  }
  const float d = tree_sum<64>(acc);
  float a0 = 0.f, a1 = 0.f;
  for (int c0 = 0; c0 < L; c0 += kBwdEntries) {
    const int n = min(kBwdEntries, L - c0);
    if (!once) fill(c0, n);
    for (int p = lane; p < n; p += 64) {
      const float yv = yb[p];
      const typename E::S ds = E::down(scale * (yv * (pb[p] - d)), z);
      Row<E>::store(y_out + start + c0 + p, yv);  // (exact: yv is a T value)
      ds_out[start + c0 + p] = ds;
      pb[p] = E::up(ds);
    }
    wave_sync();
    chain_chunk<E>(colr + c0, n, pb, kitem, k.ld, D, lane, a0, a1);
    if (!once) wave_sync();
  }
  if (lane < D) Row<E>::store(dqrow + lane, a0);
  if (lane + 64 < D) Row<E>::store(dqrow + lane + 64, a1);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
constexpr int kMinD = 8, kMaxD = 128;

template <class E>
bool takes_width(int32_t D) {
  return D >= kMinD && D <= kMaxD && D % (sizeof(typename E::S) == 2 ? 8 : 4) == 0;
}

// before any HIP call; MI_OK with *work = false: nothing to do
template <class E>
int validate(int64_t nnz, int32_t batch, int32_t M, int32_t K, int32_t D, bool* work) {
  *work = false;
  if (nnz < 0 || batch < 0 || M < 0 || K < 0 || D < 0) return MI_EINVAL;
  if (nnz > 0x7fffffffLL) return MI_ERANGE;
  if ((int64_t)batch * ((int64_t)M + 1) > 0x7fffffffLL) return MI_ERANGE;
  if (!takes_width<E>(D)) return MI_EINVAL;
  if (batch == 0 || M == 0) return MI_OK;  // no rows: nothing is written
  if (nnz > 0 && K == 0) return MI_EINVAL;
  *work = true;
  return MI_OK;
}

// a dense operand the kernels can read four columns at a time: non-null, rows of at least D elements, 16-byte
// (T: 8-byte) aligned rows
template <class E>
bool dense_ok(const Dense<E>& t, int32_t D, int32_t batch) {
  constexpr uintptr_t mask = 4 * sizeof(typename E::S) - 1;
  if (t.p == nullptr || t.ld < D || (reinterpret_cast<uintptr_t>(t.p) & mask) != 0) return false;
  if ((t.ld * sizeof(typename E::S)) & mask) return false;
  return batch <= 1 || (t.stride >= 0 && ((t.stride * sizeof(typename E::S)) & mask) == 0);
}

template <class E>
Dense<E> dense(const typename E::S* p, int64_t ld, int64_t stride) {
  return Dense<E>{const_cast<typename E::S*>(p), (long)ld, (long)stride};
}

#define MI_ATTENTION_GROUPS(LAUNCH) \
  switch (mi::pow2_ceil(D / 4)) {   \
    case 2: LAUNCH(2); break;       \
    case 4: LAUNCH(4); break;       \
    case 8: LAUNCH(8); break;       \
    case 16: LAUNCH(16); break;     \
    default: LAUNCH(32); break;     \
  }

template <class E>
int forward_entry(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t batch, int32_t M, int32_t K, int32_t D,
                  Dense<E> q, Dense<E> k, Dense<E> v, float scale, Dense<E> out, float* stats, mi_stream_t stream) {
  bool work;
  const int st = validate<E>(nnz, batch, M, K, D, &work);
  if (st != MI_OK || !work) return st;
  if (!rowptr || (nnz > 0 && !col)) return MI_EINVAL;
  if (!dense_ok(q, D, batch) || !dense_ok(out, D, batch)) return MI_EINVAL;
  if (nnz > 0 && (!dense_ok(k, D, batch) || !dense_ok(v, D, batch))) return MI_EINVAL;
  const long rows = (long)batch * M;
  const dim3 grid((unsigned)((rows + kBlock / 64 - 1) / (kBlock / 64)));
  hipStream_t s = static_cast<hipStream_t>(stream);
#define MI_ATTENTION_FWD(GG) \
  hipLaunchKernelGGL((attention_fwd_kernel<E, GG>), grid, dim3(kBlock), 0, s, rowptr, col, M, rows, D, q, k, v, scale, out, stats)
  MI_ATTENTION_GROUPS(MI_ATTENTION_FWD)
#undef MI_ATTENTION_FWD
  return mi::check_launch();
}

template <class E>
int backward_entry(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t batch, int32_t M, int32_t K, int32_t D,
                   Dense<E> q, Dense<E> k, Dense<E> v, Dense<E> dout, const float* stats, float scale, Dense<E> dq,
                   typename E::S* y, typename E::S* ds, mi_stream_t stream) {
  bool work;
  const int st = validate<E>(nnz, batch, M, K, D, &work);
  if (st != MI_OK || !work) return st;
  if (!rowptr || !stats || (nnz > 0 && (!col || !y || !ds))) return MI_EINVAL;
  if (sizeof(typename E::S) == 2 && ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(ds)) & 1u)) return MI_EINVAL;
  if (!dense_ok(q, D, batch) || !dense_ok(dout, D, batch) || !dense_ok(dq, D, batch)) return MI_EINVAL;
  if (nnz > 0 && (!dense_ok(k, D, batch) || !dense_ok(v, D, batch))) return MI_EINVAL;
  const long rows = (long)batch * M;
  const dim3 grid((unsigned)((rows + kBlock / 64 - 1) / (kBlock / 64)));
  hipStream_t s = static_cast<hipStream_t>(stream);
#define MI_ATTENTION_BWD(GG)                                                                                             \
  hipLaunchKernelGGL((attention_bwd_kernel<E, GG>), grid, dim3(kBlock), 0, s, rowptr, col, M, rows, D, q, k, v, dout, stats, \
                     scale, dq, y, ds)
  MI_ATTENTION_GROUPS(MI_ATTENTION_BWD)
#undef MI_ATTENTION_BWD
  return mi::check_launch();
}

}  // namespace

extern "C" {

// every row lives in registers and LDS: no workspace
size_t mi_sparse_attention_workspace_bytes(int64_t, int32_t, int32_t, int32_t) { return 0; }

#define MI_ATTENTION_ENTRIES(SUFFIX, CT, E)                                                                                \
  int mi_sparse_attention_##SUFFIX(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t batch, int32_t M,       \
                                   int32_t K, int32_t D, const CT* q, int64_t ldq, int64_t strideQ, const CT* k,           \
                                   int64_t ldk, int64_t strideK, const CT* v, int64_t ldv, int64_t strideV, float scale,   \
                                   CT* out, int64_t ldo, int64_t strideO, float* stats, void*, size_t, mi_stream_t stream) { \
    return forward_entry<E>(rowptr, col, nnz, batch, M, K, D, dense<E>(q, ldq, strideQ), dense<E>(k, ldk, strideK),        \
                            dense<E>(v, ldv, strideV), scale, dense<E>(out, ldo, strideO), stats, stream);                 \
  }                                                                                                                        \
  int mi_sparse_attention_backward_##SUFFIX(                                                                               \
      const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t batch, int32_t M, int32_t K, int32_t D, const CT* q, \
      int64_t ldq, int64_t strideQ, const CT* k, int64_t ldk, int64_t strideK, const CT* v, int64_t ldv, int64_t strideV,  \
      const CT* dout, int64_t lddo, int64_t strideDO, const float* stats, float scale, CT* dq, int64_t lddq,               \
      int64_t strideDQ, CT* y, CT* ds, void*, size_t, mi_stream_t stream) {                                                \
    return backward_entry<E>(rowptr, col, nnz, batch, M, K, D, dense<E>(q, ldq, strideQ), dense<E>(k, ldk, strideK),       \
                             dense<E>(v, ldv, strideV), dense<E>(dout, lddo, strideDO), stats, scale,                      \
                             dense<E>(dq, lddq, strideDQ), y, ds, stream);                                                 \
  }

MI_ATTENTION_ENTRIES(f32, float, Fp32)
MI_ATTENTION_ENTRIES(bf16, uint16_t, Lowp<Bf16>)
MI_ATTENTION_ENTRIES(f16, uint16_t, Lowp<F16>)
#undef MI_ATTENTION_ENTRIES

}  // extern "C"
