// Dense products in bfloat16 and float16 on the matrix cores: C[b] = op(A[b]) · op(B[b]), A, B and C all of one type
// T ∈ {bf16, fp16} (2-byte bit patterns at the C-ABI), every sum in fp32, one rounding per output element at the store.
//
// What it computes (contract of include/mi_spmm.h, mi_gemm_bf16 / _f16 — DESIGN.md §3.9):
//  * ONE instruction for the whole family: v_mfma_f32_16x16x32_{bf16,f16}.  Each output element is one accumulator,
//    started at +0 and carried through the k-steps 0–31, 32–63, … in ascending order; a ragged last step is zero-padded
//    in both operands (zeros written to LDS, nothing read past an operand).  The bits of C[i, j] therefore depend on
//    row i of op(A), column j of op(B), k and T only — never on m, n, the batch, the tile, the storage transposes or
//    which tile shape the launcher picks.
//  * The store narrows once: static_cast to __bf16 / _Float16 (v_cvt_pk_bf16_f32 / v_cvt_f16_f32: NaN stays NaN,
//    fp16 overflow becomes ±inf).  No integer rounding on the bits.
//
// Kernel: a 256-thread workgroup owns a BM × BN tile of one batch item (BM = 128; BN = 128, or 64 for narrow products
// and for grids too small to fill the chip); 4 waves in 2 × 2, each 16 × 16 MFMA tiles over a 64-deep k-tile.  Both
// operands are staged through registers into LDS images with k contiguous ([rows][kStr] elements: the padded row of
// mfma_device.h), double-buffered: the global loads of
// k-tile t + 1 are in flight while the MFMAs of tile t run, one barrier per k-tile.  An operand stored with k
// contiguous (A plain, B transposed) moves as 16-byte pieces; one stored k-strided (A transposed, B plain) is read as
// 4 k-rows × 8 elements and transposed in registers into 8-byte LDS writes.  The MFMA takes the B fragment as its first
// operand, so a lane's four results are four adjacent output COLUMNS of one row; the B rows of a fragment pair are
// interleaved so that a lane holds eight adjacent columns and stores them as one 16-byte piece.
// Alignment: the VEC form (operands 16-byte aligned, leading dimensions and item strides multiples of 8 elements, C
// likewise) uses 16-byte loads and stores wherever a piece lies inside the operand; the checked form (any 2-byte
// aligned operand, any leading dimension) reads and writes element by element.  Edges are checked in both.
// No float atomics, no host read-back: graph-capturable.
//
// Epilogues — the k-loop above is the same code for all three, so the order contract holds for each:
//  * kStore: C = rne_T(acc), the plain entries;
//  * kBias: C[i, j] = rne_T(acc + up(bias[j])) — one fp32 add of the exactly widened bias, one rounding.  A lane's eight
//    columns of bias move as one 16-byte load in the VEC form (bias 16-byte aligned), element by element otherwise;
//  * kPartial: P[s][i, j] = acc, fp32 and not narrowed, into a dense [S][m][n] workspace — the ranges of the deterministic
//    split-k below, which run as a batch of S items whose operands are the k-ranges (as gemm_splitk.hip does in fp32).
// Split-k: k cut into S equal ranges of whole 32-deep MFMA steps, each range the family order from +0; the combine kernel
// adds an element's partial sums in index order, ((P0 + P1) + P2) + …, then the bias, and rounds once.  No atomics.
//
// The element types are lowp_device.h's; the MFMA wrapper, half_of, the row stride kStr and the transposing store of a
// k-strided operand are mfma_device.h's, which the block-sparse and the attention units share.
#include "mfma_device.h"

namespace {

constexpr int kBK = kTileK;  // k per LDS tile (two MFMA k-steps)

enum Epilogue { kStore = 0, kBias = 1, kPartial = 2 };

struct GemmArgs {
  const uint16_t* A;
  const uint16_t* B;
  uint16_t* C;
  int m, n, k, batch;
  long lda, ldb, ldc, sA, sB, sC;
  int tiles_n;
  const uint16_t* bias;  // kBias: n elements
  float* P;              // kPartial: [batch][m][n] fp32 (ldc = n, sC = m·n), 16-byte aligned
};

// 8 contiguous elements p[0 … 7], of which the first `avail` exist (zeros for the rest; nothing read when avail ≤ 0).
// (bsr_device.h has this function with the last expression as a call: each unit's kernels change with the other's form, §3.24.)
template <bool VEC>
__device__ __forceinline__ uint4 load8(const uint16_t* p, int avail) {
  if (VEC && avail >= 8) return *reinterpret_cast<const uint4*>(p);
  unsigned short e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) e[j] = j < avail ? p[j] : (unsigned short)0;
  return uint4{e[0] | ((unsigned)e[1] << 16), e[2] | ((unsigned)e[3] << 16), e[4] | ((unsigned)e[5] << 16),
               e[6] | ((unsigned)e[7] << 16)};
}

// One operand's R × kBK tile (R rows of the output side, kBK values of k) in registers.
//  KC (k contiguous: element (r, k) at P[r·ld + k]): R·8 pieces of 8 k-values, R/32 per thread, 8 threads per row.
//  RC (rows contiguous: element (r, k) at P[k·ld + r]): 2R units of 4 k-rows × 8 rows, one per thread (R = 64: half the
//  threads), 4 pieces each, in the lane order of store_rc.
template <int R, bool KC>
struct Stage {
  static constexpr int kPieces = KC ? R / 32 : 4;
  uint4 v[kPieces];
};

template <int R, bool KC, bool VEC>
__device__ __forceinline__ void load_tile(Stage<R, KC>& s, const uint16_t* P, long ld, int row0, int rows, int k0, int K,
                                          int tid) {
  if constexpr (KC) {
#pragma unroll
    for (int i = 0; i < Stage<R, KC>::kPieces; ++i) {
      const int c = tid + i * 256, r = row0 + (c >> 3), kk = k0 + (c & 7) * 8;
      const int avail = r < rows ? K - kk : 0;
      s.v[i] = load8<VEC>(P + (long)r * ld + kk, avail);
    }
  } else {
    const int u = tid, r = row0 + (u >> 4) * 8, kk = k0 + (u & 15) * 4;
    const bool active = u < 2 * R;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int avail = active && kk + q < K ? rows - r : 0;
      s.v[q] = load8<VEC>(P + (long)(kk + q) * ld + r, avail);
    }
  }
}

template <int R, bool KC>
__device__ __forceinline__ void store_tile(const Stage<R, KC>& s, unsigned short* S, int tid) {
  if constexpr (KC) {
#pragma unroll
    for (int i = 0; i < Stage<R, KC>::kPieces; ++i) {
      const int c = tid + i * 256;
      *reinterpret_cast<uint4*>(S + (c >> 3) * kStr + (c & 7) * 8) = s.v[i];
    }
  } else {
    if (tid < 2 * R) store_rc(S, s.v, tid);
  }
}

template <class T, bool TA, bool TB, int BM, int BN, bool VEC, int EPI = kStore>
__global__ __launch_bounds__(256) void gemm_lowp_kernel(GemmArgs g) {
  constexpr int WM = BM / 2, WN = BN / 2, FM = WM / 16, FN = WN / 16;
  static_assert(FN % 2 == 0, "B fragments go in pairs (interleaved rows: 16-byte stores)");
  constexpr bool KCA = !TA, KCB = TB;
  __shared__ __attribute__((aligned(16))) unsigned short smem[2 * (BM + BN) * kStr];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wm = wid >> 1, wn = wid & 1;
  const int li = lane & 15, lg = lane >> 4;
  // XCD remap (bijective): consecutive tiles, which share A rows, on one XCD's L2
  const unsigned total = gridDim.x, bid = blockIdx.x, q8 = total / 8, rem = total % 8, xcd = bid % 8;
  const unsigned w = xcd * q8 + (xcd < rem ? xcd : rem) + bid / 8;
  const int m0 = (int)(w / g.tiles_n) * BM, n0 = (int)(w % g.tiles_n) * BN;
  const int nt = (g.k + kBK - 1) / kBK;
  // kBias: the lane's eight columns of bias per fragment pair, loaded once, ahead of the k-loop (nothing waits on them)
  uint4 bias8[FN / 2];
  if constexpr (EPI == kBias) {
#pragma unroll
    for (int p = 0; p < FN / 2; ++p) {
      const int c = n0 + wn * WN + p * 32 + 8 * lg;
      bias8[p] = load8<VEC>(g.bias + c, g.n - c);
    }
  }

  for (int b = blockIdx.y; b < g.batch; b += gridDim.y) {
    const uint16_t* A = g.A + (long)b * g.sA;
    const uint16_t* B = g.B + (long)b * g.sB;
    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    Stage<BM, KCA> sa;
    Stage<BN, KCB> sb;
    load_tile<BM, KCA, VEC>(sa, A, g.lda, m0, g.m, 0, g.k, tid);
    load_tile<BN, KCB, VEC>(sb, B, g.ldb, n0, g.n, 0, g.k, tid);
    store_tile<BM, KCA>(sa, smem, tid);
    store_tile<BN, KCB>(sb, smem + BM * kStr, tid);
    __syncthreads();

    for (int t = 0; t < nt; ++t) {
      const bool more = t + 1 < nt;
      if (more) {
        load_tile<BM, KCA, VEC>(sa, A, g.lda, m0, g.m, (t + 1) * kBK, g.k, tid);
        load_tile<BN, KCB, VEC>(sb, B, g.ldb, n0, g.n, (t + 1) * kBK, g.k, tid);
      }
      const unsigned short* As = smem + (t & 1) * (BM + BN) * kStr;
      const unsigned short* Bs = As + BM * kStr;
      // bsr_device.h's tile_mfma with FM rows of fragments, written out: as a call it changed all 96 instantiations (§3.24)
#pragma unroll
      for (int ks = 0; ks < kBK / 32; ++ks) {
        const int kofs = ks * 32 + 8 * lg;
        uint4 af[FM], bf[FN];
#pragma unroll
        for (int i = 0; i < FM; ++i) af[i] = *reinterpret_cast<const uint4*>(As + (wm * WM + i * 16 + li) * kStr + kofs);
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          // fragment pair j/2: row li of fragment j holds column 32(j/2) + 8(li/4) + 4(j%2) + li%4 of the wave's tile
          const int col = wn * WN + (j >> 1) * 32 + 8 * (li >> 2) + 4 * (j & 1) + (li & 3);
          bf[j] = *reinterpret_cast<const uint4*>(Bs + col * kStr + kofs);
        }
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j) acc[i][j] = mfma<T>(bf[j], af[i], acc[i][j]);
      }
      if (more) {
        unsigned short* Sn = smem + ((t + 1) & 1) * (BM + BN) * kStr;
        store_tile<BM, KCA>(sa, Sn, tid);
        store_tile<BN, KCB>(sb, Sn + BM * kStr, tid);
      }
      __syncthreads();
    }

    // store: lane (li, lg) holds row li of each 16-row fragment and columns 8·lg … 8·lg + 7 of each fragment pair
    if constexpr (EPI == kPartial) {
      float* P = g.P + (long)b * g.sC;
      const bool rows16 = (g.n & 3) == 0;  // every row of P starts on 16 bytes
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        const int r = m0 + wm * WM + i * 16 + li;
        if (r >= g.m) continue;
#pragma unroll
        for (int p = 0; p < FN; ++p) {
          const int c = n0 + wn * WN + (p >> 1) * 32 + 8 * lg + 4 * (p & 1);
          const f32x4 x = acc[i][p];
          float* dst = P + (long)r * g.n + c;
          if (rows16 && c + 4 <= g.n) {
            *reinterpret_cast<f32x4*>(dst) = x;
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (c + e < g.n) dst[e] = x[e];
          }
        }
      }
    } else {
      uint16_t* C = g.C + (long)b * g.sC;
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        const int r = m0 + wm * WM + i * 16 + li;
        if (r >= g.m) continue;
#pragma unroll
        for (int p = 0; p < FN / 2; ++p) {
          const int c = n0 + wn * WN + p * 32 + 8 * lg;
          f32x4 x = acc[i][2 * p], y = acc[i][2 * p + 1];
          if constexpr (EPI == kBias) {
            const uint4 bv = bias8[p];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              x[e] = __fadd_rn(x[e], up<T>(half_of(bv, e)));
              y[e] = __fadd_rn(y[e], up<T>(half_of(bv, 4 + e)));
            }
          }
          uint16_t* dst = C + (long)r * g.ldc + c;
          if (VEC && c + 8 <= g.n) {
            *reinterpret_cast<uint4*>(dst) =
                uint4{pack2<T>(x[0], x[1]), pack2<T>(x[2], x[3]), pack2<T>(y[0], y[1]), pack2<T>(y[2], y[3])};
          } else {
            const float v[8] = {x[0], x[1], x[2], x[3], y[0], y[1], y[2], y[3]};
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (c + e < g.n) dst[e] = T::down(v[e]);
          }
        }
      }
    }
  }
}

// k == 0: every row of C is the bias (rne_T(up(bias)) is the bias itself), zeros without one
__global__ void fill_b16_kernel(uint16_t* C, int m, int n, long ldc, long strideC, int batch, const uint16_t* bias) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)m * n) return;
  const uint16_t v = bias ? bias[idx % n] : (uint16_t)0;
  for (int b = blockIdx.y; b < batch; b += gridDim.y) C[b * strideC + (idx / n) * ldc + (idx % n)] = v;
}

// Split-k combine: C[i, j] = rne_T((((P[0] + P[1]) + P[2]) + …) + up(bias[j])), P [S][m][n] fp32.  W = 4: four adjacent
// columns per thread (n and ldc multiples of 4, C 8-byte aligned: 16-byte loads, 8-byte stores); W = 1: any layout.
template <class T, int W>
__global__ __launch_bounds__(256) void gemm_lowp_combine_kernel(const float* __restrict__ P, int S, long mn, int n,
                                                                uint16_t* __restrict__ C, long ldc,
                                                                const uint16_t* __restrict__ bias) {
  const long idx = ((long)blockIdx.x * blockDim.x + threadIdx.x) * W;
  if (idx >= mn) return;
  const long i = idx / n, j = idx - i * n;
  if constexpr (W == 4) {
    f32x4 t = *reinterpret_cast<const f32x4*>(P + idx);
    for (int s = 1; s < S; ++s) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(P + (long)s * mn + idx);
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] = __fadd_rn(t[e], v[e]);
    }
    if (bias) {
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] = __fadd_rn(t[e], up<T>(bias[j + e]));
    }
    *reinterpret_cast<uint2*>(C + i * ldc + j) = uint2{pack2<T>(t[0], t[1]), pack2<T>(t[2], t[3])};
  } else {
    float t = P[idx];
    for (int s = 1; s < S; ++s) t = __fadd_rn(t, P[(long)s * mn + idx]);
    if (bias) t = __fadd_rn(t, up<T>(bias[j]));
    C[i * ldc + j] = T::down(t);
  }
}

template <class T, bool TA, bool TB, int BM, int BN, int EPI>
int launch(const GemmArgs& g, bool vec, hipStream_t s) {
  const long tiles = (long)((g.m + BM - 1) / BM) * ((g.n + BN - 1) / BN);
  if (tiles > 0x7fffffffL) return MI_ERANGE;
  GemmArgs a = g;
  a.tiles_n = (g.n + BN - 1) / BN;
  const dim3 grid((unsigned)tiles, (unsigned)(g.batch < 65535 ? g.batch : 65535));
  if (vec)
    hipLaunchKernelGGL((gemm_lowp_kernel<T, TA, TB, BM, BN, true, EPI>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((gemm_lowp_kernel<T, TA, TB, BM, BN, false, EPI>), grid, dim3(256), 0, s, a);
  return mi::check_launch();
}

// The tile shape: 128 × 128 while that fills the chip, else 128 × 64 (and always for n ≤ 64: the attention
// context product probs·V and the like).  Same bits either way.  (The ranges of a split count as batch items here.)
// mi_gemm_lowp_tile_n is the rule, so that a caller can ask which one a shape takes.
template <class T, bool TA, bool TB, int EPI>
int pick(const GemmArgs& g, bool vec, hipStream_t s) {
  if (mi_gemm_lowp_tile_n(g.m, g.n, g.batch) == 64) return launch<T, TA, TB, 128, 64, EPI>(g, vec, s);
  return launch<T, TA, TB, 128, 128, EPI>(g, vec, s);
}

template <class T, int EPI>
int run(int transa, int transb, const GemmArgs& g, bool vec, hipStream_t s) {
  if (!transa && !transb) return pick<T, false, false, EPI>(g, vec, s);
  if (!transa && transb) return pick<T, false, true, EPI>(g, vec, s);
  if (transa && !transb) return pick<T, true, false, EPI>(g, vec, s);
  return pick<T, true, true, EPI>(g, vec, s);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// The checks every entry makes before its first HIP call.  MI_OK with *empty set: nothing to compute.
int validate(int transa, int transb, int32_t m, int32_t n, int32_t k, const uint16_t* A, int64_t lda, int64_t strideA,
             const uint16_t* B, int64_t ldb, int64_t strideB, const uint16_t* bias, const uint16_t* C, int64_t ldc,
             int64_t strideC, int32_t batch, bool* empty) {
  *empty = false;
  if (m < 0 || n < 0 || k < 0 || batch < 0) return MI_EINVAL;
  if (strideA < 0 || strideB < 0 || strideC < 0) return MI_EINVAL;
  if (lda < (transa ? m : k) || ldb < (transb ? k : n) || ldc < n) return MI_EINVAL;
  if (m == 0 || n == 0 || batch == 0) {
    *empty = true;
    return MI_OK;
  }
  if (!C || (k > 0 && (!A || !B))) return MI_EINVAL;
  if (odd(A) || odd(B) || odd(C) || odd(bias)) return MI_EINVAL;
  if (lda > 0x7fffffffL || ldb > 0x7fffffffL || ldc > 0x7fffffffL) return MI_ERANGE;
  return MI_OK;
}

// C = op(A)·op(B) (+ bias): the plain family order, no split.  bias == nullptr runs the kStore instantiations.
template <class T>
int gemm_lowp(int transa, int transb, int32_t m, int32_t n, int32_t k, const uint16_t* A, int64_t lda, int64_t strideA,
              const uint16_t* B, int64_t ldb, int64_t strideB, const uint16_t* bias, uint16_t* C, int64_t ldc, int64_t strideC,
              int32_t batch, hipStream_t s) {
  bool empty;
  const int st = validate(transa, transb, m, n, k, A, lda, strideA, B, ldb, strideB, bias, C, ldc, strideC, batch, &empty);
  if (st != MI_OK || empty) return st;
  if (k == 0) {
    const long total = (long)m * n, blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffL) return MI_ERANGE;
    hipLaunchKernelGGL(fill_b16_kernel, dim3((unsigned)blocks, (unsigned)(batch < 65535 ? batch : 65535)), dim3(256), 0, s, C,
                       m, n, (long)ldc, (long)strideC, batch, bias);
    return mi::check_launch();
  }
  const bool vec = aligned16(A) && aligned16(B) && aligned16(C) && aligned16(bias) && lda % 8 == 0 && ldb % 8 == 0 &&
                   ldc % 8 == 0 && strideA % 8 == 0 && strideB % 8 == 0 && strideC % 8 == 0;
  const GemmArgs g = {A, B, C, m, n, k, batch, (long)lda, (long)ldb, (long)ldc, (long)strideA, (long)strideB, (long)strideC, 0,
                      bias, nullptr};
  return bias ? run<T, kBias>(transa, transb, g, vec, s) : run<T, kStore>(transa, transb, g, vec, s);
}

size_t split_bytes(int S, int32_t m, int32_t n) { return (size_t)S * (size_t)m * (size_t)n * sizeof(float); }

// One product cut into S ranges of k (S ≥ 1, k a multiple of 32·S): partials into the workspace, then the combine.
template <class T>
int gemm_lowp_split(int transa, int transb, int32_t m, int32_t n, int32_t k, const uint16_t* A, int64_t lda, const uint16_t* B,
                    int64_t ldb, const uint16_t* bias, uint16_t* C, int64_t ldc, int S, void* workspace, size_t workspace_bytes,
                    hipStream_t s) {
  bool empty;
  const int st = validate(transa, transb, m, n, k, A, lda, 0, B, ldb, 0, bias, C, ldc, 0, 1, &empty);
  if (st != MI_OK) return st;
  if (S < 1 || (S > 1 && k % (32 * (long)S) != 0)) return MI_EINVAL;
  if (empty) return MI_OK;
  if (S == 1 || k == 0) return gemm_lowp<T>(transa, transb, m, n, k, A, lda, 0, B, ldb, 0, bias, C, ldc, 0, 1, s);
  if (!workspace || !aligned16(workspace)) return MI_EINVAL;
  if (workspace_bytes < split_bytes(S, m, n)) return MI_ENOMEM;  // never silently unsplit: the order is part of the result
  const long mn = (long)m * n;
  const bool quads = n % 4 == 0 && ldc % 4 == 0 && (reinterpret_cast<uintptr_t>(C) & 7u) == 0;
  const long blocks = ((quads ? mn / 4 : mn) + 255) / 256;
  if (blocks > 0x7fffffffL) return MI_ERANGE;
  const int32_t ks = k / S;
  // the S ranges as a batch: item s reads rows / columns [s·ks, (s + 1)·ks) of the k dimension of both operands
  const long stepA = (long)ks * (transa ? lda : 1), stepB = (long)ks * (transb ? 1 : ldb);
  const bool vec = aligned16(A) && aligned16(B) && lda % 8 == 0 && ldb % 8 == 0;  // (the steps are multiples of 32 elements)
  float* P = static_cast<float*>(workspace);
  const GemmArgs g = {A, B, nullptr, m, n, ks, S, (long)lda, (long)ldb, (long)n, stepA, stepB, mn, 0, nullptr, P};
  const int pst = run<T, kPartial>(transa, transb, g, vec, s);
  if (pst != MI_OK) return pst;
  if (quads)
    hipLaunchKernelGGL((gemm_lowp_combine_kernel<T, 4>), dim3((unsigned)blocks), dim3(256), 0, s, P, S, mn, n, C, (long)ldc, bias);
  else
    hipLaunchKernelGGL((gemm_lowp_combine_kernel<T, 1>), dim3((unsigned)blocks), dim3(256), 0, s, P, S, mn, n, C, (long)ldc, bias);
  return mi::check_launch();
}

template <class T>
int gemm_lowp_ws(int transa, int transb, int32_t m, int32_t n, int32_t k, const uint16_t* A, int64_t lda, int64_t strideA,
                 const uint16_t* B, int64_t ldb, int64_t strideB, const uint16_t* bias, uint16_t* C, int64_t ldc, int64_t strideC,
                 int32_t batch, void* workspace, size_t workspace_bytes, hipStream_t s) {
  const int S = mi_gemm_lowp_split_count(m, n, k, batch);
  if (S <= 1) return gemm_lowp<T>(transa, transb, m, n, k, A, lda, strideA, B, ldb, strideB, bias, C, ldc, strideC, batch, s);
  if (strideA < 0 || strideB < 0 || strideC < 0) return MI_EINVAL;
  return gemm_lowp_split<T>(transa, transb, m, n, k, A, lda, B, ldb, bias, C, ldc, S, workspace, workspace_bytes, s);
}

}  // namespace

extern "C" {

#define MI_LOWP_ARGS                                                                                                        \
  int transa, int transb, int32_t m, int32_t n, int32_t k, const uint16_t *A, int64_t lda, int64_t strideA, const uint16_t *B, \
      int64_t ldb, int64_t strideB
#define MI_LOWP_C uint16_t *C, int64_t ldc, int64_t strideC, int32_t batch

int mi_gemm_bf16(MI_LOWP_ARGS, MI_LOWP_C, mi_stream_t stream) {
  return gemm_lowp<Bf16>(transa, transb, m, n, k, A, lda, strideA, B, ldb, strideB, nullptr, C, ldc, strideC, batch,
                         static_cast<hipStream_t>(stream));
}

int mi_gemm_f16(MI_LOWP_ARGS, MI_LOWP_C, mi_stream_t stream) {
  return gemm_lowp<F16>(transa, transb, m, n, k, A, lda, strideA, B, ldb, strideB, nullptr, C, ldc, strideC, batch,
                        static_cast<hipStream_t>(stream));
}

int mi_gemm_bias_bf16(MI_LOWP_ARGS, const uint16_t* bias, MI_LOWP_C, mi_stream_t stream) {
  return gemm_lowp<Bf16>(transa, transb, m, n, k, A, lda, strideA, B, ldb, strideB, bias, C, ldc, strideC, batch,
                         static_cast<hipStream_t>(stream));
}

int mi_gemm_bias_f16(MI_LOWP_ARGS, const uint16_t* bias, MI_LOWP_C, mi_stream_t stream) {
  return gemm_lowp<F16>(transa, transb, m, n, k, A, lda, strideA, B, ldb, strideB, bias, C, ldc, strideC, batch,
                        static_cast<hipStream_t>(stream));
}

// How many ranges k is cut into — a function of the shape alone, fitted to the measured grid of DESIGN.md §3.10
// (profiles/r10_split_grid.log: within 1.28 × of the best S at every point, 1.05 × on average).  1: no split.
//   * one product (batch == 1) with k ≥ 2048 and at most 576 output tiles of 128 × 128 (the extent of the grid);
//   * S = the largest power of two ≤ min(2048 / tiles, k / 256, 32), halved until k is a multiple of 32·S.
int mi_gemm_lowp_split_count(int32_t m, int32_t n, int32_t k, int32_t batch) {
  constexpr long kSplitMinK = 2048, kSplitMaxTiles = 576, kSplitTarget = 2048, kSplitMinRange = 256;
  if (batch != 1 || m <= 0 || n <= 0 || k < kSplitMinK) return 1;
  const long tiles = (((long)m + 127) / 128) * (((long)n + 127) / 128);
  if (tiles > kSplitMaxTiles) return 1;
  long cap = kSplitTarget / tiles;
  if (cap > k / kSplitMinRange) cap = k / kSplitMinRange;
  if (cap > 32) cap = 32;
  int S = 1;
  while (2L * S <= cap) S *= 2;
  while (S > 1 && k % (32 * S) != 0) S /= 2;
  return S;
}

// The columns of the output tile — a function of the shape alone: 128 (the 128 × 128 tile) when n > 64 and the 128 × 128
// tiles of all items number at least 512, else 64 (the 128 × 64 tile).  The bits of the product do not depend on it.
int mi_gemm_lowp_tile_n(int32_t m, int32_t n, int32_t batch) {
  if (m <= 0 || n <= 64 || batch <= 0) return 64;
  const long wide = (((long)m + 127) / 128) * (((long)n + 127) / 128) * batch;
  return wide < 512 ? 64 : 128;
}

size_t mi_gemm_lowp_workspace_bytes(int32_t m, int32_t n, int32_t k, int32_t batch) {
  const int S = mi_gemm_lowp_split_count(m, n, k, batch);
  return S > 1 ? split_bytes(S, m, n) : 0;
}

int mi_gemm_ws_bf16(MI_LOWP_ARGS, const uint16_t* bias, MI_LOWP_C, void* workspace, size_t workspace_bytes, mi_stream_t stream) {
  return gemm_lowp_ws<Bf16>(transa, transb, m, n, k, A, lda, strideA, B, ldb, strideB, bias, C, ldc, strideC, batch, workspace,
                            workspace_bytes, static_cast<hipStream_t>(stream));
}

int mi_gemm_ws_f16(MI_LOWP_ARGS, const uint16_t* bias, MI_LOWP_C, void* workspace, size_t workspace_bytes, mi_stream_t stream) {
  return gemm_lowp_ws<F16>(transa, transb, m, n, k, A, lda, strideA, B, ldb, strideB, bias, C, ldc, strideC, batch, workspace,
                           workspace_bytes, static_cast<hipStream_t>(stream));
}

int mi_gemm_split_bf16(int transa, int transb, int32_t m, int32_t n, int32_t k, const uint16_t* A, int64_t lda, const uint16_t* B,
                       int64_t ldb, const uint16_t* bias, uint16_t* C, int64_t ldc, int32_t splits, void* workspace,
                       size_t workspace_bytes, mi_stream_t stream) {
  return gemm_lowp_split<Bf16>(transa, transb, m, n, k, A, lda, B, ldb, bias, C, ldc, splits, workspace, workspace_bytes,
                               static_cast<hipStream_t>(stream));
}

int mi_gemm_split_f16(int transa, int transb, int32_t m, int32_t n, int32_t k, const uint16_t* A, int64_t lda, const uint16_t* B,
                      int64_t ldb, const uint16_t* bias, uint16_t* C, int64_t ldc, int32_t splits, void* workspace,
                      size_t workspace_bytes, mi_stream_t stream) {
  return gemm_lowp_split<F16>(transa, transb, m, n, k, A, lda, B, ldb, bias, C, ldc, splits, workspace, workspace_bytes,
                              static_cast<hipStream_t>(stream));
}

}  // extern "C"
