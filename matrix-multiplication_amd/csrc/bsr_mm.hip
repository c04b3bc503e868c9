// Block-sparse × dense products in bfloat16 and float16 on the matrix cores: C[b] = op(A) · B[b] with A given as the kept
// 64 × 64 blocks of a CSR block list (values [n][64][64], row-major blocks, shared by every item of the batch), and the
// sampled product dA[e] = dC[I-rows, :] · B[J-rows, :]ᵀ on the same list.  All of one type T ∈ {bf16, fp16} (2-byte bit
// patterns at the C-ABI), every sum in fp32, one rounding per output element at the store.
//
// What it computes (contract of include/mi_spmm.h, mi_bsr_mm_{bf16,f16} / mi_bsr_sddmm_{bf16,f16} — DESIGN.md §3.15):
//  * ONE instruction for every product: v_mfma_f32_16x16x32_{bf16,f16}, with the k-slots of gemm_lowp.hip (lane group lg
//    of a fragment holds k = 32s + 8lg … + 7).  Each output element is ONE accumulator, started at +0, carried through
//    the blocks of its list in the order of the list and, within a block, through the two 32-deep k-steps ascending;
//    the store narrows once by static_cast (v_cvt_pk_bf16_f32 / v_cvt_f16_f32).  With the list in ascending order this is
//    the k order of gemm_lowp.hip with the unkept 64-deep k-tiles left out: for finite operands the bits of
//    mi_gemm_{bf16,f16} on the densified A, whose unkept tiles add exact zeros.  The bits never depend on the launch
//    shape, the column tile, the position in the batch or the alignment form.
//  * A block outside the list is never loaded, nor are the rows of B it would meet.  An empty list stores zeros.  A listed
//    column outside the grid or an entry id outside the values is skipped, offsets are clamped to [0, nnz]: a malformed
//    list cannot make a kernel read outside the operands.
//  * The sampled product sums over the flattened width k' = item · N + j (item-major, items ascending) in ascending
//    32-steps, a ragged last step zero-padded in both operands: the bits of mi_gemm_{bf16,f16}(transb) on
//    [64 × batch·N] operands, block by block.
//
// Product kernel: a 256-thread workgroup owns one 64-row block of the output × BN columns of one item (BN = 128; 64 for
// N ≤ 64 and for grids too small to fill the chip), 4 waves in 2 × 2, each 32 × BN/2 in 16 × 16 MFMA tiles.  Per listed
// entry it stages the 8 KiB value block (plain: k contiguous, 16-byte pieces; TRANS_A: rows contiguous, 4 k-rows × 8
// rows transposed in registers — values[entry_id[e]] through the kept permutation) and the 64 × BN tile of the dense
// operand (rows contiguous, transposed in registers) into LDS images [rows][64 + 8], double-buffered: the global loads
// of the next entry are in flight during the MFMAs of this one, one barrier per entry.  (9 + 18) KiB × 2 buffers at
// BN = 128: two workgroups per CU.  Alignment forms as in gemm_lowp.hip: VEC (B and C 16-byte aligned, leading
// dimensions and item strides multiples of 8) and checked (any 2-byte alignment, any N).  The values are always 16-byte
// aligned blocks.
// Sampled kernel: one workgroup per listed entry, 4 waves in 2 × 2 on the 64 × 64 result; both operands k-contiguous
// over the width (the NT form), walked in 64-deep tiles over the items with the same double buffer; one 8 KiB block
// written with 16-byte stores.
// No atomics, no workspace, no host read-back: graph-capturable.
#include <type_traits>

#include "bsr_device.h"

namespace {

struct MmArgs {
  const int32_t* rowptr;  // [own_blocks + 1]
  const int32_t* col;     // [nnz]: the block of the inner dimension an entry meets
  const int32_t* id;      // [nnz] or null: the block of `values` an entry reads (null: the entry's own position)
  long nnz, nvalues;
  const uint16_t* values;  // [nvalues][64][64]
  const uint16_t* B;
  uint16_t* C;
  int own_blocks, inner_blocks, n, batch, tiles_n;
  long ldb, ldc, sB, sC;
};

struct SddmmArgs {
  const int32_t* row;  // [nnz]: block row of an entry
  const int32_t* col;  // [nnz]: block column
  const int32_t* id;   // [nnz] or null: the block of `out` an entry writes
  long nvalues;
  const uint16_t* G;  // dC [batch][M][N]
  const uint16_t* B;  // [batch][K][N]
  uint16_t* out;      // [nvalues][64][64]
  int row_blocks, col_blocks, n, batch, width;  // width = batch · N
  long ldg, ldb, sG, sB;
};

// the next entry at or after p that is computed: its column inside the grid, its values inside the buffer
__device__ __forceinline__ int next_entry(const MmArgs& g, int p, int end) {
  for (; p < end; ++p) {
    if ((unsigned)g.col[p] >= (unsigned)g.inner_blocks) continue;
    const long e = g.id ? (long)g.id[p] : (long)p;
    if (e < 0 || e >= g.nvalues) continue;
    break;
  }
  return p;
}

// One listed entry in registers on its way to LDS: the value block and the 64 × BN tile of the dense operand.
template <bool TRANS_A, int BN, bool VEC>
struct Staged {
  std::conditional_t<TRANS_A, TileRC<kB>, BlockKC> a;
  TileRC<BN> b;
  __device__ __forceinline__ void load(const MmArgs& g, const uint16_t* B, int p, int n0, int tid) {
    const uint16_t* V = g.values + (g.id ? (long)g.id[p] : (long)p) * (kB * kB);
    if constexpr (TRANS_A)
      a.template load<true>(V, kB, 0, kB, tid);
    else
      a.load(V, tid);
    b.template load<VEC>(B + (long)g.col[p] * kB * g.ldb, g.ldb, n0, g.n, tid);
  }
  __device__ __forceinline__ void store(unsigned short* S, int tid) const {
    a.store(S, tid);
    b.store(S + kB * kStr, tid);
  }
};

template <class T, bool TRANS_A, int BN, bool VEC>
__global__ __launch_bounds__(256) void bsr_mm_kernel(MmArgs g) {
  constexpr int FN = BN / 32;
  static_assert(FN % 2 == 0, "B fragments go in pairs (interleaved rows: 16-byte stores)");
  constexpr int kBuf = (kB + BN) * kStr;
  __shared__ __attribute__((aligned(16))) unsigned short smem[2 * kBuf];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wm = wid >> 1, wn = wid & 1;
  const int li = lane & 15, lg = lane >> 4;
  // XCD remap (bijective): the column tiles of one block row, which share its value blocks, on one XCD's L2
  const unsigned total = gridDim.x, bid = blockIdx.x, q8 = total / 8, rem = total % 8, xcd = bid % 8;
  const unsigned w = xcd * q8 + (xcd < rem ? xcd : rem) + bid / 8;
  const int I = (int)(w / g.tiles_n), n0 = (int)(w % g.tiles_n) * BN;
  long lo = g.rowptr[I], hi = g.rowptr[I + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > g.nnz ? g.nnz : hi;
  const int beg = (int)lo, end = (int)hi;

  for (int b = blockIdx.y; b < g.batch; b += gridDim.y) {
    const uint16_t* B = g.B + (long)b * g.sB;
    f32x4 acc[2][FN];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    Staged<TRANS_A, BN, VEC> st;
    auto load = [&](int p) { st.load(g, B, p, n0, tid); };
    auto store = [&](unsigned short* S) { st.store(S, tid); };

    int p = next_entry(g, beg, end), buf = 0;
    if (p < end) {
      load(p);
      store(smem);
      __syncthreads();
    }
    while (p < end) {
      const int q = next_entry(g, p + 1, end);
      if (q < end) load(q);
      const unsigned short* As = smem + buf * kBuf;
      tile_mfma<T, FN>(acc, As, As + kB * kStr, wm, wn, li, lg);
      if (q < end) store(smem + (buf ^ 1) * kBuf);
      __syncthreads();
      p = q;
      buf ^= 1;
    }
    store_acc<T, FN, VEC>(acc, g.C + (long)b * g.sC + (long)I * kB * g.ldc, g.ldc, n0, g.n, wm, wn, li, lg);
  }
}

// 8 elements of one row at the flattened positions kk … kk + 7 of the width (position k' = item · N + j lies at
// rowp[item · stride + j]); zeros from `width` on.  VEC: a piece inside the width lies inside one item (N a multiple of
// 8, or one item) on a 16-byte boundary.
template <bool VEC>
__device__ __forceinline__ uint4 flat8(const uint16_t* rowp, long stride, int kk, int n, int width, bool one) {
  if (kk >= width) return uint4{0u, 0u, 0u, 0u};
  int item = one ? 0 : kk / n, j = kk - item * n;
  if (VEC && kk + 8 <= width) return *reinterpret_cast<const uint4*>(rowp + (long)item * stride + j);
  unsigned short e[8];
#pragma unroll
  for (int x = 0; x < 8; ++x) {
    e[x] = kk + x < width ? rowp[(long)item * stride + j] : (unsigned short)0;
    if (++j == n) j = 0, ++item;
  }
  return pack8(e);
}

template <class T, bool VEC>
__global__ __launch_bounds__(256) void bsr_sddmm_kernel(SddmmArgs g) {
  constexpr int kBuf = 2 * kB * kStr;
  __shared__ __attribute__((aligned(16))) unsigned short smem[2 * kBuf];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wm = wid >> 1, wn = wid & 1;
  const int li = lane & 15, lg = lane >> 4;
  const long p = blockIdx.x;
  const long e = g.id ? (long)g.id[p] : p;
  if (e < 0 || e >= g.nvalues) return;
  const int I = g.row[p], J = g.col[p];
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if ((unsigned)I < (unsigned)g.row_blocks && (unsigned)J < (unsigned)g.col_blocks) {
    const bool one = g.batch == 1;
    const int nt = (g.width + kB - 1) / kB;
    // pieces c = tid and tid + 256: row c / 8, k-piece c % 8 — the same k-piece for both
    const int r0 = tid >> 3, kp = (tid & 7) * 8;
    const uint16_t* Gr[2] = {g.G + ((long)I * kB + r0) * g.ldg, g.G + ((long)I * kB + r0 + 32) * g.ldg};
    const uint16_t* Br[2] = {g.B + ((long)J * kB + r0) * g.ldb, g.B + ((long)J * kB + r0 + 32) * g.ldb};
    uint4 sg[2], sb[2];
    auto load = [&](int t) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        sg[i] = flat8<VEC>(Gr[i], g.sG, t * kB + kp, g.n, g.width, one);
        sb[i] = flat8<VEC>(Br[i], g.sB, t * kB + kp, g.n, g.width, one);
      }
    };
    auto store = [&](unsigned short* S) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        *reinterpret_cast<uint4*>(S + (r0 + 32 * i) * kStr + kp) = sg[i];
        *reinterpret_cast<uint4*>(S + (kB + r0 + 32 * i) * kStr + kp) = sb[i];
      }
    };
    if (nt > 0) {
      load(0);
      store(smem);
      __syncthreads();
    }
    for (int t = 0; t < nt; ++t) {
      const bool more = t + 1 < nt;
      if (more) load(t + 1);
      const unsigned short* As = smem + (t & 1) * kBuf;
      tile_mfma<T, 2>(acc, As, As + kB * kStr, wm, wn, li, lg);
      if (more) store(smem + ((t + 1) & 1) * kBuf);
      __syncthreads();
    }
  }
  store_acc<T, 2, true>(acc, g.out + e * (kB * kB), kB, 0, kB, wm, wn, li, lg);
}

template <class T, bool TRANS_A, int BN>
int launch_mm(const MmArgs& g, bool vec, hipStream_t s) {
  MmArgs a = g;
  a.tiles_n = (g.n + BN - 1) / BN;
  const long tiles = (long)g.own_blocks * a.tiles_n;
  if (tiles > 0x7fffffffL) return MI_ERANGE;
  const dim3 grid((unsigned)tiles, (unsigned)(g.batch < 65535 ? g.batch : 65535));
  if (vec)
    hipLaunchKernelGGL((bsr_mm_kernel<T, TRANS_A, BN, true>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((bsr_mm_kernel<T, TRANS_A, BN, false>), grid, dim3(256), 0, s, a);
  return mi::check_launch();
}

// The column tile: 128 while that fills the chip, else 64 (and always for N ≤ 64) — by the shape only, same bits either way.
// mi_bsr_mm_tile_n is the rule, so that a caller can ask which one a shape takes.
template <class T, bool TRANS_A>
int pick_mm(const MmArgs& g, bool vec, hipStream_t s) {
  if (mi_bsr_mm_tile_n(g.own_blocks * kB, g.n, g.batch) == 64) return launch_mm<T, TRANS_A, 64>(g, vec, s);
  return launch_mm<T, TRANS_A, 128>(g, vec, s);
}

template <class T>
int mm_entry(const int32_t* rowptr, const int32_t* col, const int32_t* entry_id, int64_t nnz, int32_t trans_a, int32_t rows,
             int32_t inner, int32_t N, int32_t batch, const uint16_t* values, int64_t nvalues, const uint16_t* B, int64_t ldb,
             int64_t strideB, uint16_t* C, int64_t ldc, int64_t strideC, hipStream_t s) {
  if (nnz < 0 || nvalues < 0 || rows < 0 || inner < 0 || N < 0 || batch < 0) return MI_EINVAL;
  if (rows % kB != 0 || inner % kB != 0) return MI_EINVAL;
  if (strideB < 0 || strideC < 0 || ldb < N || ldc < N) return MI_EINVAL;
  if (nnz > 0x7fffffffLL || nvalues > 0x7fffffffLL) return MI_ERANGE;
  if (!entry_id && nvalues < nnz) return MI_EINVAL;
  if (rows == 0 || N == 0 || batch == 0) return MI_OK;
  if (!rowptr || !C || odd(C)) return MI_EINVAL;
  if (nnz > 0 && (!col || !values || !B || inner == 0 || !mi::aligned16(values) || odd(B))) return MI_EINVAL;
  if (ldb > 0x7fffffffL || ldc > 0x7fffffffL) return MI_ERANGE;
  const bool vec = mi::aligned16(B) && mi::aligned16(C) && ldb % 8 == 0 && ldc % 8 == 0 && strideB % 8 == 0 && strideC % 8 == 0;
  MmArgs g = {};
  g.rowptr = rowptr, g.col = col, g.id = entry_id, g.nnz = nnz, g.nvalues = nvalues, g.values = values, g.B = B, g.C = C;
  g.own_blocks = rows / kB, g.inner_blocks = inner / kB, g.n = N, g.batch = batch;
  g.ldb = ldb, g.ldc = ldc, g.sB = strideB, g.sC = strideC;
  return trans_a ? pick_mm<T, true>(g, vec, s) : pick_mm<T, false>(g, vec, s);
}

template <class T>
int sddmm_entry(const int32_t* entry_row, const int32_t* col, const int32_t* entry_id, int64_t nnz, int32_t M, int32_t K,
                int32_t N, int32_t batch, const uint16_t* dC, int64_t lddc, int64_t strideDC, const uint16_t* B, int64_t ldb,
                int64_t strideB, uint16_t* dvalues, int64_t nvalues, hipStream_t s) {
  if (nnz < 0 || nvalues < 0 || M < 0 || K < 0 || N < 0 || batch < 0) return MI_EINVAL;
  if (M % kB != 0 || K % kB != 0) return MI_EINVAL;
  if (strideDC < 0 || strideB < 0 || lddc < N || ldb < N) return MI_EINVAL;
  if (nnz > 0x7fffffffLL || nvalues > 0x7fffffffLL || (int64_t)batch * N > 0x7fffffffLL) return MI_ERANGE;
  if (!entry_id && nvalues < nnz) return MI_EINVAL;
  if (nnz == 0) return MI_OK;
  if (!entry_row || !col || !dvalues || !mi::aligned16(dvalues)) return MI_EINVAL;
  if (M == 0 || K == 0) return MI_EINVAL;  // entries on an empty grid
  const int width = batch * N;
  if (width > 0 && (!dC || !B || odd(dC) || odd(B))) return MI_EINVAL;
  if (lddc > 0x7fffffffL || ldb > 0x7fffffffL) return MI_ERANGE;
  const bool vec = mi::aligned16(dC) && mi::aligned16(B) && lddc % 8 == 0 && ldb % 8 == 0 && strideDC % 8 == 0 && strideB % 8 == 0 &&
                   (batch == 1 || N % 8 == 0);
  SddmmArgs g = {};
  g.row = entry_row, g.col = col, g.id = entry_id, g.nvalues = nvalues, g.G = dC, g.B = B, g.out = dvalues;
  g.row_blocks = M / kB, g.col_blocks = K / kB, g.n = N, g.batch = batch, g.width = width;
  g.ldg = lddc, g.ldb = ldb, g.sG = strideDC, g.sB = strideB;
  if (vec)
    hipLaunchKernelGGL((bsr_sddmm_kernel<T, true>), dim3((unsigned)nnz), dim3(256), 0, s, g);
  else
    hipLaunchKernelGGL((bsr_sddmm_kernel<T, false>), dim3((unsigned)nnz), dim3(256), 0, s, g);
  return mi::check_launch();
}

}  // namespace

extern "C" {

#define MI_BSR_MM_ARGS                                                                                                         \
  const int32_t *rowptr, const int32_t *col, const int32_t *entry_id, int64_t nnz, int32_t trans_a, int32_t rows, int32_t inner, \
      int32_t N, int32_t batch, const uint16_t *values, int64_t nvalues, const uint16_t *B, int64_t ldb, int64_t strideB,      \
      uint16_t *C, int64_t ldc, int64_t strideC, mi_stream_t stream
#define MI_BSR_MM_PASS rowptr, col, entry_id, nnz, trans_a, rows, inner, N, batch, values, nvalues, B, ldb, strideB, C, ldc, strideC

int mi_bsr_mm_bf16(MI_BSR_MM_ARGS) { return mm_entry<Bf16>(MI_BSR_MM_PASS, static_cast<hipStream_t>(stream)); }
int mi_bsr_mm_f16(MI_BSR_MM_ARGS) { return mm_entry<F16>(MI_BSR_MM_PASS, static_cast<hipStream_t>(stream)); }

#define MI_BSR_SDDMM_ARGS                                                                                                    \
  const int32_t *entry_row, const int32_t *col, const int32_t *entry_id, int64_t nnz, int32_t M, int32_t K, int32_t N,       \
      int32_t batch, const uint16_t *dC, int64_t lddc, int64_t strideDC, const uint16_t *B, int64_t ldb, int64_t strideB,    \
      uint16_t *dvalues, int64_t nvalues, mi_stream_t stream
#define MI_BSR_SDDMM_PASS entry_row, col, entry_id, nnz, M, K, N, batch, dC, lddc, strideDC, B, ldb, strideB, dvalues, nvalues

// The column tile of mi_bsr_mm_T — a function of the shape alone (rows of C, N, batch): 128 when N > 64 and the 64-row
// blocks × 128-column tiles × items number at least 512, else 64.  The bits of the product do not depend on it.
int mi_bsr_mm_tile_n(int32_t rows, int32_t N, int32_t batch) {
  if (rows <= 0 || N <= 64 || batch <= 0) return 64;
  const long wide = (long)(rows / kB) * (((long)N + 127) / 128) * batch;
  return wide < 512 ? 64 : 128;
}

int mi_bsr_sddmm_bf16(MI_BSR_SDDMM_ARGS) { return sddmm_entry<Bf16>(MI_BSR_SDDMM_PASS, static_cast<hipStream_t>(stream)); }
int mi_bsr_sddmm_f16(MI_BSR_SDDMM_ARGS) { return sddmm_entry<F16>(MI_BSR_SDDMM_PASS, static_cast<hipStream_t>(stream)); }

}  // extern "C"
