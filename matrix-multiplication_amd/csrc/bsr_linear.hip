// Block-sparse linear layer in bfloat16 and float16 on the matrix cores: Y = X·Wᵀ (+ bias) with the weight W [out, in]
// given as the kept 64 × 64 blocks of a CSR block list (values [n][64][64], row-major blocks of W) and the tokens
// X [T, in] row-major; dX = dY·W on the same kernel over the transposed list; and the weight gradient
// dvalues[e] = dY[:, O-columns]ᵀ · X[:, I-columns] on the kept blocks.  All of one type T ∈ {bf16, fp16} (2-byte bit
// patterns at the C-ABI), every sum in fp32, one rounding per output element at the store.
//
// What it computes (contract of include/mi_spmm.h, mi_bsr_linear_{bf16,f16} / mi_bsr_wgrad_{bf16,f16} — DESIGN.md §3.16):
//  * ONE instruction for every product: v_mfma_f32_16x16x32_{bf16,f16}, with the k-slots of gemm_lowp.hip (lane group lg
//    of a fragment holds k = 32s + 8lg … + 7).  Each output element is ONE accumulator, started at +0, carried through
//    the blocks of its list in the order of the list and, within a block, through the two 32-deep k-steps ascending;
//    the store narrows once by static_cast.  With the list ascending this is the k order of gemm_lowp.hip with the unkept
//    64-deep k-tiles left out: for finite operands the bits of mi_gemm_{bf16,f16} on the densified W.  The bits never
//    depend on the token tile, the workgroup numbering, the position of a token or the alignment form.
//  * A block outside the list is never loaded, nor are the columns of X it would meet.  An empty list row stores +0, or
//    the bias.  A listed column outside the grid or an entry id outside the values is skipped, offsets are clamped to
//    [0, nnz]: a malformed list cannot make a kernel read outside the operands.
//  * The weight gradient sums the tokens of a range in ascending 32-steps from +0, a ragged last step zero-padded in both
//    operands; S > 1 ranges go to fp32 partials that a combine kernel adds in index order and rounds once: the bits of
//    mi_gemm_split_{bf16,f16}(transa) with the same S, block by block.
//
// Product kernel: a 256-thread workgroup owns BM tokens × one 64-column block of the output (BM = 128; 64 for T ≤ 64 and
// for grids too small to fill the chip), 4 waves in 2 × 2, each BM/2 tokens × 32 columns in 16 × 16 MFMA tiles.  Both
// operands of the forward are k-contiguous: per listed entry the BM × 64 tile of X and the 8 KiB value block move global →
// registers → LDS in 16-byte pieces, no register transpose (TRANS_W: values[entry_id[e]] rows-contiguous, 4 k-rows × 8
// rows transposed in registers — never gathered), into LDS images [rows][64 + 8], double-buffered: the global loads of
// the next entry are in flight during the MFMAs of this one, one barrier per entry.  (18 + 9) KiB × 2 buffers at
// BM = 128: two workgroups per CU.  A lane ends with eight adjacent columns of one row: one 16-byte store.  kBias: the
// lane's eight bias values are loaded once ahead of the k-loop and added in fp32 before the one rounding.
// Workgroup numbering: see the remap in bsr_linear_kernel (the block rows of one token tile, which share X, run on one XCD).
// Weight-gradient kernel: one workgroup per (listed entry, token range), 4 waves in 2 × 2 on the 64 × 64 result; both
// operands are strided along k = tokens (the TN form): threads 0–127 stage the 64-token × 64-column tile of dY, threads
// 128–255 that of X, each as 4 token rows × 8 columns transposed in registers; 64-deep tiles with the same double buffer.
// No float atomics, no host read-back: graph-capturable.
#include <type_traits>

#include "bsr_device.h"

namespace {

struct LinArgs {
  const int32_t* rowptr;  // [own_blocks + 1]
  const int32_t* col;     // [nnz]: the 64-column block of X an entry meets
  const int32_t* id;      // [nnz] or null: the block of `values` an entry reads (null: the entry's own position)
  long nnz, nvalues;
  const uint16_t* values;  // [nvalues][64][64]
  const uint16_t* X;
  const uint16_t* bias;  // [64 · own_blocks] (BIAS)
  uint16_t* Y;
  int own_blocks, inner_blocks, tokens;
  long ldx, ldy;
};

struct WgradArgs {
  const int32_t* row;  // [nnz]: block row of an entry (64 columns of dY)
  const int32_t* col;  // [nnz]: block column (64 columns of X)
  const int32_t* id;   // [nnz] or null: the block of `out` an entry writes
  long nnz, nvalues;
  const uint16_t* G;  // dY [tokens][out]
  const uint16_t* X;  // [tokens][in]
  uint16_t* out;      // [nvalues][64][64]
  float* P;           // PARTIAL: [splits][nnz][64][64]
  int out_blocks, in_blocks, tokens, range;  // range: tokens per workgroup (a multiple of 32 when there are several)
  long ldg, ldx;
};

// BM tokens × 64 values of k of X, k contiguous (element (t, k) at P[t·ld + k]): BM·8 pieces of 8, BM/32 per thread.
template <int BM>
struct TokensKC {
  uint4 v[BM / 32];
  template <bool VEC>
  __device__ __forceinline__ void load(const uint16_t* P, long ld, int t0, int tokens, int tid) {
#pragma unroll
    for (int i = 0; i < BM / 32; ++i) {
      const int c = tid + i * 256, t = t0 + (c >> 3);
      v[i] = load8<VEC>(P + (long)t * ld + (c & 7) * 8, t < tokens ? 8 : 0);
    }
  }
  __device__ __forceinline__ void store(unsigned short* S, int tid) const {
#pragma unroll
    for (int i = 0; i < BM / 32; ++i) {
      const int c = tid + i * 256;
      *reinterpret_cast<uint4*>(S + (c >> 3) * kStr + (c & 7) * 8) = v[i];
    }
  }
};

// the next entry at or after p that is computed: its column inside the grid, its values inside the buffer
__device__ __forceinline__ int next_entry(const LinArgs& g, int p, int end) {
  for (; p < end; ++p) {
    if ((unsigned)g.col[p] >= (unsigned)g.inner_blocks) continue;
    const long e = g.id ? (long)g.id[p] : (long)p;
    if (e < 0 || e >= g.nvalues) continue;
    break;
  }
  return p;
}

// One listed entry in registers on its way to LDS: the BM × 64 tile of X and the value block.
template <bool TRANS_W, int BM, bool VEC>
struct Staged {
  TokensKC<BM> x;
  std::conditional_t<TRANS_W, TileRC<kB>, BlockKC> w;
  __device__ __forceinline__ void load(const LinArgs& g, int p, int t0, int tid) {
    const uint16_t* V = g.values + (g.id ? (long)g.id[p] : (long)p) * (kB * kB);
    if constexpr (TRANS_W)
      w.template load<true>(V, kB, 0, kB, tid);
    else
      w.load(V, tid);
    x.template load<VEC>(g.X + (long)g.col[p] * kB, g.ldx, t0, g.tokens, tid);
  }
  __device__ __forceinline__ void store(unsigned short* S, int tid) const {
    x.store(S, tid);
    w.store(S + BM * kStr, tid);
  }
};

template <class T, bool TRANS_W, int BM, bool BIAS, bool VEC>
__global__ __launch_bounds__(256) void bsr_linear_kernel(LinArgs g) {
  constexpr int WM = BM / 2, FM = WM / 16, FN = 2;
  constexpr int kBuf = (BM + kB) * kStr;
  __shared__ __attribute__((aligned(16))) unsigned short smem[2 * kBuf];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wm = wid >> 1, wn = wid & 1;
  const int li = lane & 15, lg = lane >> 4;
  // XCD remap (bijective): consecutive w on one XCD's L2.  Consecutive w are the block rows of ONE token tile, which share
  // its BM × in slice of X — the operand that does not fit an L2 (the kept blocks of a layer's weight do: every XCD ends up
  // holding them all).  Measured against the other numbering (the token tiles of one block row consecutive, which share
  // its value blocks): 1.09 – 1.24 × ahead in y at 16384 tokens, DESIGN.md §3.16.
  const unsigned total = gridDim.x, bid = blockIdx.x, q8 = total / 8, rem = total % 8, xcd = bid % 8;
  const unsigned w = xcd * q8 + (xcd < rem ? xcd : rem) + bid / 8;
  const int Pb = (int)(w % g.own_blocks), t0 = (int)(w / g.own_blocks) * BM;
  long lo = g.rowptr[Pb], hi = g.rowptr[Pb + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > g.nnz ? g.nnz : hi;
  const int beg = (int)lo, end = (int)hi;
  const int c0 = wn * 32 + 8 * lg;  // the lane's eight columns inside the block
  // the lane's eight columns of bias, loaded once, ahead of the k-loop (nothing waits on them)
  uint4 bias8 = {0u, 0u, 0u, 0u};
  if constexpr (BIAS) bias8 = load8<VEC>(g.bias + (long)Pb * kB + c0, 8);

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  Staged<TRANS_W, BM, VEC> st;

  int p = next_entry(g, beg, end), buf = 0;
  if (p < end) {
    st.load(g, p, t0, tid);
    st.store(smem, tid);
    __syncthreads();
  }
  while (p < end) {
    const int q = next_entry(g, p + 1, end);
    if (q < end) st.load(g, q, t0, tid);
    const unsigned short* Xs = smem + buf * kBuf;
    const unsigned short* Ws = Xs + BM * kStr;
    // bsr_device.h's tile_mfma with FM rows of fragments, written out: as a call it changed all 32 instantiations (§3.24)
#pragma unroll
    for (int ks = 0; ks < kB / 32; ++ks) {
      const int kofs = ks * 32 + 8 * lg;
      uint4 af[FM], bf[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i) af[i] = *reinterpret_cast<const uint4*>(Xs + (wm * WM + i * 16 + li) * kStr + kofs);
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        // row li of fragment j holds column 8(li/4) + 4j + li%4 of the wave's 32: a lane ends with eight adjacent columns
        const int c = wn * 32 + 8 * (li >> 2) + 4 * j + (li & 3);
        bf[j] = *reinterpret_cast<const uint4*>(Ws + c * kStr + kofs);
      }
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = mfma<T>(bf[j], af[i], acc[i][j]);
    }
    if (q < end) st.store(smem + (buf ^ 1) * kBuf, tid);
    __syncthreads();
    p = q;
    buf ^= 1;
  }

  // store: lane (li, lg) holds row li of each 16-row fragment and columns c0 … c0 + 7 of the block
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int t = t0 + wm * WM + i * 16 + li;
    if (t >= g.tokens) continue;
    f32x4 x = acc[i][0], y = acc[i][1];
    if constexpr (BIAS) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        x[e] = __fadd_rn(x[e], up<T>((unsigned short)half_of(bias8, e)));
        y[e] = __fadd_rn(y[e], up<T>((unsigned short)half_of(bias8, 4 + e)));
      }
    }
    uint16_t* dst = g.Y + (long)t * g.ldy + (long)Pb * kB + c0;
    if constexpr (VEC) {
      *reinterpret_cast<uint4*>(dst) = uint4{pack2<T>(x[0], x[1]), pack2<T>(x[2], x[3]), pack2<T>(y[0], y[1]), pack2<T>(y[2], y[3])};
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        dst[e] = T::down(x[e]);
        dst[4 + e] = T::down(y[e]);
      }
    }
  }
}

// 64 tokens × 64 columns of an operand stored tokens-strided (element (c, t) at P[t·ld + c]) on the way to an LDS image
// [column][token]: 128 units of 4 token rows × 8 columns, one per thread u of 128, transposed in registers into 8-byte
// LDS writes (the layout of TileRC<64>).  Tokens from t_end on are zeros and never read.
struct TokensRC {
  uint4 v[4];
  template <bool VEC>
  __device__ __forceinline__ void load(const uint16_t* P, long ld, int t0, int t_end, int u) {
    const int c = (u >> 4) * 8, kk = (u & 15) * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int t = t0 + kk + q;
      v[q] = load8<VEC>(P + (long)t * ld + c, t < t_end ? 8 : 0);
    }
  }
  __device__ __forceinline__ void store(unsigned short* S, int u) const { store_rc(S, v, u); }
};

template <class T, bool VEC, bool PARTIAL>
__global__ __launch_bounds__(256) void bsr_wgrad_kernel(WgradArgs g) {
  constexpr int kBuf = 2 * kB * kStr;
  __shared__ __attribute__((aligned(16))) unsigned short smem[2 * kBuf];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wm = wid >> 1, wn = wid & 1;
  const int li = lane & 15, lg = lane >> 4;
  const long p = blockIdx.x;
  const int s = blockIdx.y;
  const long e = g.id ? (long)g.id[p] : p;
  if (e < 0 || e >= g.nvalues) return;  // (the combine skips the entry likewise)
  const int I = g.row[p], J = g.col[p];
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if ((unsigned)I < (unsigned)g.out_blocks && (unsigned)J < (unsigned)g.in_blocks) {
    const int t_beg = s * g.range;
    const int t_end = g.tokens - t_beg < g.range ? g.tokens : t_beg + g.range;
    const int nt = t_end > t_beg ? (t_end - t_beg + kB - 1) / kB : 0;
    // threads 0–127 stage dY (the output rows), threads 128–255 stage X (the output columns)
    const int u = tid & 127;
    const bool second = tid >= 128;
    const uint16_t* src = second ? g.X + (long)J * kB : g.G + (long)I * kB;
    const long ld = second ? g.ldx : g.ldg;
    const int image = second ? kB * kStr : 0;
    TokensRC st;
    if (nt > 0) {
      st.load<VEC>(src, ld, t_beg, t_end, u);
      st.store(smem + image, u);
      __syncthreads();
    }
    for (int t = 0; t < nt; ++t) {
      const bool more = t + 1 < nt;
      if (more) st.load<VEC>(src, ld, t_beg + (t + 1) * kB, t_end, u);
      const unsigned short* As = smem + (t & 1) * kBuf;
      tile_mfma<T, 2>(acc, As, As + kB * kStr, wm, wn, li, lg);
      if (more) st.store(smem + ((t + 1) & 1) * kBuf + image, u);
      __syncthreads();
    }
  }
  if constexpr (PARTIAL) {
    float* P = g.P + ((long)s * g.nnz + p) * (kB * kB);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = wm * 32 + i * 16 + li;
#pragma unroll
      for (int j = 0; j < 2; ++j) *reinterpret_cast<f32x4*>(P + r * kB + wn * 32 + 8 * lg + 4 * j) = acc[i][j];
    }
  } else {
    store_acc<T, 2, true>(acc, g.out + e * (kB * kB), kB, 0, kB, wm, wn, li, lg);
  }
}

// dvalues[e] = rne_T((((P[0][p] + P[1][p]) + P[2][p]) + …)), four adjacent columns per thread
template <class T>
__global__ __launch_bounds__(256) void bsr_wgrad_combine_kernel(const float* __restrict__ P, int S, long nnz, const int32_t* id,
                                                                long nvalues, uint16_t* __restrict__ out) {
  const long idx = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (idx >= nnz * (kB * kB)) return;
  const long p = idx / (kB * kB);
  const long e = id ? (long)id[p] : p;
  if (e < 0 || e >= nvalues) return;
  f32x4 t = *reinterpret_cast<const f32x4*>(P + idx);
  for (int s = 1; s < S; ++s) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(P + (long)s * nnz * (kB * kB) + idx);
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = __fadd_rn(t[k], v[k]);
  }
  *reinterpret_cast<uint2*>(out + e * (kB * kB) + (idx - p * (kB * kB))) = uint2{pack2<T>(t[0], t[1]), pack2<T>(t[2], t[3])};
}

template <class T, bool TRANS_W, int BM, bool BIAS>
int launch_linear(const LinArgs& g, bool vec, hipStream_t s) {
  const long tiles = (long)g.own_blocks * ((g.tokens + BM - 1) / BM);
  if (tiles > 0x7fffffffL) return MI_ERANGE;
  const dim3 grid((unsigned)tiles);
  if (vec)
    hipLaunchKernelGGL((bsr_linear_kernel<T, TRANS_W, BM, BIAS, true>), grid, dim3(256), 0, s, g);
  else
    hipLaunchKernelGGL((bsr_linear_kernel<T, TRANS_W, BM, BIAS, false>), grid, dim3(256), 0, s, g);
  return mi::check_launch();
}

// The token tile: 128 while that fills the chip, else 64 (and always for T ≤ 64) — by the shape only, same bits either way.
// mi_bsr_linear_tile_tokens is the rule, so that a caller can ask which one a shape takes.
template <class T, bool TRANS_W, bool BIAS>
int pick_linear(const LinArgs& g, bool vec, hipStream_t s) {
  if (mi_bsr_linear_tile_tokens(g.own_blocks * kB, g.tokens) == 64) return launch_linear<T, TRANS_W, 64, BIAS>(g, vec, s);
  return launch_linear<T, TRANS_W, 128, BIAS>(g, vec, s);
}

template <class T>
int linear_entry(const int32_t* rowptr, const int32_t* col, const int32_t* entry_id, int64_t nnz, int32_t trans_w, int32_t tokens,
                 int32_t inner, int32_t outer, const uint16_t* values, int64_t nvalues, const uint16_t* X, int64_t ldx,
                 const uint16_t* bias, uint16_t* Y, int64_t ldy, hipStream_t s) {
  if (nnz < 0 || nvalues < 0 || tokens < 0 || inner < 0 || outer < 0) return MI_EINVAL;
  if (inner % kB != 0 || outer % kB != 0) return MI_EINVAL;
  if (ldx < inner || ldy < outer) return MI_EINVAL;
  if (nnz > 0x7fffffffLL || nvalues > 0x7fffffffLL) return MI_ERANGE;
  if (!entry_id && nvalues < nnz) return MI_EINVAL;
  if (tokens == 0 || outer == 0) return MI_OK;
  if (!rowptr || !Y || odd(Y) || odd(bias)) return MI_EINVAL;
  if (nnz > 0 && (!col || !values || !X || inner == 0 || !mi::aligned16(values) || odd(X))) return MI_EINVAL;
  if (ldx > 0x7fffffffL || ldy > 0x7fffffffL) return MI_ERANGE;
  const bool vec = mi::aligned16(X) && mi::aligned16(Y) && mi::aligned16(bias) && ldx % 8 == 0 && ldy % 8 == 0;
  LinArgs g = {};
  g.rowptr = rowptr, g.col = col, g.id = entry_id, g.nnz = nnz, g.nvalues = nvalues, g.values = values, g.X = X, g.bias = bias;
  g.Y = Y, g.own_blocks = outer / kB, g.inner_blocks = inner / kB, g.tokens = tokens, g.ldx = ldx, g.ldy = ldy;
  if (trans_w) return bias ? pick_linear<T, true, true>(g, vec, s) : pick_linear<T, true, false>(g, vec, s);
  return bias ? pick_linear<T, false, true>(g, vec, s) : pick_linear<T, false, false>(g, vec, s);
}

size_t wgrad_bytes(int64_t nnz, int32_t S) { return S > 1 && nnz > 0 ? (size_t)S * (size_t)nnz * kB * kB * sizeof(float) : 0; }

template <class T>
int wgrad_entry(const int32_t* entry_row, const int32_t* col, const int32_t* entry_id, int64_t nnz, int32_t tokens, int32_t out,
                int32_t in, const uint16_t* dY, int64_t lddy, const uint16_t* X, int64_t ldx, uint16_t* dvalues, int64_t nvalues,
                int32_t splits, void* workspace, size_t workspace_bytes, hipStream_t s) {
  if (nnz < 0 || nvalues < 0 || tokens < 0 || out < 0 || in < 0 || splits < 0) return MI_EINVAL;
  if (out % kB != 0 || in % kB != 0) return MI_EINVAL;
  if (lddy < out || ldx < in) return MI_EINVAL;
  if (nnz > 0x7fffffffLL || nvalues > 0x7fffffffLL) return MI_ERANGE;
  if (!entry_id && nvalues < nnz) return MI_EINVAL;
  int S = splits ? splits : mi_bsr_wgrad_split_count(nnz, tokens);
  if (S > 1 && (S > 65535 || tokens % (32 * (long)S) != 0)) return MI_EINVAL;
  if (nnz == 0) return MI_OK;
  if (!entry_row || !col || !dvalues || !mi::aligned16(dvalues)) return MI_EINVAL;
  if (out == 0 || in == 0) return MI_EINVAL;  // entries on an empty grid
  if (tokens > 0 && (!dY || !X || odd(dY) || odd(X))) return MI_EINVAL;
  if (lddy > 0x7fffffffL || ldx > 0x7fffffffL) return MI_ERANGE;
  if (tokens == 0) S = 1;  // nothing to cut: the blocks are +0
  if (S > 1) {
    if (!workspace || !mi::aligned16(workspace)) return MI_EINVAL;
    if (workspace_bytes < wgrad_bytes(nnz, S)) return MI_ENOMEM;  // never silently unsplit: the order is part of the result
  }
  const bool vec = mi::aligned16(dY) && mi::aligned16(X) && lddy % 8 == 0 && ldx % 8 == 0;
  WgradArgs g = {};
  g.row = entry_row, g.col = col, g.id = entry_id, g.nnz = nnz, g.nvalues = nvalues, g.G = dY, g.X = X, g.out = dvalues;
  g.P = static_cast<float*>(workspace), g.out_blocks = out / kB, g.in_blocks = in / kB, g.tokens = tokens;
  g.range = S > 1 ? tokens / S : tokens, g.ldg = lddy, g.ldx = ldx;
  const dim3 grid((unsigned)nnz, (unsigned)S);
  if (S == 1) {
    if (vec)
      hipLaunchKernelGGL((bsr_wgrad_kernel<T, true, false>), grid, dim3(256), 0, s, g);
    else
      hipLaunchKernelGGL((bsr_wgrad_kernel<T, false, false>), grid, dim3(256), 0, s, g);
    return mi::check_launch();
  }
  if (vec)
    hipLaunchKernelGGL((bsr_wgrad_kernel<T, true, true>), grid, dim3(256), 0, s, g);
  else
    hipLaunchKernelGGL((bsr_wgrad_kernel<T, false, true>), grid, dim3(256), 0, s, g);
  const int st = mi::check_launch();
  if (st != MI_OK) return st;
  const long blocks = (nnz * (kB * kB / 4) + 255) / 256;
  if (blocks > 0x7fffffffL) return MI_ERANGE;
  hipLaunchKernelGGL((bsr_wgrad_combine_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, s, g.P, S, (long)nnz, entry_id,
                     (long)nvalues, dvalues);
  return mi::check_launch();
}

}  // namespace

extern "C" {

#define MI_BSR_LINEAR_ARGS                                                                                                      \
  const int32_t *rowptr, const int32_t *col, const int32_t *entry_id, int64_t nnz, int32_t trans_w, int32_t tokens, int32_t inner, \
      int32_t outer, const uint16_t *values, int64_t nvalues, const uint16_t *X, int64_t ldx, const uint16_t *bias, uint16_t *Y, \
      int64_t ldy, mi_stream_t stream
#define MI_BSR_LINEAR_PASS rowptr, col, entry_id, nnz, trans_w, tokens, inner, outer, values, nvalues, X, ldx, bias, Y, ldy

int mi_bsr_linear_bf16(MI_BSR_LINEAR_ARGS) { return linear_entry<Bf16>(MI_BSR_LINEAR_PASS, static_cast<hipStream_t>(stream)); }
int mi_bsr_linear_f16(MI_BSR_LINEAR_ARGS) { return linear_entry<F16>(MI_BSR_LINEAR_PASS, static_cast<hipStream_t>(stream)); }

#define MI_BSR_WGRAD_ARGS                                                                                                    \
  const int32_t *entry_row, const int32_t *col, const int32_t *entry_id, int64_t nnz, int32_t tokens, int32_t out, int32_t in, \
      const uint16_t *dY, int64_t lddy, const uint16_t *X, int64_t ldx, uint16_t *dvalues, int64_t nvalues, int32_t splits,  \
      void *workspace, size_t workspace_bytes, mi_stream_t stream
#define MI_BSR_WGRAD_PASS \
  entry_row, col, entry_id, nnz, tokens, out, in, dY, lddy, X, ldx, dvalues, nvalues, splits, workspace, workspace_bytes

int mi_bsr_wgrad_bf16(MI_BSR_WGRAD_ARGS) { return wgrad_entry<Bf16>(MI_BSR_WGRAD_PASS, static_cast<hipStream_t>(stream)); }
int mi_bsr_wgrad_f16(MI_BSR_WGRAD_ARGS) { return wgrad_entry<F16>(MI_BSR_WGRAD_PASS, static_cast<hipStream_t>(stream)); }

// The token tile of mi_bsr_linear_T — a function of the shape alone (columns of Y, tokens): 128 when tokens > 64 and the
// 64-column blocks of Y × 128-token tiles number at least 512, else 64.  The bits of the product do not depend on it.
int mi_bsr_linear_tile_tokens(int32_t outer, int32_t tokens) {
  if (outer <= 0 || tokens <= 64) return 64;
  const long wide = (long)(outer / kB) * (((long)tokens + 127) / 128);
  return wide < 512 ? 64 : 128;
}

// How many ranges the tokens are cut into — a function of (kept blocks, tokens) alone: the rule of
// mi_gemm_lowp_split_count with the kept blocks in the place of the output tiles and the two constants fitted for this
// kernel's 64 × 64 tiles (1024 workgroups targeted, 512 tokens at least per range).  1: no split.
//   S = the largest power of two ≤ min(kTarget / nnz, tokens / kMinRange, 32), halved until tokens % (32·S) == 0.
int mi_bsr_wgrad_split_count(int64_t nnz, int64_t tokens) {
  constexpr long kSplitMinTokens = 2048, kSplitTarget = 1024, kSplitMinRange = 512;
  if (nnz <= 0 || tokens < kSplitMinTokens) return 1;
  long cap = kSplitTarget / nnz;
  if (cap > tokens / kSplitMinRange) cap = tokens / kSplitMinRange;
  if (cap > 32) cap = 32;
  int S = 1;
  while (2L * S <= cap) S *= 2;
  while (S > 1 && tokens % (32L * S) != 0) S /= 2;
  return S;
}

size_t mi_bsr_wgrad_workspace_bytes(int64_t nnz, int32_t splits) { return wgrad_bytes(nnz, splits); }

}  // extern "C"
