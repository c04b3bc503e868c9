// CSR × dense in bfloat16 and float16: values, B and C in T ∈ {bf16, fp16}, every sum in fp32.
//
// What it computes (contract of include/mi_spmm.h, mi_spmm_csr_ex_bf16 / _f16):
//   C = rne_T(C32),  C32 = what mi_spmm_csr_ex_f32 writes for the widened values and B with MI_LONG_ROWS_SPLIT
// — the fp32 kernels' arithmetic on exactly widened inputs, narrowed ONCE at the store:
//  * rows of at most kLongRow (8192) entries: one fmaf chain per output element in CSR order, from +0;
//  * longer rows: listed by the main kernel (long_list_append) and summed by the follow-up launch of this file in the
//    split order of spmm_long.hip (16·S chains over 1024-entry chunks, groups of 16 added in order, S groups in order),
//    the partial rows in fp32 in the caller's workspace;
//  * N < 4: 64 lane-strided chains and the xor-butterfly 32 … 1 of spmm_narrow_kernel (never split).
// The SDDMM (gradient of the values) and the 2-byte value gather of the backward live here too.
//
// Bytes: the product is a gather of B rows, so it moves nnz·(2N + 6) + 4(M + 1) + 2MN bytes against the fp32 form's
// nnz·(4N + 8) + 4(M + 1) + 4MN — half, at the wide widths.  The kernels are the fp32 ones' shapes with 2-byte
// elements: a lane owns 4 columns (one 8-byte load per gather), and the wide form keeps twice the gathers in flight
// (U = 16 at N = 256: 16 × 512 B per wave, the fp32 kernel's 8 × 1 KiB).
// No float atomics; no host read-back (graph-capturable).  Nothing here is shared with the fp32 plans.
#include "lowp_device.h"
#include "spmm_device.h"
#include "spmm_internal.h"

namespace {

using mi::f32x4;
using mi::LongArg;

// The mean's epilogue (MEAN instantiations only): the fp32 sum divided by the row's entry count, correctly rounded
// (mi_spmm_rows_divide_f32's division), before the one narrowing of the store.  A row without entries keeps its +0.
__device__ __forceinline__ float mean_of(float sum, int cnt) { return cnt > 0 ? __fdiv_rn(sum, (float)cnt) : sum; }
__device__ __forceinline__ f32x4 mean_of(f32x4 sum, int cnt) {
  return f32x4{mean_of(sum.x, cnt), mean_of(sum.y, cnt), mean_of(sum.z, cnt), mean_of(sum.w, cnt)};
}

// ---------------------------------------------------------------------------
// Wide rows: one wave per row, N == 256·TT, B and C 8-byte aligned with ldb, ldc multiples of 4.  col / val are
// wave-uniform (scalar unit); lane l owns columns 256t + 4l … +3.  U gathers of TT·512 B are issued before the first
// FMA consumes one; the last < U entries go as one guarded batch (loads together, FMAs in entry order).
// grid = ⌈M/4⌉, block = 256.
// ---------------------------------------------------------------------------
template <class T, int TT, int U, bool MEAN = false>
__global__ __launch_bounds__(256) void lowp_wave_row_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                            const unsigned short* __restrict__ val,
                                                            const unsigned short* __restrict__ B, unsigned short* __restrict__ C,
                                                            int M, long ldb, long ldc, LongArg la) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (row >= M) return;
  int p = rowptr[row];
  const int end = rowptr[row + 1];
  const int cnt = end - p;
  if (end - p > la.thresh) {  // left to the follow-up launch
    if (lane == 0) long_list_append(la, (int)row, end - p);
    return;
  }
  const unsigned short* Bl = B + lane * 4;
  f32x4 acc[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (; p + U <= end; p += U) {
    float v[U];
    f32x4 x[U][TT];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      v[u] = up<T>(val[p + u]);
      const unsigned short* src = Bl + (long)col[p + u] * ldb;
#pragma unroll
      for (int t = 0; t < TT; ++t) x[u][t] = load4<T, true>(src + t * 256, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int t = 0; t < TT; ++t) acc[t] = fma4(v[u], x[u][t], acc[t]);
  }
  const int rem = end - p;  // 0 … U-1, wave-uniform
  if (rem > 0) {
    float v[U];
    f32x4 x[U][TT];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u < rem) {
        v[u] = up<T>(val[p + u]);
        const unsigned short* src = Bl + (long)col[p + u] * ldb;
#pragma unroll
        for (int t = 0; t < TT; ++t) x[u][t] = load4<T, true>(src + t * 256, 0, 0);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (u < rem)
#pragma unroll
        for (int t = 0; t < TT; ++t) acc[t] = fma4(v[u], x[u][t], acc[t]);
  }
  unsigned short* Cl = C + row * ldc + lane * 4;
#pragma unroll
  for (int t = 0; t < TT; ++t) store4<T, true>(Cl + t * 256, 0, 0, MEAN ? mean_of(acc[t], cnt) : acc[t]);
}

// ---------------------------------------------------------------------------
// Every other N ≥ 4: G lanes per row (a power of two ≤ 64), 64/G rows per wave, 4 columns per lane and tile, TT tiles
// per pass, wider rows in passes (col / val re-read once per pass).  A chunk of EPC entries is loaded one entry per lane
// (EPC / G registers per lane when G < 8) and handed round the group by compile-time lane broadcasts (mi_lanes.h);
// 8 gathers per lane in flight.  VEC: 8-byte loads and stores (N, ldb, ldc multiples of 4, B and C 8-byte aligned);
// otherwise 2-byte elements at any alignment and any ldb (offset views, odd leading dimensions).
// grid = ⌈M / (4·64/G)⌉, block = 256.
// ---------------------------------------------------------------------------
template <class T, int G, int TT, bool VEC, bool MEAN = false>
__global__ __launch_bounds__(256) void lowp_group_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                         const unsigned short* __restrict__ val,
                                                         const unsigned short* __restrict__ B, unsigned short* __restrict__ C,
                                                         int M, int N, long ldb, long ldc, LongArg la) {
  constexpr int RPW = 64 / G;
  constexpr int EPC = G < 8 ? 8 : G;  // entries per chunk
  constexpr int CHK = EPC / G;        // chunk registers per lane
  constexpr int UI = 8;               // gathers in flight per lane and tile
  const int lane = threadIdx.x & 63;
  const int gl = lane & (G - 1);
  const long row = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW + lane / G;
  const bool live = row < M;
  int start = 0, end = 0;
  if (live) {
    start = rowptr[row];
    end = rowptr[row + 1];
  }
  const bool skipped = end - start > la.thresh;  // left to the follow-up launch
  if (skipped) {
    if (gl == 0) long_list_append(la, (int)row, end - start);
    end = start;
  }
  for (int n0 = 0; n0 < N; n0 += G * 4 * TT) {  // wave-uniform pass loop
    f32x4 acc[TT];
    int coff[TT];
    bool on[TT];
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      coff[t] = n0 + (t * G + gl) * 4;
      on[t] = coff[t] < N;
    }
    for (int p = start; p < end; p += EPC) {  // trip count differs between groups, not inside one
      int myc[CHK];
      float myv[CHK];
#pragma unroll
      for (int k = 0; k < CHK; ++k) {
        const int idx = p + k * G + gl;
        myc[k] = idx < end ? col[idx] : 0;
        myv[k] = idx < end ? up<T>(val[idx]) : 0.f;
      }
      const int cnt = end - p < EPC ? end - p : EPC;  // group-uniform
      mi::static_for<EPC / UI>([&](auto b_) {
        constexpr int b = UI * decltype(b_)::value;
        if (b < cnt) {
          float v[UI];
          f32x4 x[UI][TT];
          mi::static_for<UI>([&](auto u_) {
            constexpr int e = b + decltype(u_)::value;
            const int c = mi::group_lane<G, e % G, false>(myc[e / G]);
            v[e - b] = mi::group_lane<G, e % G, false>(myv[e / G]);
            if (e < cnt) {
              const unsigned short* src = B + (long)c * ldb;
#pragma unroll
              for (int t = 0; t < TT; ++t)
                if (on[t]) x[e - b][t] = load4<T, VEC>(src + coff[t], coff[t], N);
            }
          });
#pragma unroll
          for (int u = 0; u < UI; ++u)
            if (b + u < cnt)
#pragma unroll
              for (int t = 0; t < TT; ++t)
                if (on[t]) acc[t] = fma4(v[u], x[u][t], acc[t]);
        }
      });
    }
    if (live && !skipped) {
      unsigned short* dst = C + row * ldc;
#pragma unroll
      for (int t = 0; t < TT; ++t)
        if (on[t]) store4<T, VEC>(dst + coff[t], coff[t], N, MEAN ? mean_of(acc[t], end - start) : acc[t]);
    }
  }
}

// ---------------------------------------------------------------------------
// N < 4: one wave per row, lane l chains the entries l, l+64, …, the 64 partial sums added by the xor-butterfly
// 32, 16, …, 1 — spmm_narrow_kernel's order, for every row length.  grid = ⌈M/4⌉.
// ---------------------------------------------------------------------------
template <class T, bool MEAN = false>
__global__ __launch_bounds__(256) void lowp_narrow_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                          const unsigned short* __restrict__ val,
                                                          const unsigned short* __restrict__ B, unsigned short* __restrict__ C,
                                                          int M, int N, long ldb, long ldc) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int start = rowptr[row], end = rowptr[row + 1];
  float acc[3] = {0.f, 0.f, 0.f};
  for (int p = start + lane; p < end; p += 64) {
    const float v = up<T>(val[p]);
    const unsigned short* brow = B + (long)col[p] * ldb;
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (j < N) acc[j] = __builtin_fmaf(v, up<T>(brow[j]), acc[j]);
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    if (j < N) {
      float s = acc[j];
#pragma unroll
      for (int w = 32; w >= 1; w >>= 1) s += __shfl_xor(s, w, 64);
      if (lane == 0) C[row * ldc + j] = T::down(MEAN ? mean_of(s, end - start) : s);
    }
  }
}

// ---------------------------------------------------------------------------
// The follow-up launch: rows beyond the threshold, listed by the main kernel in the workspace layout of spmm_long.hip
// (mi::long_ws_layout; entries {row, slot base, S, partial base, arrivals}, slot → entry map, fp32 partial rows).
// Slot s = group g of its row's S groups; a 16-wave workgroup takes one slot at a time (grid-stride).  Wave w runs
// chain q = 16g + w over the chunks q, q + 16S, … (1024 entries each, in increasing position) for 256 columns at a time,
// 8 gathers in flight; the 16 chains meet in LDS and are added in order w = 0 … 15.  S == 1: that sum is the row, narrowed
// and stored.  S > 1: the group sum goes to its fp32 partial row; the last of the row's S workgroups to arrive
// (agent-scope release by every deliverer, acquire by the last) adds the partial rows in order g = 0 … S-1 and stores.
// The last workgroup of the launch resets the four counters (the workspace leaves with a zero header).
// ---------------------------------------------------------------------------
struct LowpLongWs {
  int cap_e, cap_s;
  long owner_off;    // ints
  long partial_off;  // bytes
};

template <class T, bool VEC, bool MEAN = false>
__global__ __launch_bounds__(1024) void lowp_long_rows_kernel(int* __restrict__ ws, LowpLongWs lw,
                                                              const int* __restrict__ rowptr, const int* __restrict__ col,
                                                              const unsigned short* __restrict__ val,
                                                              const unsigned short* __restrict__ B,
                                                              unsigned short* __restrict__ C, int N, long ldb, long ldc) {
  __shared__ __attribute__((aligned(16))) float red[kLongWaves][256];
  __shared__ int last_arrival;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nent = min(ws[0], lw.cap_e);
  const int nslots = min(ws[1], lw.cap_s);
  const int* owner = ws + lw.owner_off;
  float* partial = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + lw.partial_off);
  for (int s = blockIdx.x; s < nslots; s += gridDim.x) {
    const int e = owner[s];
    if (e < 0 || e >= nent) continue;
    int* ent = ws + 4 + kLongEnt * (long)e;
    const int row = ent[0], sb = ent[1], S = ent[2], pb = ent[3];
    if (S <= 0 || s - sb < 0 || s - sb >= S) continue;  // an entry that did not fit its caps
    const int g = s - sb;
    const int start = rowptr[row], end = rowptr[row + 1];
    const long stride = (long)kLongWaves * S * kLongChunk;
    for (int n0 = 0; n0 < N; n0 += 256) {
      const int j = n0 + 4 * lane;
      const bool on = j < N;
      const bool vec = VEC && j + 4 <= N;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (long cb = start + ((long)g * kLongWaves + w) * kLongChunk; cb < end; cb += stride) {
        const int ce = cb + kLongChunk < end ? (int)(cb + kLongChunk) : end;
        for (int p = (int)cb; p < ce; p += 8) {
          const int rem = ce - p;  // wave-uniform
          float v[8];
          f32x4 x[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            if (u < rem) {
              v[u] = up<T>(val[p + u]);
              const unsigned short* src = B + (long)col[p + u] * ldb + j;
              if (on) x[u] = vec ? load4<T, true>(src, j, N) : load4<T, false>(src, j, N);
            }
          }
#pragma unroll
          for (int u = 0; u < 8; ++u)
            if (u < rem && on) acc = fma4(v[u], x[u], acc);
        }
      }
      *reinterpret_cast<f32x4*>(&red[w][4 * lane]) = acc;
      __syncthreads();
      if (tid < 256 && n0 + tid < N) {
        float sum = red[0][tid];
#pragma unroll
        for (int q = 1; q < kLongWaves; ++q) sum += red[q][tid];
        if (S == 1) C[(long)row * ldc + n0 + tid] = T::down(MEAN ? mean_of(sum, end - start) : sum);
        else partial[(long)(pb + g) * N + n0 + tid] = sum;
      }
      __syncthreads();
    }
    if (S > 1) {
      __threadfence();  // release this workgroup's partial row
      __syncthreads();
      if (tid == 0) {
        const int before = __hip_atomic_fetch_add(&ent[4], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        last_arrival = before == S - 1;
        if (last_arrival) __threadfence();  // acquire the others'
      }
      __syncthreads();
      if (last_arrival) {
        for (int c = tid; c < N; c += blockDim.x) {
          const float* pr = partial + (long)pb * N + c;
          float tot = __builtin_nontemporal_load(pr);
          for (int q = 1; q < S; ++q) tot += __builtin_nontemporal_load(pr + (long)q * N);
          C[(long)row * ldc + c] = T::down(MEAN ? mean_of(tot, end - start) : tot);
        }
      }
      __syncthreads();
    }
  }
  // every workgroup has read the counters above: the last one to finish zeroes them
  __syncthreads();
  if (tid == 0) {
    const int done = __hip_atomic_fetch_add(&ws[3], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (done == (int)gridDim.x - 1) {
      ws[0] = 0;
      ws[1] = 0;
      ws[2] = 0;
      ws[3] = 0;
    }
  }
}

// ---------------------------------------------------------------------------
// SDDMM on T-typed dC and B:  out[p] = rne_T(Σ_j dC[row(p), j] · B[col[p], j]), the sum in sddmm_kernel's order
// (convert.hip; oracle_sddmm_csr_f32): lane l chains columns 256t + 4l + c (t ascending, c = 0 … 3, j < N) with fmaf,
// the 64 lane sums added by the xor tree 32, 16, …, 1.  One wave per row of A; the row's entries 64 at a time, 8 gathers
// in flight; the 64 × 64 partial sums of a batch go through ONE joint tree (level w: lanes with bit w set keep the upper
// half of the remaining values — each level pairs exactly what the butterfly pairs), lane i ends with entry i.
// ---------------------------------------------------------------------------
template <class T, bool VEC>
__global__ __launch_bounds__(256) void lowp_sddmm_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, int M,
                                                         int N, const unsigned short* __restrict__ dC, long lddc,
                                                         const unsigned short* __restrict__ B, long ldb,
                                                         unsigned short* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (row >= M) return;
  const int start = rowptr[row], end = rowptr[row + 1];
  if (start == end) return;
  constexpr int U = 8;
  const unsigned short* xrow = dC + row * lddc;
  for (int p0 = start; p0 < end; p0 += 64) {
    const int cnt = end - p0 < 64 ? end - p0 : 64;
    const int mycol = lane < cnt ? col[p0 + lane] : 0;
    float s[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) s[i] = 0.f;
    for (int t0 = 0; 256 * t0 < N; ++t0) {  // 256 columns at a time: each lane's chain simply continues
      const int j = 256 * t0 + 4 * lane;
      const bool on = j < N;
      const f32x4 x = on ? load4<T, VEC>(xrow + j, j, N) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 64; i += U) {
        if (i < cnt) {
          f32x4 y[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const unsigned short* brow = B + (long)__builtin_amdgcn_readlane(mycol, i + u) * ldb;  // row 0 past cnt
            y[u] = on ? load4<T, VEC>(brow + j, j, N) : f32x4{0.f, 0.f, 0.f, 0.f};
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            float acc = s[i + u];
            // columns at or beyond N are not part of the chain (their +0 would turn a −0 sum into +0)
            if (j + 0 < N) acc = __builtin_fmaf(x.x, y[u].x, acc);
            if (j + 1 < N) acc = __builtin_fmaf(x.y, y[u].y, acc);
            if (j + 2 < N) acc = __builtin_fmaf(x.z, y[u].z, acc);
            if (j + 3 < N) acc = __builtin_fmaf(x.w, y[u].w, acc);
            s[i + u] = acc;
          }
        }
      }
    }
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
      const bool hi = (lane & w) != 0;
#pragma unroll
      for (int k = 0; k < w; ++k) {
        const float keep = hi ? s[k + w] : s[k];
        const float send = hi ? s[k] : s[k + w];
        s[k] = keep + __shfl_xor(send, w, 64);
      }
    }
    if (lane < cnt) out[p0 + lane] = T::down(s[0]);
  }
}

// dst[p] = src[perm[p]] for 2-byte values: four entries per lane (16-byte perm loads, 8-byte stores where aligned).
template <bool VEC>
__global__ __launch_bounds__(256) void gather_b16_kernel(const unsigned short* __restrict__ src, const int* __restrict__ perm,
                                                         long n, unsigned short* __restrict__ dst) {
  const long p = 4 * ((long)blockIdx.x * 256 + threadIdx.x);
  if (p >= n) return;
  if (VEC && p + 4 <= n) {
    const int4 q = *reinterpret_cast<const int4*>(perm + p);
    const u32x2 w = {(unsigned)src[q.x] | ((unsigned)src[q.y] << 16), (unsigned)src[q.z] | ((unsigned)src[q.w] << 16)};
    *reinterpret_cast<u32x2*>(dst + p) = w;
  } else {
    for (long i = p; i < n && i < p + 4; ++i) dst[i] = src[perm[i]];
  }
}

template <class T, int G, int TT, bool VEC, bool MEAN>
int launch_group(const int* rowptr, const int* col, const unsigned short* val, const unsigned short* B, unsigned short* C,
                 int M, int N, long ldb, long ldc, const LongArg& la, hipStream_t s) {
  constexpr int rows_per_block = 4 * (64 / G);
  const long blocks = ((long)M + rows_per_block - 1) / rows_per_block;
  if (blocks > 0x7fffffffL) return MI_ERANGE;
  hipLaunchKernelGGL((lowp_group_kernel<T, G, TT, VEC, MEAN>), dim3((unsigned)blocks), dim3(256), 0, s, rowptr, col, val, B, C, M,
                     N, ldb, ldc, la);
  return mi::check_launch();
}

template <class T, bool VEC, bool MEAN>
int dispatch_group(const int* rowptr, const int* col, const unsigned short* val, const unsigned short* B, unsigned short* C,
                   int M, int N, long ldb, long ldc, const LongArg& la, hipStream_t s) {
  const int nq = (N + 3) / 4;  // column quads
  const int G = nq >= 64 ? 64 : mi::pow2_ceil(nq);
#define MI_LOWP_GROUP(G_, TT_) return launch_group<T, G_, TT_, VEC, MEAN>(rowptr, col, val, B, C, M, N, ldb, ldc, la, s)
  switch (G) {
    case 1: MI_LOWP_GROUP(1, 1);
    case 2: MI_LOWP_GROUP(2, 1);
    case 4: MI_LOWP_GROUP(4, 1);
    case 8: MI_LOWP_GROUP(8, 1);
    case 16: MI_LOWP_GROUP(16, 1);
    case 32: MI_LOWP_GROUP(32, 1);
    default: break;
  }
  const int tiles = (nq + 63) / 64;
  if (tiles <= 1) MI_LOWP_GROUP(64, 1);
  if (tiles == 2) MI_LOWP_GROUP(64, 2);
  MI_LOWP_GROUP(64, 4);
#undef MI_LOWP_GROUP
}

template <class T, bool MEAN = false>
int spmm_lowp(const int32_t* rowptr, const int32_t* col, const uint16_t* val, int64_t nnz, int32_t M, int32_t K, int32_t N,
              const uint16_t* B, int64_t ldb, uint16_t* C, int64_t ldc, int long_rows, void* workspace,
              size_t workspace_bytes, hipStream_t s) {
  // every check before the first HIP call
  if (M < 0 || K < 0 || N < 0 || nnz < 0) return MI_EINVAL;
  if (long_rows != MI_LONG_ROWS_AUTO && long_rows != MI_LONG_ROWS_NONE && long_rows != MI_LONG_ROWS_SPLIT &&
      long_rows != MI_LONG_ROWS_AUTO_ZEROED)
    return MI_EINVAL;  // (MI_LONG_ROWS_PREPARED: no inspector handles on this path)
  if (ldb < N || ldc < N) return MI_EINVAL;
  if (nnz > 0x7fffffffLL) return MI_ERANGE;
  if (M == 0 || N == 0) return MI_OK;
  if (!rowptr || !C) return MI_EINVAL;
  if (nnz > 0 && (!col || !val || !B)) return MI_EINVAL;
  if ((reinterpret_cast<uintptr_t>(C) & 1u) || (reinterpret_cast<uintptr_t>(B) & 1u)) return MI_EINVAL;
  // AUTO / AUTO_ZEROED mean SPLIT here, whatever the fp32 plan would be (N < 4 keeps the narrow order: never split)
  const bool split = N >= 4 && nnz > kLongRow && long_rows != MI_LONG_ROWS_NONE;
  const mi::LongWs lw = mi::long_ws_layout(nnz, N);
  if (split) {
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u) != 0) return MI_EINVAL;
    if (workspace_bytes < lw.bytes) return MI_ENOMEM;
  }
  if (N < 4) {
    const long blocks = ((long)M + 3) / 4;
    if (blocks > 0x7fffffffL) return MI_ERANGE;
    hipLaunchKernelGGL((lowp_narrow_kernel<T, MEAN>), dim3((unsigned)blocks), dim3(256), 0, s, rowptr, col, val, B, C, M, N, (long)ldb,
                       (long)ldc);
    return mi::check_launch();
  }
  int* ws = static_cast<int*>(workspace);
  LongArg la = {0x7fffffff, 0, 0, 0, nullptr, nullptr, nullptr, 0};
  if (split) {
    if (long_rows != MI_LONG_ROWS_AUTO_ZEROED) MI_HIP_TRY(hipMemsetAsync(ws, 0, 16, s));
    la.thresh = kLongRow;
    la.cap_e = (int)lw.cap_e, la.cap_s = (int)lw.cap_s, la.cap_p = (int)lw.cap_p;
    la.ws = ws;
  }
  const bool vec = N % 4 == 0 && ldb % 4 == 0 && ldc % 4 == 0 && aligned8(B) && aligned8(C);
  int st;
  if (vec && (N == 256 || N == 512 || N == 1024)) {
    const long blocks = ((long)M + 3) / 4;
    if (blocks > 0x7fffffffL) return MI_ERANGE;
#define MI_LOWP_WAVE(TT_, U_)                                                                                          \
  hipLaunchKernelGGL((lowp_wave_row_kernel<T, TT_, U_, MEAN>), dim3((unsigned)blocks), dim3(256), 0, s, rowptr, col, val, B, C, M, \
                     (long)ldb, (long)ldc, la)
    if (N == 256) MI_LOWP_WAVE(1, 16);
    else if (N == 512) MI_LOWP_WAVE(2, 8);
    else MI_LOWP_WAVE(4, 4);
#undef MI_LOWP_WAVE
    st = mi::check_launch();
  } else if (vec) {
    st = dispatch_group<T, true, MEAN>(rowptr, col, val, B, C, M, N, ldb, ldc, la, s);
  } else {
    st = dispatch_group<T, false, MEAN>(rowptr, col, val, B, C, M, N, ldb, ldc, la, s);
  }
  if (st != MI_OK || !split) return st;
  // one follow-up launch: sums the listed rows (or finds none) and resets the counters
  const LowpLongWs lws = {(int)lw.cap_e, (int)lw.cap_s, (long)lw.owner_off, (long)lw.partial_off};
  const unsigned grid = (unsigned)(lw.cap_s < 512 ? lw.cap_s : 512);
  const bool lvec = ldb % 4 == 0 && aligned8(B);
  if (lvec)
    hipLaunchKernelGGL((lowp_long_rows_kernel<T, true, MEAN>), dim3(grid), dim3(1024), 0, s, ws, lws, rowptr, col, val, B, C, N,
                       (long)ldb, (long)ldc);
  else
    hipLaunchKernelGGL((lowp_long_rows_kernel<T, false, MEAN>), dim3(grid), dim3(1024), 0, s, ws, lws, rowptr, col, val, B, C, N,
                       (long)ldb, (long)ldc);
  return mi::check_launch();
}

template <class T>
int sddmm_lowp(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t M, int32_t K, int32_t N, const uint16_t* dC,
               int64_t lddc, const uint16_t* B, int64_t ldb, uint16_t* out, hipStream_t s) {
  if (M < 0 || N < 0 || K < 0 || nnz < 0) return MI_EINVAL;
  if (N > 0 && (lddc < N || ldb < N)) return MI_EINVAL;
  if (M == 0 || nnz == 0) return MI_OK;
  if (!rowptr || !col || !out) return MI_EINVAL;
  if (N > 0 && (!dC || !B)) return MI_EINVAL;
  if ((reinterpret_cast<uintptr_t>(dC) & 1u) || (reinterpret_cast<uintptr_t>(B) & 1u)) return MI_EINVAL;
  const long blocks = ((long)M + 3) / 4;
  if (blocks > 0x7fffffffL) return MI_ERANGE;
  const bool vec = N % 4 == 0 && lddc % 4 == 0 && ldb % 4 == 0 && aligned8(dC) && aligned8(B);
  if (vec)
    hipLaunchKernelGGL((lowp_sddmm_kernel<T, true>), dim3((unsigned)blocks), dim3(256), 0, s, rowptr, col, M, N, dC, (long)lddc,
                       B, (long)ldb, out);
  else
    hipLaunchKernelGGL((lowp_sddmm_kernel<T, false>), dim3((unsigned)blocks), dim3(256), 0, s, rowptr, col, M, N, dC,
                       (long)lddc, B, (long)ldb, out);
  return mi::check_launch();
}

}  // namespace

namespace mi {

int spmm_lowp_mean(bool bf16, const int32_t* rowptr, const int32_t* col, const uint16_t* val, int64_t nnz, int32_t M, int32_t K,
                   int32_t N, const uint16_t* B, int64_t ldb, uint16_t* C, int64_t ldc, int long_rows, void* workspace,
                   size_t workspace_bytes, hipStream_t s) {
  return bf16 ? spmm_lowp<Bf16, true>(rowptr, col, val, nnz, M, K, N, B, ldb, C, ldc, long_rows, workspace, workspace_bytes, s)
              : spmm_lowp<F16, true>(rowptr, col, val, nnz, M, K, N, B, ldb, C, ldc, long_rows, workspace, workspace_bytes, s);
}

}  // namespace mi

extern "C" {

int mi_spmm_csr_ex_bf16(const int32_t* rowptr, const int32_t* col, const uint16_t* val, int64_t nnz, int32_t M, int32_t K,
                        int32_t N, const uint16_t* B, int64_t ldb, uint16_t* C, int64_t ldc, int long_rows, void* workspace,
                        size_t workspace_bytes, mi_stream_t stream) {
  return spmm_lowp<Bf16>(rowptr, col, val, nnz, M, K, N, B, ldb, C, ldc, long_rows, workspace, workspace_bytes,
                         static_cast<hipStream_t>(stream));
}

int mi_spmm_csr_ex_f16(const int32_t* rowptr, const int32_t* col, const uint16_t* val, int64_t nnz, int32_t M, int32_t K,
                       int32_t N, const uint16_t* B, int64_t ldb, uint16_t* C, int64_t ldc, int long_rows, void* workspace,
                       size_t workspace_bytes, mi_stream_t stream) {
  return spmm_lowp<F16>(rowptr, col, val, nnz, M, K, N, B, ldb, C, ldc, long_rows, workspace, workspace_bytes,
                        static_cast<hipStream_t>(stream));
}

int mi_sddmm_csr_bf16(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t M, int32_t K, int32_t N,
                      const uint16_t* dC, int64_t lddc, const uint16_t* B, int64_t ldb, uint16_t* out_val, mi_stream_t stream) {
  return sddmm_lowp<Bf16>(rowptr, col, nnz, M, K, N, dC, lddc, B, ldb, out_val, static_cast<hipStream_t>(stream));
}

int mi_sddmm_csr_f16(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t M, int32_t K, int32_t N,
                     const uint16_t* dC, int64_t lddc, const uint16_t* B, int64_t ldb, uint16_t* out_val, mi_stream_t stream) {
  return sddmm_lowp<F16>(rowptr, col, nnz, M, K, N, dC, lddc, B, ldb, out_val, static_cast<hipStream_t>(stream));
}

int mi_gather_b16(const uint16_t* src, const int32_t* perm, int64_t n, uint16_t* dst, mi_stream_t stream) {
  if (n < 0) return MI_EINVAL;
  if (n == 0) return MI_OK;
  if (!src || !perm || !dst) return MI_EINVAL;
  const long quads = (n + 3) / 4;
  const long blocks = (quads + 255) / 256;
  if (blocks > 0x7fffffffL) return MI_ERANGE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mi::aligned16(perm) && aligned8(dst))
    hipLaunchKernelGGL(gather_b16_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, src, perm, (long)n, dst);
  else
    hipLaunchKernelGGL(gather_b16_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, src, perm, (long)n, dst);
  return mi::check_launch();
}

}  // extern "C"
