/*
 * mi_spmm.h — C-ABI of the MI355X (gfx950) SpMM hot path.
 *
 * This is the drop-in boundary below the `custom_mm` pybind module: plain
 * pointers, sizes and a HIP stream handle; no torch types.  Every entry point
 * enqueues work on `stream` and returns without synchronising.  Return value:
 * 0 (MI_OK) or a negative MI_E* code; `mi_status_string` names it and
 * `mi_last_hip_error` gives the hipError_t behind an MI_EHIP.
 *
 * Each entry cites the reference interface (relative to the reference repo
 * smoorjani/matrix-multiplication) it replaces.  All device pointers must be
 * valid for the sizes stated; index arrays are int32, values are float32 (bfloat16 / float16 in the
 * low-precision entries, which say so).
 */
#ifndef MI_SPMM_H_
#define MI_SPMM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_SPMM_ABI_VERSION 1

typedef void* mi_stream_t; /* a hipStream_t; NULL = the null stream */

enum {
  MI_OK = 0,
  MI_EINVAL = -1,   /* bad argument (null pointer, negative size, bad flag)   */
  MI_ERANGE = -2,   /* a size does not fit the 32-bit index math of the path  */
  MI_EHIP = -3,     /* a HIP runtime call / kernel launch failed              */
  MI_ENOMEM = -4,   /* workspace too small                                    */
  MI_EUNSORTED = -5 /* host inspector: COO rows not sorted (coo2csr contract) */
};

int mi_spmm_abi_version(void);
const char* mi_status_string(int status);
/* hipError_t (as int) recorded by the last MI_EHIP on this thread, else 0. */
int mi_last_hip_error(void);
const char* mi_last_hip_error_string(void);

/* ------------------------------------------------------------------------ *
 * K1 / B1 / B2 — C[M,N] = A_csr[M,K] · B[K,N], row-major B (ldb) and C (ldc).
 * Replaces  spmm_kernel<float,SUM,true> + naive_spmm_wrapper
 *           (src/naive_sparse_mm.cu:24-101, :104-136), reached from
 *           custom_mm.naive_spmm (src/custom_mm.cpp:166-179), and
 *           cusparse_mm_wrapper (src/baseline_mm.cu:167-216), reached from
 *           custom_mm.cusparse_mmul (src/custom_mm.cpp:203-217).
 * Per output element the products are accumulated with fused multiply-add in
 * CSR order (p = rowptr[r] … rowptr[r+1]-1), so the result does not depend on
 * the launch geometry.  Every element of C is written (zeros for empty rows).
 * Exception, N < 4 (SpMV-like): 64 lane-strided chains (lane l takes the row's
 * non-zeros l, l+64, …) combined by a xor-butterfly (32, 16, …, 1) — also a fixed,
 * launch-independent order, restated by the oracle.
 *
 * The `nnz` argument of every SpMM / SDDMM entry (nnz_total for the batched ones):
 *   rowptr's last entry  ≤  nnz  ≤  the number of entries `col` / `val` hold.
 * It picks the plan and sizes the long-row workspace; the kernels walk the rows through
 * rowptr and never read col / val at an index ≥ max(nnz, rowptr's last entry), so a CAPACITY (arrays
 * sized for every element of a dense operand, filled without a read-back) is a valid count
 * and gives the same bits as the exact one.  A count BELOW rowptr's last entry is outside
 * the contract wherever a long-row workspace is in use (its lists are sized from it); without
 * one (mi_spmm_csr_f32, MI_LONG_ROWS_NONE, the batched forms) it only steers the plan — the
 * 16-byte col / val loads of MI_SPMM_LDS_B take their clamp from max(nnz, rowptr's last entry),
 * read on the device.  It must never exceed the array length.
 * ------------------------------------------------------------------------ */
int mi_spmm_csr_f32(const int32_t* rowptr, const int32_t* col, const float* val,
                    int64_t nnz, int32_t M, int32_t K, int32_t N,
                    const float* B, int64_t ldb, float* C, int64_t ldc,
                    mi_stream_t stream);

/* Skew-robust form.  With a workspace of mi_spmm_csr_workspace_bytes(nnz, N) bytes (16-byte
 * aligned; ≈ nnz·N/8192 + nnz/400 bytes), rows with more than 8192 non-zeros are not left to a
 * single wave.  Such a row of `len` non-zeros is summed by S = clamp(len/32768, 1, 128) 16-wave
 * workgroups: its 1024-non-zero chunks are dealt round-robin to 16·S fmaf chains (chain q takes
 * chunks q, q+16S, …, in increasing position), workgroup g adds chains 16g … 16g+15 in that
 * order, and the S workgroup sums are added in order g = 0 … S-1 (then + bias).  The order
 * depends on the row length only.  Rows up to 8192 non-zeros keep the plain CSR-order chain, so
 * results equal mi_spmm_csr_f32 for them.  When the plan (mi_spmm_csr_f32_plan) is MI_SPMM_SLAB
 * or MI_SPMM_NARROW no row is split: every row keeps that plan's own order.  bias (N entries)
 * may be NULL.  This is what custom_mm.naive_spmm / cusparse_mmul call.
 * The workspace also lets the column-panel plans look at the MATRIX, not only at its shape (round 5): its last 64 bytes take
 * the verdicts of a probe launch — per window of 2048 rows, do the rows of B it gathers span ≤ 0.4 of B — that runs ahead of
 * the passes whenever B is below the Infinity-Cache regime (768 MiB); the panel kernels read them on the device, and on a
 * banded / block-diagonal matrix the first pass takes every column while the others return (one pass's chain: the same
 * bits; no read-back, capturable).  Without a workspace the passes always stay passes.  Reference: src/naive_sparse_mm.cu:24-136
 * is one kernel for any matrix; the plans and their adaptation are this library's. */
size_t mi_spmm_csr_workspace_bytes(int64_t nnz, int32_t N);
int mi_spmm_csr_ws_f32(const int32_t* rowptr, const int32_t* col, const float* val,
                       int64_t nnz, int32_t M, int32_t K, int32_t N, const float* B,
                       int64_t ldb, const float* bias, float* C, int64_t ldc,
                       void* workspace, size_t workspace_bytes, mi_stream_t stream);

/* The same product with the long-row rule pinned by the caller instead of following the plan:
 *   MI_LONG_ROWS_AUTO   what mi_spmm_csr_ws_f32 does (split unless the plan is SLAB / NARROW);
 *   MI_LONG_ROWS_NONE   every row keeps the plain CSR-order chain; workspace may be NULL — also the
 *                       cheap call when the caller knows no row exceeds mi_spmm_long_row_threshold()
 *                       non-zeros (one launch, no list building);
 *   MI_LONG_ROWS_SPLIT  rows beyond the threshold are always summed in the split order above, also
 *                       under the SLAB plan (workspace required).
 * A row shard of a larger matrix uses this to sum its rows exactly as the whole matrix would
 * (mi_spmm_auto_splits_long_rows on the WHOLE problem gives the rule), which keeps the
 * row-sharded multi-GPU result bit-identical to the single-GPU one (sharded.py).
 * No counterpart in the reference (single device, one wave per row: src/naive_sparse_mm.cu:24-101). */
/* MI_LONG_ROWS_PREPARED: as SPLIT, and the list of long rows in `workspace` was already built by
 * mi_spmm_long_rows_prepare for this matrix (same nnz and N): the per-call memset + list-building
 * launch are skipped — the inspector–executor form (custom_mm.cusparse_inspect / tiledspmm_inspect_*). */
/* MI_LONG_ROWS_AUTO_ZEROED: as AUTO, and the caller keeps the first 16 bytes of `workspace` ZERO between products:
 * they are zero on entry and zero again once the product's kernels have run (one workspace per stream, reused —
 * what custom_mm.naive_spmm / cusparse_mmul do).  Saves the per-product memset: a product is then exactly two
 * launches — the main kernel, which lists the rows it skips, and one follow-up that sums them (or finds none). */
enum { MI_LONG_ROWS_AUTO = -1, MI_LONG_ROWS_NONE = 0, MI_LONG_ROWS_SPLIT = 1, MI_LONG_ROWS_PREPARED = 2,
       MI_LONG_ROWS_AUTO_ZEROED = 3 };
/* Inspector step for MI_LONG_ROWS_PREPARED: lists the rows beyond the threshold once.  workspace ≥
 * mi_spmm_csr_workspace_bytes(nnz, N); it must stay untouched between the products that use it,
 * and products sharing one workspace must be ordered on one stream (the partial-row area is reused).
 * Replaces what TiledSpMM_inspect amortises in the reference (src/sparse_mm.cu:137-368). */
int mi_spmm_long_rows_prepare(const int32_t* rowptr, int32_t M, int64_t nnz, int32_t N,
                              void* workspace, size_t workspace_bytes, mi_stream_t stream);
int mi_spmm_csr_ex_f32(const int32_t* rowptr, const int32_t* col, const float* val,
                       int64_t nnz, int32_t M, int32_t K, int32_t N, const float* B,
                       int64_t ldb, const float* bias, float* C, int64_t ldc, int long_rows,
                       void* workspace, size_t workspace_bytes, mi_stream_t stream);
/* 1 when mi_spmm_csr_ws_f32 would split long rows for this problem, 0 when not (no GPU work). */
int mi_spmm_auto_splits_long_rows(int64_t nnz, int32_t M, int32_t K, int32_t N, const float* B,
                                  int64_t ldb, const float* C, int64_t ldc);
int mi_spmm_long_row_threshold(void);

/* As above with a kernel-variant override, for benchmarks and tests.
 * variant: MI_SPMM_AUTO or one of the MI_SPMM_* ids below; an id that cannot
 * handle the shape returns MI_EINVAL. */
enum {
  MI_SPMM_AUTO = 0,
  MI_SPMM_WAVE_ROW_U4 = 1,  /* one wave per row, float4 lanes, 4 B-rows in flight  */
  MI_SPMM_WAVE_ROW_U8 = 2,  /* … 8 in flight                                       */
  MI_SPMM_WAVE_ROW_U16 = 3, /* … 16 in flight                                      */
  MI_SPMM_GROUP_VEC4 = 4,   /* G = N/4 lanes per row, 64/G rows per wave            */
  MI_SPMM_GROUP_SCALAR = 5, /* any N / alignment: one float per lane                */
  MI_SPMM_WAVE_ROW_VL = 6,  /* wave per row, col/val via vector load + readlane     */
  MI_SPMM_PANELS_2 = 7,     /* N = 256: K cut into 2 column panels, one launch per   */
  MI_SPMM_PANELS_3 = 8,     /*   panel (Infinity-Cache blocking of B ≥ 768 MiB; L2   */
                            /*   blocking of 6 MiB < B ≤ 128 MiB with P ≈ |B| / 4 MiB); … 3 panels. */
                            /*   Rows whose columns descend somewhere are detected   */
                            /*   and summed in plain CSR order, so the result equals */
                            /*   the one-pass kernels' for every legal CSR input     */
  MI_SPMM_PANELS_4 = 9,
  MI_SPMM_PANELS_5 = 10,
  MI_SPMM_PANELS_6 = 11,
  MI_SPMM_PANELS_8 = 12,
  MI_SPMM_GROUP_VEC2 = 13,  /* G = N/2 lanes per row, 8 B per lane                    */
  MI_SPMM_COLTILE = 14,     /* wide N: XCD-aware column tiles so each XCD's L2 holds its B slice */
  MI_SPMM_COLTILE_PANELS = 15, /* wide N and tall K: column tiles × row panels of B, one launch per panel */
  MI_SPMM_NARROW = 16,      /* N < 4: wave per row, lanes over non-zeros, shuffle reduction (own order) */
  MI_SPMM_SLAB = 17,        /* moderate density, N ≥ 128: 128 rows × 256 columns per workgroup, B staged
                               through LDS in 64-row slabs, one ds_read_b128 per non-zero           */
  MI_SPMM_LDS_B = 18,       /* K·N·4 ≤ 128 KB (N ≤ 256, N % 4 == 0): an item's whole B copied into LDS, rows
                               gather from there — batched products of small matrices (pruned attention) */
  MI_SPMM_GROUP_PANELS_2 = 19, /* N ≤ 128 (float4 lanes), B beyond the Infinity Cache: the lane-group kernel in 2 column   */
  MI_SPMM_GROUP_PANELS_3 = 20, /*   panels (3, 4), one launch per panel, C carried; a pass takes the entries whose running */
  MI_SPMM_GROUP_PANELS_4 = 21, /*   maximum of the row's columns lies in its panel: CSR order kept for every legal input   */
  MI_SPMM_GROUP_PANELS_6 = 22,
  MI_SPMM_GROUP_PANELS_8 = 23,
  MI_SPMM_GROUP_VEC4U = 24, /* any N ≥ 4 at any 4-byte alignment: four floats per lane on dword-aligned 16-byte accesses, a
                               row's partial last quad shifted back onto its neighbour (same chain, same bits) */
  MI_SPMM_VARIANT_COUNT = 25
};
/* The two forms of MI_SPMM_LDS_B (same bits): 16 lanes per row (any tile width), or — tiles of 64 / 128 columns — a
 * quad per row with 16-byte loads of col / val (what BERT's head size runs).  form: -1 by rule (default), 0 the 16-lane
 * form only, 1 the quad form wherever it covers the shape.  Process-wide; a developer / test knob. */
int mi_spmm_ldsb_set_form(int form);
int mi_spmm_csr_f32_variant(int variant, const int32_t* rowptr, const int32_t* col,
                            const float* val, int64_t nnz, int32_t M, int32_t K,
                            int32_t N, const float* B, int64_t ldb, float* C,
                            int64_t ldc, mi_stream_t stream);
/* mi_spmm_csr_ex_f32 with the plan pinned (benchmarks and tests: bias and the long-row rule on a chosen kernel). */
int mi_spmm_csr_ex_variant_f32(int variant, const int32_t* rowptr, const int32_t* col, const float* val,
                               int64_t nnz, int32_t M, int32_t K, int32_t N, const float* B, int64_t ldb,
                               const float* bias, float* C, int64_t ldc, int long_rows, void* workspace,
                               size_t workspace_bytes, mi_stream_t stream);

/* What MI_SPMM_AUTO resolves to for this problem (no GPU work), how many kernel
 * launches a variant issues per product, and the kernel's name as profilers show
 * it — so a benchmark can attribute launch durations. */
int mi_spmm_csr_f32_plan(int64_t nnz, int32_t M, int32_t K, int32_t N, const float* B,
                         int64_t ldb, const float* C, int64_t ldc);
int mi_spmm_variant_launches(int variant);
const char* mi_spmm_variant_name(int variant);

/* ------------------------------------------------------------------------ *
 * Row schedules — the inspector's format for degree-skewed matrices (power-law row lengths: adjacency matrices).
 * Counterpart of what the reference's inspector builds once per matrix (TiledSpMM_inspect: footprint tiles + warp-sliced
 * ELL, src/sparse_mm.cu:137-368) and of the merge-spmm lineage of its kernel (src/naive_sparse_mm.cu:20-21); here the CSR
 * arrays stay as they are and the inspector builds the ORDER in which rows are handed to waves:
 *     order[slot] = row, rows by descending length class (exact below 32 entries, eight classes per octave above).
 * Longest rows first (no serial chain left for the end of the grid), rows sharing a wave / workgroup alike in length, and
 * the rows beyond a heavy length — chosen from nnz, see mi_spmm_schedule_info — in a launch of their own with more gathers in
 * flight per row on the schedule's side stream, beside the launch(es) of the rest.  Every row's fmaf chain is that of the
 * unscheduled product: mi_spmm_csr_scheduled_f32 returns the SAME BITS as mi_spmm_csr_ex_f32 for every plan and long-row
 * mode (plans that cannot take a row order — column tiles, MI_SPMM_SLAB, MI_SPMM_LDS_B, MI_SPMM_NARROW — run unscheduled).
 * LOCALITY the row order hides (the reference compacts each block's footprint of B through `mapindex`, src/sparse_mm.cu:62-68,
 * 259): given the columns, the inspector also tries the rows in the order of their median column inside a length class, MEASURES
 * what a window of 2048 consecutive slots then touches of B against the natural order (its FOOTPRINT: the 256ths of B that hold
 * three quarters of its gathers), and keeps that order only when the natural order is not local already (footprint > 40 % of
 * B) and the new one more than halves it — a banded or
 * community-structured matrix whose rows arrive shuffled then gathers like the unshuffled one.  Same bits, again.
 *   mi_spmm_schedule_create: `order` (device; M ints, 2·M when col is given) is caller-owned and must outlive the schedule; workspace ≥
 *     mi_spmm_schedule_workspace_bytes(M) is only used during the call.  col may be NULL (no locality pass).  Builds on
 *     `stream` and SYNCHRONISES it (reads ≈ 1.5 KiB back: the class table, the window statistics): inspection time, not
 *     capturable.  N: the dense width the schedule will mostly be used with.
 *   Products on one schedule must be ordered on one stream (they share its fork / join events).  The side stream itself is ONE per
 *   device for every schedule of the process (a stream per schedule ran out of hardware queues): unrelated products may see a
 *   false order between their ordinary launches, nothing else.
 *   mi_spmm_schedule_info: info[MI_SPMM_SCHEDULE_INFO_LEN] = {rows, heavy slots, heavy length, non-empty classes, lower bound of the longest row,
 *     flags (1: has a side stream; 2: ACTIVE — an order costs the locality of consecutive rows, so a matrix of short, alike
 *     rows keeps its products unscheduled: active with heavy rows, with a locality order, or mean ≥ 16 entries with ≥ 2 % of the
 *     entries in rows of ≥ 1.5 × the mean; 4: locality order), nnz, N, a window's footprint in natural order / in this order (‰ of B), mean row span (‰ of
 *     K) (-1: not measured), 0}.
 *   (Heavy slots: the rows of the length classes above the heavy length's own — by the rule at most 128 rows, the longest classes.)
 *   mi_spmm_schedule_set_heavy: another heavy length (0: every row; ≥ the longest: none) / every launch in line on the caller's
 *     stream instead of the rest beside the heavy launch — tests and A/B measurements; makes the schedule active.
 *   mi_spmm_csr_scheduled_f32: mi_spmm_csr_ex_variant_f32 (variant MI_SPMM_AUTO = by plan) on the schedule.
 * ------------------------------------------------------------------------ */
typedef struct mi_spmm_schedule mi_spmm_schedule_t;
size_t mi_spmm_schedule_workspace_bytes(int32_t M);
/* The build in two halves for callers that must not synchronise: _begin enqueues the build of both candidate orders (`order`:
 * by length class; `order_locality`, M ints, may be NULL: + by median column) and the copies of the class table and the window
 * statistics to host_out (MI_SCHEDULE_HOST_INTS ints; pinned memory keeps the copies asynchronous); once those have landed
 * (an event behind them), _finish reads them on the host, picks the order and creates the object.  mi_spmm_schedule_create =
 * _begin + a stream synchronise + _finish, with the locality order in the SECOND half of `order` (2·M ints when col != NULL). */
#define MI_SCHEDULE_HOST_INTS 512
int mi_spmm_schedule_begin(const int32_t* rowptr, const int32_t* col, int32_t M, int32_t K, int64_t nnz, int32_t N,
                           int32_t* order, int32_t* order_locality, void* workspace, size_t workspace_bytes,
                           int32_t* host_out, mi_stream_t stream);
int mi_spmm_schedule_finish(const int32_t* host_out, int32_t* order, int32_t* order_locality, int32_t M, int32_t K, int64_t nnz,
                            int32_t N, mi_spmm_schedule_t** out);
int mi_spmm_schedule_create(const int32_t* rowptr, const int32_t* col, int32_t M, int32_t K, int64_t nnz, int32_t N,
                            int32_t* order, void* workspace, size_t workspace_bytes, mi_stream_t stream,
                            mi_spmm_schedule_t** out);
int mi_spmm_schedule_destroy(mi_spmm_schedule_t* schedule);
#define MI_SPMM_SCHEDULE_INFO_LEN 12 /* entries mi_spmm_schedule_info writes */
int mi_spmm_schedule_info(const mi_spmm_schedule_t* schedule, int64_t* info);
int mi_spmm_schedule_set_heavy(mi_spmm_schedule_t* schedule, int32_t heavy_len, int use_side_stream);
int mi_spmm_csr_scheduled_f32(const mi_spmm_schedule_t* schedule, int variant, const int32_t* rowptr, const int32_t* col,
                              const float* val, int64_t nnz, int32_t M, int32_t K, int32_t N, const float* B, int64_t ldb,
                              const float* bias, float* C, int64_t ldc, int long_rows, void* workspace,
                              size_t workspace_bytes, mi_stream_t stream);
/* The column-major executor (mi_spmm_csr_colmajor_ex_f32, below: B3 / K2) on a schedule — what an inspector handle runs for a
 * degree-skewed matrix (custom_mm.cusparse_mmul_opt / tiledspmm_mm).  schedule may be NULL or inactive: then exactly
 * mi_spmm_csr_colmajor_ex_f32.  Same bits either way. */
int mi_spmm_csr_colmajor_sched_f32(const mi_spmm_schedule_t* schedule, const int32_t* rowptr, const int32_t* col,
                                   const float* val, int64_t nnz, int32_t M, int32_t K, int32_t N, const float* B,
                                   int64_t ldb, float* C, int64_t ldc, int long_rows, void* long_rows_workspace,
                                   size_t long_rows_workspace_bytes, void* workspace, size_t workspace_bytes,
                                   mi_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Batched form — `batch` independent products in ONE launch:
 *   C[b] (M×N) = A[b] (M×K, CSR) · B[b] (K×N).
 * rowptr is [batch, M+1]; entry rowptr[b*(M+1)+r] indexes into col/val with
 * the batch item's base ALREADY included (a "rowptr of rowptrs": item b's
 * nonzeros are rowptr[b*(M+1)] … rowptr[b*(M+1)+M]-1).  strideB / strideC are
 * element strides between consecutive items (strideB = 0 broadcasts one B).
 * Replaces the Python recursion + torch.stack of naive_matmul
 * (matmuls.py:289-293) and the dead batch_idx feature of spmm_kernel
 * (src/naive_sparse_mm.cu:36,52-53,86).
 * ------------------------------------------------------------------------ */
int mi_spmm_csr_batched_f32(const int32_t* rowptr, const int32_t* col,
                            const float* val, int64_t nnz_total, int32_t batch,
                            int32_t M, int32_t K, int32_t N, const float* B,
                            int64_t ldb, int64_t strideB, float* C, int64_t ldc,
                            int64_t strideC, mi_stream_t stream);
/* … with a kernel-variant override, for benchmarks and tests (a variant that does not take
 * batches, or not this shape, returns MI_EINVAL), and what AUTO resolves to for a batch. */
/* The batched product with the values read THROUGH A PERMUTATION: entry p of the batched CSR (rowptr, col) has the
 * value val[perm[p]] — the transposed pattern of a batched CSR tensor with the permutation that carries the values
 * into it (matmuls caches both per tensor; the reference has no backward for this input, matmuls.py:245-256), so a
 * backward needs no gathered copy of the values.  Same bits as mi_spmm_csr_batched_f32 on the gathered values.
 * Returns MI_OK after launching, 1 (nothing launched) when AUTO's plan for the problem is not the LDS-resident-B
 * kernel, the only one that takes a permutation — the caller then gathers and calls mi_spmm_csr_batched_f32. */
int mi_spmm_csr_batched_perm_f32(const int32_t* rowptr, const int32_t* col, const float* val,
                                 const int32_t* perm, int64_t nnz_total, int32_t batch, int32_t M,
                                 int32_t K, int32_t N, const float* B, int64_t ldb, int64_t strideB,
                                 float* C, int64_t ldc, int64_t strideC, mi_stream_t stream);
int mi_spmm_csr_batched_variant_f32(int variant, const int32_t* rowptr, const int32_t* col,
                                    const float* val, int64_t nnz_total, int32_t batch,
                                    int32_t M, int32_t K, int32_t N, const float* B,
                                    int64_t ldb, int64_t strideB, float* C, int64_t ldc,
                                    int64_t strideC, mi_stream_t stream);
/* Y[i] (K × N) = A[i]ᵀ · X[i] for a batched CSR A (rowptr [batch, M + 1] with base offsets, as above), X [batch, M, N],
 * WITHOUT transposing A: the output tile is kept in registers, every wave walks the item's rows in ascending order and
 * picks the entries of its columns (csrc/spmm_at.hip).  Per output element the terms arrive by ascending row, entries of
 * one row in CSR order — the chain of csr_transpose + mi_spmm_csr_batched_f32, bit for bit.  N ≤ 64.  Returns 1 (nothing
 * launched) for shapes it does not cover.  The gradient of V in pruned attention (reference matmuls.py:245-256 has no
 * backward for a batched CSR operand; the forward's per-call conversion is :289-297). */
int mi_spmm_csr_batched_at_f32(const int32_t* rowptr, const int32_t* col, const float* val, int64_t nnz_total,
                               int32_t batch, int32_t M, int32_t K, int32_t N, const float* X, int64_t ldx,
                               int64_t strideX, float* Y, int64_t ldy, int64_t strideY, mi_stream_t stream);
/* torch's batched CSR indices (int64 crow [batch, M + 1] from 0 per item, int64 col [batch · per_item]) → int32 offsets
 * with the items' bases added and int32 columns, in one launch. */
int mi_batched_csr_narrow_i64(const int64_t* crow, const int64_t* col, int32_t batch, int32_t M, int64_t per_item,
                              int32_t* offsets, int32_t* columns, mi_stream_t stream);
int mi_spmm_csr_batched_f32_plan(int64_t nnz_total, int32_t batch, int32_t M, int32_t K, int32_t N,
                                 const float* B, int64_t ldb, int64_t strideB, const float* C,
                                 int64_t ldc, int64_t strideC);

/* ------------------------------------------------------------------------ *
 * B3 / K2 executor — column-major dense operands:
 *   C (M×N, column-major, ldc ≥ M) = A_csr (M×K) · B (K×N, column-major, ldb ≥ K)
 * i.e. the caller holds activations X = Bᵀ as row-major [N,K] and receives
 * Y = Cᵀ as row-major [N,M].
 * Replaces torch_cusparse_mm_wrapper (src/baseline_mm.cu:272-321) behind
 * custom_mm.cusparse_mmul_opt (src/custom_mm.cpp:259-270) and
 * kernel_TiledELL / TiledSpMM_multiply (src/sparse_mm.cu:39-99, :371-385)
 * behind custom_mm.tiledspmm_mm (src/custom_mm.cpp:337-348).
 * `workspace` must hold mi_spmm_colmajor_workspace_bytes(M,K,N) bytes.
 * ------------------------------------------------------------------------ */
size_t mi_spmm_colmajor_workspace_bytes(int32_t M, int32_t K, int32_t N);
int mi_spmm_csr_colmajor_f32(const int32_t* rowptr, const int32_t* col,
                             const float* val, int64_t nnz, int32_t M, int32_t K,
                             int32_t N, const float* B, int64_t ldb, float* C,
                             int64_t ldc, void* workspace, size_t workspace_bytes,
                             mi_stream_t stream);
/* The same executor with the long-row rule of mi_spmm_csr_ex_f32 (MI_LONG_ROWS_*) and its own
 * long-row workspace (mi_spmm_csr_workspace_bytes(nnz, N); may be NULL for MI_LONG_ROWS_NONE, which
 * is what the plain entry above uses): skewed weight matrices reach the split path through the
 * inspector handles, which prepare the list once (MI_LONG_ROWS_PREPARED). */
/* 1 when the executor runs its NATIVE form for this problem (MI_LONG_ROWS_NONE only): the LDS-slab
 * kernel reading B column-major and writing C column-major directly — transposing slab loads, transposed
 * tile store, no transposed copies; 0 when it transposes B in and C out around the row-major kernel.
 * Host-side decision (plan + a cost comparison), no GPU work; the result bits are the same either way. */
int mi_spmm_colmajor_native_form(int64_t nnz, int32_t M, int32_t K, int32_t N, const float* B,
                                 int64_t ldb, const float* C, int64_t ldc);
/* Which form the executor takes (MI_LONG_ROWS_NONE): 1 = native (above); 2 = B transposed in, then the
 * one-wave-per-row kernel writing C column-major from its epilogue (16 rows per workgroup meet in LDS and
 * leave as 64-byte pieces) — no transposed copy of C; 0 = B transposed in, row-major kernel, C transposed
 * out.  `workspace` is the executor's workspace (its address decides the vector width of the kernel). */
int mi_spmm_colmajor_form(int64_t nnz, int32_t M, int32_t K, int32_t N, const float* B, int64_t ldb,
                          const float* C, int64_t ldc, const void* workspace);
int mi_spmm_csr_colmajor_ex_f32(const int32_t* rowptr, const int32_t* col,
                                const float* val, int64_t nnz, int32_t M, int32_t K,
                                int32_t N, const float* B, int64_t ldb, float* C,
                                int64_t ldc, int long_rows, void* long_rows_workspace,
                                size_t long_rows_workspace_bytes, void* workspace,
                                size_t workspace_bytes, mi_stream_t stream);

/* ------------------------------------------------------------------------ *
 * K5 — dense fp32 product, row-major, optional batch and transposes:
 *   C[b] (m×n) = op(A[b]) · op(B[b]),   op(X) = X or Xᵀ
 * A[b] is stored (transa ? k×m : m×k) with leading dimension lda, B[b] is
 * stored (transb ? n×k : k×n) with ldb, C[b] m×n with ldc; stride* are element
 * strides between batch items (0 broadcasts).  alpha = 1, beta = 0.
 * Replaces cublas_mm_wrapper / cublas_bmm_wrapper
 * (src/baseline_mm.cu:52-102, :105-155) behind custom_mm.cublas_mmul /
 * cublas_bmm (src/custom_mm.cpp:104-164).  Products are accumulated over k in
 * increasing order with fused multiply-add (exact-fp32 MFMA), one rounding per
 * product.
 * ------------------------------------------------------------------------ */
int mi_gemm_f32(int transa, int transb, int32_t m, int32_t n, int32_t k,
                const float* A, int64_t lda, int64_t strideA, const float* B,
                int64_t ldb, int64_t strideB, float* C, int64_t ldc,
                int64_t strideC, int32_t batch, mi_stream_t stream);

/* Two products that share one large operand, in ONE launch that reads it once:
 *     C1[b] = A[b] · B1[b]   ([m, k]·[k, n])        C2[b] = A[b]ᵀ · B2[b]   ([k, m]·[m, n])
 * all operands contiguous row-major, `batch` items.  The backward of `scores = cublasTransbMM.apply(q, k)` (reference
 * README.md:69-77, matmuls.py:131-152): dQ = dS·K (A = dS, B1 = K) and dK = dSᵀ·Q (B2 = Q) — two launches of
 * mi_gemm_f32 read the 403 MB of dS twice.  Every output element is the same k-ordered fused-multiply-add chain as
 * mi_gemm_f32's: same bits.  Returns MI_OK after launching, 1 (nothing launched) for shapes the fused form does not
 * cover — it takes n = 64, k = 64, 128, 256 or 512, m a multiple of 64 (BERT-base / -large attention heads) — the
 * caller then runs the two plain products. */
int mi_gemm_pair_a_at_f32(const float* A, const float* B1, const float* B2, float* C1, float* C2,
                          int32_t batch, int32_t m, int32_t k, int32_t n, mi_stream_t stream);

/* Deterministic split-k (what custom_mm.cublas_mmul / cublas_bmm call): products with few output tiles and a long k — weight
 * gradients over thousands of tokens — leave most of the chip idle as one chain per element.  mi_gemm_split_count(m, n, k, batch)
 * is a function of the SHAPE alone: 1 (the plain chain) unless batch == 1, k ≥ 4096 and fewer than 128 output tiles of 128 × 128;
 * else S = the largest power of two ≤ min(320 / tiles, k / 1024) with k % (32·S) == 0.  With S > 1, k is cut into S equal ranges,
 * each the usual k-ordered fmaf chain from zero, and an element's S partial sums are added in index order ((p0 + p1) + p2) + …,
 * then the bias — a fixed order the oracle restates (oracle_gemm_f32).  The reference's criterion is torch.allclose at 1e-5 with
 * cuBLAS's unspecified order (tests/cublas_kernel_test.py:27-28, src/baseline_mm.cu:96-101).  workspace ≥
 * mi_gemm_workspace_bytes (S·m·n floats; 0 when S == 1), 16-byte aligned; too small a workspace is MI_ENOMEM, never a silent
 * plain chain.  mi_gemm_f32 / mi_gemm_bias_f32 (no workspace) always run the plain chain. */
int mi_gemm_split_count(int32_t m, int32_t n, int32_t k, int32_t batch);
size_t mi_gemm_workspace_bytes(int32_t m, int32_t n, int32_t k, int32_t batch);
int mi_gemm_ws_f32(int transa, int transb, int32_t m, int32_t n, int32_t k, const float* A, int64_t lda, int64_t strideA,
                   const float* B, int64_t ldb, int64_t strideB, const float* bias, float* C, int64_t ldc, int64_t strideC,
                   int32_t batch, void* workspace, size_t workspace_bytes, mi_stream_t stream);

/* Which kernel family mi_gemm_f32 / mi_gemm_bias_f32 take (process-wide; every
 * plan produces the same bits — tests pin one to compare it with another):
 * AUTO picks; TILES = one output tile (or a short chain) per 4-wave workgroup;
 * DUO = the persistent 8-wave kernel whose halves run in anti-phase (whole
 * 128-row tiles only: MI_EINVAL when pinned on a shape it cannot take). */
#define MI_GEMM_PLAN_AUTO 0
#define MI_GEMM_PLAN_TILES 1
#define MI_GEMM_PLAN_DUO 2
int mi_gemm_set_plan(int plan);

/* ------------------------------------------------------------------------ *
 * Fused "sparsify on the fly" form: A is given DENSE (batch × M×K, leading
 * dimension lda, item stride strideA) and its exact zeros are skipped inside the
 * kernel, in ascending column order — bit-identical to mi_dense_to_csr_* followed
 * by mi_spmm_csr_batched_f32, without materialising a CSR.  B[b] is K×N
 * (strideB = 0 shares one B); bias (N entries) may be NULL.
 * Replaces `a.to_sparse_csr()` + get_sparse_tensor_properties + spmm_kernel per
 * call / per slice (reference matmuls.py:289-297, :178-187).
 * Supported when mi_spmm_dense_skip_supported(...) != 0 (N ≤ 256, N % 4 == 0,
 * 16-byte aligned B and C rows); otherwise MI_EINVAL — use the CSR entry points.
 * ------------------------------------------------------------------------ */
int mi_spmm_dense_skip_supported(int32_t N, int64_t lda, int64_t ldb, int64_t ldc,
                                 const float* A, const float* B, const float* C);
int mi_spmm_dense_skip_f32(const float* A, int64_t lda, int64_t strideA, int32_t batch,
                           int32_t M, int32_t K, int32_t N, const float* B, int64_t ldb,
                           int64_t strideB, const float* bias, float* C, int64_t ldc,
                           int64_t strideC, mi_stream_t stream);

/* Gated form of the product above, for callers that must keep the zero-skipping
 * semantics of `a.to_sparse_csr()` (reference matmuls.py:295-296: a zero of A
 * never meets B) while normally taking the dense MFMA product (mi_gemm_f32), in
 * which 0·inf = nan: the launch does nothing unless *gate != 0 (device memory,
 * read when the kernel starts), so
 *     mi_gemm_f32(...);  mi_nonfinite_flag_f32(B, ..., gate);  this(..., gate)
 * leaves the dense product in C when B is finite (where both agree bit for bit)
 * and overwrites it with the zero-skipping product when B holds an inf / nan —
 * decided on the device, nothing read back, graph-capturable.  Any N % 4 == 0
 * (column tiles of 256 inside one launch); gate == NULL always runs.
 * mi_nonfinite_flag_f32 writes *flag = 1 if x (rows×cols, leading dimension ld)
 * holds an inf or nan, else 0. */
int mi_spmm_dense_skip_gated_f32(const float* A, int64_t lda, int64_t strideA, int32_t batch,
                                 int32_t M, int32_t K, int32_t N, const float* B, int64_t ldb,
                                 int64_t strideB, const float* bias, float* C, int64_t ldc,
                                 int64_t strideC, const int32_t* gate, mi_stream_t stream);
int mi_nonfinite_flag_f32(const float* x, int64_t rows, int64_t cols, int64_t ld, int32_t* flag,
                          mi_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Fused FC-layer epilogues:  C = (product) + bias, bias[N] (resp. bias[n]) added
 * to every row AFTER the accumulation chain (one extra rounding, exactly what
 * `output = t.clone(); output += self.bias` computes).  bias may be NULL.
 * Replace the separate clone + add of cublasLinear / cusparseLinear.forward
 * (reference benchmarks/cublas_fc_layer.py:41-45, cusparse_fc_layer.py:41-45).
 * ------------------------------------------------------------------------ */
int mi_spmm_csr_bias_f32(const int32_t* rowptr, const int32_t* col, const float* val,
                         int64_t nnz, int32_t M, int32_t K, int32_t N, const float* B,
                         int64_t ldb, const float* bias, float* C, int64_t ldc,
                         mi_stream_t stream);
int mi_gemm_bias_f32(int transa, int transb, int32_t m, int32_t n, int32_t k,
                     const float* A, int64_t lda, int64_t strideA, const float* B,
                     int64_t ldb, int64_t strideB, const float* bias, float* C,
                     int64_t ldc, int64_t strideC, int32_t batch, mi_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Dense → CSR on the device (exact-zero test, columns ascending within a row),
 * batched: `batch` matrices of rows×cols (leading dimension ld, item stride
 * `stride`).  Two steps so the caller can size col/val without a host sync
 * per item:
 *   1. mi_dense_to_csr_count: writes rowptr[batch*(rows+1)] as a "rowptr of
 *      rowptrs" (see mi_spmm_csr_batched_f32); rowptr[batch*(rows+1)-1] is the
 *      total nnz.  `workspace` ≥ mi_dense_to_csr_workspace_bytes(batch, rows).
 *   2. mi_dense_to_csr_fill: writes col / val (capacity ≥ total nnz).
 * Replaces dense_to_csr (src/baseline_mm.cu:218-264, cusparseDenseToSparse)
 * and the per-slice torch `to_sparse_csr()` of naive_matmul (matmuls.py:295-296).
 * ------------------------------------------------------------------------ */
size_t mi_dense_to_csr_workspace_bytes(int32_t batch, int32_t rows);
int mi_dense_to_csr_count(const float* dense, int32_t batch, int32_t rows,
                          int32_t cols, int64_t ld, int64_t stride,
                          int32_t* rowptr, void* workspace, size_t workspace_bytes,
                          mi_stream_t stream);
int mi_dense_to_csr_fill(const float* dense, int32_t batch, int32_t rows,
                         int32_t cols, int64_t ld, int64_t stride,
                         const int32_t* rowptr, int32_t* col, float* val,
                         mi_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Device CSR transpose (A M×K → Aᵀ K×M, columns ascending within each row of
 * Aᵀ, stable for duplicates): used by the backward pass  grad_B = Aᵀ · dC.
 * Hand-written least-significant-digit counting passes over the column index (csr_transpose.hip):
 * two passes for K·batch ≤ 2²⁰, three beyond; no atomics, deterministic.
 * `workspace` ≥ mi_csr_transpose_workspace_bytes(M, K, nnz) (≈ 8–12 bytes per non-zero plus the
 * per-tile digit tables), 16-byte aligned.  No counterpart in the reference (its backward
 * re-sparsifies a strided view, matmuls.py:319-325, SURVEY.md §8a defect 1).
 * Batched form: `batch` matrices in the batched-CSR layout of mi_spmm_csr_batched_f32 (rowptr
 * [batch, M+1] with global offsets) → t_rowptr [batch, K+1] in the same layout, item b's
 * transposed entries at t_rowptr[b*(K+1)] … ; one set of launches for the whole batch.
 * ------------------------------------------------------------------------ */
size_t mi_csr_transpose_workspace_bytes(int32_t M, int32_t K, int64_t nnz);
int mi_csr_transpose_f32(const int32_t* rowptr, const int32_t* col, const float* val,
                         int64_t nnz, int32_t M, int32_t K, int32_t* t_rowptr,
                         int32_t* t_col, float* t_val, void* workspace,
                         size_t workspace_bytes, mi_stream_t stream);
/* Which plan transposes (process-wide; every plan gives the same bits — tests pin one to compare it with the other):
 *   TABLES    per-(tile, digit) count tables, one count launch + three scan launches ahead of every scatter pass;
 *   ONE_SWEEP the columns are read once for counting: the first pass's count launch also counts the last pass's
 *             digits per group of bins, and the last scatter launch finds its tiles' offsets by decoupled look-back
 *             inside those groups (status words published / polled with agent-scope accesses, tiles handed out by
 *             tickets so every wait is on a running workgroup) — no second count pass over the intermediate array,
 *             no scan of its table; one matrix, 2¹⁰ < K ≤ 2²⁰ (two passes), ≥ 4 M non-zeros, nnz < 2³⁰ —
 *             mi_csr_transpose_one_sweep_applies says whether a problem qualifies;
 *   AUTO      ONE_SWEEP where it applies and pays (≥ 33 M non-zeros), else TABLES.  Pinning ONE_SWEEP on a problem it
 *             does not cover: MI_EINVAL.
 * mi_csr_transpose_check (synchronises `stream`; a debugging aid) reads back the one-sweep plan's give-up flag from
 * the workspace of the last transpose: MI_EHIP if a look-back poll ran into its limit (never on a correct run). */
#define MI_TRANSPOSE_PLAN_AUTO 0
#define MI_TRANSPOSE_PLAN_TABLES 1
#define MI_TRANSPOSE_PLAN_ONE_SWEEP 2
int mi_csr_transpose_set_plan(int plan);
int mi_csr_transpose_one_sweep_applies(int32_t batch, int32_t M, int32_t K, int64_t nnz);
/* 1 when the next mi_csr_transpose*_f32 of this problem runs the one-sweep plan under the plan in force (the only plan
 * whose give-up flag mi_csr_transpose_check can report). */
int mi_csr_transpose_auto_takes_one_sweep(int32_t batch, int32_t M, int32_t K, int64_t nnz);
int mi_csr_transpose_check(const void* workspace, size_t workspace_bytes, int32_t batch, int32_t M,
                           int32_t K, int64_t nnz, mi_stream_t stream);
size_t mi_csr_transpose_batched_workspace_bytes(int32_t batch, int32_t M, int32_t K, int64_t nnz);
/* 1 when the batch is transposed by the one-workgroup-per-item plan (items small enough for a [waves][K] table in LDS,
 * ≤ 256 K entries per item, ≥ 64 items or ≤ 128 K entries in all; plan AUTO): one launch, no workspace used, ≈ 20× faster
 * than the general plan on pruned-attention batches — cheap enough to transpose the VALUES on every backward instead of
 * keeping a permutation (matmuls._batched_csr_backward).  Same stable order, same bits. */
int mi_csr_transpose_batched_in_lds(int64_t nnz, int32_t batch, int32_t M, int32_t K);
int mi_csr_transpose_batched_f32(const int32_t* rowptr, const int32_t* col, const float* val,
                                 int64_t nnz, int32_t batch, int32_t M, int32_t K,
                                 int32_t* t_rowptr, int32_t* t_col, float* t_val,
                                 void* workspace, size_t workspace_bytes, mi_stream_t stream);

/* ------------------------------------------------------------------------ *
 * SDDMM on A's pattern:  out[p] = Σ_j dC[row(p), j] · B[col[p], j]
 * = the gradient of C = A·B with respect to A's stored values.  Any N; fixed summation order
 * (lane l of 64 chains columns 256t + 4l + c, then a xor tree), restated by the oracle.
 * ------------------------------------------------------------------------ */
int mi_sddmm_csr_f32(const int32_t* rowptr, const int32_t* col, int64_t nnz,
                     int32_t M, int32_t K, int32_t N, const float* dC, int64_t lddc,
                     const float* B, int64_t ldb, float* out_val,
                     mi_stream_t stream);

/* SDDMM on a BATCHED CSR pattern (rowptr [batch, M+1] with global offsets, as mi_spmm_csr_batched_f32):
 *   out[p] = Σ_j dC[item][row(p), j] · B[item][col[p], j]      (strideB = 0: one B shared by every item)
 * = the gradient of the stored values of a batched CSR tensor (the reference has no backward for this input,
 * matmuls.py:245-256).  Same bits as mi_sddmm_csr_f32 on the block-diagonal matrix of the batch.  Returns MI_OK after
 * launching the LDS-resident form (an item's B staged in LDS once per workgroup, N ≤ 64, K·N·4 ≤ 128 KB, ≥ 16384 rows
 * of ≥ 4 non-zeros on average), 1 — nothing launched — for every other problem: the caller then runs mi_sddmm_csr_f32
 * on the block-diagonal form. */
int mi_sddmm_csr_batched_f32(const int32_t* rowptr, const int32_t* col, int64_t nnz_total, int32_t batch,
                             int32_t M, int32_t K, int32_t N, const float* dC, int64_t lddc,
                             int64_t strideDC, const float* B, int64_t ldb, int64_t strideB,
                             float* out_val, mi_stream_t stream);

/* dst[p] = src[perm[p]], p < n: the stored values of a CSR tensor carried into its cached transposed pattern by the
 * permutation mi_csr_transpose_* produced for the values 0, 1, 2, … (matmuls' backward; replaces the reference-side
 * `index_select`).  perm entries must lie in [0, length of src). */
int mi_gather_f32(const float* src, const int32_t* perm, int64_t n, float* dst, mi_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Low precision: CSR × dense in bfloat16 / float16 (values, B and C all of the entry's type T; stored as uint16_t bit
 * patterns), every sum in fp32.  With up() the exact widening to fp32 and rne_T the round-to-nearest-even narrowing
 * that torch's Tensor.to(T) does, the product writes
 *     C = rne_T(C32),   C32 = what mi_spmm_csr_ex_f32 writes for up(val), up(B) with MI_LONG_ROWS_SPLIT:
 * the plain CSR-order fmaf chain for rows of up to mi_spmm_long_row_threshold() entries, the split order of the K1
 * section for longer rows, the xor-butterfly order for N < 4 — and ONE rounding per element, at the store.  NaN stays
 * NaN (its payload is not part of the contract); every other value, ±0, ±inf, overflow (fp16 above 65504) and results
 * in T's subnormal range included, is exactly rne_T of the fp32 result.
 *   long_rows: MI_LONG_ROWS_AUTO, _AUTO_ZEROED and _SPLIT all mean SPLIT here, whatever the fp32 plan would be (its SLAB
 *   and NARROW plans do not split; this path has no plan-dependent exception).  _NONE: every row keeps the plain chain
 *   (one launch; the same bits when no row exceeds the threshold).  _PREPARED → MI_EINVAL (no inspector handles here).
 *   workspace: mi_spmm_csr_workspace_bytes(nnz, N) bytes, 16-byte aligned, required when nnz exceeds the threshold,
 *   N ≥ 4 and the mode splits (else MI_EINVAL; too small: MI_ENOMEM).  The partial rows of split rows are fp32.
 *   _AUTO_ZEROED keeps the zero-header contract of the fp32 entries, so one workspace per stream serves both.
 *   B and C: any 2-byte-aligned pointer, any ldb ≥ N and ldc ≥ N (odd values and column-offset views included).
 * Checked before any HIP call: negative sizes, ldb < N, ldc < N, the mode, null pointers (col / val / B may be NULL
 * only when nnz == 0) → MI_EINVAL; M == 0 or N == 0 → MI_OK.  No host read-back, no float atomics: graph-capturable.
 * A product is the main kernel plus, when it may split, one follow-up launch that sums the listed rows (or finds none).
 * No counterpart in the reference (float32 only: src/naive_sparse_mm.cu:24-136). */
int mi_spmm_csr_ex_bf16(const int32_t* rowptr, const int32_t* col, const uint16_t* val, int64_t nnz,
                        int32_t M, int32_t K, int32_t N, const uint16_t* B, int64_t ldb,
                        uint16_t* C, int64_t ldc, int long_rows, void* workspace, size_t workspace_bytes,
                        mi_stream_t stream);
int mi_spmm_csr_ex_f16(const int32_t* rowptr, const int32_t* col, const uint16_t* val, int64_t nnz,
                       int32_t M, int32_t K, int32_t N, const uint16_t* B, int64_t ldb,
                       uint16_t* C, int64_t ldc, int long_rows, void* workspace, size_t workspace_bytes,
                       mi_stream_t stream);
/* SDDMM in low precision: out_val[p] = rne_T(mi_sddmm_csr_f32 on up(dC), up(B)) — the same fp32 order (lane l of 64
 * chains columns 256t + 4l + c, then the xor tree), one rounding.  Same argument rules as mi_sddmm_csr_f32; dC and B
 * 2-byte aligned with any lddc, ldb ≥ N. */
int mi_sddmm_csr_bf16(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t M, int32_t K, int32_t N,
                      const uint16_t* dC, int64_t lddc, const uint16_t* B, int64_t ldb, uint16_t* out_val,
                      mi_stream_t stream);
int mi_sddmm_csr_f16(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t M, int32_t K, int32_t N,
                     const uint16_t* dC, int64_t lddc, const uint16_t* B, int64_t ldb, uint16_t* out_val,
                     mi_stream_t stream);
/* mi_gather_f32 for 2-byte values (bf16 / fp16 bit patterns moved untouched): dst[p] = src[perm[p]], p < n. */
int mi_gather_b16(const uint16_t* src, const int32_t* perm, int64_t n, uint16_t* dst, mi_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Low precision: dense products in bfloat16 / float16 on the matrix cores.  The arguments mirror mi_gemm_f32's
 *   C[b] (m×n) = op(A[b]) · op(B[b]),   A, B and C all of the entry's type T, stored as uint16_t bit patterns;
 * transposes, leading dimensions and item strides (0 broadcasts) as there; alpha = 1, beta = 0.
 * Every sum is fp32 and each element is rounded ONCE, at the store (round-to-nearest-even, the narrowing torch's
 * Tensor.to(T) does).  NaN stays NaN (its payload is not part of the contract); fp16 results beyond 65504 in magnitude
 * round to ±inf (from 65520 up) or to ±65504 (below it), as that narrowing does.
 * One order for the whole family: every output element is accumulated from +0 by v_mfma_f32_16x16x32_{bf16,f16} over
 * the k-steps 0–31, 32–63, … in ascending order, a ragged last step zero-padded.  So the bits of C[i, j] depend only on
 * row i of op(A), column j of op(B), k and T — not on m, n, the batch size or position, the tile the element lands in,
 * the storage transposes or the kernel the entry picks.  (Not the fp32 entries' fmaf chain: the MFMA sums 32 products
 * per step.)
 * A, B and C: any 2-byte-aligned pointer, any lda / ldb / ldc at least the stored row length (odd values and
 * column-offset views included; 16-byte-aligned operands with leading dimensions and strides that are multiples of 8
 * take the vector loads and stores).
 * Checked before any HIP call: negative sizes or strides, a leading dimension shorter than its row, null or odd
 * pointers (A and B may be NULL when k == 0) → MI_EINVAL; m == 0, n == 0 or batch == 0 → MI_OK (nothing launched);
 * k == 0 writes zeros.
 * mi_gemm_set_plan does not apply to these entries (there is one kernel family).  No float atomics, no split-k (that is
 * mi_gemm_ws_bf16 / _f16 below), no host read-back: graph-capturable.  No counterpart in the reference (float32 only:
 * src/baseline_mm.cu:52-155). */
int mi_gemm_bf16(int transa, int transb, int32_t m, int32_t n, int32_t k,
                 const uint16_t* A, int64_t lda, int64_t strideA, const uint16_t* B,
                 int64_t ldb, int64_t strideB, uint16_t* C, int64_t ldc,
                 int64_t strideC, int32_t batch, mi_stream_t stream);
int mi_gemm_f16(int transa, int transb, int32_t m, int32_t n, int32_t k,
                const uint16_t* A, int64_t lda, int64_t strideA, const uint16_t* B,
                int64_t ldb, int64_t strideB, uint16_t* C, int64_t ldc,
                int64_t strideC, int32_t batch, mi_stream_t stream);

/* The fused FC epilogue in low precision: mi_gemm_bf16 / _f16 with a bias of the same type T,
 *   C[b][i, j] = rne_T(acc[i, j] + up(bias[j])),
 * acc the fp32 accumulator the plain entry would narrow (same k-loop, same order), up() the exact widening of bias[j],
 * one fp32 add, ONE rounding per element.  bias: n elements, any 2-byte-aligned pointer (16-byte aligned for the vector
 * form), or NULL — then the entry IS the plain one (same kernel, same bits).  Checked before any HIP call as there, an
 * odd bias pointer included → MI_EINVAL; k == 0 writes the bias into every row (zeros without one).  Never splits k. */
int mi_gemm_bias_bf16(int transa, int transb, int32_t m, int32_t n, int32_t k,
                      const uint16_t* A, int64_t lda, int64_t strideA, const uint16_t* B,
                      int64_t ldb, int64_t strideB, const uint16_t* bias, uint16_t* C, int64_t ldc,
                      int64_t strideC, int32_t batch, mi_stream_t stream);
int mi_gemm_bias_f16(int transa, int transb, int32_t m, int32_t n, int32_t k,
                     const uint16_t* A, int64_t lda, int64_t strideA, const uint16_t* B,
                     int64_t ldb, int64_t strideB, const uint16_t* bias, uint16_t* C, int64_t ldc,
                     int64_t strideC, int32_t batch, mi_stream_t stream);

/* Deterministic split-k in low precision, for products with a long k and few output tiles (the FC weight gradient
 * dYᵀ·x over thousands of tokens), which leave most of the chip idle as one accumulator per element.
 * mi_gemm_lowp_split_count(m, n, k, batch) is a function of the SHAPE alone: 1 unless batch == 1, k ≥ 2048 and at most
 * 576 output tiles of 128 × 128; else S = the largest power of two ≤ min(2048 / tiles, k / 256, 32), halved until
 * k % (32·S) == 0 (whole MFMA k-steps per range).  (Not mi_gemm_split_count: another tile, sixteen times the MFMA rate.)
 * With S > 1, k is cut into S equal ranges; range s runs the family order of mi_gemm_bf16 from +0 into an fp32 partial
 * P[s] (not narrowed), and
 *   C[i, j] = rne_T((((P[0] + P[1]) + P[2]) + …) + up(bias[j]))
 * with fp32 round-to-nearest adds in index order, the bias (optional) last: one rounding to T per element, no float
 * atomics, no host read-back, graph-capturable, the same bits on every run.  S == 1 calls mi_gemm_bias_*: its bits.
 * workspace ≥ mi_gemm_lowp_workspace_bytes (S·m·n·4 for S > 1, else 0), 16-byte aligned: NULL or unaligned with S > 1
 * → MI_EINVAL, too small → MI_ENOMEM, never a silent unsplit product (the order is part of the result).  Other checks
 * as mi_gemm_bias_*, all before any HIP call.
 * mi_gemm_split_bf16 / _f16 take the number of ranges from the caller (one product; splits ≥ 1, k % (32·splits) == 0,
 * else MI_EINVAL; workspace ≥ splits·m·n·4): what mi_gemm_ws_* run with splits = mi_gemm_lowp_split_count, and how the
 * rule's grid is measured (tools/bench_gemm_lowp_split.py).
 * mi_gemm_lowp_tile_n(m, n, batch) is the width of the output tile every entry of this family launches for a shape — a
 * function of the SHAPE alone: 128 (the 128 × 128 tile) when n > 64 and ceil(m/128) · ceil(n/128) · batch ≥ 512, else 64
 * (the 128 × 64 tile; also for an empty shape).  For the partials of a split, batch is the number of ranges.  The bits of
 * no result depend on it (see above); it is exported so that a test can tell which tile it ran. */
int mi_gemm_lowp_split_count(int32_t m, int32_t n, int32_t k, int32_t batch);
int mi_gemm_lowp_tile_n(int32_t m, int32_t n, int32_t batch);
size_t mi_gemm_lowp_workspace_bytes(int32_t m, int32_t n, int32_t k, int32_t batch);
int mi_gemm_ws_bf16(int transa, int transb, int32_t m, int32_t n, int32_t k,
                    const uint16_t* A, int64_t lda, int64_t strideA, const uint16_t* B,
                    int64_t ldb, int64_t strideB, const uint16_t* bias, uint16_t* C, int64_t ldc,
                    int64_t strideC, int32_t batch, void* workspace, size_t workspace_bytes, mi_stream_t stream);
int mi_gemm_ws_f16(int transa, int transb, int32_t m, int32_t n, int32_t k,
                   const uint16_t* A, int64_t lda, int64_t strideA, const uint16_t* B,
                   int64_t ldb, int64_t strideB, const uint16_t* bias, uint16_t* C, int64_t ldc,
                   int64_t strideC, int32_t batch, void* workspace, size_t workspace_bytes, mi_stream_t stream);
int mi_gemm_split_bf16(int transa, int transb, int32_t m, int32_t n, int32_t k, const uint16_t* A, int64_t lda,
                       const uint16_t* B, int64_t ldb, const uint16_t* bias, uint16_t* C, int64_t ldc, int32_t splits,
                       void* workspace, size_t workspace_bytes, mi_stream_t stream);
int mi_gemm_split_f16(int transa, int transb, int32_t m, int32_t n, int32_t k, const uint16_t* A, int64_t lda,
                      const uint16_t* B, int64_t ldb, const uint16_t* bias, uint16_t* C, int64_t ldc, int32_t splits,
                      void* workspace, size_t workspace_bytes, mi_stream_t stream);

/* Column sums dst[j] = Σ_r src[r, j] (src rows×n, leading dimension ld): the bias gradient of
 * the FC layers (autograd of `output += self.bias`, reference benchmarks/cublas_fc_layer.py:44-45).
 * Fixed summation order (per row chunk: 4 waves × 4 interleaved row chains, added in a fixed
 * order; chunks — 64 rows up to 64 Ki rows, larger beyond — added in order), no atomics.
 * workspace ≥ mi_colsum_workspace_bytes(rows, n). */
size_t mi_colsum_workspace_bytes(int32_t rows, int32_t n);
int mi_colsum_f32(const float* src, int32_t rows, int32_t n, int64_t ld, float* dst,
                  void* workspace, size_t workspace_bytes, mi_stream_t stream);
/* … of bfloat16 / float16 values (the bias gradient of a low-precision layer): widened on load, the SAME fp32 order and
 * fp32 partials in the same workspace (mi_colsum_workspace_bytes serves all three), one rounding at the store:
 *   mi_colsum_T(src) == rne_T(mi_colsum_f32(up(src)))   bit for bit.
 * src, dst: 2-byte aligned (odd → MI_EINVAL); 8-byte loads of 4 columns when n and ld are multiples of 4 and src is
 * 8-byte aligned, 2-byte elements otherwise (odd ld, column-offset views). */
int mi_colsum_bf16(const uint16_t* src, int32_t rows, int32_t n, int64_t ld, uint16_t* dst,
                   void* workspace, size_t workspace_bytes, mi_stream_t stream);
int mi_colsum_f16(const uint16_t* src, int32_t rows, int32_t n, int64_t ld, uint16_t* dst,
                  void* workspace, size_t workspace_bytes, mi_stream_t stream);

/* Dense 2-D transpose  dst[cols, rows] = src[rows, cols]ᵀ (row-major, ld's). */
int mi_transpose_f32(const float* src, int32_t rows, int32_t cols, int64_t ld_src,
                     float* dst, int64_t ld_dst, mi_stream_t stream);

/* ------------------------------------------------------------------------ *
 * HOST inspector step (no GPU): COO (sorted by row) → CSR, keeping the input
 * order inside a row.  Replaces TiledSpMM_coo2csr (src/sparse_mm.cu:110-134).
 * rowptr has M+1 entries; col_out / val_out have nnz entries.
 * ------------------------------------------------------------------------ */
int mi_coo_to_csr_host(int32_t M, int64_t nnz, const int32_t* coo_row,
                       const int32_t* coo_col, const float* coo_val,
                       int32_t* rowptr, int32_t* col_out, float* val_out);

/* ------------------------------------------------------------------------ *
 * Peer mappings (multi-GPU exchange) — NEW relative to the reference, which is
 * single-device (`cudaSetDevice(0)`, src/sparse_mm.cu:295; no collective, no peer access).
 * One process per GPU; rank A exports the allocation its C buffer lives in, the 64 handle bytes + the
 * buffer's offset travel to the peers by whatever channel the host side has (torch.distributed's
 * all_gather_object), every peer opens the handle and copies its row blocks straight into A's C
 * (device-to-device over xGMI).  Lifetimes are EXPLICIT: a mapping lives from mi_ipc_open to the matching
 * mi_ipc_close; opens of one handle in one process are counted (one hipIpcOpenMemHandle, closed with the
 * last mi_ipc_close).  The exporter keeps the allocation alive until every peer has closed (the host side
 * puts a barrier between the peers' closes and the free).  No stream argument: these are host calls.
 *   mi_ipc_export : handle_out[MI_IPC_HANDLE_BYTES], *offset_out = dev_ptr − base of its allocation,
 *                   *alloc_bytes_out (may be NULL) = size of that allocation
 *   mi_ipc_open   : *base_out = the peer allocation's base in this process (add the offset)
 *   mi_ipc_close  : drops one open of that handle; MI_EINVAL if it is not open here
 *   mi_ipc_open_count : opens not yet closed in this process (tests: nothing is left mapped)
 * ------------------------------------------------------------------------ */
#define MI_IPC_HANDLE_BYTES 64
/* ------------------------------------------------------------------------ *
 * Reductions other than sum over a row's products: torch.sparse.mm(A, B, reduce=...)
 * (aten::_sparse_mm_reduce_impl), which torch implements for CSR on the CPU only.  The reference's Reducer
 * (src/naive_reducer.cuh:23-101) has MIN / MAX branches, but its wrapper pins reduce = "sum"
 * (src/naive_sparse_mm.cu:119).
 *   MI_REDUCE_SUM   the bits of mi_spmm_csr_ws_f32 with the same workspace;
 *   MI_REDUCE_MEAN  those bits divided by the row's entry count (correctly rounded); an empty row gives +0;
 *   MI_REDUCE_AMAX  with p_e = val[e] · B[col[e], j] (one fp32 multiply): the sequential scan "start at (-inf, nnz),
 *                   take (p_e, e) iff p_e > cur || isnan(p_e)", i.e. the largest e with a NaN product if there is one,
 *                   else the smallest e attaining the maximum (-0 == +0 is a tie; the output keeps p_e's sign), else
 *                   (-inf, nnz); an empty row gives (+0, nnz);
 *   MI_REDUCE_AMIN  the same with <.
 * arg (int32, [M, ldarg], may be NULL; only for AMAX / AMIN) receives the selected entry index e (nnz: none).
 * With a workspace of mi_spmm_csr_reduce_workspace_bytes(nnz, N) bytes (16-byte aligned), rows with more than 8192
 * entries are cut into max(1, len / 16384) chunks, one workgroup each (AMAX / AMIN: same result — the selection does
 * not depend on the split; SUM / MEAN: mi_spmm_csr_ws_f32's long-row order).  NULL: every row is one wave's.
 * Validation before any HIP call: an unknown code, or arg with SUM / MEAN → MI_EINVAL; M == 0 or N == 0 → MI_OK;
 * nnz ≥ 2³¹ → MI_ERANGE; a NULL required pointer → MI_EINVAL.  No host synchronisation: graph-capturable.
 * ------------------------------------------------------------------------ */
enum { MI_REDUCE_SUM = 0, MI_REDUCE_MEAN = 1, MI_REDUCE_AMAX = 2, MI_REDUCE_AMIN = 3 };
size_t mi_spmm_csr_reduce_workspace_bytes(int64_t nnz, int32_t N);
int mi_spmm_csr_reduce_f32(const int32_t* rowptr, const int32_t* col, const float* val, int64_t nnz,
                           int32_t M, int32_t K, int32_t N, const float* B, int64_t ldb, float* C,
                           int64_t ldc, int32_t* arg, int64_t ldarg, int reduce, void* workspace,
                           size_t workspace_bytes, mi_stream_t stream);
/* out[i, :] = in[i, :] / (rowptr[i+1] − rowptr[i]), correctly rounded; rows without entries are copied.
 * in == out is allowed (the mean's epilogue; its gradient g / count out of place). */
int mi_spmm_rows_divide_f32(const int32_t* rowptr, int32_t M, int32_t N, const float* in, int64_t ldin,
                            float* out, int64_t ldout, mi_stream_t stream);
/* Gradients of AMAX / AMIN given the forward's arg, without float atomics (deterministic):
 *   grad_val[e] = Σ_j [arg[i, j] == e] · G[i, j] · B[col[e], j]      (one wave per row, j ascending, then a xor tree)
 *   grad_B[k, j] = Σ_t [arg[i, j] == perm[t]] · val[perm[t]] · G[i, j] (i = t_col[t]; over row k of Aᵀ in order)
 * grad_B runs on Aᵀ's pattern (t_rowptr [K+1], t_col = original rows) and the permutation perm that carries an entry of
 * Aᵀ to its index in A (what mi_csr_transpose_f32 gives for the values 0, 1, 2, …). */
int mi_spmm_reduce_grad_val_f32(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t M, int32_t K,
                                int32_t N, const float* B, int64_t ldb, const float* G, int64_t ldg,
                                const int32_t* arg, int64_t ldarg, float* grad_val, mi_stream_t stream);
int mi_spmm_reduce_grad_b_f32(const int32_t* t_rowptr, const int32_t* t_col, const int32_t* perm,
                              const float* val, int64_t nnz, int32_t M, int32_t K, int32_t N, const float* G,
                              int64_t ldg, const int32_t* arg, int64_t ldarg, float* grad_b, int64_t ldgb,
                              mi_stream_t stream);

/* ------------------------------------------------------------------------ *
 * The reductions in bfloat16 / float16 (T): val, B, C, G and both gradients of the entry's type T, stored as uint16_t bit
 * patterns, any 2-byte-aligned pointer (an odd one → MI_EINVAL) and any leading dimension ≥ N (odd values and
 * column-offset views included); arg stays int32, the workspace that of mi_spmm_csr_reduce_workspace_bytes (its
 * (value, arg) partials stay fp32 / int32: one size for every dtype).  The rule of the low-precision section above: the
 * fp32 result of the exactly widened operands (up), narrowed ONCE, at the store (rne_T; NaN stays NaN, its payload is not
 * part of the contract; fp16 overflow goes to ±inf).  Each entry takes the argument list of its _f32 twin and validates it
 * the same way, before any HIP call.
 *   MI_REDUCE_SUM   the bits of mi_spmm_csr_ex_T (MI_LONG_ROWS_SPLIT with a workspace, MI_LONG_ROWS_NONE without).
 *   MI_REDUCE_MEAN  C = rne_T(C32 / count): C32 the fp32 sum of mi_spmm_csr_ex_T's contract (long rows split, the
 *                   CSR-order fmaf chain, the butterfly for N < 4), "/" the correctly rounded fp32 division of
 *                   mi_spmm_rows_divide_f32, an empty row +0.  ONE narrowing: the sum is NOT narrowed to T and then
 *                   divided (that is a second rounding and other bits).  The division is the epilogue of the sum kernels.
 *   MI_REDUCE_AMAX / _AMIN  p_e = up(val[e]) · up(B[col[e], j]), one fp32 multiply (exact for both types wherever it
 *                   neither overflows nor underflows fp32); the selection rule of mi_spmm_csr_reduce_f32 applied to these
 *                   fp32 products; C = rne_T(p_arg) and arg the fp32 path's arg for the widened operands — never a choice
 *                   among values that only tie after narrowing.  fp16: a selected product beyond 65504 is stored as ±inf
 *                   while arg stays the fp32 choice.
 * mi_spmm_rows_divide_T: out = rne_T(up(in) / count), rows without entries copied; in == out allowed.
 * mi_spmm_reduce_grad_val_T = rne_T(mi_spmm_reduce_grad_val_f32(up(B), up(G), arg)) and mi_spmm_reduce_grad_b_T =
 * rne_T(mi_spmm_reduce_grad_b_f32(up(val), up(G), arg)): the fp32 kernels' summation orders, no float atomics.
 * The gradient of MEAN (matmuls.sparse_mm_reduce): g' = rne_T(up(g) / count) is materialised in T by
 * mi_spmm_rows_divide_T, then the T sum backward runs on g' (mi_sddmm_csr_T; mi_spmm_csr_ex_T on Aᵀ) — this extra rounding
 * of g' is part of the contract.
 * ------------------------------------------------------------------------ */
int mi_spmm_csr_reduce_bf16(const int32_t* rowptr, const int32_t* col, const uint16_t* val, int64_t nnz,
                            int32_t M, int32_t K, int32_t N, const uint16_t* B, int64_t ldb, uint16_t* C,
                            int64_t ldc, int32_t* arg, int64_t ldarg, int reduce, void* workspace,
                            size_t workspace_bytes, mi_stream_t stream);
int mi_spmm_csr_reduce_f16(const int32_t* rowptr, const int32_t* col, const uint16_t* val, int64_t nnz,
                           int32_t M, int32_t K, int32_t N, const uint16_t* B, int64_t ldb, uint16_t* C,
                           int64_t ldc, int32_t* arg, int64_t ldarg, int reduce, void* workspace,
                           size_t workspace_bytes, mi_stream_t stream);
int mi_spmm_rows_divide_bf16(const int32_t* rowptr, int32_t M, int32_t N, const uint16_t* in, int64_t ldin,
                             uint16_t* out, int64_t ldout, mi_stream_t stream);
int mi_spmm_rows_divide_f16(const int32_t* rowptr, int32_t M, int32_t N, const uint16_t* in, int64_t ldin,
                            uint16_t* out, int64_t ldout, mi_stream_t stream);
int mi_spmm_reduce_grad_val_bf16(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t M, int32_t K,
                                 int32_t N, const uint16_t* B, int64_t ldb, const uint16_t* G, int64_t ldg,
                                 const int32_t* arg, int64_t ldarg, uint16_t* grad_val, mi_stream_t stream);
int mi_spmm_reduce_grad_val_f16(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t M, int32_t K,
                                int32_t N, const uint16_t* B, int64_t ldb, const uint16_t* G, int64_t ldg,
                                const int32_t* arg, int64_t ldarg, uint16_t* grad_val, mi_stream_t stream);
int mi_spmm_reduce_grad_b_bf16(const int32_t* t_rowptr, const int32_t* t_col, const int32_t* perm,
                               const uint16_t* val, int64_t nnz, int32_t M, int32_t K, int32_t N,
                               const uint16_t* G, int64_t ldg, const int32_t* arg, int64_t ldarg,
                               uint16_t* grad_b, int64_t ldgb, mi_stream_t stream);
int mi_spmm_reduce_grad_b_f16(const int32_t* t_rowptr, const int32_t* t_col, const int32_t* perm,
                              const uint16_t* val, int64_t nnz, int32_t M, int32_t K, int32_t N,
                              const uint16_t* G, int64_t ldg, const int32_t* arg, int64_t ldarg,
                              uint16_t* grad_b, int64_t ldgb, mi_stream_t stream);

/* ------------------------------------------------------------------------ *
 * CSR row softmax — NEW relative to the reference: torch.sparse.softmax(A, dim = -1) for a CSR tensor (torch implements it
 * for COO only; DGL / PyG call it "edge softmax"), and its backward.  The softmax runs over the STORED entries of each
 * row: explicit zeros are entries like any other, duplicate columns are separate entries, an empty row writes nothing.
 * The columns are never read, so the entries take the offsets and the values only.
 *   rowptr  int32 [batch, M + 1], item i's offsets with its base added (the "rowptr of rowptrs" layout of
 *           mi_spmm_csr_batched_f32): row r of item i is rowptr[i·(M+1) + r] … rowptr[i·(M+1) + r + 1].  batch = 1: a 2-d CSR.
 *   nnz     the number of stored entries (an upper bound is enough: it only picks the lane-group width)
 *   forward   y_p  = e_p / Σ_q e_q,  e_p = exp(t_p − max_q t_q),  t_p = fl32(scale · x_p)
 *   backward  dx_p = scale · y_p · (dy_p − Σ_q dy_q · y_q)   from the forward's OUTPUT y
 * Arithmetic and order (the bits of a row depend on that row's entries and `scale` alone — not on the lane-group width
 * the launch took, on neighbouring rows, or on batch / M): t_p is one fp32 multiply, never fused; the maximum is exact and
 * skips NaN; e_p = E + E·lo with E = expf(hi) (the accurate exponential) and hi + lo = t_p − m exactly (two-sum: the
 * subtraction's rounding, half an ulp of a difference of up to 64, would otherwise dominate the error); entry p goes into chain p mod 64, a chain starts at +0 and
 * adds in increasing p; the 64 chains are combined by the xor tree c_i ← c_i + c_(i xor d), d = 32, 16, 8, 4, 2, 1;
 * y_p = fl(e_p · fl(1 / s)).  Backward: the chains take fmaf(dy_p, y_p, chain), the same tree gives d, and
 * dx_p = fl(scale · fl(y_p · fl(dy_p − d))).  No float atomics; the same bits on every run.
 * Special values follow that arithmetic, as torch.softmax of the row's entries: an explicit −inf entry gives 0; a row
 * holding a NaN or a +inf gives NaN in every entry; a row of only −inf gives NaN.
 * bfloat16 / float16 (T; uint16_t bit patterns, 2-byte aligned — an odd pointer → MI_EINVAL): the rule of the
 * low-precision section: entries widened exactly, every operation in fp32, one rounding at the store —
 *   mi_csr_softmax_T(x) == rne_T(mi_csr_softmax_f32(up(x)))  and
 *   mi_csr_softmax_backward_T(y, dy) == rne_T(mi_csr_softmax_backward_f32(up(y), up(dy)))   bit for bit.
 * In place is allowed: y may be x, dx may be dy (or y).
 * Rows of any length (10⁶ entries and more) are served by the one launch: up to 8 entries per lane of a row's lane group
 * in registers (read once, written once), up to 4096 (backward: 2048) entries through one workgroup's LDS (read once,
 * written once), longer ones streamed by that workgroup (three reads, one write).
 * mi_csr_softmax_workspace_bytes is 0: no entry uses a workspace; `workspace` / `workspace_bytes` are accepted for the
 * uniform argument list and ignored.  No host synchronisation, no read-back: graph-capturable.
 * Validation before any HIP call: negative nnz / batch / M → MI_EINVAL; nnz ≥ 2³¹ or batch·(M+1) ≥ 2³¹ → MI_ERANGE;
 * nnz == 0, batch == 0 or M == 0 → MI_OK, nothing touched; a NULL rowptr / x / y / dy / dx with work to do → MI_EINVAL.
 * ------------------------------------------------------------------------ */
size_t mi_csr_softmax_workspace_bytes(int64_t nnz, int32_t batch, int32_t M);
int mi_csr_softmax_f32(const int32_t* rowptr, int64_t nnz, int32_t batch, int32_t M, const float* x, float scale,
                       float* y, void* workspace, size_t workspace_bytes, mi_stream_t stream);
int mi_csr_softmax_bf16(const int32_t* rowptr, int64_t nnz, int32_t batch, int32_t M, const uint16_t* x, float scale,
                        uint16_t* y, void* workspace, size_t workspace_bytes, mi_stream_t stream);
int mi_csr_softmax_f16(const int32_t* rowptr, int64_t nnz, int32_t batch, int32_t M, const uint16_t* x, float scale,
                       uint16_t* y, void* workspace, size_t workspace_bytes, mi_stream_t stream);
int mi_csr_softmax_backward_f32(const int32_t* rowptr, int64_t nnz, int32_t batch, int32_t M, const float* y,
                                const float* dy, float scale, float* dx, void* workspace, size_t workspace_bytes,
                                mi_stream_t stream);
int mi_csr_softmax_backward_bf16(const int32_t* rowptr, int64_t nnz, int32_t batch, int32_t M, const uint16_t* y,
                                 const uint16_t* dy, float scale, uint16_t* dx, void* workspace, size_t workspace_bytes,
                                 mi_stream_t stream);
int mi_csr_softmax_backward_f16(const int32_t* rowptr, int64_t nnz, int32_t batch, int32_t M, const uint16_t* y,
                                const uint16_t* dy, float scale, uint16_t* dx, void* workspace, size_t workspace_bytes,
                                mi_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Fused sparse attention — NEW relative to the reference: out = softmax(scale · q·kᵀ restricted to a CSR pattern) · v in
 * ONE launch, and the row side of its backward in ONE launch; no score or probability array is written forward.  The
 * result has the bits of the three entries it replaces, run one after the other (mi_sddmm_csr_T → mi_csr_softmax_T →
 * mi_spmm_csr_T), and the backward those of their backward entries:
 *   rowptr  int32 [batch, M + 1] with the items' bases (the layout of mi_csr_softmax_T; batch = 1: a 2-d pattern);
 *   col     int32 [nnz], item-local columns in [0, K), any order, duplicates allowed (entries like any other);
 *   q [batch][M][D], k and v [batch][K][D], out [batch][M][D]: leading dimension ld ≥ D and item stride in elements; rows
 *           16-byte aligned (T: 8-byte) — base, ld and stride; D a multiple of 4 (T: of 8) in 8 … 128, else MI_EINVAL;
 *   stats   float [batch·M][2] = (m, 1 / s) of every row (forward: written, may be NULL; backward: read, required).
 * Order, per row r with entries p in CSR order:
 *   s_p   = the SDDMM order of mi_sddmm_csr_f32: lane l of 64 chains columns 4l + c (c = 0 … 3) with fmaf from +0, lanes
 *           beyond D / 4 hold +0, xor tree 32 … 1 (the steps that meet only empty lanes add +0 and are kept);
 *   t_p   = fl(scale · s_p), never fused; m = max t_p; e_p = the two-sum exponential of mi_csr_softmax_f32; chain p mod 64
 *           from +0 in increasing p, xor tree 32 … 1 → s; y_p = fl(e_p · fl(1 / s));
 *   out[r, j] = ONE fmaf chain from +0 over the row's entries in CSR order, for every row length — the plain order of
 *           mi_spmm_csr_f32 / mi_spmm_csr_batched_f32.  mi_spmm_csr_f32 itself splits rows beyond
 *           mi_spmm_long_row_threshold() (8192) entries under its AUTO rule: such rows differ from the 2-d composition;
 *   backward  t_p, y_p as above (recomputed from q, k and the row's stats: the same bits); dP_p = the SDDMM order on
 *           (dO[r, :], v[col_p, :]); d = the chains fmaf(dP_p, y_p, ·) p mod 64 and their tree;
 *           dS_p = fl(scale · fl(y_p · fl(dP_p − d))); dq[r, :] = the CSR-order fmaf chain of dS_p · k[col_p, :].
 *           y [nnz] and dS [nnz] are written in CSR order for the column-side products dv = Pᵀ·dO and dk = dSᵀ·q, which
 *           run on the transposed pattern through mi_spmm_csr_T / mi_spmm_csr_batched_f32.
 * bfloat16 / float16 (T): every stage in fp32 on exactly widened inputs, narrowed (rne) once per stage — s, y, dP and dS
 * in registers between the stages, out, dq, y and dS at the store: the 2-d composition in T, bit for bit, for any batch.
 * Special values follow the arithmetic: a −inf score gives probability 0; a NaN or +inf score gives a NaN row; a row whose
 * scores are all −inf gives NaN.  A row without entries gives a zero row of out and dq.
 * Row lengths: up to 2048 entries (backward: 1024) stay in the wave's LDS slice; longer rows are streamed by the same
 * wave with recomputation (forward three score passes, backward two).  Any length, one launch, no read-back.
 * mi_sparse_attention_workspace_bytes is 0; `workspace` / `workspace_bytes` are accepted and ignored.  No atomics, no host
 * synchronisation: graph-capturable; the same bits on every run, whatever the neighbouring rows or the batch.
 * Validation before any HIP call: a negative size → MI_EINVAL; nnz ≥ 2³¹ or batch·(M+1) ≥ 2³¹ → MI_ERANGE; an unsupported
 * D → MI_EINVAL; batch == 0 or M == 0 → MI_OK, nothing touched (nnz == 0 with rows: zero rows are written); a NULL or
 * misaligned pointer, ld < D, or K == 0 with entries → MI_EINVAL.
 * ------------------------------------------------------------------------ */
size_t mi_sparse_attention_workspace_bytes(int64_t nnz, int32_t batch, int32_t M, int32_t D);
int mi_sparse_attention_f32(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t batch, int32_t M, int32_t K,
                            int32_t D, const float* q, int64_t ldq, int64_t strideQ, const float* k, int64_t ldk,
                            int64_t strideK, const float* v, int64_t ldv, int64_t strideV, float scale, float* out,
                            int64_t ldo, int64_t strideO, float* stats, void* workspace, size_t workspace_bytes,
                            mi_stream_t stream);
int mi_sparse_attention_backward_f32(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t batch, int32_t M,
                                     int32_t K, int32_t D, const float* q, int64_t ldq, int64_t strideQ, const float* k,
                                     int64_t ldk, int64_t strideK, const float* v, int64_t ldv, int64_t strideV,
                                     const float* dout, int64_t lddo, int64_t strideDO, const float* stats, float scale,
                                     float* dq, int64_t lddq, int64_t strideDQ, float* y, float* ds, void* workspace,
                                     size_t workspace_bytes, mi_stream_t stream);
int mi_sparse_attention_bf16(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t batch, int32_t M, int32_t K,
                            int32_t D, const uint16_t* q, int64_t ldq, int64_t strideQ, const uint16_t* k, int64_t ldk,
                            int64_t strideK, const uint16_t* v, int64_t ldv, int64_t strideV, float scale, uint16_t* out,
                            int64_t ldo, int64_t strideO, float* stats, void* workspace, size_t workspace_bytes,
                            mi_stream_t stream);
int mi_sparse_attention_backward_bf16(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t batch, int32_t M,
                                     int32_t K, int32_t D, const uint16_t* q, int64_t ldq, int64_t strideQ, const uint16_t* k,
                                     int64_t ldk, int64_t strideK, const uint16_t* v, int64_t ldv, int64_t strideV,
                                     const uint16_t* dout, int64_t lddo, int64_t strideDO, const float* stats, float scale,
                                     uint16_t* dq, int64_t lddq, int64_t strideDQ, uint16_t* y, uint16_t* ds, void* workspace,
                                     size_t workspace_bytes, mi_stream_t stream);
int mi_sparse_attention_f16(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t batch, int32_t M, int32_t K,
                            int32_t D, const uint16_t* q, int64_t ldq, int64_t strideQ, const uint16_t* k, int64_t ldk,
                            int64_t strideK, const uint16_t* v, int64_t ldv, int64_t strideV, float scale, uint16_t* out,
                            int64_t ldo, int64_t strideO, float* stats, void* workspace, size_t workspace_bytes,
                            mi_stream_t stream);
int mi_sparse_attention_backward_f16(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t batch, int32_t M,
                                     int32_t K, int32_t D, const uint16_t* q, int64_t ldq, int64_t strideQ, const uint16_t* k,
                                     int64_t ldk, int64_t strideK, const uint16_t* v, int64_t ldv, int64_t strideV,
                                     const uint16_t* dout, int64_t lddo, int64_t strideDO, const float* stats, float scale,
                                     uint16_t* dq, int64_t lddq, int64_t strideDQ, uint16_t* y, uint16_t* ds, void* workspace,
                                     size_t workspace_bytes, mi_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Block-sparse attention on the matrix cores — NEW relative to the reference: out = softmax(scale · q·kᵀ + mask) · v in
 * bfloat16 / float16 (T, 2-byte bit patterns), where the mask keeps the 64 × 64 blocks a CSR block layout lists and,
 * with causal != 0, the positions j ≤ i; and its backward:
 *   rowptr   int32 [layouts][Sq/64 + 1] with the layouts' bases, col int32 [nnz] layout-local key blocks in any order
 *            (a duplicate block is unsupported: it would count twice); item i of the batch uses layout i mod layouts;
 *   t_rowptr int32 [layouts][Sk/64 + 1], t_col [nnz]: the transposed lists (backward: key block → its query blocks);
 *   q, out, dout, dq [batch][Sq][D]; k, v, dk, dv [batch][Sk][D]: leading dimension ld ≥ D and item stride in elements,
 *            base 16-byte aligned, ld and stride multiples of 8; D ∈ {32, 64, 96, 128}; Sq, Sk multiples of 64;
 *   lse      float [batch][Sq], 16-byte aligned: m + ln Σ exp(t − m) of every query row, −inf for a row that sees nothing
 *            (forward: written; backward: read);
 *   workspace (backward) mi_block_attention_workspace_bytes(batch, Sq) bytes, 16-byte aligned: δ = rowsum(dO ∘ O).
 * Arithmetic: every product is v_mfma_f32_16x16x32_T with fp32 accumulators; scores, maxima, sums, lse and δ stay fp32;
 * P is narrowed to T only as the operand of P·V / dOᵀ·P, dS only as the operand of dS·K / dSᵀ·Q; out, dq, dk, dv are
 * rounded once at the store.  A query block walks its list in CSR order with the online softmax (running maximum and
 * sum); the backward recomputes P = exp(t − lse) per tile (a −inf lse gives 0); dk and dv are summed per key block over
 * the transposed list in its order.  Blocks outside the list are never read; causal skips listed blocks above the
 * diagonal (needs Sq == Sk).  A row that sees nothing gives zero rows of out and dq, a key nobody sees zero rows of dk
 * and dv.  No atomics, no host synchronisation: graph-capturable; the bits of an output depend on its item and its
 * layout only.  A listed block outside the grid is skipped, offsets are clamped to [0, nnz].
 * Validation before any HIP call: a negative size, an unsupported D, Sq or Sk not a multiple of 64, causal with
 * Sq != Sk → MI_EINVAL; nnz ≥ 2³¹ → MI_ERANGE; batch == 0 or Sq == 0 → MI_OK, nothing touched; layouts == 0, a NULL or
 * misaligned pointer, ld < D, Sk == 0 with entries → MI_EINVAL; a short workspace → MI_ENOMEM.
 * ------------------------------------------------------------------------ */
size_t mi_block_attention_workspace_bytes(int32_t batch, int32_t Sq);
int mi_block_attention_fwd_bf16(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t layouts, int32_t batch,
                                int32_t Sq, int32_t Sk, int32_t D, int32_t causal, const uint16_t* q, int64_t ldq,
                                int64_t strideQ, const uint16_t* k, int64_t ldk, int64_t strideK, const uint16_t* v,
                                int64_t ldv, int64_t strideV, float scale, uint16_t* out, int64_t ldo, int64_t strideO,
                                float* lse, mi_stream_t stream);
int mi_block_attention_fwd_f16(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t layouts, int32_t batch,
                               int32_t Sq, int32_t Sk, int32_t D, int32_t causal, const uint16_t* q, int64_t ldq,
                               int64_t strideQ, const uint16_t* k, int64_t ldk, int64_t strideK, const uint16_t* v,
                               int64_t ldv, int64_t strideV, float scale, uint16_t* out, int64_t ldo, int64_t strideO,
                               float* lse, mi_stream_t stream);
int mi_block_attention_bwd_bf16(const int32_t* rowptr, const int32_t* col, const int32_t* t_rowptr, const int32_t* t_col,
                                int64_t nnz, int32_t layouts, int32_t batch, int32_t Sq, int32_t Sk, int32_t D,
                                int32_t causal, const uint16_t* q, int64_t ldq, int64_t strideQ, const uint16_t* k,
                                int64_t ldk, int64_t strideK, const uint16_t* v, int64_t ldv, int64_t strideV,
                                const uint16_t* out, int64_t ldo, int64_t strideO, const uint16_t* dout, int64_t lddo,
                                int64_t strideDO, const float* lse, float scale, uint16_t* dq, int64_t lddq,
                                int64_t strideDQ, uint16_t* dk, int64_t lddk, int64_t strideDK, uint16_t* dv, int64_t lddv,
                                int64_t strideDV, void* workspace, size_t workspace_bytes, mi_stream_t stream);
int mi_block_attention_bwd_f16(const int32_t* rowptr, const int32_t* col, const int32_t* t_rowptr, const int32_t* t_col,
                               int64_t nnz, int32_t layouts, int32_t batch, int32_t Sq, int32_t Sk, int32_t D,
                               int32_t causal, const uint16_t* q, int64_t ldq, int64_t strideQ, const uint16_t* k,
                               int64_t ldk, int64_t strideK, const uint16_t* v, int64_t ldv, int64_t strideV,
                               const uint16_t* out, int64_t ldo, int64_t strideO, const uint16_t* dout, int64_t lddo,
                               int64_t strideDO, const float* lse, float scale, uint16_t* dq, int64_t lddq,
                               int64_t strideDQ, uint16_t* dk, int64_t lddk, int64_t strideDK, uint16_t* dv, int64_t lddv,
                               int64_t strideDV, void* workspace, size_t workspace_bytes, mi_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Block-sparse attention with grouped-query heads and per-item lengths: the entries above with four more
 * arguments in front of the stream.  Everything said there holds; in addition:
 *   group      ≥ 1: query items per k / v item.  batch counts QUERY items (q, out, dout, dq, lse, the workspace and the
 *              layouts — item i uses layout i mod layouts — are indexed by them); k, v, dk and dv have batch / group items
 *              and query item i reads k / v item i / group (heads of a group adjacent: torch's enable_gqa convention).
 *              dk and dv of a k / v item are summed over its group's query items in ascending order and, within each,
 *              over that item's transposed list in its order — one fp32 accumulator of one wave, rounded once;
 *   q_lens,
 *   k_lens     int32 [lens_count] on the device, 4-byte aligned, each nullable (NULL: every position of that side exists);
 *              query item i has the lengths of entry i / (batch / lens_count).  A length is clamped to [0, Sq] / [0, Sk]
 *              where it is read.  Query position r exists iff r < q_len, key position j iff j < k_len: the softmax of a row
 *              runs over the visible AND existing keys; a query row at or beyond q_len gives a zero row of out and dq and
 *              −inf as its lse (δ in the workspace: 0) and adds nothing to dk / dv; a key at or beyond k_len gets zero
 *              rows of dk / dv.  A listed block wholly beyond a length is skipped like an unlisted one; in a block that
 *              straddles a length the rows beyond it enter no product, whatever memory holds there (NaN included);
 *   lens_count the entries of q_lens / k_lens; ignored when both are NULL.
 * Validation before any HIP call, beside the plain entries': group < 1, batch % group != 0; with a length array:
 * lens_count < 1, batch % lens_count != 0, (batch / lens_count) % group != 0 (the heads of a group share one length), a
 * misaligned length pointer → MI_EINVAL.  The plain entries are the group = 1, q_lens = k_lens = NULL case of these.
 * ------------------------------------------------------------------------ */
int mi_block_attention_fwd_ex_bf16(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t layouts, int32_t batch,
                                   int32_t Sq, int32_t Sk, int32_t D, int32_t causal, const uint16_t* q, int64_t ldq,
                                   int64_t strideQ, const uint16_t* k, int64_t ldk, int64_t strideK, const uint16_t* v,
                                   int64_t ldv, int64_t strideV, float scale, uint16_t* out, int64_t ldo, int64_t strideO,
                                   float* lse, int32_t group, const int32_t* q_lens, const int32_t* k_lens,
                                   int32_t lens_count, mi_stream_t stream);
int mi_block_attention_fwd_ex_f16(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t layouts, int32_t batch,
                                  int32_t Sq, int32_t Sk, int32_t D, int32_t causal, const uint16_t* q, int64_t ldq,
                                  int64_t strideQ, const uint16_t* k, int64_t ldk, int64_t strideK, const uint16_t* v,
                                  int64_t ldv, int64_t strideV, float scale, uint16_t* out, int64_t ldo, int64_t strideO,
                                  float* lse, int32_t group, const int32_t* q_lens, const int32_t* k_lens,
                                  int32_t lens_count, mi_stream_t stream);
int mi_block_attention_bwd_ex_bf16(const int32_t* rowptr, const int32_t* col, const int32_t* t_rowptr, const int32_t* t_col,
                                   int64_t nnz, int32_t layouts, int32_t batch, int32_t Sq, int32_t Sk, int32_t D,
                                   int32_t causal, const uint16_t* q, int64_t ldq, int64_t strideQ, const uint16_t* k,
                                   int64_t ldk, int64_t strideK, const uint16_t* v, int64_t ldv, int64_t strideV,
                                   const uint16_t* out, int64_t ldo, int64_t strideO, const uint16_t* dout, int64_t lddo,
                                   int64_t strideDO, const float* lse, float scale, uint16_t* dq, int64_t lddq,
                                   int64_t strideDQ, uint16_t* dk, int64_t lddk, int64_t strideDK, uint16_t* dv, int64_t lddv,
                                   int64_t strideDV, void* workspace, size_t workspace_bytes, int32_t group,
                                   const int32_t* q_lens, const int32_t* k_lens, int32_t lens_count, mi_stream_t stream);
int mi_block_attention_bwd_ex_f16(const int32_t* rowptr, const int32_t* col, const int32_t* t_rowptr, const int32_t* t_col,
                                  int64_t nnz, int32_t layouts, int32_t batch, int32_t Sq, int32_t Sk, int32_t D,
                                  int32_t causal, const uint16_t* q, int64_t ldq, int64_t strideQ, const uint16_t* k,
                                  int64_t ldk, int64_t strideK, const uint16_t* v, int64_t ldv, int64_t strideV,
                                  const uint16_t* out, int64_t ldo, int64_t strideO, const uint16_t* dout, int64_t lddo,
                                  int64_t strideDO, const float* lse, float scale, uint16_t* dq, int64_t lddq,
                                  int64_t strideDQ, uint16_t* dk, int64_t lddk, int64_t strideDK, uint16_t* dv, int64_t lddv,
                                  int64_t strideDV, void* workspace, size_t workspace_bytes, int32_t group,
                                  const int32_t* q_lens, const int32_t* k_lens, int32_t lens_count, mi_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Block-sparse attention for decoding: the T newest tokens of every item against a key / value cache,
 * forward only, in bfloat16 / float16 (2-byte bit patterns).  Token t of k / v item c stands at pos = k_len − T + t and
 * sees key j iff j ≤ pos and the layout lists 64-block (pos / 64, j / 64); a token with pos < 0, or one that sees nothing,
 * gives a zero row of out and −inf as its lse.
 *   rowptr, col, nnz, layouts   the block lists of mi_block_attention_fwd_* over Smax/64 × Smax/64 blocks; k / v item c
 *              uses layout c mod layouts — the `group` query heads of a k / v head share its layout;
 *   items, heads   items = B · heads k / v items; item c is head c % heads of batch item c / heads.  items, T ≤ 65535;
 *   q, out     query item c · group + g (g < group), token t: q + (c · group + g) · strideQ + t · ldq, D elements; out
 *              likewise with ldo, strideO; 16-byte aligned, ld ≥ D, ld and stride multiples of 8;
 *   k, v       the cache, never copied: key j of item c at k + (c / heads) · batchK + (c % heads) · headK + j · ldk; 16-byte
 *              aligned, ldk ≥ D, every stride a multiple of 8 elements ([B, heads, Smax, D] and [B, Smax, heads, D] both fit);
 *   k_lens     int32 [lens_count] on the device, required; item c has entry c / (items / lens_count); clamped to [0, Smax];
 *   group      query heads per k / v head, 1 … 16: the own rows of ONE 16-row MFMA tile, a k / v tile read once for all;
 *   chunk      ≥ 1: the list of layout row pos / 64 is cut into chunks of `chunk` consecutive entries by list position
 *              (skipped entries do not move the cut); one workgroup per chunk, its four waves taking entries w, w + 4, …;
 *              partials (maximum, sum, fp32 accumulator) are merged in ascending wave order, then in ascending chunk order
 *              by a second launch (none when Smax/64 ≤ chunk); out is rounded once.  The bits of a row depend on its own
 *              item's operands, its list, pos and chunk only.  No atomics, no read-back: graph-capturable;
 *   lse        float32 [items · group][T];
 *   workspace  mi_block_attention_decode_workspace_bytes(...) bytes, 16-byte aligned: `group` rows of D + 2 floats per
 *              (item, token, chunk); 0 bytes (may be NULL) when there is one chunk.
 * Validation before any HIP call: group outside [1, 16], D ∉ {32, 64, 96, 128}, chunk < 1, Smax not a multiple of 64, items or
 * T > 65535, items % heads != 0, lens_count < 1 or items % lens_count != 0, a NULL / misaligned pointer, a stride that is
 * not a multiple of 8 or a leading dimension < D → MI_EINVAL; a short workspace → MI_ENOMEM; items == 0 or T == 0 → MI_OK,
 * nothing touched.  Offsets are clamped to nnz and a column outside the grid is skipped.
 * ------------------------------------------------------------------------ */
size_t mi_block_attention_decode_workspace_bytes(int32_t items, int32_t T, int32_t group, int32_t D, int32_t Smax,
                                                 int32_t chunk);
int mi_block_attention_decode_bf16(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t layouts, int32_t items,
                                   int32_t heads, int32_t T, int32_t Smax, int32_t D, const uint16_t* q, int64_t ldq,
                                   int64_t strideQ, const uint16_t* k, int64_t ldk, int64_t headK, int64_t batchK,
                                   const uint16_t* v, int64_t ldv, int64_t headV, int64_t batchV, const int32_t* k_lens,
                                   int32_t lens_count, int32_t group, int32_t chunk, float scale, uint16_t* out, int64_t ldo,
                                   int64_t strideO, float* lse, void* workspace, size_t workspace_bytes, mi_stream_t stream);
int mi_block_attention_decode_f16(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t layouts, int32_t items,
                                  int32_t heads, int32_t T, int32_t Smax, int32_t D, const uint16_t* q, int64_t ldq,
                                  int64_t strideQ, const uint16_t* k, int64_t ldk, int64_t headK, int64_t batchK,
                                  const uint16_t* v, int64_t ldv, int64_t headV, int64_t batchV, const int32_t* k_lens,
                                  int32_t lens_count, int32_t group, int32_t chunk, float scale, uint16_t* out, int64_t ldo,
                                  int64_t strideO, float* lse, void* workspace, size_t workspace_bytes, mi_stream_t stream);

/* ------------------------------------------------------------------------ *
 * … over a paged cache: mi_block_attention_decode_* with k and v given as ONE POOL OF PAGES and a block
 * table per batch item.  The arguments are those of mi_block_attention_decode_* except:
 *   k_pages, v_pages   the pool, never copied: row r of head h of pool page e at k_pages + e · pageK + h · headK + r · ldk
 *              (v likewise); 16-byte aligned, ldk ≥ D, every stride a multiple of 8 elements ([P, heads, page, D] and
 *              [P, page, heads, D] both fit).  With pages == 0 the pool is never read and may be NULL;
 *   block_table, table_ld   int32 on the device, 4-byte aligned: row c / heads, table_ld ≥ Smax / page entries apart, holds
 *              the pool page of each of the item's Smax / page logical pages — all heads of a batch item share its row.
 *              Key j of k / v item c is row j % page of head c % heads of pool page block_table[(c / heads) · table_ld +
 *              j / page].  An entry outside [0, pages) makes the keys of its logical page INVISIBLE: nothing is loaded,
 *              their scores are −inf.  Entries of pages wholly beyond pos or only in unlisted blocks are never read;
 *   pages      pool pages P ≥ 0;
 *   page       keys per page: a power of two ≥ 16.  Smax, the logical length, is a multiple of page (and of 64).
 * For a pool and table whose seen entries are in range, out and lse have the bits of mi_block_attention_decode_* with the
 * same chunk on the gathered cache — independent of pages, of where the pages lie and of page.  The workspace is that of
 * mi_block_attention_decode_workspace_bytes.  No atomics, no read-back: graph-capturable while k_lens, the pool and the
 * table are updated in place.
 * Validation before any HIP call: everything mi_block_attention_decode_* refuses, page < 16 or not a power of two,
 * Smax % page != 0, pages < 0, a NULL or misaligned block_table (with Smax > 0), table_ld < Smax / page, a NULL / misaligned
 * pool pointer or a bad pool stride (with pages > 0) → MI_EINVAL; a short workspace → MI_ENOMEM.
 * ------------------------------------------------------------------------ */
int mi_block_attention_decode_paged_bf16(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t layouts, int32_t items,
                                         int32_t heads, int32_t T, int32_t Smax, const int32_t* block_table, int64_t table_ld,
                                         int32_t pages, int32_t page, int32_t D, const uint16_t* q, int64_t ldq, int64_t strideQ,
                                         const uint16_t* k_pages, int64_t ldk, int64_t headK, int64_t pageK,
                                         const uint16_t* v_pages, int64_t ldv, int64_t headV, int64_t pageV,
                                         const int32_t* k_lens, int32_t lens_count, int32_t group, int32_t chunk, float scale,
                                         uint16_t* out, int64_t ldo, int64_t strideO, float* lse, void* workspace,
                                         size_t workspace_bytes, mi_stream_t stream);
int mi_block_attention_decode_paged_f16(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t layouts, int32_t items,
                                        int32_t heads, int32_t T, int32_t Smax, const int32_t* block_table, int64_t table_ld,
                                        int32_t pages, int32_t page, int32_t D, const uint16_t* q, int64_t ldq, int64_t strideQ,
                                        const uint16_t* k_pages, int64_t ldk, int64_t headK, int64_t pageK,
                                        const uint16_t* v_pages, int64_t ldv, int64_t headV, int64_t pageV,
                                        const int32_t* k_lens, int32_t lens_count, int32_t group, int32_t chunk, float scale,
                                        uint16_t* out, int64_t ldo, int64_t strideO, float* lse, void* workspace,
                                        size_t workspace_bytes, mi_stream_t stream);

/* ------------------------------------------------------------------------ *
 * … over an FP8 cache: mi_block_attention_decode_* and mi_block_attention_decode_paged_* with k and v (or
 * the pool) stored as OCP e4m3fn bytes — gfx950's native 8-bit float; not the FNUZ encoding, not e5m2 — and a float32 scale
 * per k / v head.  q, out, lse and every other argument are the parents'; the differences:
 *   k, v / k_pages, v_pages   bytes, never copied; the strides are in elements (= bytes): 16-byte aligned, ldk ≥ D, every
 *              stride a multiple of 16;
 *   k_scale, k_scale_count, v_scale, v_scale_count   float32 on the device, 4-byte aligned, read by the kernels and never
 *              read back; a count of 1: one scale for all heads, a count of `heads`: head c % heads has its own; NULL: 1.
 *              The real key is k8 · k_scale[h], the real value v8 · v_scale[h].  Non-finite or non-positive scales are the
 *              caller's business.
 * Arithmetic: every byte is widened to T in registers — exact: each finite e4m3fn code is a bfloat16 and a float16 — and the
 * statements of the parents follow, with two differences: a score is multiplied by scale · k_scale[h], ONE fp32 product taken
 * once per workgroup, in the place of scale; the stored element is narrow((O / L) · v_scale[h]), one rounding.  lse is that
 * of the real scores.  So with both scales NULL, out and lse have the bits of the parent on the widened cache with the same
 * chunk; with k_scale = s for all heads and v_scale = 2^n, out has the parent's bits at scale' = fl32(scale · s), times 2^n,
 * and lse the parent's bits; and the paged call has the bits of the contiguous one on the gathered cache.  P is never
 * narrowed to fp8 and no fp8 MFMA is used.  Nothing beyond pos, in an unlisted block, between the rows or in an invalid page
 * is loaded: a NaN byte (0x7F / 0xFF) there reaches no output.  Workspace: mi_block_attention_decode_workspace_bytes.
 * Graph-capturable while k_lens, the cache, the table and the scales are updated in place.
 * Validation before any HIP call: everything the parents refuse (with 16 for 8 in the cache's strides), a scale count other
 * than 1 or heads, a misaligned scale pointer → MI_EINVAL; a short workspace → MI_ENOMEM.
 * ------------------------------------------------------------------------ */
int mi_block_attention_decode_fp8_bf16(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t layouts,
                                       int32_t items, int32_t heads, int32_t T, int32_t Smax, int32_t D, const uint16_t* q,
                                       int64_t ldq, int64_t strideQ, const uint8_t* k, int64_t ldk, int64_t headK,
                                       int64_t batchK, const uint8_t* v, int64_t ldv, int64_t headV, int64_t batchV,
                                       const int32_t* k_lens, int32_t lens_count, int32_t group, int32_t chunk, float scale,
                                       const float* k_scale, int32_t k_scale_count, const float* v_scale,
                                       int32_t v_scale_count, uint16_t* out, int64_t ldo, int64_t strideO, float* lse,
                                       void* workspace, size_t workspace_bytes, mi_stream_t stream);
int mi_block_attention_decode_fp8_f16(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t layouts,
                                      int32_t items, int32_t heads, int32_t T, int32_t Smax, int32_t D, const uint16_t* q,
                                      int64_t ldq, int64_t strideQ, const uint8_t* k, int64_t ldk, int64_t headK,
                                      int64_t batchK, const uint8_t* v, int64_t ldv, int64_t headV, int64_t batchV,
                                      const int32_t* k_lens, int32_t lens_count, int32_t group, int32_t chunk, float scale,
                                      const float* k_scale, int32_t k_scale_count, const float* v_scale,
                                      int32_t v_scale_count, uint16_t* out, int64_t ldo, int64_t strideO, float* lse,
                                      void* workspace, size_t workspace_bytes, mi_stream_t stream);
int mi_block_attention_decode_paged_fp8_bf16(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t layouts,
                                             int32_t items, int32_t heads, int32_t T, int32_t Smax,
                                             const int32_t* block_table, int64_t table_ld, int32_t pages, int32_t page,
                                             int32_t D, const uint16_t* q, int64_t ldq, int64_t strideQ,
                                             const uint8_t* k_pages, int64_t ldk, int64_t headK, int64_t pageK,
                                             const uint8_t* v_pages, int64_t ldv, int64_t headV, int64_t pageV,
                                             const int32_t* k_lens, int32_t lens_count, int32_t group, int32_t chunk,
                                             float scale, const float* k_scale, int32_t k_scale_count, const float* v_scale,
                                             int32_t v_scale_count, uint16_t* out, int64_t ldo, int64_t strideO, float* lse,
                                             void* workspace, size_t workspace_bytes, mi_stream_t stream);
int mi_block_attention_decode_paged_fp8_f16(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t layouts,
                                            int32_t items, int32_t heads, int32_t T, int32_t Smax,
                                            const int32_t* block_table, int64_t table_ld, int32_t pages, int32_t page,
                                            int32_t D, const uint16_t* q, int64_t ldq, int64_t strideQ,
                                            const uint8_t* k_pages, int64_t ldk, int64_t headK, int64_t pageK,
                                            const uint8_t* v_pages, int64_t ldv, int64_t headV, int64_t pageV,
                                            const int32_t* k_lens, int32_t lens_count, int32_t group, int32_t chunk,
                                            float scale, const float* k_scale, int32_t k_scale_count, const float* v_scale,
                                            int32_t v_scale_count, uint16_t* out, int64_t ldo, int64_t strideO, float* lse,
                                            void* workspace, size_t workspace_bytes, mi_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Block-sparse prefill attention over the KV cache: the T ≥ 1 newest tokens of every item — a whole prompt
 * or one chunk of it — against the cache of mi_block_attention_decode_* in its four forms, forward only.  The rule is the
 * decode entries': token t of k / v item c stands at pos = clamp(k_len, 0, Smax) − T + t and sees key j iff j ≤ pos and the
 * layout lists 64-block (pos / 64, j / 64).  The arguments are the decode entries' without `chunk` and the workspace, with:
 *   q          read through its own strides, never copied: token t of query head g of k / v item c at q + (c / heads) · batchQ +
 *              ((c % heads) · group + g) · headQ + t · ldq, D elements; 16-byte aligned, every stride a non-negative multiple
 *              of 8 elements — q_out of mi_rope_kv_append_* and the q slice of a fused projection both fit;
 *   group      query heads per k / v head, any value ≥ 1; items and T have no bound but int32 (an item loop serves what
 *              lies beyond the grid);
 *   new_lens, new_lens_count   NULL, or int32 on the device, 4-byte aligned, 1 or items / heads entries: batch item b has
 *              n = clamp(new_lens[b], 0, T) new tokens, standing in the LAST n of the T slots (mi_rope_kv_append_*'s
 *              convention).  Slot t holds a token iff t ≥ T − n and pos ≥ 0;
 *   out, lse   out as in the decode entries, lse float32 [items · group][T].  EVERY row of both is written exactly once by
 *              the one launch: a slot without a token, and a token that sees nothing, get a zero row and −inf.
 * Order of summation: a workgroup owns the positions [64r, 64r + 64) ∩ [k_len − T, k_len) of one query head and walks the
 * list of layout row r in list order, as mi_block_attention_fwd_ex_* with causal = 1 and q_lens = k_lens walks it: for a cache
 * whose seen table entries are in range, the out and lse rows of existing tokens have the BITS of that entry on the gathered
 * (fp8: widened) cache with q scattered to its positions and the layout repeated per query head.  So a paged call has the
 * bits of the contiguous call on the gathered cache, an fp8 call with NULL scales those of the 2-byte call on the widened
 * cache, a strided cache those of its contiguous clone; a row's bits depend on its item's operands, its list and pos, never
 * on T, new_lens, the batch or the launch.  With scales: a score is multiplied by scale · k_scale[h], one fp32 product; with
 * a non-NULL v_scale the stored element is narrow(fl32((O / L) · v_scale[h])).
 * Never read: positions outside the listed blocks, blocks above the diagonal, positions at or beyond k_len (staged as
 * zeros), the gaps between rows, pages whose table entry lies outside [0, pages) — such an entry hides its page's keys.
 * No atomics, no workspace, no read-back: graph-capturable while k_lens, new_lens, the cache, the table and the scales
 * change in place.
 * Validation before any HIP call: what the decode entries refuse through the same cache checks (but no bound on group,
 * items or T), a misaligned new_lens or a count other than 1 or items / heads → MI_EINVAL; items == 0 or T == 0 → MI_OK,
 * nothing touched.
 * ------------------------------------------------------------------------ */
#define MI_BLOCK_ATTENTION_PREFILL_LIST \
  const int32_t *rowptr, const int32_t *col, int64_t nnz, int32_t layouts, int32_t items, int32_t heads, int32_t T, int32_t Smax
#define MI_BLOCK_ATTENTION_PREFILL_TABLE const int32_t *block_table, int64_t table_ld, int32_t pages, int32_t page
/* (paged: k, batchK, v, batchV of the operand list are k_pages, pageK, v_pages, pageV) */
#define MI_BLOCK_ATTENTION_PREFILL_OPERANDS(CT)                                                                                \
  const uint16_t *q, int64_t ldq, int64_t headQ, int64_t batchQ, const CT *k, int64_t ldk, int64_t headK, int64_t batchK,      \
      const CT *v, int64_t ldv, int64_t headV, int64_t batchV, const int32_t *k_lens, int32_t lens_count,                      \
      const int32_t *new_lens, int32_t new_lens_count, int32_t group, float scale
#define MI_BLOCK_ATTENTION_PREFILL_SCALES const float *k_scale, int32_t k_scale_count, const float *v_scale, int32_t v_scale_count
#define MI_BLOCK_ATTENTION_PREFILL_OUT uint16_t *out, int64_t ldo, int64_t strideO, float *lse, mi_stream_t stream
int mi_block_attention_prefill_bf16(MI_BLOCK_ATTENTION_PREFILL_LIST, int32_t D, MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint16_t),
                                    MI_BLOCK_ATTENTION_PREFILL_OUT);
int mi_block_attention_prefill_f16(MI_BLOCK_ATTENTION_PREFILL_LIST, int32_t D, MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint16_t),
                                   MI_BLOCK_ATTENTION_PREFILL_OUT);
int mi_block_attention_prefill_paged_bf16(MI_BLOCK_ATTENTION_PREFILL_LIST, MI_BLOCK_ATTENTION_PREFILL_TABLE, int32_t D,
                                          MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint16_t), MI_BLOCK_ATTENTION_PREFILL_OUT);
int mi_block_attention_prefill_paged_f16(MI_BLOCK_ATTENTION_PREFILL_LIST, MI_BLOCK_ATTENTION_PREFILL_TABLE, int32_t D,
                                         MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint16_t), MI_BLOCK_ATTENTION_PREFILL_OUT);
int mi_block_attention_prefill_fp8_bf16(MI_BLOCK_ATTENTION_PREFILL_LIST, int32_t D, MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint8_t),
                                        MI_BLOCK_ATTENTION_PREFILL_SCALES, MI_BLOCK_ATTENTION_PREFILL_OUT);
int mi_block_attention_prefill_fp8_f16(MI_BLOCK_ATTENTION_PREFILL_LIST, int32_t D, MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint8_t),
                                       MI_BLOCK_ATTENTION_PREFILL_SCALES, MI_BLOCK_ATTENTION_PREFILL_OUT);
int mi_block_attention_prefill_paged_fp8_bf16(MI_BLOCK_ATTENTION_PREFILL_LIST, MI_BLOCK_ATTENTION_PREFILL_TABLE, int32_t D,
                                              MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint8_t), MI_BLOCK_ATTENTION_PREFILL_SCALES,
                                              MI_BLOCK_ATTENTION_PREFILL_OUT);
int mi_block_attention_prefill_paged_fp8_f16(MI_BLOCK_ATTENTION_PREFILL_LIST, MI_BLOCK_ATTENTION_PREFILL_TABLE, int32_t D,
                                             MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint8_t), MI_BLOCK_ATTENTION_PREFILL_SCALES,
                                             MI_BLOCK_ATTENTION_PREFILL_OUT);

/* ------------------------------------------------------------------------ *
 * Split key walks for the prefill entries: a short chunk behind a long cached prefix has few position
 * tiles, so one workgroup per (tile, query head) leaves most of the chip idle.  These entries cut the list of a tile's
 * layout row BY LIST POSITION into parts of `split` entries — entry p of a list [beg, end) belongs to part (p − beg) / split;
 * a skipped entry (outside the grid, above the diagonal, beyond k_len) stays in its part — and give every (tile, query
 * head, part) to a workgroup of the first launch; a second launch merges the parts.  parts_max = ⌈(Smax / 64) / split⌉,
 * from the shape alone; with parts_max == 1 the call IS the unsplit entry: one launch, the workspace not looked at.
 *   split      ≥ 1, list entries of a part;
 *   workspace, workspace_bytes   16-byte aligned device memory of at least
 *              mi_block_attention_prefill_split_workspace_bytes(items, group, T, D, Smax, split) =
 *              items · group · (⌈T / 64⌉ + 1) · parts_max · 64 · (D + 2) · 4 bytes (0 when parts_max ≤ 1; MI_EINVAL for arguments
 *              the entries refuse, MI_ERANGE beyond int64).  Partial (query item, tile, part) holds o [64][D], then m [64],
 *              then l [64], float32; only partials of parts below ⌈(end − beg) / split⌉ of tiles that hold a token are
 *              written, by plain vector stores, and only those are read.  No memset, no atomics, no read-back.
 * The bits.  A part gives per own row the running maximum m, the row sum l and the unnormalised fp32 accumulator o of the
 * unsplit walk's statements over its entries in list order; a row without a token, or whose part computes nothing, gives
 * (−inf, 0) and zeros.  Parts merge in ascending order: M = max mᵢ, L = Σ lᵢ·wᵢ, O = Σ oᵢ·wᵢ with wᵢ = 1 if mᵢ == M, else
 * exp(mᵢ − M); the store is the unsplit entry's (narrow(O · (1 / L)), the scaled statement with a v_scale, lse = M + log L,
 * zero and −inf when L == 0).  So a row whose list holds at most `split` entries has the bits of the unsplit entry; a
 * row's bits depend on its item's operands, its list, pos and split, never on T, new_lens, the batch or the launch; paged
 * equals contiguous on the gathered cache, fp8 with NULL scales the 2-byte entry on the widened cache.  Rows with more
 * than one part agree with the unsplit entry to rounding.  Every row of out and lse is written exactly once, by the
 * second launch.
 * Validation before any HIP call: what the prefill entries refuse, split < 1, and (parts_max > 1) a NULL or misaligned
 * workspace → MI_EINVAL; a short workspace → MI_ENOMEM; items == 0 or T == 0 → MI_OK, nothing touched.
 * ------------------------------------------------------------------------ */
int64_t mi_block_attention_prefill_split_workspace_bytes(int32_t items, int32_t group, int32_t T, int32_t D, int32_t Smax,
                                                         int32_t split);
#define MI_BLOCK_ATTENTION_PREFILL_SPLIT_OUT                                                                                   \
  uint16_t *out, int64_t ldo, int64_t strideO, float *lse, int32_t split, void *workspace, size_t workspace_bytes,             \
      mi_stream_t stream
int mi_block_attention_prefill_split_bf16(MI_BLOCK_ATTENTION_PREFILL_LIST, int32_t D, MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint16_t),
                                          MI_BLOCK_ATTENTION_PREFILL_SPLIT_OUT);
int mi_block_attention_prefill_split_f16(MI_BLOCK_ATTENTION_PREFILL_LIST, int32_t D, MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint16_t),
                                         MI_BLOCK_ATTENTION_PREFILL_SPLIT_OUT);
int mi_block_attention_prefill_split_paged_bf16(MI_BLOCK_ATTENTION_PREFILL_LIST, MI_BLOCK_ATTENTION_PREFILL_TABLE, int32_t D,
                                                MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint16_t), MI_BLOCK_ATTENTION_PREFILL_SPLIT_OUT);
int mi_block_attention_prefill_split_paged_f16(MI_BLOCK_ATTENTION_PREFILL_LIST, MI_BLOCK_ATTENTION_PREFILL_TABLE, int32_t D,
                                               MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint16_t), MI_BLOCK_ATTENTION_PREFILL_SPLIT_OUT);
int mi_block_attention_prefill_split_fp8_bf16(MI_BLOCK_ATTENTION_PREFILL_LIST, int32_t D, MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint8_t),
                                              MI_BLOCK_ATTENTION_PREFILL_SCALES, MI_BLOCK_ATTENTION_PREFILL_SPLIT_OUT);
int mi_block_attention_prefill_split_fp8_f16(MI_BLOCK_ATTENTION_PREFILL_LIST, int32_t D, MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint8_t),
                                             MI_BLOCK_ATTENTION_PREFILL_SCALES, MI_BLOCK_ATTENTION_PREFILL_SPLIT_OUT);
int mi_block_attention_prefill_split_paged_fp8_bf16(MI_BLOCK_ATTENTION_PREFILL_LIST, MI_BLOCK_ATTENTION_PREFILL_TABLE, int32_t D,
                                                    MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint8_t), MI_BLOCK_ATTENTION_PREFILL_SCALES,
                                                    MI_BLOCK_ATTENTION_PREFILL_SPLIT_OUT);
int mi_block_attention_prefill_split_paged_fp8_f16(MI_BLOCK_ATTENTION_PREFILL_LIST, MI_BLOCK_ATTENTION_PREFILL_TABLE, int32_t D,
                                                   MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint8_t), MI_BLOCK_ATTENTION_PREFILL_SCALES,
                                                   MI_BLOCK_ATTENTION_PREFILL_SPLIT_OUT);

/* ------------------------------------------------------------------------ *
 * The fused KV-cache append: the write side of the decode entries above.  ONE launch writes the keys AND the
 * values of the T newest tokens of every k / v item into the cache of mi_block_attention_decode_* — contiguous or paged,
 * 2-byte or e4m3fn bytes — at the positions the lengths name.
 *   items, heads   as in the decode entries: items = B · heads, item c is head c % heads of batch item c / heads; items ≤ 65535;
 *   k_new, v_new   the source, 2-byte patterns (bfloat16 or float16), never copied: token t of item c at k_new + (c / heads) ·
 *              batchKn + (c % heads) · headKn + t · ldkn, D elements (v_new likewise); 16-byte aligned, every stride a
 *              non-negative multiple of 8 elements — two slices of one fused projection [B, T, Hq + 2·heads, D] fit;
 *   k, v       the destination with the strides of the decode entries: row j of item c at k + (c / heads) · batchK +
 *              (c % heads) · headK + j · ldk; 16-byte aligned, ldk ≥ D, every stride a multiple of 8 elements (16 e4m3fn bytes);
 *              paged (k_pages, pageK …): row r of head h of pool page e at k_pages + e · pageK + h · headK + r · ldk, with
 *              block_table, table_ld, pages, page as in mi_block_attention_decode_paged_*; Smax = the logical pages · page;
 *   k_lens     int32 [lens_count] on the device, the lengths AFTER the append — what the decode entry receives next; item c
 *              has entry c / (items / lens_count).  NOT clamped.
 * Token t of item c goes to pos = k_len − T + t.  It is written iff 0 ≤ pos < Smax and, paged, block_table[(c / heads) ·
 * table_ld + pos / page] lies in [0, pages); otherwise it is DROPPED — nothing is stored for it anywhere, nothing wraps or
 * moves.  Everything the rule does not write keeps its bytes (other rows, the gap between rows, unreferenced pages).  The
 * source must not overlap the destination; two (item, token) pairs mapped to one pool row stay inside the operands, but which
 * write lands is unspecified.
 *   _b16       a bit copy, the same for both 2-byte types (NaN payloads and −0 kept);
 *   _fp8_T     the stored byte is that of torch's CPU expression (float32(x) / scale[h]).clamp(−448, 448).to(float8_e4m3fn):
 *              an IEEE float32 division, the clamp, one round-to-nearest-even into OCP e4m3fn; a NaN quotient becomes a NaN
 *              code (byte & 0x7F == 0x7F).  k_scale, k_scale_count, v_scale, v_scale_count as in the fp8 decode entries: read
 *              on the device, never read back; NULL is 1.
 * No atomics, no workspace, no read-back: graph-capturable while k_lens, the table and the scales are updated in place.
 * Validation before any HIP call: D ∉ {32, 64, 96, 128}, a negative size, items > 65535, items % heads != 0, lens_count < 1 or
 * items % lens_count != 0, a NULL / misaligned pointer, a stride that is negative or no multiple of 8 (cache of bytes: 16), ldk
 * < D, page < 16 or no power of two, Smax % page != 0, pages < 0, table_ld < Smax / page, a scale count other than 1 or heads
 * → MI_EINVAL; items · T · D/8 ≥ 2³¹ → MI_ERANGE; items == 0 or T == 0 → MI_OK, nothing touched; Smax == 0 or pages == 0 →
 * MI_OK, every token dropped (the destination may be NULL).
 * ------------------------------------------------------------------------ */
int mi_kv_append_b16(int32_t items, int32_t heads, int32_t T, int32_t Smax, int32_t D, const uint16_t* k_new, int64_t ldkn,
                     int64_t headKn, int64_t batchKn, const uint16_t* v_new, int64_t ldvn, int64_t headVn, int64_t batchVn,
                     uint16_t* k, int64_t ldk, int64_t headK, int64_t batchK, uint16_t* v, int64_t ldv, int64_t headV,
                     int64_t batchV, const int32_t* k_lens, int32_t lens_count, mi_stream_t stream);
int mi_kv_append_paged_b16(int32_t items, int32_t heads, int32_t T, int32_t Smax, const int32_t* block_table, int64_t table_ld,
                           int32_t pages, int32_t page, int32_t D, const uint16_t* k_new, int64_t ldkn, int64_t headKn,
                           int64_t batchKn, const uint16_t* v_new, int64_t ldvn, int64_t headVn, int64_t batchVn,
                           uint16_t* k_pages, int64_t ldk, int64_t headK, int64_t pageK, uint16_t* v_pages, int64_t ldv,
                           int64_t headV, int64_t pageV, const int32_t* k_lens, int32_t lens_count, mi_stream_t stream);
int mi_kv_append_fp8_bf16(int32_t items, int32_t heads, int32_t T, int32_t Smax, int32_t D, const uint16_t* k_new, int64_t ldkn,
                          int64_t headKn, int64_t batchKn, const uint16_t* v_new, int64_t ldvn, int64_t headVn, int64_t batchVn,
                          uint8_t* k, int64_t ldk, int64_t headK, int64_t batchK, uint8_t* v, int64_t ldv, int64_t headV,
                          int64_t batchV, const int32_t* k_lens, int32_t lens_count, const float* k_scale, int32_t k_scale_count,
                          const float* v_scale, int32_t v_scale_count, mi_stream_t stream);
int mi_kv_append_fp8_f16(int32_t items, int32_t heads, int32_t T, int32_t Smax, int32_t D, const uint16_t* k_new, int64_t ldkn,
                         int64_t headKn, int64_t batchKn, const uint16_t* v_new, int64_t ldvn, int64_t headVn, int64_t batchVn,
                         uint8_t* k, int64_t ldk, int64_t headK, int64_t batchK, uint8_t* v, int64_t ldv, int64_t headV,
                         int64_t batchV, const int32_t* k_lens, int32_t lens_count, const float* k_scale, int32_t k_scale_count,
                         const float* v_scale, int32_t v_scale_count, mi_stream_t stream);
int mi_kv_append_paged_fp8_bf16(int32_t items, int32_t heads, int32_t T, int32_t Smax, const int32_t* block_table,
                                int64_t table_ld, int32_t pages, int32_t page, int32_t D, const uint16_t* k_new, int64_t ldkn,
                                int64_t headKn, int64_t batchKn, const uint16_t* v_new, int64_t ldvn, int64_t headVn,
                                int64_t batchVn, uint8_t* k_pages, int64_t ldk, int64_t headK, int64_t pageK, uint8_t* v_pages,
                                int64_t ldv, int64_t headV, int64_t pageV, const int32_t* k_lens, int32_t lens_count,
                                const float* k_scale, int32_t k_scale_count, const float* v_scale, int32_t v_scale_count,
                                mi_stream_t stream);
int mi_kv_append_paged_fp8_f16(int32_t items, int32_t heads, int32_t T, int32_t Smax, const int32_t* block_table,
                               int64_t table_ld, int32_t pages, int32_t page, int32_t D, const uint16_t* k_new, int64_t ldkn,
                               int64_t headKn, int64_t batchKn, const uint16_t* v_new, int64_t ldvn, int64_t headVn,
                               int64_t batchVn, uint8_t* k_pages, int64_t ldk, int64_t headK, int64_t pageK, uint8_t* v_pages,
                               int64_t ldv, int64_t headV, int64_t pageV, const int32_t* k_lens, int32_t lens_count,
                               const float* k_scale, int32_t k_scale_count, const float* v_scale, int32_t v_scale_count,
                               mi_stream_t stream);

/* ------------------------------------------------------------------------ *
 * The fused rotary embedding + KV-cache append: the step in front of mi_kv_append_*, fused into it.  ONE
 * launch rotates q and the new keys by position with the caller's cos / sin tables, writes the rotated keys and the values
 * into the cache of mi_block_attention_decode_* — contiguous or paged, 2-byte or e4m3fn bytes — and the rotated q into q_out.
 * items, heads, T, Smax, D, k_new, v_new, k, v (k_pages, v_pages), block_table, table_ld, pages, page, k_lens, the scales and
 * their strides and alignments are those of mi_kv_append_*, with one difference: lens_count is 1 or B = items / heads (q has
 * no k / v head, so a length per k / v item has no meaning here).  Added to them:
 *   q_heads    Hq ≥ 1 query heads per batch item; no relation to `heads` is required;
 *   q          the queries, 2-byte patterns read through their own strides like k_new: token t of head h of batch item b at
 *              q + b · batchQ + h · headQ + t · ldq, D elements; 16-byte aligned, every stride a non-negative multiple of 8;
 *   q_out      receives the rotated q, with strides of its own under the same rules; q_out == q (same strides) rotates in place;
 *   k_out      NULL — the rotated k goes to the cache only — or, under the same rules, an operand [B, heads, T, D] that ALSO
 *              receives the rotated k in the source type; k_out == k_new (same strides) rotates in place;
 *   cos, sin   float32 [table_rows][ld] on the device, 16-byte aligned, ld ≥ rotary_dim / 2 and a multiple of 4: row p holds
 *              the rotary_dim / 2 cosines / sines of position p.  No trigonometry is computed: the tables define the angles;
 *   rotary_dim R, a multiple of 16 with 16 ≤ R ≤ D: elements d ≥ R of q and k are bit copies;
 *   interleaved  0: pair i is (x[i], x[i + R/2]) — the NeoX halves; non-zero: (x[2i], x[2i + 1]) — GPT-J;
 *   new_lens   NULL, or int32 [B] on the device: batch item b has n = clamp(new_lens[b], 0, T) new tokens, standing in the LAST
 *              n of the T slots.  NULL: n = T.
 * The rule.  pos = k_len − T + t in 64 bits, k_len not clamped.  Slot t of batch item b HOLDS A TOKEN iff t ≥ T − n and
 * 0 ≤ pos < table_rows.  No token: the slot's rows of q_out, and of k_out if given, are written as zeros and nothing is stored
 * into the cache.  A token: its q rows and its k row are rotated by table row pos; q goes to q_out, k to k_out if given; k and
 * v are written into the cache iff mi_kv_append_*'s condition holds (0 ≤ pos < Smax and, paged, the table entry in [0, pages)),
 * and dropped otherwise — q is still rotated.  Everything the rule does not write keeps its bytes.
 * Bits.  With c = cos[pos · ld + i], s = sin[pos · ld + i] and the pair (a, b) widened exactly to float32:
 *     a' = fl32(fl32(a·c) − fl32(b·s))        b' = fl32(fl32(b·c) + fl32(a·s))
 * two products and one sum, each rounded to float32, never contracted into an fma, float32 subnormals kept; then ONE
 * round-to-nearest-even to the source type — torch's CPU result of (a.float() * c − b.float() * s).to(T).  A NaN result is a
 * NaN of unspecified payload.  Elements d ≥ R of q and k, and all of v, are bit copies.  An fp8 cache receives the bytes of
 * mi_kv_append_fp8_T applied to the rotated k AFTER its rounding to the source type, and to v: all four forms leave the cache
 * that mi_kv_append_* leaves for the rounded rotated k.
 * No atomics, no workspace, no read-back: graph-capturable while k_lens, new_lens, the tables and the scales are updated in
 * place.  Operands other than q_out == q and k_out == k_new must not overlap what is written.
 * Validation before any HIP call: what mi_kv_append_* refuses, lens_count other than 1 or items / heads, q_heads < 0 (or 0 with
 * work to do), table_rows < 0, rotary_dim < 16, > D or no multiple of 16, a NULL / misaligned q or q_out or a stride of theirs
 * (or of a non-NULL k_out) that is negative or no multiple of 8, ld < rotary_dim / 2 or no multiple of 4, NULL / misaligned cos
 * or sin with table_rows > 0, a new_lens that is not 4-byte aligned → MI_EINVAL; B · (q_heads + 2 · heads) · T · D/8 ≥ 2³¹ →
 * MI_ERANGE; items == 0 or T == 0 → MI_OK, nothing touched.  Smax == 0 or pages == 0: every k / v row is dropped (the
 * destination may be NULL), q is still rotated.
 * ------------------------------------------------------------------------ */
#define MI_ROPE_KV_APPEND_OPERANDS(CT)                                                                                           \
  int32_t q_heads, const uint16_t *q, int64_t ldq, int64_t headQ, int64_t batchQ, uint16_t *q_out, int64_t ldqo, int64_t headQo, \
      int64_t batchQo, const uint16_t *k_new, int64_t ldkn, int64_t headKn, int64_t batchKn, const uint16_t *v_new,              \
      int64_t ldvn, int64_t headVn, int64_t batchVn, uint16_t *k_out, int64_t ldko, int64_t headKo, int64_t batchKo,             \
      const float *cos, const float *sin, int32_t table_rows, int64_t ld, int32_t rotary_dim, int32_t interleaved, CT *k,        \
      int64_t ldk, int64_t headK, int64_t batchK, CT *v, int64_t ldv, int64_t headV, int64_t batchV, const int32_t *k_lens,      \
      int32_t lens_count, const int32_t *new_lens
int mi_rope_kv_append_bf16(int32_t items, int32_t heads, int32_t T, int32_t Smax, int32_t D, MI_ROPE_KV_APPEND_OPERANDS(uint16_t),
                           mi_stream_t stream);
int mi_rope_kv_append_f16(int32_t items, int32_t heads, int32_t T, int32_t Smax, int32_t D, MI_ROPE_KV_APPEND_OPERANDS(uint16_t),
                          mi_stream_t stream);
/* (paged: k, batchK, v, batchV of the operand list are k_pages, pageK, v_pages, pageV) */
int mi_rope_kv_append_paged_bf16(int32_t items, int32_t heads, int32_t T, int32_t Smax, const int32_t* block_table,
                                 int64_t table_ld, int32_t pages, int32_t page, int32_t D, MI_ROPE_KV_APPEND_OPERANDS(uint16_t),
                                 mi_stream_t stream);
int mi_rope_kv_append_paged_f16(int32_t items, int32_t heads, int32_t T, int32_t Smax, const int32_t* block_table,
                                int64_t table_ld, int32_t pages, int32_t page, int32_t D, MI_ROPE_KV_APPEND_OPERANDS(uint16_t),
                                mi_stream_t stream);
int mi_rope_kv_append_fp8_bf16(int32_t items, int32_t heads, int32_t T, int32_t Smax, int32_t D, MI_ROPE_KV_APPEND_OPERANDS(uint8_t),
                               const float* k_scale, int32_t k_scale_count, const float* v_scale, int32_t v_scale_count,
                               mi_stream_t stream);
int mi_rope_kv_append_fp8_f16(int32_t items, int32_t heads, int32_t T, int32_t Smax, int32_t D, MI_ROPE_KV_APPEND_OPERANDS(uint8_t),
                              const float* k_scale, int32_t k_scale_count, const float* v_scale, int32_t v_scale_count,
                              mi_stream_t stream);
int mi_rope_kv_append_paged_fp8_bf16(int32_t items, int32_t heads, int32_t T, int32_t Smax, const int32_t* block_table,
                                     int64_t table_ld, int32_t pages, int32_t page, int32_t D, MI_ROPE_KV_APPEND_OPERANDS(uint8_t),
                                     const float* k_scale, int32_t k_scale_count, const float* v_scale, int32_t v_scale_count,
                                     mi_stream_t stream);
int mi_rope_kv_append_paged_fp8_f16(int32_t items, int32_t heads, int32_t T, int32_t Smax, const int32_t* block_table,
                                    int64_t table_ld, int32_t pages, int32_t page, int32_t D, MI_ROPE_KV_APPEND_OPERANDS(uint8_t),
                                    const float* k_scale, int32_t k_scale_count, const float* v_scale, int32_t v_scale_count,
                                    mi_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Query-aware key-block selection for decoding: per-block key bounds kept next to the cache, a selection
 * kernel that scores every 64-key block against the newest tokens' queries and lists the K best per token, and a decode
 * entry that walks those lists in the place of a CSR layout.  bfloat16 / float16 (2-byte bit patterns), D ∈ {32, 64, 96,
 * 128}; items, heads, Smax, k_lens, lens_count, the cache operands and the paged arguments as in
 * mi_block_attention_decode{,_paged}_*.  Nothing is read back, there are no atomics: every entry is graph-capturable.
 *
 * mi_kv_block_bounds{,_paged}_T: bounds [items][Smax/64][2][D] of T, 16-byte aligned: bounds[c][J][0][d] = min and
 *   bounds[c][J][1][d] = max of k[c][j][d] over the SEEN keys j of block J — 64J ≤ j < min(64J + 64, clamp(k_len, 0, Smax))
 *   and, paged, the table entry of j's logical page in [0, pages).  A block without a seen key is not written.  last == 0
 *   refreshes every block with a seen key, last = n ≥ 1 only those holding a position of [k_len − n, k_len).  Exact, and a
 *   function of the seen keys alone (the 16-bit patterns are compared in one total order in which −0 < +0; with NaN keys
 *   the result is unspecified).  Rows at or beyond k_len, between the rows and behind invalid table entries are never read.
 *   MI_EINVAL: D, Smax % 64, last < 0, items > 65535, heads / lens_count that do not divide items, null or misaligned
 *   pointers, strides that are no multiples of 8 elements or ldk < D, the page rules.  Smax == 0 or items == 0: MI_OK.
 *
 * mi_block_select_T: q — head g of item c, token t at q + (c / heads)·batchQ + ((c % heads)·group + g)·headQ + t·ldq, 16-byte
 *   aligned, strides multiples of 8 elements —, bounds as above.  Token t stands at pos = clamp(k_len, 0, Smax) − T + t; its
 *   candidates are the blocks J ≤ pos / 64; s_g(J) = Σ_d max(q[g,d]·lo[J,d], q[g,d]·hi[J,d]) in fp32 (every product exact; the
 *   order of the sum is fixed: block_select.hip's header), score(J) = max_g s_g(J); a NaN score ranks below every number.
 *   The candidates among the first `sink` blocks and the `local` blocks ending at pos / 64 are always listed and count toward
 *   K; the other slots go to the rest in (score descending, index ascending).  block_ids int32 [items][T][K] receives the list
 *   in ASCENDING block index and −1 from block_counts[c][t] = min(K, candidates) on (0 for pos < 0); scores, if not null,
 *   float32 [items][T][Smax/64]: the candidates' scores, −inf elsewhere.  Bounds of non-candidates are never read.
 *   MI_EINVAL: K < 1, sink < 0, local < 1, sink + local > K, group outside 1 … 16, Smax/64 > mi_block_select_max_blocks()
 *   (16 384: the scores of one token live in the LDS of one workgroup), D, Smax % 64, items > 65535, pointers, strides.
 *
 * mi_block_attention_decode_lists{,_paged}_T: mi_block_attention_decode{,_paged}_T with the list of token t of item c given
 *   as the first clamp(block_counts[c·T + t], 0, K) entries of row c·T + t of block_ids [items][T][K] (int32, 4-byte aligned)
 *   — in the place of row pos / 64 of a layout.  An entry outside [0, Smax/64) or wholly beyond pos is skipped inside its
 *   chunk; a block listed twice counts twice.  The chunks — and the workspace:
 *   mi_block_attention_decode_workspace_bytes(items, T, group, D, 64·K, chunk) — are those of K list positions.  For token t,
 *   out and lse have the bits of mi_block_attention_decode{,_paged}_T with T = 1, k_len = pos + 1, the same chunk and a layout
 *   whose row pos / 64 lists the same blocks in the same order.  MI_EINVAL: what that entry refuses but for the layout, K < 1
 *   or 64·K beyond int32, null or misaligned block_ids / block_counts; MI_ERANGE: items·T·K beyond int32.
 * ------------------------------------------------------------------------ */
#define MI_KV_BLOCK_BOUNDS_OPERANDS                                                                                      \
  int32_t D, const uint16_t *k, int64_t ldk, int64_t headK, int64_t batchK, const int32_t *k_lens, int32_t lens_count, \
      int32_t last, uint16_t *bounds, mi_stream_t stream
int mi_kv_block_bounds_bf16(int32_t items, int32_t heads, int32_t Smax, MI_KV_BLOCK_BOUNDS_OPERANDS);
int mi_kv_block_bounds_f16(int32_t items, int32_t heads, int32_t Smax, MI_KV_BLOCK_BOUNDS_OPERANDS);
/* (k and batchK: k_pages and its page stride) */
int mi_kv_block_bounds_paged_bf16(int32_t items, int32_t heads, int32_t Smax, const int32_t* block_table, int64_t table_ld,
                                  int32_t pages, int32_t page, MI_KV_BLOCK_BOUNDS_OPERANDS);
int mi_kv_block_bounds_paged_f16(int32_t items, int32_t heads, int32_t Smax, const int32_t* block_table, int64_t table_ld,
                                 int32_t pages, int32_t page, MI_KV_BLOCK_BOUNDS_OPERANDS);

int32_t mi_block_select_max_blocks(void);
#define MI_BLOCK_SELECT_OPERANDS                                                                                                \
  int32_t items, int32_t heads, int32_t T, int32_t Smax, int32_t D, int32_t group, const uint16_t *q, int64_t ldq, int64_t headQ, \
      int64_t batchQ, const uint16_t *bounds, const int32_t *k_lens, int32_t lens_count, int32_t K, int32_t sink, int32_t local,  \
      int32_t *block_ids, int32_t *block_counts, float *scores, mi_stream_t stream
int mi_block_select_bf16(MI_BLOCK_SELECT_OPERANDS);
int mi_block_select_f16(MI_BLOCK_SELECT_OPERANDS);

/* (the return type stands on a line of its own: these four take lists, not the rowptr / col / nnz / layouts head that the
 * one-line declarations `int mi_block_attention_decode…(` of the eight layout entries share) */
#define MI_DECODE_LISTS_OPERANDS                                                                                                \
  int32_t D, const uint16_t *q, int64_t ldq, int64_t strideQ, const uint16_t *k, int64_t ldk, int64_t headK, int64_t batchK,     \
      const uint16_t *v, int64_t ldv, int64_t headV, int64_t batchV, const int32_t *k_lens, int32_t lens_count, int32_t group,  \
      int32_t chunk, float scale, uint16_t *out, int64_t ldo, int64_t strideO, float *lse, void *workspace,                     \
      size_t workspace_bytes, mi_stream_t stream
int
mi_block_attention_decode_lists_bf16(const int32_t* block_ids, const int32_t* block_counts, int32_t K, int32_t items,
                                         int32_t heads, int32_t T, int32_t Smax, MI_DECODE_LISTS_OPERANDS);
int
mi_block_attention_decode_lists_f16(const int32_t* block_ids, const int32_t* block_counts, int32_t K, int32_t items,
                                        int32_t heads, int32_t T, int32_t Smax, MI_DECODE_LISTS_OPERANDS);
int
mi_block_attention_decode_lists_paged_bf16(const int32_t* block_ids, const int32_t* block_counts, int32_t K, int32_t items,
                                               int32_t heads, int32_t T, int32_t Smax, const int32_t* block_table,
                                               int64_t table_ld, int32_t pages, int32_t page, MI_DECODE_LISTS_OPERANDS);
int
mi_block_attention_decode_lists_paged_f16(const int32_t* block_ids, const int32_t* block_counts, int32_t K, int32_t items,
                                              int32_t heads, int32_t T, int32_t Smax, const int32_t* block_table,
                                              int64_t table_ld, int32_t pages, int32_t page, MI_DECODE_LISTS_OPERANDS);

/* ------------------------------------------------------------------------ *
 * … over an FP8 (OCP e4m3fn) cache: the bounds of a cache of e4m3fn bytes and the decode entry that walks the
 * caller's lists over one.  k (and v) are bytes, their strides count bytes and are multiples of 16; everything not said here is
 * the entry above of the same name.
 *
 * mi_kv_block_bounds{,_paged}_fp8_T: mi_kv_block_bounds{,_paged}_T over a cache of e4m3fn bytes, with bounds of T — THE SUFFIX
 *   IS THE BOUNDS' TYPE.  Every finite e4m3fn code is a T, and the widening is strictly monotone in the total order the bounds
 *   are taken in (−0 < +0 included), so the result is, bit for bit, that of mi_kv_block_bounds{,_paged}_T on the cache widened to
 *   T; −0 is stored as 0x8000.  The bytes are compared as they are and only the 2·D results of a block are widened.  The scales
 *   of the cache are no operand: positive per-head scales change neither a minimum nor the ranking of the blocks of a head, and
 *   mi_block_select_T's scores of these bounds are those of the UNSCALED widened keys (the bound of the real q·k is
 *   score · k_scale[h]).  NaN codes (0x7f, 0xff) among the seen keys: unspecified, nothing faults.  MI_EINVAL as above, with
 *   strides that are no multiples of 16 bytes.
 *
 * mi_block_attention_lists_decode{,_paged}_fp8_T: mi_block_attention_decode_lists{,_paged}_T over an fp8 cache, with the four
 *   scale parameters of mi_block_attention_decode{,_paged}_fp8_T after `scale`.  For token t, out and lse have the bits of
 *   mi_block_attention_decode{,_paged}_fp8_T with T = 1, k_len = pos + 1, the same chunk and scales and a layout whose row
 *   pos / 64 lists the same blocks in the same order; without scales, those of mi_block_attention_decode_lists{,_paged}_T on the
 *   widened cache.  MI_EINVAL: what the lists entries and the fp8 entries refuse.  (`lists` stands before `decode` in the name:
 *   the entries `mi_block_attention_decode…` are a closed family.)
 * ------------------------------------------------------------------------ */
#define MI_KV_BLOCK_BOUNDS_FP8_OPERANDS                                                                                 \
  int32_t D, const uint8_t *k, int64_t ldk, int64_t headK, int64_t batchK, const int32_t *k_lens, int32_t lens_count, \
      int32_t last, uint16_t *bounds, mi_stream_t stream
int mi_kv_block_bounds_fp8_bf16(int32_t items, int32_t heads, int32_t Smax, MI_KV_BLOCK_BOUNDS_FP8_OPERANDS);
int mi_kv_block_bounds_fp8_f16(int32_t items, int32_t heads, int32_t Smax, MI_KV_BLOCK_BOUNDS_FP8_OPERANDS);
int mi_kv_block_bounds_paged_fp8_bf16(int32_t items, int32_t heads, int32_t Smax, const int32_t* block_table, int64_t table_ld,
                                      int32_t pages, int32_t page, MI_KV_BLOCK_BOUNDS_FP8_OPERANDS);
int mi_kv_block_bounds_paged_fp8_f16(int32_t items, int32_t heads, int32_t Smax, const int32_t* block_table, int64_t table_ld,
                                     int32_t pages, int32_t page, MI_KV_BLOCK_BOUNDS_FP8_OPERANDS);

#define MI_LISTS_DECODE_FP8_OPERANDS                                                                                            \
  int32_t D, const uint16_t *q, int64_t ldq, int64_t strideQ, const uint8_t *k, int64_t ldk, int64_t headK, int64_t batchK,      \
      const uint8_t *v, int64_t ldv, int64_t headV, int64_t batchV, const int32_t *k_lens, int32_t lens_count, int32_t group,   \
      int32_t chunk, float scale, const float *k_scale, int32_t k_scale_count, const float *v_scale, int32_t v_scale_count,     \
      uint16_t *out, int64_t ldo, int64_t strideO, float *lse, void *workspace, size_t workspace_bytes, mi_stream_t stream
int mi_block_attention_lists_decode_fp8_bf16(const int32_t* block_ids, const int32_t* block_counts, int32_t K, int32_t items,
                                             int32_t heads, int32_t T, int32_t Smax, MI_LISTS_DECODE_FP8_OPERANDS);
int mi_block_attention_lists_decode_fp8_f16(const int32_t* block_ids, const int32_t* block_counts, int32_t K, int32_t items,
                                            int32_t heads, int32_t T, int32_t Smax, MI_LISTS_DECODE_FP8_OPERANDS);
int mi_block_attention_lists_decode_paged_fp8_bf16(const int32_t* block_ids, const int32_t* block_counts, int32_t K, int32_t items,
                                                   int32_t heads, int32_t T, int32_t Smax, const int32_t* block_table,
                                                   int64_t table_ld, int32_t pages, int32_t page, MI_LISTS_DECODE_FP8_OPERANDS);
int mi_block_attention_lists_decode_paged_fp8_f16(const int32_t* block_ids, const int32_t* block_counts, int32_t K, int32_t items,
                                                  int32_t heads, int32_t T, int32_t Smax, const int32_t* block_table,
                                                  int64_t table_ld, int32_t pages, int32_t page, MI_LISTS_DECODE_FP8_OPERANDS);

/* ------------------------------------------------------------------------ *
 * Tree-masked decode for speculative decoding: the sixteen decode entries above — the layout entries
 * mi_block_attention_decode{,_paged}{,_fp8}_T and the list entries mi_block_attention_decode_lists{,_paged}_T,
 * mi_block_attention_lists_decode{,_paged}_fp8_T — as mi_block_attention_tree_decode{,_lists}{,_paged}{,_fp8}_T, with two
 * parameters between `scale` (or the four scale parameters) and `out`:
 *   tree_mask  int64 words [mask_rows][T] on the device, 8-byte aligned, read by the kernel and never read back
 *   mask_rows  1 — one row of words for the whole batch — or the batch size items / heads
 * The T newest tokens of an item are the nodes of a drafted tree, stored in the window [base, base + T) of the cache with
 * base = clamp(k_len, 0, Smax) − T.  Token t stands at pos = base + t, as in the parents, and sees key j iff the parent's rule
 * holds (j ≤ pos and its list names block j / 64) AND (j < base, or j == pos, or bit j − base of tree_mask[b][t] is set).  Bits at
 * or above t are never looked at, a token always sees itself; the word (2 << t) − 1, or all ones, gives the parent entry's bits.
 * A hidden key is treated like a key beyond pos: never loaded, staged as zeros, its score −inf — a NaN in a hidden slot reaches
 * no output.  Chunks, the deal to the waves, the order of the merges, the workspace, out and lse are the parent's.
 * Validation before any HIP call: what the parent refuses; T > 64 (before the empty call is answered with MI_OK); then, for a
 * call that is not empty, a null or misaligned tree_mask and a mask_rows that is neither 1 nor items / heads — MI_EINVAL.
 * (`tree` stands before `decode` in the name: the entries `mi_block_attention_decode…` are a closed family.)
 * ------------------------------------------------------------------------ */
#define MI_TREE_DECODE_OPERANDS(CT)                                                                                             \
  int32_t D, const uint16_t *q, int64_t ldq, int64_t strideQ, const CT *k, int64_t ldk, int64_t headK, int64_t batchK,           \
      const CT *v, int64_t ldv, int64_t headV, int64_t batchV, const int32_t *k_lens, int32_t lens_count, int32_t group,        \
      int32_t chunk, float scale
#define MI_TREE_DECODE_SCALES const float *k_scale, int32_t k_scale_count, const float *v_scale, int32_t v_scale_count
#define MI_TREE_DECODE_OUT                                                                                                      \
  const int64_t *tree_mask, int32_t mask_rows, uint16_t *out, int64_t ldo, int64_t strideO, float *lse, void *workspace,        \
      size_t workspace_bytes, mi_stream_t stream
#define MI_TREE_DECODE_LAYOUT \
  const int32_t *rowptr, const int32_t *col, int64_t nnz, int32_t layouts, int32_t items, int32_t heads, int32_t T, int32_t Smax
#define MI_TREE_DECODE_LISTS \
  const int32_t *block_ids, const int32_t *block_counts, int32_t K, int32_t items, int32_t heads, int32_t T, int32_t Smax
#define MI_TREE_DECODE_TABLE const int32_t *block_table, int64_t table_ld, int32_t pages, int32_t page
int mi_block_attention_tree_decode_bf16(MI_TREE_DECODE_LAYOUT, MI_TREE_DECODE_OPERANDS(uint16_t), MI_TREE_DECODE_OUT);
int mi_block_attention_tree_decode_f16(MI_TREE_DECODE_LAYOUT, MI_TREE_DECODE_OPERANDS(uint16_t), MI_TREE_DECODE_OUT);
int mi_block_attention_tree_decode_paged_bf16(MI_TREE_DECODE_LAYOUT, MI_TREE_DECODE_TABLE, MI_TREE_DECODE_OPERANDS(uint16_t),
                                              MI_TREE_DECODE_OUT);
int mi_block_attention_tree_decode_paged_f16(MI_TREE_DECODE_LAYOUT, MI_TREE_DECODE_TABLE, MI_TREE_DECODE_OPERANDS(uint16_t),
                                             MI_TREE_DECODE_OUT);
int mi_block_attention_tree_decode_fp8_bf16(MI_TREE_DECODE_LAYOUT, MI_TREE_DECODE_OPERANDS(uint8_t), MI_TREE_DECODE_SCALES,
                                            MI_TREE_DECODE_OUT);
int mi_block_attention_tree_decode_fp8_f16(MI_TREE_DECODE_LAYOUT, MI_TREE_DECODE_OPERANDS(uint8_t), MI_TREE_DECODE_SCALES,
                                           MI_TREE_DECODE_OUT);
int mi_block_attention_tree_decode_paged_fp8_bf16(MI_TREE_DECODE_LAYOUT, MI_TREE_DECODE_TABLE, MI_TREE_DECODE_OPERANDS(uint8_t),
                                                  MI_TREE_DECODE_SCALES, MI_TREE_DECODE_OUT);
int mi_block_attention_tree_decode_paged_fp8_f16(MI_TREE_DECODE_LAYOUT, MI_TREE_DECODE_TABLE, MI_TREE_DECODE_OPERANDS(uint8_t),
                                                 MI_TREE_DECODE_SCALES, MI_TREE_DECODE_OUT);
int mi_block_attention_tree_decode_lists_bf16(MI_TREE_DECODE_LISTS, MI_TREE_DECODE_OPERANDS(uint16_t), MI_TREE_DECODE_OUT);
int mi_block_attention_tree_decode_lists_f16(MI_TREE_DECODE_LISTS, MI_TREE_DECODE_OPERANDS(uint16_t), MI_TREE_DECODE_OUT);
int mi_block_attention_tree_decode_lists_paged_bf16(MI_TREE_DECODE_LISTS, MI_TREE_DECODE_TABLE, MI_TREE_DECODE_OPERANDS(uint16_t),
                                                    MI_TREE_DECODE_OUT);
int mi_block_attention_tree_decode_lists_paged_f16(MI_TREE_DECODE_LISTS, MI_TREE_DECODE_TABLE, MI_TREE_DECODE_OPERANDS(uint16_t),
                                                   MI_TREE_DECODE_OUT);
int mi_block_attention_tree_decode_lists_fp8_bf16(MI_TREE_DECODE_LISTS, MI_TREE_DECODE_OPERANDS(uint8_t), MI_TREE_DECODE_SCALES,
                                                  MI_TREE_DECODE_OUT);
int mi_block_attention_tree_decode_lists_fp8_f16(MI_TREE_DECODE_LISTS, MI_TREE_DECODE_OPERANDS(uint8_t), MI_TREE_DECODE_SCALES,
                                                 MI_TREE_DECODE_OUT);
int mi_block_attention_tree_decode_lists_paged_fp8_bf16(MI_TREE_DECODE_LISTS, MI_TREE_DECODE_TABLE, MI_TREE_DECODE_OPERANDS(uint8_t),
                                                        MI_TREE_DECODE_SCALES, MI_TREE_DECODE_OUT);
int mi_block_attention_tree_decode_lists_paged_fp8_f16(MI_TREE_DECODE_LISTS, MI_TREE_DECODE_TABLE, MI_TREE_DECODE_OPERANDS(uint8_t),
                                                       MI_TREE_DECODE_SCALES, MI_TREE_DECODE_OUT);

/* ------------------------------------------------------------------------ *
 * Sliding windows and sink keys for decode: the sixteen plain decode entries — the layout entries
 * mi_block_attention_decode{,_paged}{,_fp8}_T and the list entries mi_block_attention_decode_lists{,_paged}_T,
 * mi_block_attention_lists_decode{,_paged}_fp8_T — as mi_block_attention_window_decode{,_lists}{,_paged}{,_fp8}_T, with two
 * parameters between `scale` (or the four scale parameters) and `out`:
 *   window  W ≥ 1: the token sees its last W keys, ITSELF INCLUDED (HF's sliding_window, FlashAttention's window_size = (W − 1, 0))
 *   sink    S ≥ 0: … and the first S keys of the cache (StreamingLLM's sink tokens)
 * Token t stands at pos = clamp(k_len, 0, Smax) − T + t, as in the parents, and sees key j iff the parent's rule holds (j ≤ pos,
 * its list names block j / 64, its page is valid) AND (j > pos − W or j < S).  A hidden key is treated like a key beyond pos:
 * never loaded, staged as zeros, its score −inf — a NaN in a hidden slot reaches no output.  A listed block J with 64 J ≥ S and
 * 64 J + 63 ≤ pos − W is wholly hidden and is skipped like a block beyond pos: it keeps its list position, so chunks, the deal to
 * the waves, the order of the merges, the workspace, out and lse are the parent's.  W = 2³¹ − 1, or S ≥ Smax, gives the parent
 * entry's bits.  A token that sees nothing has a zero row and lse −inf.
 * Validation before any HIP call: window < 1 or sink < 0 — MI_EINVAL, before anything else; then what the parent refuses.
 * (`window` stands before `decode` in the name: the entries `mi_block_attention_decode…` are a closed family.)
 * ------------------------------------------------------------------------ */
#define MI_WINDOW_DECODE_OUT                                                                                                    \
  int32_t window, int32_t sink, uint16_t *out, int64_t ldo, int64_t strideO, float *lse, void *workspace, size_t workspace_bytes, \
      mi_stream_t stream
int mi_block_attention_window_decode_bf16(MI_TREE_DECODE_LAYOUT, MI_TREE_DECODE_OPERANDS(uint16_t), MI_WINDOW_DECODE_OUT);
int mi_block_attention_window_decode_f16(MI_TREE_DECODE_LAYOUT, MI_TREE_DECODE_OPERANDS(uint16_t), MI_WINDOW_DECODE_OUT);
int mi_block_attention_window_decode_paged_bf16(MI_TREE_DECODE_LAYOUT, MI_TREE_DECODE_TABLE, MI_TREE_DECODE_OPERANDS(uint16_t),
                                                MI_WINDOW_DECODE_OUT);
int mi_block_attention_window_decode_paged_f16(MI_TREE_DECODE_LAYOUT, MI_TREE_DECODE_TABLE, MI_TREE_DECODE_OPERANDS(uint16_t),
                                               MI_WINDOW_DECODE_OUT);
int mi_block_attention_window_decode_fp8_bf16(MI_TREE_DECODE_LAYOUT, MI_TREE_DECODE_OPERANDS(uint8_t), MI_TREE_DECODE_SCALES,
                                              MI_WINDOW_DECODE_OUT);
int mi_block_attention_window_decode_fp8_f16(MI_TREE_DECODE_LAYOUT, MI_TREE_DECODE_OPERANDS(uint8_t), MI_TREE_DECODE_SCALES,
                                             MI_WINDOW_DECODE_OUT);
int mi_block_attention_window_decode_paged_fp8_bf16(MI_TREE_DECODE_LAYOUT, MI_TREE_DECODE_TABLE, MI_TREE_DECODE_OPERANDS(uint8_t),
                                                    MI_TREE_DECODE_SCALES, MI_WINDOW_DECODE_OUT);
int mi_block_attention_window_decode_paged_fp8_f16(MI_TREE_DECODE_LAYOUT, MI_TREE_DECODE_TABLE, MI_TREE_DECODE_OPERANDS(uint8_t),
                                                   MI_TREE_DECODE_SCALES, MI_WINDOW_DECODE_OUT);
int mi_block_attention_window_decode_lists_bf16(MI_TREE_DECODE_LISTS, MI_TREE_DECODE_OPERANDS(uint16_t), MI_WINDOW_DECODE_OUT);
int mi_block_attention_window_decode_lists_f16(MI_TREE_DECODE_LISTS, MI_TREE_DECODE_OPERANDS(uint16_t), MI_WINDOW_DECODE_OUT);
int mi_block_attention_window_decode_lists_paged_bf16(MI_TREE_DECODE_LISTS, MI_TREE_DECODE_TABLE, MI_TREE_DECODE_OPERANDS(uint16_t),
                                                      MI_WINDOW_DECODE_OUT);
int mi_block_attention_window_decode_lists_paged_f16(MI_TREE_DECODE_LISTS, MI_TREE_DECODE_TABLE, MI_TREE_DECODE_OPERANDS(uint16_t),
                                                     MI_WINDOW_DECODE_OUT);
int mi_block_attention_window_decode_lists_fp8_bf16(MI_TREE_DECODE_LISTS, MI_TREE_DECODE_OPERANDS(uint8_t), MI_TREE_DECODE_SCALES,
                                                    MI_WINDOW_DECODE_OUT);
int mi_block_attention_window_decode_lists_fp8_f16(MI_TREE_DECODE_LISTS, MI_TREE_DECODE_OPERANDS(uint8_t), MI_TREE_DECODE_SCALES,
                                                   MI_WINDOW_DECODE_OUT);
int mi_block_attention_window_decode_lists_paged_fp8_bf16(MI_TREE_DECODE_LISTS, MI_TREE_DECODE_TABLE, MI_TREE_DECODE_OPERANDS(uint8_t),
                                                          MI_TREE_DECODE_SCALES, MI_WINDOW_DECODE_OUT);
int mi_block_attention_window_decode_lists_paged_fp8_f16(MI_TREE_DECODE_LISTS, MI_TREE_DECODE_TABLE, MI_TREE_DECODE_OPERANDS(uint8_t),
                                                         MI_TREE_DECODE_SCALES, MI_WINDOW_DECODE_OUT);

/* ------------------------------------------------------------------------ *
 * Compaction after a speculative step: mi_kv_compact{,_paged} move the accepted path's k / v rows to the front
 * of the window of the T ≤ 64 drafted slots, in place, in one launch for k and v.  The cache is that of mi_kv_append_* (items,
 * heads, Smax, D, the strides IN ELEMENTS, block_table, table_ld, pages, page as there); elem_bytes is 2 (bfloat16 / float16) or 1
 * (e4m3fn): rows are bit copies.
 *   k_lens         [lens_count], lens_count 1 or items / heads: the lengths that STILL COUNT the T drafted slots; not clamped, not written
 *   accept         int32 [items / heads][T]: offsets into the window;   accept_counts  int32 [items / heads]
 * With base = k_len − T and n = clamp(accept_counts[b], 0, T): for i < n, row base + i of every k / v head of batch item b becomes
 * the OLD row base + accept[b][i] — every source row of an (item, head) is read before any is written.  A row whose offset lies
 * outside [0, T), whose source or destination row lies outside [0, Smax), or (paged) behind a table entry outside [0, pages) is
 * left unwritten; rows at or beyond n and everything else keep their bytes.  No atomics, no read-back: graph-capturable.
 * MI_EINVAL before any HIP call: elem_bytes, T > 64, what mi_kv_append_* refuses about sizes and the cache, a null or misaligned
 * k_lens, accept or accept_counts.  MI_OK for items == 0 or T == 0.
 * ------------------------------------------------------------------------ */
#define MI_KV_COMPACT_OPERANDS                                                                                                 \
  int32_t D, int32_t elem_bytes, void *k, int64_t ldk, int64_t headK, int64_t batchK, void *v, int64_t ldv, int64_t headV,     \
      int64_t batchV, const int32_t *k_lens, int32_t lens_count, const int32_t *accept, const int32_t *accept_counts, mi_stream_t stream
int mi_kv_compact(int32_t items, int32_t heads, int32_t T, int32_t Smax, MI_KV_COMPACT_OPERANDS);int mi_kv_compact_paged(int32_t items, int32_t heads, int32_t T, int32_t Smax, const int32_t* block_table, int64_t table_ld,
                        int32_t pages, int32_t page, MI_KV_COMPACT_OPERANDS);

/* ------------------------------------------------------------------------ *
 * The fused rotary embedding + KV-cache append with EXPLICIT POSITIONS: the eight mi_rope_kv_append_* entries
 * as mi_rope_pos_kv_append{,_paged}{,_fp8}_T, with one parameter after new_lens:
 *   positions  int32 [items / heads][T] on the device, 4-byte aligned, read by the kernel and never read back
 * Slot t of batch item b is rotated — its k row and its q rows alike — with row positions[b][t] of cos / sin in the place of row
 * pos = k_len − T + t, and is still written where the parent writes it: q_out's and k_out's row t, the cache row pos.  A tree
 * node is so rotated by prefix length + depth while it is stored in slot t.  The slot holds a token iff the parent's conditions
 * hold (t ≥ T − n, 0 ≤ pos < table_rows) AND 0 ≤ positions[b][t] < table_rows; otherwise zero rows and nothing into the cache,
 * as there.  The arithmetic is the parent's: two products, one sum, no fma, one rounding; positions[b][t] = pos gives its bits.
 * MI_EINVAL before any HIP call: what the parent refuses, a null or misaligned positions.  (`pos` stands before `kv_append` in
 * the name: the entries `mi_rope_kv_append…` are a closed family.)
 * ------------------------------------------------------------------------ */
int mi_rope_pos_kv_append_bf16(int32_t items, int32_t heads, int32_t T, int32_t Smax, int32_t D, MI_ROPE_KV_APPEND_OPERANDS(uint16_t),
                               const int32_t* positions, mi_stream_t stream);
int mi_rope_pos_kv_append_f16(int32_t items, int32_t heads, int32_t T, int32_t Smax, int32_t D, MI_ROPE_KV_APPEND_OPERANDS(uint16_t),
                              const int32_t* positions, mi_stream_t stream);
int mi_rope_pos_kv_append_paged_bf16(int32_t items, int32_t heads, int32_t T, int32_t Smax, const int32_t* block_table,
                                     int64_t table_ld, int32_t pages, int32_t page, int32_t D, MI_ROPE_KV_APPEND_OPERANDS(uint16_t),
                                     const int32_t* positions, mi_stream_t stream);
int mi_rope_pos_kv_append_paged_f16(int32_t items, int32_t heads, int32_t T, int32_t Smax, const int32_t* block_table,
                                    int64_t table_ld, int32_t pages, int32_t page, int32_t D, MI_ROPE_KV_APPEND_OPERANDS(uint16_t),
                                    const int32_t* positions, mi_stream_t stream);
int mi_rope_pos_kv_append_fp8_bf16(int32_t items, int32_t heads, int32_t T, int32_t Smax, int32_t D,
                                   MI_ROPE_KV_APPEND_OPERANDS(uint8_t), const int32_t* positions, const float* k_scale,
                                   int32_t k_scale_count, const float* v_scale, int32_t v_scale_count, mi_stream_t stream);
int mi_rope_pos_kv_append_fp8_f16(int32_t items, int32_t heads, int32_t T, int32_t Smax, int32_t D,
                                  MI_ROPE_KV_APPEND_OPERANDS(uint8_t), const int32_t* positions, const float* k_scale,
                                  int32_t k_scale_count, const float* v_scale, int32_t v_scale_count, mi_stream_t stream);
int mi_rope_pos_kv_append_paged_fp8_bf16(int32_t items, int32_t heads, int32_t T, int32_t Smax, const int32_t* block_table,
                                         int64_t table_ld, int32_t pages, int32_t page, int32_t D,
                                         MI_ROPE_KV_APPEND_OPERANDS(uint8_t), const int32_t* positions, const float* k_scale,
                                         int32_t k_scale_count, const float* v_scale, int32_t v_scale_count, mi_stream_t stream);
int mi_rope_pos_kv_append_paged_fp8_f16(int32_t items, int32_t heads, int32_t T, int32_t Smax, const int32_t* block_table,
                                        int64_t table_ld, int32_t pages, int32_t page, int32_t D,
                                        MI_ROPE_KV_APPEND_OPERANDS(uint8_t), const int32_t* positions, const float* k_scale,
                                        int32_t k_scale_count, const float* v_scale, int32_t v_scale_count, mi_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Key-block selection per POSITION TILE for chunked prefill: mi_block_select_tiles_T scores every 64-key
 * block against the queries of a whole 64-position tile of the chunk on the matrix cores and lists the K best per tile.
 * q, bounds, k_lens, group, K, sink, local and the limits are mi_block_select_T's; new_lens, new_lens_count the prefill
 * entries'.  X = ⌈T / 64⌉ + 1 tiles per item; the geometry is the prefill entries': with klen = clamp(k_len, 0, Smax),
 * n = clamp(new_len, 0, T) (T for a NULL new_lens), tile x of item c is layout row r = ⌊(klen − T) / 64⌋ + x and its tokens the
 * positions pos ∈ [64r, 64r + 64) ∩ [max(klen − n, 0), klen), slot pos − (klen − T).  A tile without a token: count 0, a row of
 * −1, scores −inf.  Else the candidates are the blocks J ≤ r, and
 *   s_{t,g}(J) = [q⁻ | q⁺] · [lo | hi]ᵀ in fp32 on the matrix cores (v_mfma_f32_16x16x32 in ascending k from +0) — the score
 *   Σ_d max(q_d·lo_d, q_d·hi_d) of mi_block_select_T in another order of summation: q⁻ holds the elements of q whose sign bit
 *   is set, q⁺ the others —, score(J) = max over the tile's tokens and the group's heads (a NaN term is passed over while
 *   another is a number; a slot without a token takes no part).
 * Forced blocks (the first `sink`, the `local` ending at r), the order (score descending, index ascending; −0 as +0; NaN
 * lowest), count = min(K, candidates), the list in ASCENDING block index and −1 from count on are mi_block_select_T's.
 * block_ids int32 [items][X][K], block_counts int32 [items][X], scores NULL or float32 [items][X][Smax/64] (the candidates'
 * scores, −inf elsewhere; the selection is an exact function of them).  Bounds of non-candidates and q of slots without a
 * token are never read.  With an inf or NaN in q or bounds the product form may give NaN (0 · inf) where mi_block_select_T
 * has a number: then only the structure holds — the count, ascending distinct candidates, every forced block listed, no
 * store outside the row.  No atomics, no read-back: graph-capturable.
 * MI_EINVAL, before any HIP call: what mi_block_select_T refuses, a misaligned new_lens or a count other than 1 or
 * items / heads.  items == 0 or T == 0: MI_OK.
 * ------------------------------------------------------------------------ */
#define MI_BLOCK_SELECT_TILES_OPERANDS                                                                                          \
  int32_t items, int32_t heads, int32_t T, int32_t Smax, int32_t D, int32_t group, const uint16_t *q, int64_t ldq, int64_t headQ, \
      int64_t batchQ, const uint16_t *bounds, const int32_t *k_lens, int32_t lens_count, const int32_t *new_lens,               \
      int32_t new_lens_count, int32_t K, int32_t sink, int32_t local, int32_t *block_ids, int32_t *block_counts, float *scores, \
      mi_stream_t stream
int mi_block_select_tiles_bf16(MI_BLOCK_SELECT_TILES_OPERANDS);
int mi_block_select_tiles_f16(MI_BLOCK_SELECT_TILES_OPERANDS);

/* ------------------------------------------------------------------------ *
 * Prefill over the caller's lists, mi_block_attention_lists_prefill{,_paged}{,_fp8}_T: mi_block_attention_prefill{,_paged}{,_fp8}_T with the list of POSITION
 * TILE x of k / v item c given as a row of block_ids, in the place of a layout row.  X = ⌈T / 64⌉ + 1 tiles per item, from the
 * shape alone; tile x of item c is layout row r = ⌊(clamp(k_len, 0, Smax) − T) / 64⌋ + x of the prefill entries and holds the
 * slots whose pos lies in [64r, 64r + 64).
 *   block_ids     int32 [items][X][K], 4-byte aligned; block_counts int32 [items][X]; K ≥ 1.  The list of tile x of item c
 *                 is the first clamp(block_counts[c·X + x], 0, K) entries of row c·X + x; the group's query heads share it.
 *                 An entry outside [0, Smax/64) — the −1 padding —, above r, or at or beyond ⌈k_len / 64⌉ is skipped; a
 *                 block listed twice counts twice.  The row of a tile without a token is not looked at.
 * Everything after the two bounds of the list is the prefill entries' walk, statement for statement: out and lse have the
 * BITS of mi_block_attention_prefill{,_paged}{,_fp8}_T with a layout per k / v item whose row r lists the same blocks in the
 * same order.  Every row of out and lse is written exactly once by the one launch.  No atomics, no workspace, no read-back:
 * graph-capturable while the lists, k_lens, new_lens, the cache, the table and the scales change in place.
 * Validation before any HIP call: what the prefill entry of the same form refuses but for the layout, K < 1, a null or
 * misaligned block_ids / block_counts → MI_EINVAL; items · X · K beyond int32 → MI_ERANGE; items == 0 or T == 0 → MI_OK.
 * There are no split forms: a list has K entries.  (`lists` stands before `prefill` in the name, as in
 * mi_block_attention_lists_decode…: the entries `mi_block_attention_prefill…` are the closed family of the sixteen above.)
 * ------------------------------------------------------------------------ */
#define MI_BLOCK_ATTENTION_PREFILL_LISTS_HEAD \
  const int32_t *block_ids, const int32_t *block_counts, int32_t K, int32_t items, int32_t heads, int32_t T, int32_t Smax
int mi_block_attention_lists_prefill_bf16(MI_BLOCK_ATTENTION_PREFILL_LISTS_HEAD, int32_t D,
                                          MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint16_t), MI_BLOCK_ATTENTION_PREFILL_OUT);
int mi_block_attention_lists_prefill_f16(MI_BLOCK_ATTENTION_PREFILL_LISTS_HEAD, int32_t D,
                                         MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint16_t), MI_BLOCK_ATTENTION_PREFILL_OUT);
int mi_block_attention_lists_prefill_paged_bf16(MI_BLOCK_ATTENTION_PREFILL_LISTS_HEAD, MI_BLOCK_ATTENTION_PREFILL_TABLE, int32_t D,
                                                MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint16_t), MI_BLOCK_ATTENTION_PREFILL_OUT);
int mi_block_attention_lists_prefill_paged_f16(MI_BLOCK_ATTENTION_PREFILL_LISTS_HEAD, MI_BLOCK_ATTENTION_PREFILL_TABLE, int32_t D,
                                               MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint16_t), MI_BLOCK_ATTENTION_PREFILL_OUT);
int mi_block_attention_lists_prefill_fp8_bf16(MI_BLOCK_ATTENTION_PREFILL_LISTS_HEAD, int32_t D,
                                              MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint8_t), MI_BLOCK_ATTENTION_PREFILL_SCALES,
                                              MI_BLOCK_ATTENTION_PREFILL_OUT);
int mi_block_attention_lists_prefill_fp8_f16(MI_BLOCK_ATTENTION_PREFILL_LISTS_HEAD, int32_t D,
                                             MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint8_t), MI_BLOCK_ATTENTION_PREFILL_SCALES,
                                             MI_BLOCK_ATTENTION_PREFILL_OUT);
int mi_block_attention_lists_prefill_paged_fp8_bf16(MI_BLOCK_ATTENTION_PREFILL_LISTS_HEAD, MI_BLOCK_ATTENTION_PREFILL_TABLE,
                                                    int32_t D, MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint8_t),
                                                    MI_BLOCK_ATTENTION_PREFILL_SCALES, MI_BLOCK_ATTENTION_PREFILL_OUT);
int mi_block_attention_lists_prefill_paged_fp8_f16(MI_BLOCK_ATTENTION_PREFILL_LISTS_HEAD, MI_BLOCK_ATTENTION_PREFILL_TABLE,
                                                   int32_t D, MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint8_t),
                                                   MI_BLOCK_ATTENTION_PREFILL_SCALES, MI_BLOCK_ATTENTION_PREFILL_OUT);

/* ------------------------------------------------------------------------ *
 * Sliding windows and sink keys for prefill: the sixteen UNSPLIT prefill entries — the layout entries
 * mi_block_attention_prefill{,_paged}{,_fp8}_T and the list entries mi_block_attention_lists_prefill{,_paged}{,_fp8}_T — as
 * mi_block_attention_window_prefill{,_lists}{,_paged}{,_fp8}_T, with `window, sink` (as above) between `scale` (or the four scale
 * parameters) and `out`.  The own row at pos — the tile geometry of the parents — sees key j iff the parent's rule holds AND
 * (j > pos − window or j < sink): a test per element beside the diagonal's.  A listed block J with 64 J ≥ sink and
 * 64 J + 63 ≤ 64 r − window, r the tile's layout row, is hidden from every position the tile can hold and is never loaded; a block
 * that some row of the tile sees is loaded as in the parents.  Everything else — the order of summation, new_lens, the zero rows
 * and lse −inf of slots without a token and of rows that see nothing — is the parent's; window = 2³¹ − 1, or sink ≥ Smax, gives
 * the parent entry's bits.  There is no split form: a windowed row's list is short.
 * Validation before any HIP call: window < 1 or sink < 0 — MI_EINVAL, before anything else; then what the parent refuses.
 * ------------------------------------------------------------------------ */
#define MI_WINDOW_PREFILL_OUT int32_t window, int32_t sink, uint16_t *out, int64_t ldo, int64_t strideO, float *lse, mi_stream_t stream
int mi_block_attention_window_prefill_bf16(MI_BLOCK_ATTENTION_PREFILL_LIST, int32_t D, MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint16_t),
                                           MI_WINDOW_PREFILL_OUT);
int mi_block_attention_window_prefill_f16(MI_BLOCK_ATTENTION_PREFILL_LIST, int32_t D, MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint16_t),
                                          MI_WINDOW_PREFILL_OUT);
int mi_block_attention_window_prefill_paged_bf16(MI_BLOCK_ATTENTION_PREFILL_LIST, MI_BLOCK_ATTENTION_PREFILL_TABLE, int32_t D,
                                                 MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint16_t), MI_WINDOW_PREFILL_OUT);
int mi_block_attention_window_prefill_paged_f16(MI_BLOCK_ATTENTION_PREFILL_LIST, MI_BLOCK_ATTENTION_PREFILL_TABLE, int32_t D,
                                                MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint16_t), MI_WINDOW_PREFILL_OUT);
int mi_block_attention_window_prefill_fp8_bf16(MI_BLOCK_ATTENTION_PREFILL_LIST, int32_t D, MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint8_t),
                                               MI_BLOCK_ATTENTION_PREFILL_SCALES, MI_WINDOW_PREFILL_OUT);
int mi_block_attention_window_prefill_fp8_f16(MI_BLOCK_ATTENTION_PREFILL_LIST, int32_t D, MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint8_t),
                                              MI_BLOCK_ATTENTION_PREFILL_SCALES, MI_WINDOW_PREFILL_OUT);
int mi_block_attention_window_prefill_paged_fp8_bf16(MI_BLOCK_ATTENTION_PREFILL_LIST, MI_BLOCK_ATTENTION_PREFILL_TABLE, int32_t D,
                                                     MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint8_t), MI_BLOCK_ATTENTION_PREFILL_SCALES,
                                                     MI_WINDOW_PREFILL_OUT);
int mi_block_attention_window_prefill_paged_fp8_f16(MI_BLOCK_ATTENTION_PREFILL_LIST, MI_BLOCK_ATTENTION_PREFILL_TABLE, int32_t D,
                                                    MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint8_t), MI_BLOCK_ATTENTION_PREFILL_SCALES,
                                                    MI_WINDOW_PREFILL_OUT);
int mi_block_attention_window_prefill_lists_bf16(MI_BLOCK_ATTENTION_PREFILL_LISTS_HEAD, int32_t D,
                                                 MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint16_t), MI_WINDOW_PREFILL_OUT);
int mi_block_attention_window_prefill_lists_f16(MI_BLOCK_ATTENTION_PREFILL_LISTS_HEAD, int32_t D,
                                                MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint16_t), MI_WINDOW_PREFILL_OUT);
int mi_block_attention_window_prefill_lists_paged_bf16(MI_BLOCK_ATTENTION_PREFILL_LISTS_HEAD, MI_BLOCK_ATTENTION_PREFILL_TABLE, int32_t D,
                                                       MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint16_t), MI_WINDOW_PREFILL_OUT);
int mi_block_attention_window_prefill_lists_paged_f16(MI_BLOCK_ATTENTION_PREFILL_LISTS_HEAD, MI_BLOCK_ATTENTION_PREFILL_TABLE, int32_t D,
                                                      MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint16_t), MI_WINDOW_PREFILL_OUT);
int mi_block_attention_window_prefill_lists_fp8_bf16(MI_BLOCK_ATTENTION_PREFILL_LISTS_HEAD, int32_t D,
                                                     MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint8_t), MI_BLOCK_ATTENTION_PREFILL_SCALES,
                                                     MI_WINDOW_PREFILL_OUT);
int mi_block_attention_window_prefill_lists_fp8_f16(MI_BLOCK_ATTENTION_PREFILL_LISTS_HEAD, int32_t D,
                                                    MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint8_t), MI_BLOCK_ATTENTION_PREFILL_SCALES,
                                                    MI_WINDOW_PREFILL_OUT);
int mi_block_attention_window_prefill_lists_paged_fp8_bf16(MI_BLOCK_ATTENTION_PREFILL_LISTS_HEAD, MI_BLOCK_ATTENTION_PREFILL_TABLE,
                                                           int32_t D, MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint8_t),
                                                           MI_BLOCK_ATTENTION_PREFILL_SCALES, MI_WINDOW_PREFILL_OUT);
int mi_block_attention_window_prefill_lists_paged_fp8_f16(MI_BLOCK_ATTENTION_PREFILL_LISTS_HEAD, MI_BLOCK_ATTENTION_PREFILL_TABLE,
                                                          int32_t D, MI_BLOCK_ATTENTION_PREFILL_OPERANDS(uint8_t),
                                                          MI_BLOCK_ATTENTION_PREFILL_SCALES, MI_WINDOW_PREFILL_OUT);

/* ------------------------------------------------------------------------ *
 * Block-sparse (BSR) × dense products on the matrix cores — NEW relative to the reference: C[b] = op(A) · B[b] in
 * bfloat16 / float16 (T, 2-byte bit patterns) with A given as the kept 64 × 64 blocks of a CSR block list, shared by
 * every item of the batch, and the sampled product on the same list:
 *   rowptr   int32 [rows/64 + 1], col int32 [nnz]: for each 64-row block of C the blocks of A it sums over — col is the
 *            64-block of the inner dimension (the 64 rows of B) the entry meets.  trans_a == 0: the block rows of A and
 *            their block columns; trans_a != 0: the TRANSPOSED list (block columns of A and their block rows), every
 *            block used transposed.  A duplicate block is unsupported (it would count twice);
 *   entry_id int32 [nnz] or NULL: entry p reads (sddmm: writes) block entry_id[p] of values; NULL: block p;
 *   values   [nvalues][64][64], row-major blocks, 16-byte aligned;
 *   B [batch][inner][N], C [batch][rows][N]: leading dimension ≥ N and item stride in elements, any 2-byte alignment
 *            (16-byte aligned bases with leading dimensions and strides multiples of 8 run the 16-byte form);
 *   sddmm:   entry_row, col int32 [nnz]: block row and block column of entry p; dC [batch][M][N], B [batch][K][N];
 *            dvalues [nvalues][64][64], 16-byte aligned: dvalues[e] = Σ over the items of dC[I-rows, :] · B[J-rows, :]ᵀ.
 * Arithmetic (all three products): every product is v_mfma_f32_16x16x32_T with fp32 accumulators, in the k-slots of
 * mi_gemm_T; every output element is ONE accumulator started at +0 and rounded once at the store, by the static_cast
 * narrowing of mi_gemm_T; the bits do not depend on the launch shape, the column tile, the position in the batch or the
 * alignment form.
 *   C = A·B:     element (i, j) walks the entries of its block row in the order of the list (the caller gives it in
 *                ascending block column) and, within a block, the two 32-deep k-steps ascending;
 *   dB = Aᵀ·dC:  element (k, j) walks the transposed list of block column k/64 (ascending block row), each block used
 *                transposed;
 *   dvalues[e]:  the sum runs over the flattened width k' = item · N + j (item-major, items ascending) in ascending
 *                32-steps, a ragged last step zero-padded in both operands.
 * For finite operands and ascending lists these are, bit for bit, mi_gemm_T(A_dense, B), mi_gemm_T(transa, A_dense, dC)
 * and the kept blocks of mi_gemm_T(transb, dC, B) on the flattened operands: the same instruction in the same order, an
 * unkept block contributing only exact zero products to the dense run.  A block outside the list is never loaded, nor
 * the rows of B it would meet: NaN or inf there reaches no output.  An empty list stores zeros.  A listed column outside
 * the grid or an entry id outside [0, nvalues) is skipped (sddmm: the block is zero / not written), offsets are clamped
 * to [0, nnz].  No atomics, no workspace, no host synchronisation: graph-capturable.
 * mi_bsr_mm_tile_n(rows, N, batch) is the column tile mi_bsr_mm_T launches for a shape — a function of the SHAPE alone:
 * 128 when N > 64 and (rows/64) · ceil(N/128) · batch ≥ 512, else 64 (also for an empty shape).  The bits of C do not
 * depend on it; it is exported so that a test can tell which tile it ran.
 * Validation before any HIP call: a negative size or stride, rows / inner / M / K not a multiple of 64, ld < N,
 * nvalues < nnz without entry ids → MI_EINVAL; nnz, nvalues or batch · N (sddmm) ≥ 2³¹ → MI_ERANGE; rows, N or batch
 * == 0 (sddmm: nnz == 0) → MI_OK, nothing touched; a NULL, odd or (values, dvalues) not 16-byte aligned pointer → MI_EINVAL.
 * ------------------------------------------------------------------------ */
int mi_bsr_mm_bf16(const int32_t* rowptr, const int32_t* col, const int32_t* entry_id, int64_t nnz, int32_t trans_a,
                   int32_t rows, int32_t inner, int32_t N, int32_t batch, const uint16_t* values, int64_t nvalues,
                   const uint16_t* B, int64_t ldb, int64_t strideB, uint16_t* C, int64_t ldc, int64_t strideC,
                   mi_stream_t stream);
int mi_bsr_mm_f16(const int32_t* rowptr, const int32_t* col, const int32_t* entry_id, int64_t nnz, int32_t trans_a,
                  int32_t rows, int32_t inner, int32_t N, int32_t batch, const uint16_t* values, int64_t nvalues,
                  const uint16_t* B, int64_t ldb, int64_t strideB, uint16_t* C, int64_t ldc, int64_t strideC,
                  mi_stream_t stream);
int mi_bsr_sddmm_bf16(const int32_t* entry_row, const int32_t* col, const int32_t* entry_id, int64_t nnz, int32_t M,
                      int32_t K, int32_t N, int32_t batch, const uint16_t* dC, int64_t lddc, int64_t strideDC,
                      const uint16_t* B, int64_t ldb, int64_t strideB, uint16_t* dvalues, int64_t nvalues,
                      mi_stream_t stream);
int mi_bsr_sddmm_f16(const int32_t* entry_row, const int32_t* col, const int32_t* entry_id, int64_t nnz, int32_t M,
                     int32_t K, int32_t N, int32_t batch, const uint16_t* dC, int64_t lddc, int64_t strideDC,
                     const uint16_t* B, int64_t ldb, int64_t strideB, uint16_t* dvalues, int64_t nvalues,
                     mi_stream_t stream);
int mi_bsr_mm_tile_n(int32_t rows, int32_t N, int32_t batch);

/* ------------------------------------------------------------------------ *
 * Block-sparse linear layer on the matrix cores — NEW relative to the reference: Y = X·Wᵀ (+ bias) in bfloat16 / float16
 * (T, 2-byte bit patterns) with the weight W [outer-of-the-forward = out, in] given as its kept 64 × 64 blocks, the tokens
 * X [tokens, in] row-major; dX = dY·W on the same kernel; the weight gradient on the kept blocks.
 *
 * mi_bsr_linear_T:  Y[t, 64·P + c] = Σ over the entries p of list row P, in list order, Σ_k X[t, 64·col[p] + k] · Wblk(c, k)
 *   rowptr   int32 [outer/64 + 1], col int32 [nnz]: for each 64-column block P of Y the 64-column blocks of X it sums over;
 *   entry_id int32 [nnz] or NULL: entry p reads block entry_id[p] of values; NULL: block p;
 *   trans_w == 0 (the forward): P a block row of W, the list its kept block columns, Wblk(c, k) = values[e][c][k];
 *   trans_w != 0 (dX = dY·W):   P a block column of W, the list the block rows that keep it (the TRANSPOSED list),
 *                               Wblk(c, k) = values[e][k][c]; X is dY;
 *   values   [nvalues][64][64], row-major blocks of W, 16-byte aligned;
 *   X [tokens][inner], Y [tokens][outer]: leading dimensions ldx ≥ inner, ldy ≥ outer in elements, any 2-byte alignment
 *            (16-byte aligned bases with leading dimensions multiples of 8 run the 16-byte form); any tokens ≥ 0;
 *   bias     [outer] or NULL, any 2-byte alignment: Y = rne_T(acc + up(bias[64·P + c])) — one fp32 add of the exactly
 *            widened bias, one rounding (the epilogue of mi_gemm_bias_T).
 * mi_bsr_wgrad_T:   dvalues[entry_id[p]][o][i] = Σ_t dY[t, 64·entry_row[p] + o] · X[t, 64·col[p] + i]
 *   entry_row, col int32 [nnz]: block row (of `out`) and block column (of `in`) of entry p; entry_id as above (written);
 *   dY [tokens][out], X [tokens][in] with lddy ≥ out, ldx ≥ in; dvalues [nvalues][64][64], 16-byte aligned;
 *   splits   the number S of equal token ranges (0: mi_bsr_wgrad_split_count(nnz, tokens)); S > 1 needs
 *            tokens % (32·S) == 0 and a 16-byte aligned workspace of mi_bsr_wgrad_workspace_bytes(nnz, S) =
 *            S·nnz·64·64·4 bytes (smaller: MI_ENOMEM — never a silent unsplit product).
 * mi_bsr_wgrad_split_count(nnz, tokens) is a function of those two numbers alone: 1 below 2048 tokens, else the largest
 *   power of two ≤ min(1024 / nnz, tokens / 512, 32) (at least 1), halved until tokens % (32·S) == 0.
 * mi_bsr_linear_tile_tokens(outer, tokens) is the token tile mi_bsr_linear_T launches for a shape — a function of the
 *   SHAPE alone: 128 when tokens > 64 and (outer/64) · ceil(tokens/128) ≥ 512, else 64 (also for an empty shape).  The
 *   bits of Y do not depend on it; it is exported so that a test can tell which tile it ran.
 *
 * Arithmetic: every product is v_mfma_f32_16x16x32_T with fp32 accumulators in the k-slots of mi_gemm_T; every output
 * element is ONE accumulator started at +0, carried through its list in the order given (the caller gives it ascending)
 * and, within a block, through the two 32-deep k-steps ascending, and rounded once at the store (static_cast narrowing).
 * The bits do not depend on the token tile, the workgroup numbering, the position of a token, the alignment form or the
 * order of the layout the lists were sorted from.  The weight gradient sums the tokens of a range in ascending 32-steps
 * from +0, a ragged last step zero-padded in both operands; with S > 1 range s goes to an fp32 partial P[s][p][64][64],
 * not narrowed, and a combine kernel stores rne_T((((P[0] + P[1]) + P[2]) + …)) with fp32 adds in index order.
 * For finite operands and ascending lists these are, bit for bit, mi_gemm_bias_T / mi_gemm_T(transb, X, W_dense),
 * mi_gemm_T(dY, W_dense) and the kept blocks of mi_gemm_split_T(transa, dY, X, splits = S) (S = 1: mi_gemm_T(transa)):
 * the same instruction in the same order, an unkept block contributing only exact zero products to the dense run.
 * A block outside the list is never loaded, nor the columns of X (of dY) it would meet: NaN or inf there reaches no
 * output.  An empty list row stores +0, or the bias.  A listed column outside the grid or an entry id outside
 * [0, nvalues) is skipped (wgrad: the block is zero / not written), offsets are clamped to [0, nnz].  No float atomics,
 * no host synchronisation: graph-capturable.
 * Validation before any HIP call: a negative size, inner / outer / out / in not a multiple of 64, ld below the width,
 * nvalues < nnz without entry ids, splits < 0 or tokens not a multiple of 32·splits → MI_EINVAL; nnz, nvalues or a
 * leading dimension ≥ 2³¹ → MI_ERANGE; tokens or outer == 0 (wgrad: nnz == 0) → MI_OK, nothing touched; a NULL or odd
 * pointer, values / dvalues / workspace not 16-byte aligned → MI_EINVAL; a workspace too small → MI_ENOMEM.
 * ------------------------------------------------------------------------ */
int mi_bsr_linear_bf16(const int32_t* rowptr, const int32_t* col, const int32_t* entry_id, int64_t nnz, int32_t trans_w,
                       int32_t tokens, int32_t inner, int32_t outer, const uint16_t* values, int64_t nvalues,
                       const uint16_t* X, int64_t ldx, const uint16_t* bias, uint16_t* Y, int64_t ldy, mi_stream_t stream);
int mi_bsr_linear_f16(const int32_t* rowptr, const int32_t* col, const int32_t* entry_id, int64_t nnz, int32_t trans_w,
                      int32_t tokens, int32_t inner, int32_t outer, const uint16_t* values, int64_t nvalues,
                      const uint16_t* X, int64_t ldx, const uint16_t* bias, uint16_t* Y, int64_t ldy, mi_stream_t stream);
int mi_bsr_wgrad_bf16(const int32_t* entry_row, const int32_t* col, const int32_t* entry_id, int64_t nnz, int32_t tokens,
                      int32_t out, int32_t in, const uint16_t* dY, int64_t lddy, const uint16_t* X, int64_t ldx,
                      uint16_t* dvalues, int64_t nvalues, int32_t splits, void* workspace, size_t workspace_bytes,
                      mi_stream_t stream);
int mi_bsr_wgrad_f16(const int32_t* entry_row, const int32_t* col, const int32_t* entry_id, int64_t nnz, int32_t tokens,
                     int32_t out, int32_t in, const uint16_t* dY, int64_t lddy, const uint16_t* X, int64_t ldx,
                     uint16_t* dvalues, int64_t nvalues, int32_t splits, void* workspace, size_t workspace_bytes,
                     mi_stream_t stream);
int mi_bsr_wgrad_split_count(int64_t nnz, int64_t tokens);
int mi_bsr_linear_tile_tokens(int32_t outer, int32_t tokens);
size_t mi_bsr_wgrad_workspace_bytes(int64_t nnz, int32_t splits);

int mi_ipc_export(const void* dev_ptr, void* handle_out, int64_t* offset_out, int64_t* alloc_bytes_out);
int mi_ipc_open(const void* handle, void** base_out);
int mi_ipc_close(const void* handle);
int mi_ipc_open_count(void);

/* Replaces dummy_kernel_launch (src/baseline_mm.cu:24-35): launches a 64×64
 * grid on the stream; each thread writes its global id into out[4096]
 * (the reference printf()s it). */
int mi_dummy_kernel(int32_t* out, mi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MI_SPMM_H_ */
