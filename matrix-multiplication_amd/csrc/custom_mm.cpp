// custom_mm — pybind11 module with the reference's 16 entry points
// (smoorjani/matrix-multiplication src/custom_mm.cpp:393-416, same names, same
// positional signatures, same "caller allocates C, callee fills it and returns
// the same tensor" convention), backed by the MI355X C-ABI library
// libmi_spmm.so (include/mi_spmm.h).
//
// This layer only validates tensors, extracts pointers / leading dimensions,
// looks up torch's current HIP stream for the tensors' device and calls the
// C-ABI.  There is no CPU fallback: every compute entry point requires device
// tensors and raises otherwise.
//
// Differences from the reference that are deliberate:
//  * work is enqueued on torch's current stream of the tensors' device, not on
//    the legacy default stream (reference naive_sparse_mm.cu:117,133);
//  * dtype, device, shape and layout are checked (the reference reads
//    data_ptr() of whatever it is given, README.md:44); strided / transposed
//    views are handled through leading dimensions or copied, never misread.
//    The CONTENTS of CSR arrays (columns in range, offsets monotone) are trusted on
//    the per-product entry points, as in the reference; `validate_csr` checks them on
//    request and the inspector entry points check them once at inspect time;
//  * the inspect-style registries hold tensor references (the reference keeps
//    raw pointers and later cudaFree()s torch memory, custom_mm.cpp:249-251,
//    :272-277), are mutex-protected, and an unknown layer name raises instead
//    of aliasing handle 0 (custom_mm.cpp:260-263, :338-341).
#include <torch/extension.h>

#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>

#include <array>
#include <cstdlib>
#include <initializer_list>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <unordered_map>
#include <utility>

#include "mi_spmm.h"

namespace {
#include "custom_mm_helpers.inc"
#include "custom_mm_reference.inc"
#include "custom_mm_extras.inc"
#include "custom_mm_inspect.inc"
#include "custom_mm_reduce.inc"
#include "custom_mm_softmax.inc"
#include "custom_mm_attention.inc"
#include "custom_mm_block_attention.inc"
#include "custom_mm_kv_cache.inc"
#include "custom_mm_block_attention_decode.inc"
#include "custom_mm_block_attention_prefill.inc"
#include "custom_mm_kv_append.inc"
#include "custom_mm_kv_compact.inc"
#include "custom_mm_rope_kv_append.inc"
#include "custom_mm_kv_block_bounds.inc"
#include "custom_mm_block_select.inc"
#include "custom_mm_block_attention_decode_lists.inc"
#include "custom_mm_block_attention_prefill_lists.inc"
#include "custom_mm_bsr.inc"
#include "custom_mm_bsr_linear.inc"

// ---- handle init / destroy (reference custom_mm.cpp:361-391) ----------------
// There are no vendor handles on this path; init checks that the C-ABI library
// this module was linked against has the expected ABI (printing to stderr on
// mismatch, like the reference's init failures) and all four are idempotent.
void init_backend(const char* name) {
  if (mi_spmm_abi_version() != MI_SPMM_ABI_VERSION)
    std::cerr << name << " initialization error: libmi_spmm ABI " << mi_spmm_abi_version()
              << " != " << MI_SPMM_ABI_VERSION << std::endl;
}
void init_cublas_handle() { init_backend("cuBLAS-path"); }
void destroy_cublas_handle() {}
void init_cusparse_handle() { init_backend("cuSPARSE-path"); }
void destroy_cusparse_handle() {}

// reference baseline_mm.cu:24-35 prints every thread id of a 64×64 launch;
// this launches the same grid, checks the ids on the host and prints one line.
void dummy_kernel_launch() {
  const auto dev = torch::Device(torch::kCUDA, c10::hip::current_device());
  torch::Tensor out = torch::full({4096}, -1, torch::dtype(torch::kInt32).device(dev));
  check_status(mi_dummy_kernel(out.data_ptr<int32_t>(), stream_of(out)), "dummy_kernel");
  torch::Tensor host = out.cpu();  // synchronises, like the reference's cudaDeviceSynchronize
  const bool ok = host.equal(torch::arange(4096, torch::kInt32));
  std::cout << "dummy_kernel: 64 blocks x 64 threads ran, ids " << (ok ? "0..4095 ok" : "WRONG")
            << std::endl;
  TORCH_CHECK(ok, "dummy_kernel wrote wrong thread ids");
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("init_cublas", &init_cublas_handle, "Create cuBLAS handle.");
  m.def("destroy_cublas", &destroy_cublas_handle, "Destroy cuBLAS handle.");

  m.def("init_cusparse", &init_cusparse_handle, "Create cuSPARSE handle.");
  m.def("destroy_cusparse", &destroy_cusparse_handle, "Destroy cuSPARSE handle.");

  m.def("cublas_mmul", &cublas_mmul, "cuBLAS Torch Matrix Multiplication");
  m.def("cublas_bmm", &cublas_bmm, "cuBLAS Batched Torch Matrix Multiplication");
  m.def("cusparse_mmul", &cusparse_mmul, "cuSPARSE Torch Matrix Multiplication");

  m.def("dummy_kernel", &dummy_kernel_launch, "Launch dummy kernel.");
  m.def("naive_spmm", &naive_spmm, "A naive implementation of Sparse Matrix Multiplication");

  m.def("tiledspmm_inspect_csr", &tiledspmm_inspect_csr, "Inspect function for TiledSpMM with CSR input");
  m.def("tiledspmm_inspect_coo", &tiledspmm_inspect_coo, "Inspect function for TiledSpMM with COO input");
  m.def("tiledspmm_mm", &tiledspmm_mm, "MM function for TiledSpMM");
  m.def("tiledspmm_clean", &tiledspmm_clean, "Cleanup function for TiledSpMM");

  m.def("cusparse_inspect", &cusparse_inspect, "Inspect function for CuSPARSE with CSR input");
  m.def("cusparse_mmul_opt", &cusparse_mmul_opt, "MM function for CuSPARSE");
  m.def("cusparse_clean", &cusparse_clean, "Cleanup function for CuSPARSE");
  m.def("cusparse_mmul_opt_t", &cusparse_mmul_opt_t, "column-major product with the cached transpose: C = A^T B");
  m.def("tiledspmm_mm_t", &tiledspmm_mm_t, "column-major product with the cached transpose: C = A^T B");
  m.def("inspect_info", &inspect_info, "what an inspector handle holds (layer, tiled)");

  // additions (not in the reference): one-launch batching and the sparse backward
  m.def("dense_to_csr", &dense_to_csr, "Device dense -> batched CSR (values, columns, offsets)");
  m.def("dense_row_offsets", &dense_row_offsets, "Device dense -> row offsets [batch, rows+1] only (no host sync)");
  m.def("dense_to_csr_fill", &dense_to_csr_fill, "(values, columns) for the offsets of dense_row_offsets");
  m.def("naive_spmm_batched", &naive_spmm_batched, "Batched CSR x dense in one launch");
  m.def("csr_transpose", &csr_transpose, "Device CSR transpose (values, columns, offsets)");
  m.def("csr_transpose_batched", &csr_transpose_batched, "Batched device CSR transpose (values, columns, offsets [batch, cols+1])");
  m.def("csr_transpose_in_lds", [](int64_t nnz, int64_t batch, int64_t rows, int64_t cols) {
          return rows <= INT32_MAX && cols <= INT32_MAX && batch <= INT32_MAX &&
                 mi_csr_transpose_batched_in_lds(nnz, (int32_t)batch, (int32_t)rows, (int32_t)cols) == 1;
        }, "does csr_transpose_batched run the one-workgroup-per-item LDS plan on this batch (cheap: transpose per backward)");
  m.def("sddmm", &sddmm, "Sampled dense-dense product on a CSR pattern");
  m.def("cublas_bmm_pair", &cublas_bmm_pair,
        "dA = dC.B and dB = dC^T.A in one launch that reads dC once; (dC, B, A, dA, dB) -> launched?");
  m.def("sddmm_batched", &sddmm_batched,
        "SDDMM on a batched CSR pattern into out[nnz]; False (nothing launched) if the LDS-resident form does not take it");
  m.def("gather_perm", &gather_perm, "values[perm] (int32 perm) as a new tensor");
  m.def("naive_spmm_batched_perm", &naive_spmm_batched_perm,
        "naive_spmm_batched with entry p's value = A_values[perm[p]]; False (nothing launched) if the plan takes no permutation");
  m.def("naive_spmm_batched_at", &naive_spmm_batched_at,
        "C[i] = A[i]^T X[i] for a batched CSR A without transposing it; False (nothing launched) if the shape is not covered");
  m.def("batched_csr_narrow", &batched_csr_narrow,
        "(int32 offsets [batch, rows+1] with the items' bases, int32 columns) of int64 crow [batch, rows+1] / col [batch, per_item]");
  m.def("naive_spmm_dense", &naive_spmm_dense,
        "A·B with A dense, zeros skipped in the kernel; False if the shape is not covered");
  m.def("naive_spmm_dense_bias", &naive_spmm_dense_bias, "as naive_spmm_dense, + bias in the epilogue");
  m.def("nonfinite_flag", &nonfinite_flag, "int32[1] device tensor: 1 if the tensor holds an inf / nan (nothing read back)");
  m.def("naive_spmm_dense_gated", &naive_spmm_dense_gated,
        "naive_spmm_dense as a launch that runs only when flag[0] != 0 on the device; (A, B, C, flag, dry_run) -> covered?");
  m.def("cublas_mmul_bias", &cublas_mmul_bias, "op(A) op(B) + bias, fused epilogue");
  m.def("cublas_mmul_splitk", &cublas_mmul_splitk, py::arg("A"), py::arg("B"), py::arg("C"), py::arg("transa"), py::arg("transb"),
        py::arg("bias") = py::none(), py::arg("splits") = 0,
        "bfloat16 / float16 op(A) op(B) (+ bias) with the deterministic split of k (splits = 0: the rule of gemm_lowp_split_count)");
  m.def("gemm_lowp_split_count", &gemm_lowp_split_count, "ranges cublas_mmul_splitk cuts k into for an m x n x k product (shape only)");
  m.def("gemm_lowp_tile_n", &gemm_lowp_tile_n,
        "(m, n, batch): 64 or 128, the width of the output tile a bfloat16 / float16 dense product launches (shape only; same bits)");
  m.def("column_sums", &column_sums, "sum over rows of a 2-d tensor (bias gradient)");
  m.def("naive_spmm_bias", &naive_spmm_bias, "CSR x dense + bias, fused epilogue");
  m.def("naive_spmm_ex", &naive_spmm_ex, "naive_spmm with the long-row rule pinned (-1 auto, 0 none, 1 split)");
  m.def("naive_spmm_bias_ex", &naive_spmm_bias_ex, "naive_spmm_bias with the long-row rule pinned (-1 auto, 0 none, 1 split)");
  m.def("spmm_plan", &spmm_plan, "(variant, kernel name, launches, splits_long_rows) of the AUTO plan");
  m.def("validate_csr", &validate_csr, "opt-in check of CSR contents (offsets monotone, columns in range); raises");
  py::class_<PySchedule, std::shared_ptr<PySchedule>>(m, "SpmmSchedule")
      .def("info", &PySchedule::info, "rows, heavy_rows, heavy_length, classes, longest_at_least, side_stream, active, locality_order, window spans, nnz, width")
      .def("set_heavy", &PySchedule::set_heavy, py::arg("heavy_length"), py::arg("side_stream") = true,
           "another heavy length / the heavy launch in line (tests, A/B)")
      .def_readonly("order", &PySchedule::order, "int32 [rows] on the device: slot -> row, rows by descending length class");
  m.def("spmm_schedule", &spmm_schedule, py::arg("A_offsets"), py::arg("nnzA"), py::arg("A_rows"), py::arg("N"),
        py::arg("A_columns") = py::none(), py::arg("A_cols") = 0,
        "Inspector: the row schedule of a CSR matrix (offsets, nnz, rows, dense width; with the columns: also tries the locality order)");
  m.def("naive_spmm_scheduled", &naive_spmm_scheduled, py::arg("schedule"), py::arg("A_values"), py::arg("A_columns"),
        py::arg("A_offsets"), py::arg("nnzA"), py::arg("A_rows"), py::arg("A_cols"), py::arg("B"), py::arg("C"),
        py::arg("bias") = py::none(), py::arg("long_rows") = -1, py::arg("variant") = 0,
        "naive_spmm on a row schedule: the same bits, rows handed to waves longest first");
  m.def("auto_schedule_stats", &auto_schedule_stats, "the automatic row schedules of the plain entry points: enabled, entries, pending, active, inactive, built");
  m.def("auto_schedule_clear", &auto_schedule_clear, "forget every automatic row schedule");
  m.def("ipc_export", &ipc_export, "(handle bytes, offset, allocation bytes) of a device buffer, for a peer process to map");
  m.def("ipc_open", &ipc_open, "a peer's exported buffer as a tensor (valid until ipc_close of the handle)");
  m.def("ipc_close", &ipc_close, "drop one open of a peer handle");
  m.def("ipc_open_count", []() { return mi_ipc_open_count(); }, "peer mappings not yet closed in this process");
  m.def("long_row_threshold", &long_row_threshold, "rows with more non-zeros are 'long' (split rule)");
  m.def("naive_spmm_reduce", &naive_spmm_reduce, py::arg("A_values"), py::arg("A_columns"), py::arg("A_offsets"),
        py::arg("nnzA"), py::arg("A_rows"), py::arg("A_cols"), py::arg("B"), py::arg("C"), py::arg("reduce"),
        py::arg("arg") = py::none(),
        "CSR x dense with reduce = sum / mean / amax / amin (torch.sparse.mm); amax / amin write the selected entries to arg");
  m.def("spmm_rows_divide", &spmm_rows_divide, "out = in / (entries of the row), per row (mean and its gradient)");
  m.def("spmm_reduce_grad_val", &spmm_reduce_grad_val, "amax / amin: gradient of A's stored values from the forward's arg");
  m.def("spmm_reduce_grad_b", &spmm_reduce_grad_b, "amax / amin: gradient of B on A^T's pattern and permutation");
  m.def("csr_softmax", &csr_softmax,
        "(values, offsets [batch, rows+1], nnz, batch, rows, scale, out): softmax over the stored entries of every CSR row");
  m.def("csr_softmax_backward", &csr_softmax_backward,
        "(y, dy, offsets, nnz, batch, rows, scale, out): out = scale * y * (dy - sum over the row of dy * y)");
  m.def("sparse_attention_fwd", &sparse_attention_fwd,
        "(offsets [batch, rows+1], columns, nnz, batch, rows, cols, q, k, v, scale, out, stats [batch*rows, 2]): "
        "out = softmax(scale * q k^T on the pattern) v in one launch");
  m.def("sparse_attention_bwd", &sparse_attention_bwd,
        "(offsets, columns, nnz, batch, rows, cols, q, k, v, dout, stats, scale, dq, y, ds): dq, and y, ds [nnz] in CSR order");
  m.def("block_attention_forward", &block_attention_forward,
        "(offsets [layouts, Sq/64+1], columns, nnz, q, k, v, scale, causal, out, lse [batch, Sq]): "
        "out = softmax(scale * q k^T + block mask) v on the matrix cores, bfloat16 / float16");
  m.def("block_attention_backward", &block_attention_backward,
        "(offsets, columns, t_offsets, t_columns, nnz, q, k, v, out, dout, lse, scale, causal, dq, dk, dv): (dq, dk, dv)");
  m.def("block_attention_forward_ex", &block_attention_forward_ex,
        "(offsets, columns, nnz, q [batch, Sq, D], k, v [batch / group, Sk, D], scale, causal, out, lse, q_lens or None, k_lens or None): "
        "block_attention_forward with grouped-query heads (query item i reads k / v item i / group) and per-item lengths (int32)");
  m.def("block_attention_backward_ex", &block_attention_backward_ex,
        "(offsets, columns, t_offsets, t_columns, nnz, q, k, v, out, dout, lse, scale, causal, dq, dk, dv, q_lens or None, "
        "k_lens or None): (dq, dk, dv); dk, dv [batch / group, Sk, D] summed over the group in one accumulator");
  m.def("block_attention_decode", &block_attention_decode,
        "(offsets [layouts, Smax/64+1], columns, nnz, q [B, Hq, T, D], k, v [B, Hkv, Smax, D] through their own strides, "
        "k_lens int32 [B] or [1], scale, chunk, out, lse [B, Hq, T]): the T newest tokens against the cache, the list cut into "
        "chunks of `chunk` entries and merged in order");
  m.def("block_attention_decode_paged", &block_attention_decode_paged,
        "(offsets [layouts, Smax/64+1], columns, nnz, q [B, Hq, T, D], k_pages, v_pages [P, Hkv, page, D] through their own strides, "
        "block_table int32 [B, W] (Smax = W * page; last stride 1, any row stride >= W), k_lens int32 [B] or [1], scale, chunk, out, "
        "lse [B, Hq, T]): block_attention_decode over a pool of pages; an entry outside [0, P) hides its page's keys");
  m.def("block_attention_decode_fp8", &block_attention_decode_fp8,
        "(offsets, columns, nnz, q [B, Hq, T, D] bfloat16 / float16, k, v [B, Hkv, Smax, D] float8_e4m3fn through their own strides "
        "(multiples of 16), k_lens, scale, k_scale, v_scale (None or float32 device tensors of 1 or Hkv entries), chunk, out, lse): "
        "block_attention_decode over an fp8 cache, every byte widened exactly in registers");
  m.def("block_attention_decode_paged_fp8", &block_attention_decode_paged_fp8,
        "(offsets, columns, nnz, q, k_pages, v_pages [P, Hkv, page, D] float8_e4m3fn, block_table int32 [B, W], k_lens, scale, "
        "k_scale, v_scale, chunk, out, lse): block_attention_decode_paged over an fp8 pool");
  m.def("block_attention_prefill", &block_attention_prefill,
        "(offsets [layouts, Smax/64+1], columns, nnz, q [B, Hq, T, D] through its own strides, k, v [B, Hkv, Smax, D] through "
        "theirs, k_lens int32 [B] or [1], new_lens None or int32 [B] or [1], scale, out, lse [B, Hq, T]): the T newest tokens "
        "against the cache in 64-row position tiles, the bits of the causal training forward placed in the cache");
  m.def("block_attention_prefill_paged", &block_attention_prefill_paged,
        "(offsets, columns, nnz, q, k_pages, v_pages [P, Hkv, page, D], block_table int32 [B, W], k_lens, new_lens, scale, out, "
        "lse): block_attention_prefill over a pool of pages; an entry outside [0, P) hides its page's keys");
  m.def("block_attention_prefill_fp8", &block_attention_prefill_fp8,
        "(offsets, columns, nnz, q, k, v [B, Hkv, Smax, D] float8_e4m3fn, k_lens, new_lens, scale, k_scale, v_scale (None or "
        "float32 device tensors of 1 or Hkv entries), out, lse): block_attention_prefill over an fp8 cache");
  m.def("block_attention_prefill_paged_fp8", &block_attention_prefill_paged_fp8,
        "(offsets, columns, nnz, q, k_pages, v_pages [P, Hkv, page, D] float8_e4m3fn, block_table, k_lens, new_lens, scale, "
        "k_scale, v_scale, out, lse): block_attention_prefill_paged over an fp8 pool");
  m.def("block_attention_prefill_split", &block_attention_prefill_split,
        "(block_attention_prefill's arguments, split): the list of a tile's layout row cut by list position into parts of `split` "
        "entries, one workgroup per (tile, query head, part), a second launch merging the parts in ascending order; the "
        "workspace of the partials comes from torch's allocator");
  m.def("block_attention_prefill_split_paged", &block_attention_prefill_split_paged,
        "(block_attention_prefill_paged's arguments, split): block_attention_prefill_split over a pool of pages");
  m.def("block_attention_prefill_split_fp8", &block_attention_prefill_split_fp8,
        "(block_attention_prefill_fp8's arguments, split): block_attention_prefill_split over an fp8 cache");
  m.def("block_attention_prefill_split_paged_fp8", &block_attention_prefill_split_paged_fp8,
        "(block_attention_prefill_paged_fp8's arguments, split): block_attention_prefill_split_paged over an fp8 pool");
  m.def("kv_append", &kv_append,
        "(k_new, v_new [B, Hkv, T, D] bfloat16 / float16 through their own strides, k, v [B, Hkv, Smax, D] of that dtype or "
        "float8_e4m3fn, k_lens int32 [B] or [1] — the lengths AFTER the append —, k_scale, v_scale (None or float32 device tensors "
        "of 1 or Hkv entries)): token t of item b written at k_lens[b] - T + t, or dropped outside [0, Smax); one launch for k and v");
  m.def("kv_append_paged", &kv_append_paged,
        "(k_new, v_new, k_pages, v_pages [P, Hkv, page, D], block_table int32 [B, W], k_lens, k_scale, v_scale): kv_append into a "
        "pool of pages; a token whose table entry lies outside [0, P) is dropped");
  m.def("kv_compact", &kv_compact,
        "(k, v [B, Hkv, Smax, D] bfloat16 / float16 / float8_e4m3fn through their own strides, k_lens int32 [B] or [1] — still "
        "counting the T drafted slots —, accept int32 [B, T], accept_counts int32 [B], T <= 64): row k_lens[b] - T + i becomes the old "
        "row k_lens[b] - T + accept[b, i] for i < accept_counts[b], every source row read before any is written; one launch for k and v");
  m.def("kv_compact_paged", &kv_compact_paged,
        "(k_pages, v_pages [P, Hkv, page, D], block_table int32 [B, W], k_lens, accept, accept_counts, T): kv_compact over a pool of "
        "pages; a row behind an entry outside [0, P) is neither read nor written");
  m.def("rope_kv_append", &rope_kv_append,
        "(q [B, Hq, T, D], k_new, v_new [B, Hkv, T, D] bfloat16 / float16 through their own strides, cos, sin float32 [Pmax, R/2], "
        "k, v [B, Hkv, Smax, D] of that dtype or float8_e4m3fn, k_lens int32 [B] or [1] — the lengths AFTER the append —, new_lens "
        "int32 [B] or None, q_out [B, Hq, T, D], k_out [B, Hkv, T, D] or None, rotary_dim R, interleaved, k_scale, v_scale): q and "
        "k_new rotated by table row k_lens[b] - T + t; rotated q to q_out, rotated k and v into the cache as kv_append writes them, "
        "in one launch; returns q_out");
  m.def("rope_kv_append_paged", &rope_kv_append_paged,
        "(q, k_new, v_new, cos, sin, k_pages, v_pages [P, Hkv, page, D], block_table int32 [B, W], k_lens, new_lens, q_out, k_out, "
        "rotary_dim, interleaved, k_scale, v_scale): rope_kv_append into a pool of pages");
  m.def("rope_kv_append_pos", &rope_kv_append_pos,
        "(rope_kv_append's arguments, positions int32 [B, T]): slot t of item b is rotated by table row positions[b, t] and still "
        "written to row k_lens[b] - T + t; a slot whose position lies outside [0, Pmax) holds no token");
  m.def("rope_kv_append_paged_pos", &rope_kv_append_paged_pos,
        "(rope_kv_append_paged's arguments, positions int32 [B, T]): rope_kv_append_pos into a pool of pages");
  m.def("kv_block_bounds", &kv_block_bounds,
        "(k [B, Hkv, Smax, D] bfloat16 / float16 through its own strides, k_lens int32 [B] or [1], last, bounds [B, Hkv, Smax/64, 2, D]): "
        "the minimum and maximum of the seen keys of every 64-key block, in place; last = 0 every block that holds a key, n >= 1 "
        "the blocks of the n newest positions; a block without a key is not written");
  m.def("kv_block_bounds_paged", &kv_block_bounds_paged,
        "(k_pages [P, Hkv, page, D], block_table int32 [B, W], k_lens, last, bounds): kv_block_bounds over a pool of pages; the "
        "keys behind an entry outside [0, P) are left out");
  m.def("block_select", &block_select,
        "(q [B, Hq, T, D] through its own strides, bounds [B, Hkv, Smax/64, 2, D], k_lens, K, sink, local, block_ids int32 "
        "[B, Hkv, T, K], block_counts int32 [B, Hkv, T], scores float32 [B, Hkv, T, Smax/64] or None): the K best candidate blocks "
        "of every token by the bounds' upper estimate of q·k, forced sink / local blocks included, in ascending block index");
  m.def("block_select_tiles", &block_select_tiles,
        "(q [B, Hq, T, D] through its own strides, bounds [B, Hkv, Smax/64, 2, D], k_lens, new_lens int32 [B] / [1] or None, K, sink, "
        "local, block_ids int32 [B, Hkv, X, K], block_counts int32 [B, Hkv, X], scores float32 [B, Hkv, X, Smax/64] or None; "
        "X = ceil(T/64) + 1): block_select per 64-position tile of a prefill chunk, scored on the matrix cores");
  m.def("block_attention_decode_lists", &block_attention_decode_lists,
        "(block_ids int32 [B, Hkv, T, K], block_counts int32 [B, Hkv, T], q [B, Hq, T, D], k, v [B, Hkv, Smax, D] through their own "
        "strides, k_lens, scale, chunk, out, lse): block_attention_decode with the list of (k / v item, token) given as a row of "
        "block_ids in the place of a layout row");
  m.def("block_attention_decode_lists_paged", &block_attention_decode_lists_paged,
        "(block_ids, block_counts, q, k_pages, v_pages [P, Hkv, page, D], block_table int32 [B, W], k_lens, scale, chunk, out, lse): "
        "block_attention_decode_lists over a pool of pages");
  m.def("block_attention_tree_decode", &block_attention_tree_decode,
        "(block_attention_decode's arguments with tree_mask int64 [B, T] or [T], T <= 64, before chunk): token t sees the draft key "
        "k_len - T + i, i < t, iff bit i of its word is set; the cached prefix and itself always");
  m.def("block_attention_tree_decode_paged", &block_attention_tree_decode_paged,
        "(block_attention_decode_paged's arguments with tree_mask before chunk): block_attention_tree_decode over a pool of pages");
  m.def("block_attention_tree_decode_fp8", &block_attention_tree_decode_fp8,
        "(block_attention_decode_fp8's arguments with tree_mask before chunk): block_attention_tree_decode over an fp8 cache");
  m.def("block_attention_tree_decode_paged_fp8", &block_attention_tree_decode_paged_fp8,
        "(block_attention_decode_paged_fp8's arguments with tree_mask before chunk): block_attention_tree_decode over an fp8 pool");
  m.def("block_attention_tree_decode_lists", &block_attention_tree_decode_lists,
        "(block_attention_decode_lists' arguments with tree_mask int64 [B, T] or [T], T <= 64, before chunk): the tree rule over the "
        "caller's lists");
  m.def("block_attention_tree_decode_lists_paged", &block_attention_tree_decode_lists_paged,
        "(block_attention_decode_lists_paged's arguments with tree_mask before chunk)");
  m.def("block_attention_tree_lists_decode_fp8", &block_attention_tree_lists_decode_fp8,
        "(block_attention_lists_decode_fp8's arguments with tree_mask before chunk)");
  m.def("block_attention_tree_lists_decode_paged_fp8", &block_attention_tree_lists_decode_paged_fp8,
        "(block_attention_lists_decode_paged_fp8's arguments with tree_mask before chunk)");
  m.def("block_attention_window_decode", &block_attention_window_decode,
        "(block_attention_decode's arguments with window >= 1 and sink >= 0, ints, before chunk): the token at pos sees key j iff the "
        "plain rule holds and (j > pos - window or j < sink); the window counts the token itself");
  m.def("block_attention_window_decode_paged", &block_attention_window_decode_paged,
        "(block_attention_decode_paged's arguments with window, sink before chunk): block_attention_window_decode over a pool of pages");
  m.def("block_attention_window_decode_fp8", &block_attention_window_decode_fp8,
        "(block_attention_decode_fp8's arguments with window, sink before chunk): block_attention_window_decode over an fp8 cache");
  m.def("block_attention_window_decode_paged_fp8", &block_attention_window_decode_paged_fp8,
        "(block_attention_decode_paged_fp8's arguments with window, sink before chunk): block_attention_window_decode over an fp8 pool");
  m.def("block_attention_window_decode_lists", &block_attention_window_decode_lists,
        "(block_attention_decode_lists' arguments with window, sink before chunk): the window rule over the caller's lists");
  m.def("block_attention_window_decode_lists_paged", &block_attention_window_decode_lists_paged,
        "(block_attention_decode_lists_paged's arguments with window, sink before chunk)");
  m.def("block_attention_window_lists_decode_fp8", &block_attention_window_lists_decode_fp8,
        "(block_attention_lists_decode_fp8's arguments with window, sink before chunk)");
  m.def("block_attention_window_lists_decode_paged_fp8", &block_attention_window_lists_decode_paged_fp8,
        "(block_attention_lists_decode_paged_fp8's arguments with window, sink before chunk)");
  m.def("kv_block_bounds_fp8", &kv_block_bounds_fp8,
        "(k [B, Hkv, Smax, D] float8_e4m3fn through its own strides (multiples of 16 bytes), k_lens, last, bounds [B, Hkv, Smax/64, 2, D] "
        "bfloat16 / float16): kv_block_bounds over an fp8 cache — the bits of kv_block_bounds on the cache widened to bounds' dtype");
  m.def("kv_block_bounds_paged_fp8", &kv_block_bounds_paged_fp8,
        "(k_pages [P, Hkv, page, D] float8_e4m3fn, block_table int32 [B, W], k_lens, last, bounds): kv_block_bounds_fp8 over a pool of "
        "pages");
  m.def("block_attention_lists_decode_fp8", &block_attention_lists_decode_fp8,
        "(block_ids, block_counts, q, k, v [B, Hkv, Smax, D] float8_e4m3fn, k_lens, scale, k_scale, v_scale (None or float32 device "
        "tensors of 1 or Hkv entries), chunk, out, lse): block_attention_decode_lists over an fp8 cache");
  m.def("block_attention_lists_decode_paged_fp8", &block_attention_lists_decode_paged_fp8,
        "(block_ids, block_counts, q, k_pages, v_pages [P, Hkv, page, D] float8_e4m3fn, block_table int32 [B, W], k_lens, scale, k_scale, "
        "v_scale, chunk, out, lse): block_attention_lists_decode_fp8 over a pool of pages");
  m.def("block_attention_lists_prefill", &block_attention_prefill_lists,
        "(block_ids int32 [B, Hkv, ceil(T/64) + 1, K], block_counts int32 [B, Hkv, ceil(T/64) + 1], q [B, Hq, T, D], k, v "
        "[B, Hkv, Smax, D] through their own strides, k_lens, new_lens int32 [B] / [1] or None, scale, out, lse): "
        "block_attention_prefill with the list of (k / v item, position tile) given as a row of block_ids in the place of a layout row");
  m.def("block_attention_lists_prefill_paged", &block_attention_prefill_lists_paged,
        "(block_ids, block_counts, q, k_pages, v_pages [P, Hkv, page, D], block_table int32 [B, W], k_lens, new_lens, scale, out, lse): "
        "block_attention_lists_prefill over a pool of pages");
  m.def("block_attention_lists_prefill_fp8", &block_attention_prefill_lists_fp8,
        "(block_ids, block_counts, q, k, v [B, Hkv, Smax, D] float8_e4m3fn, k_lens, new_lens, scale, k_scale, v_scale (None or float32 "
        "device tensors of 1 or Hkv entries), out, lse): block_attention_lists_prefill over an fp8 cache");
  m.def("block_attention_lists_prefill_paged_fp8", &block_attention_prefill_lists_paged_fp8,
        "(block_ids, block_counts, q, k_pages, v_pages [P, Hkv, page, D] float8_e4m3fn, block_table int32 [B, W], k_lens, new_lens, scale, "
        "k_scale, v_scale, out, lse): block_attention_lists_prefill_fp8 over a pool of pages");
  m.def("block_attention_window_prefill", &block_attention_window_prefill,
        "(block_attention_prefill's arguments with window >= 1 and sink >= 0, ints, before out): the token at pos sees key j iff the "
        "plain rule holds and (j > pos - window or j < sink); the window counts the token itself");
  m.def("block_attention_window_prefill_paged", &block_attention_window_prefill_paged,
        "(block_attention_prefill_paged's arguments with window, sink before out)");
  m.def("block_attention_window_prefill_fp8", &block_attention_window_prefill_fp8,
        "(block_attention_prefill_fp8's arguments with window, sink before out)");
  m.def("block_attention_window_prefill_paged_fp8", &block_attention_window_prefill_paged_fp8,
        "(block_attention_prefill_paged_fp8's arguments with window, sink before out)");
  m.def("block_attention_window_lists_prefill", &block_attention_window_prefill_lists,
        "(block_attention_lists_prefill's arguments with window, sink before out): the window rule over the caller's lists");
  m.def("block_attention_window_lists_prefill_paged", &block_attention_window_prefill_lists_paged,
        "(block_attention_lists_prefill_paged's arguments with window, sink before out)");
  m.def("block_attention_window_lists_prefill_fp8", &block_attention_window_prefill_lists_fp8,
        "(block_attention_lists_prefill_fp8's arguments with window, sink before out)");
  m.def("block_attention_window_lists_prefill_paged_fp8", &block_attention_window_prefill_lists_paged_fp8,
        "(block_attention_lists_prefill_paged_fp8's arguments with window, sink before out)");
  m.def("bsr_mm", &bsr_mm,
        "(offsets [rows/64+1], columns, entry_ids or None, nnz, values [n, 64, 64], B [batch, inner, N], C [batch, rows, N], trans_a): "
        "C = op(A) B with A in 64 x 64 blocks on the matrix cores, bfloat16 / float16");
  m.def("bsr_sddmm", &bsr_sddmm,
        "(entry_row, columns, entry_ids or None, nnz, dC [batch, M, N], B [batch, K, N], dvalues [n, 64, 64]): "
        "dvalues[e] = sum over the items of dC[I-rows] B[J-rows]^T on the kept blocks");
  m.def("bsr_linear", &bsr_linear,
        "(offsets [outer/64+1], columns, entry_ids or None, nnz, values [n, 64, 64], X [T, inner], bias [outer] or None, Y [T, outer], "
        "trans_w): Y = X op(W)^T (+ bias) with W in 64 x 64 blocks on the matrix cores, bfloat16 / float16");
  m.def("bsr_wgrad", &bsr_wgrad, py::arg("entry_row"), py::arg("columns"), py::arg("entry_ids"), py::arg("nnz"), py::arg("dY"),
        py::arg("X"), py::arg("dvalues"), py::arg("splits") = 0,
        "dvalues[e] = dY[:, O-columns]^T X[:, I-columns] on the kept blocks, the tokens cut into `splits` ranges (0: the rule)");
  m.def("bsr_wgrad_split_count", &bsr_wgrad_split_count, "ranges bsr_wgrad cuts the tokens into for (kept blocks, tokens)");
  m.def("bsr_mm_tile_n", &bsr_mm_tile_n, "(rows, N, batch): 64 or 128, the column tile bsr_mm launches (shape only; same bits)");
  m.def("bsr_linear_tile_tokens", &bsr_linear_tile_tokens,
        "(outer, tokens): 64 or 128, the token tile bsr_linear launches (shape only; same bits)");
  // Handles and automatic schedules own HIP streams and events: they are released while the interpreter — and with it the HIP
  // runtime — is still up (left to the destructors of the statics they segfaulted at process exit after the runtime had gone:
  // a program that never called cusparse_clean / auto_schedule_clear ended with exit code 139 AFTER its last line of output).
  py::module_::import("atexit").attr("register")(py::cpp_function([]() {
    auto_schedule_clear();
    std::lock_guard<std::mutex> lock(g_registry_mutex);
    g_cusparse_layers.clear();
    g_tiled_layers.clear();
  }));
}
