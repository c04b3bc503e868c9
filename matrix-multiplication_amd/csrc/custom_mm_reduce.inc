// custom_mm — CSR × dense with reduce = sum / mean / amax / amin (torch.sparse.mm's `reduce`) and the gradients of amax / amin
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace (one translation unit; the
// split is for readers).  Not compiled on its own.  Contract: include/mi_spmm.h, mi_spmm_csr_reduce_f32 and its bfloat16 / float16
// twins: every entry takes float32 operands, or all of its value operands in bfloat16 or all in float16.

int reduce_code(const std::string& reduce, const char* what) {
  if (reduce == "sum") return MI_REDUCE_SUM;
  if (reduce == "mean") return MI_REDUCE_MEAN;
  if (reduce == "amax") return MI_REDUCE_AMAX;
  if (reduce == "amin") return MI_REDUCE_AMIN;
  throw std::invalid_argument(std::string(what) + ": reduce must be one of sum, mean, amax, amin; got '" + reduce + "'");
}

// C = A ⊙_reduce B.  sum: exactly naive_spmm; mean: naive_spmm, then each row divided by its count in place (bfloat16 /
// float16: the division is the sum kernels' epilogue, before the one rounding); amax / amin: the selection kernels, the
// selected entry indices into `arg` (int32 [A_rows, N]) when it is given.
torch::Tensor naive_spmm_reduce(torch::Tensor A_values, torch::Tensor A_columns, torch::Tensor A_offsets, int64_t nnzA,
                                int64_t A_rows, int64_t A_cols, torch::Tensor B, torch::Tensor C, const std::string& reduce,
                                c10::optional<torch::Tensor> arg) {
  const char* what = "naive_spmm_reduce";
  const int code = reduce_code(reduce, what);
  const bool selects = code == MI_REDUCE_AMAX || code == MI_REDUCE_AMIN;
  TORCH_CHECK(!(arg.has_value() && arg->defined()) || selects, what, ": arg is only defined for amax / amin");
  TORCH_CHECK(nnzA < (int64_t)1 << 31, what, ": nnzA does not fit int32 indices");
  const bool lowp_mean = code == MI_REDUCE_MEAN && is_lowp(A_values.scalar_type());
  if (!selects && !lowp_mean) {
    spmm_impl(A_values, A_columns, A_offsets, nnzA, A_rows, A_cols, B, C, what, nullptr, MI_LONG_ROWS_AUTO, nullptr,
              MI_SPMM_AUTO, true, true);
    if (code == MI_REDUCE_MEAN && C.numel() > 0) {
      c10::hip::HIPGuard guard(C.device().index());
      check_status(mi_spmm_rows_divide_f32(A_offsets.data_ptr<int32_t>(), (int32_t)A_rows, (int32_t)C.size(1),
                                           C.data_ptr<float>(), C.size(1), C.data_ptr<float>(), C.size(1), stream_of(C)),
                   what);
    }
    return C;
  }
  const torch::ScalarType dt = value_dtype(what, {{"A_values", &A_values}, {"B", &B}, {"C", &C}}, true);
  const Csr a = csr_arrays(what, &A_values, &A_columns, A_offsets, nnzA, A_rows, A_cols);
  check_same_device(what, a.device, {&B, &C});
  TORCH_CHECK(B.dim() == 2 && C.dim() == 2 && B.size(0) == A_cols && C.size(0) == A_rows && C.size(1) == B.size(1), what,
              ": B must be [A_cols, N] and C [A_rows, N]");
  TORCH_CHECK(C.is_contiguous(), what, ": C must be contiguous");
  const int64_t N = B.size(1);
  check_sizes(what, {N});
  int32_t* arg_ptr = nullptr;
  if (arg.has_value() && arg->defined()) {
    check_device_i32(*arg, "arg");
    check_same_device(what, C.device(), {&*arg});
    TORCH_CHECK(arg->dim() == 2 && arg->size(0) == A_rows && arg->size(1) == N && arg->is_contiguous(), what,
                ": arg must be a contiguous int32 [A_rows, N]");
    arg_ptr = arg->data_ptr<int32_t>();
  }
  c10::hip::HIPGuard guard(C.device().index());
  // the hub-row list and partial rows (a fresh block of the caching allocator: capturable; the entry zeroes its header)
  torch::Tensor ws;
  if (nnzA > mi_spmm_long_row_threshold() && N > 0)
    ws = byte_workspace(C.device(), mi_spmm_csr_reduce_workspace_bytes(nnzA, (int32_t)N));
  void* const ws_ptr = ws.defined() ? ws.data_ptr() : nullptr;
  const size_t ws_size = ws.defined() ? (size_t)ws.numel() : 0;
  if (is_lowp(dt)) {  // B as it is where it is row-major (column-offset views, odd leading dimensions: the 2-byte element forms)
    const RowMajorB b = row_major_b(B);
    check_status((dt == torch::kBFloat16 ? mi_spmm_csr_reduce_bf16 : mi_spmm_csr_reduce_f16)(
                     a.offsets, a.columns, a.b16(), nnzA, a.rows, a.cols, (int32_t)N, b16_or_null(b.keep), b.ld,
                     static_cast<uint16_t*>(C.data_ptr()), ld1(N), arg_ptr, ld1(N), code, ws_ptr, ws_size, stream_of(C)),
                 what);
    return C;
  }
  torch::Tensor Bc = B.contiguous();
  check_status(mi_spmm_csr_reduce_f32(a.offsets, a.columns, a.f32(), nnzA, a.rows, a.cols, (int32_t)N, Bc.data_ptr<float>(),
                                      ld1(N), C.data_ptr<float>(), ld1(N), arg_ptr, ld1(N), code, ws_ptr, ws_size, stream_of(C)),
               what);
  return C;
}

// out = in / count(row) per row (rows without entries copied); out may be in.
torch::Tensor spmm_rows_divide(torch::Tensor A_offsets, int64_t A_rows, torch::Tensor in, torch::Tensor out) {
  const char* what = "spmm_rows_divide";
  const torch::ScalarType dt = value_dtype(what, {{"in", &in}, {"out", &out}}, true);
  const Csr a = csr_arrays(what, nullptr, nullptr, A_offsets, 0, A_rows, 0);
  check_same_device(what, a.device, {&in, &out});
  TORCH_CHECK(in.dim() == 2 && in.size(0) == A_rows && out.sizes() == in.sizes(), what, ": in and out must be [A_rows, N]");
  TORCH_CHECK(in.is_contiguous() && out.is_contiguous(), what, ": in and out must be contiguous");
  const int64_t N = in.size(1);
  check_sizes(what, {N});
  c10::hip::HIPGuard guard(out.device().index());
  if (is_lowp(dt))
    check_status((dt == torch::kBFloat16 ? mi_spmm_rows_divide_bf16 : mi_spmm_rows_divide_f16)(
                     a.offsets, a.rows, (int32_t)N, static_cast<const uint16_t*>(in.data_ptr()), ld1(N),
                     static_cast<uint16_t*>(out.data_ptr()), ld1(N), stream_of(out)),
                 what);
  else
    check_status(mi_spmm_rows_divide_f32(a.offsets, a.rows, (int32_t)N, in.data_ptr<float>(), ld1(N), out.data_ptr<float>(),
                                         ld1(N), stream_of(out)),
                 what);
  return out;
}

// grad of the stored values for amax / amin: [nnzA], entry e gets Σ_j [arg[i, j] == e] G[i, j] B[col[e], j]
torch::Tensor spmm_reduce_grad_val(torch::Tensor A_columns, torch::Tensor A_offsets, int64_t nnzA, int64_t A_rows,
                                   int64_t A_cols, torch::Tensor B, torch::Tensor G, torch::Tensor arg) {
  const char* what = "spmm_reduce_grad_val";
  const torch::ScalarType dt = value_dtype(what, {{"B", &B}, {"G", &G}}, true);
  const Csr a = csr_arrays(what, nullptr, &A_columns, A_offsets, nnzA, A_rows, A_cols);
  check_device_i32(arg, "arg");
  check_same_device(what, a.device, {&B, &G, &arg});
  TORCH_CHECK(G.dim() == 2 && B.dim() == 2 && G.size(0) == A_rows && B.size(0) == A_cols && G.size(1) == B.size(1) &&
                  arg.sizes() == G.sizes() && arg.is_contiguous(),
              what, ": G and arg must be [A_rows, N] and B [A_cols, N]");
  const int64_t N = B.size(1);
  check_sizes(what, {N});
  torch::Tensor Gc = G.contiguous(), Bc = B.contiguous();
  c10::hip::HIPGuard guard(G.device().index());
  torch::Tensor out = torch::empty({nnzA}, Gc.options());
  if (is_lowp(dt))
    check_status((dt == torch::kBFloat16 ? mi_spmm_reduce_grad_val_bf16 : mi_spmm_reduce_grad_val_f16)(
                     a.offsets, a.columns, nnzA, a.rows, a.cols, (int32_t)N, b16_or_null(Bc), ld1(N), b16_or_null(Gc), ld1(N),
                     arg.data_ptr<int32_t>(), ld1(N), static_cast<uint16_t*>(out.data_ptr()), stream_of(Gc)),
                 what);
  else
    check_status(mi_spmm_reduce_grad_val_f32(a.offsets, a.columns, nnzA, a.rows, a.cols, (int32_t)N, Bc.data_ptr<float>(),
                                             ld1(N), Gc.data_ptr<float>(), ld1(N), arg.data_ptr<int32_t>(), ld1(N),
                                             out.data_ptr<float>(), stream_of(Gc)),
                 what);
  return out;
}

// grad of B for amax / amin: [A_cols, N] over the rows of Aᵀ (t_offsets [A_cols+1], t_columns = rows of A, perm = entry of
// Aᵀ → index in A)
torch::Tensor spmm_reduce_grad_b(torch::Tensor t_offsets, torch::Tensor t_columns, torch::Tensor perm, torch::Tensor A_values,
                                 int64_t nnzA, int64_t A_rows, int64_t A_cols, torch::Tensor G, torch::Tensor arg) {
  const char* what = "spmm_reduce_grad_b";
  const torch::ScalarType dt = value_dtype(what, {{"A_values", &A_values}, {"G", &G}}, true);
  // the CSR of Aᵀ (A_cols × A_rows) with A's values read through perm
  const Csr t = csr_arrays(what, &A_values, &t_columns, t_offsets, nnzA, A_cols, A_rows, c10::nullopt, &perm,
                           {"A_values", "t_columns", "t_offsets"});
  check_device_i32(arg, "arg");
  check_same_device(what, t.device, {&G, &arg});
  TORCH_CHECK(G.dim() == 2 && G.size(0) == A_rows && arg.sizes() == G.sizes() && arg.is_contiguous(), what,
              ": G and arg must be [A_rows, N]");
  const int64_t N = G.size(1);
  check_sizes(what, {N});
  torch::Tensor Gc = G.contiguous();
  c10::hip::HIPGuard guard(G.device().index());
  torch::Tensor out = torch::empty({A_cols, N}, Gc.options());
  if (is_lowp(dt))
    check_status((dt == torch::kBFloat16 ? mi_spmm_reduce_grad_b_bf16 : mi_spmm_reduce_grad_b_f16)(
                     t.offsets, t.columns, t.perm, t.b16(), nnzA, t.cols, t.rows, (int32_t)N, b16_or_null(Gc), ld1(N),
                     arg.data_ptr<int32_t>(), ld1(N), static_cast<uint16_t*>(out.data_ptr()), ld1(N), stream_of(Gc)),
                 what);
  else
    check_status(mi_spmm_reduce_grad_b_f32(t.offsets, t.columns, t.perm, t.f32(), nnzA, t.cols, t.rows, (int32_t)N,
                                           Gc.data_ptr<float>(), ld1(N), arg.data_ptr<int32_t>(), ld1(N), out.data_ptr<float>(),
                                           ld1(N), stream_of(Gc)),
                 what);
  return out;
}
