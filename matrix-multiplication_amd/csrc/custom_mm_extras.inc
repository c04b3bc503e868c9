// custom_mm — additions to the reference surface used by matmuls.py / fc_layers.py: batched CSR, conversions, transpose, SDDMM, dense-skip, fused pair
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace (one translation unit; the
// split is for readers).  Not compiled on its own.
// ---- additions to the reference surface (used by matmuls.py) -----------------
// The reference batches by Python recursion + torch.stack with one
// to_sparse_csr() per slice (matmuls.py:289-297) and has no working backward
// (SURVEY.md §8a defects 1-2); these four entry points give matmuls.py the
// one-launch batched forward and the sparse backward.  They are extra names:
// the 16 reference names keep their exact signatures.

// dense [..., rows, cols] → (values f32[nnz], columns i32[nnz], offsets i32[batch, rows+1]);
// offsets are global over the batch ("rowptr of rowptrs", include/mi_spmm.h).
// Device counterpart of dense_to_csr (reference src/baseline_mm.cu:218-264).
// Step 1 alone: the row offsets [batch, rows+1] (global over the batch; the last entry is the total
// nnz) — no host read-back, so a caller can look at the density before paying for the fill.
torch::Tensor dense_row_offsets(torch::Tensor dense) {
  check_device_f32(dense, "dense");
  TORCH_CHECK(dense.dim() >= 2, "dense_to_csr: expected at least a 2-d tensor");
  torch::Tensor d = dense.contiguous();
  const int64_t rows = d.size(-2), cols = d.size(-1);
  const int64_t batch = rows * cols > 0 ? d.numel() / (rows * cols) : [&] {
    int64_t b = 1;
    for (int64_t i = 0; i + 2 < d.dim(); ++i) b *= d.size(i);
    return b;
  }();
  TORCH_CHECK(rows <= INT32_MAX && cols <= INT32_MAX && batch <= INT32_MAX, "dense_to_csr: dimension too large");
  TORCH_CHECK(d.numel() <= INT32_MAX, "dense_to_csr: more than 2^31-1 elements cannot be indexed by int32 offsets");
  c10::hip::HIPGuard guard(d.device().index());
  auto iopt = torch::dtype(torch::kInt32).device(d.device());
  torch::Tensor offsets = torch::empty({batch, rows + 1}, iopt);
  const size_t ws_bytes = mi_dense_to_csr_workspace_bytes((int32_t)batch, (int32_t)rows);
  torch::Tensor ws = byte_workspace(d.device(), ws_bytes, 1);
  check_status(mi_dense_to_csr_count(d.data_ptr<float>(), (int32_t)batch, (int32_t)rows, (int32_t)cols, cols,
                                     rows * cols, offsets.data_ptr<int32_t>(), ws.data_ptr(), ws_bytes,
                                     stream_of(d)),
               "dense_to_csr(count)");
  return offsets;
}

// Step 2: (values, columns) for offsets produced by dense_row_offsets on the same tensor; nnz is
// the caller's host copy of offsets[-1, -1].
std::tuple<torch::Tensor, torch::Tensor> dense_to_csr_fill(torch::Tensor dense, torch::Tensor offsets, int64_t nnz) {
  check_device_f32(dense, "dense");
  check_device_i32(offsets, "offsets");
  check_same_device("dense_to_csr_fill", dense.device(), {&offsets});
  TORCH_CHECK(dense.dim() >= 2 && nnz >= 0 && nnz <= dense.numel(), "dense_to_csr_fill: bad arguments");
  torch::Tensor d = dense.contiguous();
  const int64_t rows = d.size(-2), cols = d.size(-1);
  const int64_t batch = rows * cols > 0 ? d.numel() / (rows * cols) : 0;
  TORCH_CHECK(offsets.is_contiguous() && offsets.numel() == batch * (rows + 1) || nnz == 0,
              "dense_to_csr_fill: offsets must be the [batch, rows + 1] tensor of dense_row_offsets");
  c10::hip::HIPGuard guard(d.device().index());
  torch::Tensor columns = torch::empty({nnz}, torch::dtype(torch::kInt32).device(d.device()));
  torch::Tensor values = torch::empty({nnz}, torch::dtype(torch::kFloat32).device(d.device()));
  if (nnz > 0)
    check_status(mi_dense_to_csr_fill(d.data_ptr<float>(), (int32_t)batch, (int32_t)rows, (int32_t)cols, cols,
                                      rows * cols, offsets.data_ptr<int32_t>(), columns.data_ptr<int32_t>(),
                                      values.data_ptr<float>(), stream_of(d)),
                 "dense_to_csr(fill)");
  return std::make_tuple(values, columns);
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> dense_to_csr(torch::Tensor dense) {
  torch::Tensor offsets = dense_row_offsets(dense);
  // one host read-back per call (not per slice) to size col / val
  const int64_t nnz = offsets.numel() > 0 ? offsets.view({-1})[offsets.numel() - 1].item<int32_t>() : 0;
  auto vc = dense_to_csr_fill(dense, offsets, nnz);
  return std::make_tuple(std::get<0>(vc), std::get<1>(vc), offsets);
}

// C[b] = A[b]·B[b] for a batched CSR (offsets [batch, A_rows+1], global) in one
// launch; B is [batch, K, N] or [K, N] (shared by every item), C is [batch, M, N].
torch::Tensor naive_spmm_batched(torch::Tensor A_values, torch::Tensor A_columns, torch::Tensor A_offsets,
                                 int64_t nnzA, int64_t batch, int64_t A_rows, int64_t A_cols,
                                 torch::Tensor B, torch::Tensor C) {
  const char* what = "naive_spmm_batched";
  value_dtype(what, {{"A_values", &A_values}, {"B", &B}, {"C", &C}});
  const Csr a = csr_arrays(what, &A_values, &A_columns, A_offsets, nnzA, A_rows, A_cols, batch);
  check_same_device(what, a.device, {&B, &C});
  TORCH_CHECK(batch <= 65535, what, ": at most 65535 items per launch");
  TORCH_CHECK(C.dim() == 3 && C.is_contiguous() && C.size(0) == batch && C.size(1) == A_rows, what,
              ": C must be contiguous [batch, A_rows, N]");
  const int64_t N = C.size(2);
  check_sizes(what, {N});
  const auto b = batched_b(what, B, batch, A_cols, N);
  c10::hip::HIPGuard guard(C.device().index());
  check_status(mi_spmm_csr_batched_f32(a.offsets, a.columns, a.f32(), nnzA, a.batch, a.rows, a.cols, (int32_t)N,
                                       b.first.data_ptr<float>(), ld1(N), b.second, C.data_ptr<float>(), ld1(N), A_rows * N,
                                       stream_of(C)),
               what);
  return C;
}

// naive_spmm_batched with the values read through a permutation (entry p has the value A_values[perm[p]]): the
// transposed pattern of a batched CSR tensor in a backward, without a gathered copy of the values.  Returns false
// (nothing launched) when the plan for the problem does not take a permutation: gather and call naive_spmm_batched.
bool naive_spmm_batched_perm(torch::Tensor A_values, torch::Tensor perm, torch::Tensor A_columns, torch::Tensor A_offsets,
                             int64_t nnzA, int64_t batch, int64_t A_rows, int64_t A_cols, torch::Tensor B,
                             torch::Tensor C) {
  const char* what = "naive_spmm_batched_perm";
  value_dtype(what, {{"A_values", &A_values}, {"B", &B}, {"C", &C}});
  const Csr a = csr_arrays(what, &A_values, &A_columns, A_offsets, nnzA, A_rows, A_cols, batch, &perm);
  check_same_device(what, a.device, {&B, &C});
  TORCH_CHECK(batch <= 65535, what, ": at most 65535 items per launch");
  TORCH_CHECK(C.dim() == 3 && C.is_contiguous() && C.size(0) == batch && C.size(1) == A_rows, what,
              ": C must be contiguous [batch, A_rows, N]");
  const int64_t N = C.size(2);
  check_sizes(what, {N});
  const auto b = batched_b(what, B, batch, A_cols, N);
  c10::hip::HIPGuard guard(C.device().index());
  const int st = mi_spmm_csr_batched_perm_f32(a.offsets, a.columns, a.f32(), a.perm, nnzA, a.batch, a.rows, a.cols, (int32_t)N,
                                              b.first.data_ptr<float>(), ld1(N), b.second, C.data_ptr<float>(), ld1(N),
                                              A_rows * N, stream_of(C));
  if (st == 1) return false;
  check_status(st, what);
  return true;
}

// C[i] (A_cols × N) = A[i]ᵀ · X[i] for a batched CSR A [batch, A_rows, A_cols] (offsets with base, as naive_spmm_batched)
// and X [batch, A_rows, N] — no transpose of A is built (mi_spmm_csr_batched_at_f32).  Returns false (nothing launched)
// when the shape is not covered (N > 64): transpose and call naive_spmm_batched.
bool naive_spmm_batched_at(torch::Tensor A_values, torch::Tensor A_columns, torch::Tensor A_offsets, int64_t nnzA,
                           int64_t batch, int64_t A_rows, int64_t A_cols, torch::Tensor X, torch::Tensor C) {
  const char* what = "naive_spmm_batched_at";
  value_dtype(what, {{"A_values", &A_values}, {"X", &X}, {"C", &C}});
  const Csr a = csr_arrays(what, &A_values, &A_columns, A_offsets, nnzA, A_rows, A_cols, batch);
  check_same_device(what, a.device, {&X, &C});
  TORCH_CHECK(C.dim() == 3 && C.is_contiguous() && C.size(0) == batch && C.size(1) == A_cols, what,
              ": C must be contiguous [batch, A_cols, N]");
  const int64_t N = C.size(2);
  check_sizes(what, {N});
  TORCH_CHECK(X.dim() == 3 && X.size(0) == batch && X.size(1) == A_rows && X.size(2) == N, what, ": X must be [batch, A_rows, N]");
  torch::Tensor Xc = X.contiguous();
  c10::hip::HIPGuard guard(C.device().index());
  const int st = mi_spmm_csr_batched_at_f32(a.offsets, a.columns, a.f32(), nnzA, a.batch, a.rows, a.cols, (int32_t)N,
                                            Xc.data_ptr<float>(), ld1(N), A_rows * N, C.data_ptr<float>(), ld1(N), A_cols * N,
                                            stream_of(C));
  if (st == 1) return false;
  check_status(st, what);
  return true;
}

// (offsets int32 [batch, rows + 1] with the items' bases added, columns int32 [batch · per_item]) of a batched torch CSR
// tensor's int64 index tensors crow [batch, rows + 1] / col [batch, per_item], in one launch (mi_batched_csr_narrow_i64).
std::tuple<torch::Tensor, torch::Tensor> batched_csr_narrow(torch::Tensor crow, torch::Tensor col) {
  const char* what = "batched_csr_narrow";
  TORCH_CHECK(crow.is_cuda() && col.is_cuda() && crow.scalar_type() == torch::kInt64 && col.scalar_type() == torch::kInt64,
              what, ": int64 device tensors expected");
  TORCH_CHECK(crow.dim() == 2 && col.dim() == 2 && crow.size(0) == col.size(0) && crow.size(1) >= 1, what,
              ": crow [batch, rows + 1] and col [batch, per_item] expected");
  TORCH_CHECK(crow.is_contiguous() && col.is_contiguous(), what, ": contiguous index tensors expected");
  check_same_device(what, crow.device(), {&col});
  const int64_t batch = crow.size(0), rows = crow.size(1) - 1, per_item = col.size(1);
  TORCH_CHECK(batch <= INT32_MAX && rows <= INT32_MAX && batch * per_item <= INT32_MAX, what, ": too large for int32 indices");
  c10::hip::HIPGuard guard(crow.device().index());
  torch::Tensor off = torch::empty({batch, rows + 1}, torch::dtype(torch::kInt32).device(crow.device()));
  torch::Tensor c32 = torch::empty({batch * per_item}, torch::dtype(torch::kInt32).device(crow.device()));
  check_status(mi_batched_csr_narrow_i64(crow.data_ptr<int64_t>(), col.data_ptr<int64_t>(), (int32_t)batch, (int32_t)rows, per_item,
                                         off.data_ptr<int32_t>(), c32.data_ptr<int32_t>(), stream_of(off)), what);
  return std::make_tuple(off, c32);
}

// C[b] = A[b]·B[b] (+ bias) with A DENSE [batch…, M, K]: exact zeros are skipped inside the
// kernel (no CSR is built).  B is [batch…, K, N] or [K, N] (shared), C [batch…, M, N].
// Returns false (and does nothing) when the fused kernel does not cover the shape, so the
// caller can take the dense_to_csr + naive_spmm_batched route instead.
bool spmm_dense_impl(const torch::Tensor& A, const torch::Tensor& B, const torch::Tensor* bias, torch::Tensor C,
                     const char* what) {
  value_dtype(what, {{"A", &A}, {"B", &B}, {"C", &C}});
  check_same_device(what, C.device(), {&A, &B});
  TORCH_CHECK(A.dim() >= 2 && C.dim() == A.dim(), what, ": A and C must have the same rank (>= 2)");
  TORCH_CHECK(C.is_contiguous(), what, ": C must be contiguous");
  torch::Tensor Ac = A.contiguous(), Bc = B.contiguous();
  const int64_t M = Ac.size(-2), K = Ac.size(-1), N = C.size(-1);
  const int64_t batch = M * K > 0 ? Ac.numel() / (M * K) : (C.numel() / std::max<int64_t>(C.size(-2) * N, 1));
  TORCH_CHECK(C.size(-2) == M, what, ": C must have ", M, " rows");
  int64_t strideB = 0;
  if (Bc.dim() == 2) {
    TORCH_CHECK(Bc.size(0) == K && Bc.size(1) == N, what, ": B must be [", K, ", ", N, "]");
  } else {
    TORCH_CHECK(Bc.dim() == Ac.dim() && Bc.size(-2) == K && Bc.size(-1) == N && Bc.numel() == batch * K * N, what,
                ": B must be [batch…, ", K, ", ", N, "] with A's batch dims");
    strideB = K * N;
  }
  TORCH_CHECK(C.numel() == batch * M * N, what, ": C must be [batch…, ", M, ", ", N, "]");
  check_sizes(what, {M, K, N, batch});
  const torch::Tensor bias_keep = bias_of(what, bias, N, C);
  const float* bias_ptr = f32_or_null(bias_keep);
  if (batch == 0 || M == 0 || N == 0) return true;
  // The kernel covers up to 256 columns; wider products (up to 1024 columns) run as column tiles of
  // 256 — every column of C is its own chain, so the bits are the same — at the price of scanning A once
  // per tile.  That keeps them free of the CSR route's host read-back (nnz sizes the CSR arrays), i.e.
  // stream-ordered and graph-capturable; beyond 1024 columns the L2-blocked CSR plans are the better tool.
  constexpr int64_t kTile = 256, kMaxN = 1024;
  if (N > kMaxN || N % 4 != 0 || (M * N) % 4 != 0 || (bias_ptr && (reinterpret_cast<uintptr_t>(bias_ptr) & 15u)))
    return false;
  for (int64_t n0 = 0; n0 < N; n0 += kTile)
    if (!mi_spmm_dense_skip_supported((int32_t)std::min(kTile, N - n0), K, N, N, Ac.data_ptr<float>(),
                                      Bc.data_ptr<float>() + n0, C.data_ptr<float>() + n0))
      return false;
  c10::hip::HIPGuard guard(C.device().index());
  for (int64_t n0 = 0; n0 < N; n0 += kTile)
    check_status(mi_spmm_dense_skip_f32(Ac.data_ptr<float>(), ld1(K), M * K, (int32_t)batch,
                                        (int32_t)M, (int32_t)K, (int32_t)std::min(kTile, N - n0),
                                        Bc.data_ptr<float>() + n0, N, strideB, bias_ptr ? bias_ptr + n0 : nullptr,
                                        C.data_ptr<float>() + n0, N, M * N, stream_of(C)),
                 what);
  return true;
}

bool naive_spmm_dense(torch::Tensor A, torch::Tensor B, torch::Tensor C) {
  return spmm_dense_impl(A, B, nullptr, C, "naive_spmm_dense");
}

bool naive_spmm_dense_bias(torch::Tensor A, torch::Tensor B, torch::Tensor bias, torch::Tensor C) {
  return spmm_dense_impl(A, B, &bias, C, "naive_spmm_dense_bias");
}

// dA = dC·B and dB = dCᵀ·A of C = A·Bᵀ (the backward of cublasTransbMM) in ONE launch that reads dC once:
// dC [batch…, m, k], B [batch…, k, n], A [batch…, m, n] contiguous with equal batch dims → dA [batch…, m, n],
// dB [batch…, k, n] (caller-allocated).  False (nothing launched) when the fused form does not cover the shapes.
bool cublas_bmm_pair(torch::Tensor dC, torch::Tensor B, torch::Tensor A, torch::Tensor dA, torch::Tensor dB) {
  const char* what = "cublas_bmm_pair";
  for (const torch::Tensor* t : {&dC, &B, &A, &dA, &dB}) check_device_f32(*t, "operand");
  check_same_device(what, dA.device(), {&dC, &B, &A, &dB});
  if (dC.dim() < 2 || B.dim() != dC.dim() || A.dim() != dC.dim() || dA.dim() != dC.dim() || dB.dim() != dC.dim()) return false;
  const int64_t m = dC.size(-2), k = dC.size(-1), n = B.size(-1);
  const int64_t batch = m * k > 0 ? dC.numel() / (m * k) : 0;
  if (!(dC.is_contiguous() && B.is_contiguous() && A.is_contiguous() && dA.is_contiguous() && dB.is_contiguous())) return false;
  if (B.size(-2) != k || A.size(-2) != m || A.size(-1) != n || B.numel() != batch * k * n || A.numel() != batch * m * n ||
      dA.numel() != batch * m * n || dB.numel() != batch * k * n || dA.size(-2) != m || dA.size(-1) != n ||
      dB.size(-2) != k || dB.size(-1) != n)
    return false;
  if (batch <= 0 || batch > INT32_MAX || m > INT32_MAX || k > INT32_MAX || n > INT32_MAX) return false;
  c10::hip::HIPGuard guard(dA.device().index());
  const int st = mi_gemm_pair_a_at_f32(dC.data_ptr<float>(), B.data_ptr<float>(), A.data_ptr<float>(), dA.data_ptr<float>(),
                                       dB.data_ptr<float>(), (int32_t)batch, (int32_t)m, (int32_t)k, (int32_t)n,
                                       stream_of(dA));
  if (st == 1) return false;
  check_status(st, what);
  return true;
}

// int32[1] on B's device: 1 when B holds an inf or a nan, else 0 (stream-ordered, nothing read back).
torch::Tensor nonfinite_flag(torch::Tensor B) {
  check_device_f32(B, "B");
  torch::Tensor Bc = B.contiguous();
  c10::hip::HIPGuard guard(B.device().index());
  torch::Tensor flag = torch::empty({1}, torch::dtype(torch::kInt32).device(B.device()));
  check_status(mi_nonfinite_flag_f32(Bc.data_ptr<float>(), 1, Bc.numel(), std::max<int64_t>(Bc.numel(), 1),
                                     flag.data_ptr<int32_t>(), stream_of(B)),
               "nonfinite_flag");
  return flag;
}

// The zero-skipping product of naive_spmm_dense as a GATED launch: it runs only when flag[0] != 0 on the device
// (see mi_spmm_dense_skip_gated_f32).  A [batch…, M, K] dense, B [K, N] or [batch…, K, N], C [batch…, M, N].
// `dry_run` only answers whether the shape is covered (no launch).  Returns false when it is not.
bool naive_spmm_dense_gated(torch::Tensor A, torch::Tensor B, torch::Tensor C, torch::Tensor flag, bool dry_run) {
  const char* what = "naive_spmm_dense_gated";
  check_device_f32(A, "A");
  check_device_f32(B, "B");
  check_device_f32(C, "C");
  check_same_device(what, C.device(), {&A, &B});
  TORCH_CHECK(A.dim() >= 2 && C.dim() == A.dim(), what, ": A and C must have the same rank (>= 2)");
  TORCH_CHECK(C.is_contiguous(), what, ": C must be contiguous");
  const int64_t M = A.size(-2), K = A.size(-1), N = C.size(-1);
  const int64_t batch = M * K > 0 ? A.numel() / (M * K) : (C.numel() / std::max<int64_t>(C.size(-2) * N, 1));
  TORCH_CHECK(C.size(-2) == M, what, ": C must have ", M, " rows");
  int64_t strideB = 0;
  if (B.dim() == 2) {
    TORCH_CHECK(B.size(0) == K && B.size(1) == N, what, ": B must be [", K, ", ", N, "]");
  } else {
    TORCH_CHECK(B.dim() == A.dim() && B.size(-2) == K && B.size(-1) == N && B.numel() == batch * K * N, what,
                ": B must be [batch…, ", K, ", ", N, "] with A's batch dims");
    strideB = K * N;
  }
  TORCH_CHECK(C.numel() == batch * M * N, what, ": C must be [batch…, ", M, ", ", N, "]");
  TORCH_CHECK(M <= INT32_MAX && K <= INT32_MAX && N <= INT32_MAX && batch <= INT32_MAX, what, ": dimension too large");
  if (N % 4 != 0 || (K * N) % 4 != 0 || (M * N) % 4 != 0 || N > 256 * 65535) return false;
  if (dry_run) return true;
  TORCH_CHECK(flag.defined() && flag.is_cuda() && flag.scalar_type() == torch::kInt32 && flag.numel() >= 1 &&
                  flag.device() == C.device(),
              what, ": flag must be an int32 device tensor on C's device");
  if (batch == 0 || M == 0 || N == 0) return true;
  torch::Tensor Ac = A.contiguous(), Bc = B.contiguous();
  if ((reinterpret_cast<uintptr_t>(Bc.data_ptr<float>()) & 15u) || (reinterpret_cast<uintptr_t>(C.data_ptr<float>()) & 15u)) {
    Bc = Bc.clone();  // a contiguous view at an odd offset: give the kernel an aligned copy
    TORCH_CHECK((reinterpret_cast<uintptr_t>(C.data_ptr<float>()) & 15u) == 0, what, ": C must be 16-byte aligned");
  }
  c10::hip::HIPGuard guard(C.device().index());
  check_status(mi_spmm_dense_skip_gated_f32(Ac.data_ptr<float>(), std::max<int64_t>(K, 1), M * K, (int32_t)batch,
                                            (int32_t)M, (int32_t)K, (int32_t)N, Bc.data_ptr<float>(), N, strideB, nullptr,
                                            C.data_ptr<float>(), N, M * N, flag.data_ptr<int32_t>(), stream_of(C)),
               what);
  return true;
}

// CSR of A (A_rows×A_cols) → CSR of Aᵀ: (values, columns, offsets[A_cols+1]).
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> csr_transpose(torch::Tensor A_values,
                                                                      torch::Tensor A_columns,
                                                                      torch::Tensor A_offsets, int64_t nnzA,
                                                                      int64_t A_rows, int64_t A_cols) {
  const char* what = "csr_transpose";
  value_dtype(what, {{"A_values", &A_values}});
  const Csr a = csr_arrays(what, &A_values, &A_columns, A_offsets, nnzA, A_rows, A_cols);
  c10::hip::HIPGuard guard(A_values.device().index());
  auto iopt = torch::dtype(torch::kInt32).device(A_values.device());
  torch::Tensor t_off = torch::empty({A_cols + 1}, iopt);
  torch::Tensor t_col = torch::empty({nnzA}, iopt);
  torch::Tensor t_val = torch::empty({nnzA}, A_values.options());
  const size_t ws_bytes = mi_csr_transpose_workspace_bytes(a.rows, a.cols, nnzA);
  torch::Tensor ws = byte_workspace(a.device, ws_bytes, 1);
  const mi_stream_t stream = stream_of(A_values);
  auto run = [&]() {
    check_status(mi_csr_transpose_f32(a.offsets, a.columns, a.f32(), nnzA, a.rows, a.cols, t_off.data_ptr<int32_t>(),
                                      t_col.data_ptr<int32_t>(), t_val.data_ptr<float>(), ws.data_ptr(), ws_bytes, stream),
                 what);
  };
  run();
  // The one-sweep plan (≥ 33 M non-zeros) hands offsets between workgroups by look-back; a poll that runs into its spin
  // limit sets a flag and goes on with a wrong offset (never seen on a correct run).  Its callers keep what comes out of
  // here for a tensor's or a handle's lifetime, so the flag is read here (one synchronisation behind a ≥ 1 ms launch; not
  // under stream capture, where nothing may be read back) and a give-up re-runs the transpose on the table plan
  // (advisor, round 4).
  if (mi_csr_transpose_auto_takes_one_sweep(1, a.rows, a.cols, nnzA) == 1 && !stream_is_capturing(stream) &&
      mi_csr_transpose_check(ws.data_ptr(), ws_bytes, 1, a.rows, a.cols, nnzA, stream) != MI_OK) {
    mi_csr_transpose_set_plan(MI_TRANSPOSE_PLAN_TABLES);
    try {
      run();
    } catch (...) {
      mi_csr_transpose_set_plan(MI_TRANSPOSE_PLAN_AUTO);
      throw;
    }
    mi_csr_transpose_set_plan(MI_TRANSPOSE_PLAN_AUTO);
  }
  return std::make_tuple(t_val, t_col, t_off);
}

// Batched CSR (offsets [batch, A_rows+1], global) → the batched CSR of the transposes
// (values, columns, offsets [batch, A_cols+1]); one set of launches for the whole batch.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> csr_transpose_batched(torch::Tensor A_values,
                                                                              torch::Tensor A_columns,
                                                                              torch::Tensor A_offsets, int64_t nnzA,
                                                                              int64_t batch, int64_t A_rows,
                                                                              int64_t A_cols) {
  const char* what = "csr_transpose_batched";
  value_dtype(what, {{"A_values", &A_values}});
  const Csr a = csr_arrays(what, &A_values, &A_columns, A_offsets, nnzA, A_rows, A_cols, batch);
  c10::hip::HIPGuard guard(A_values.device().index());
  auto iopt = torch::dtype(torch::kInt32).device(A_values.device());
  torch::Tensor t_off = torch::empty({batch, A_cols + 1}, iopt);
  torch::Tensor t_col = torch::empty({nnzA}, iopt);
  torch::Tensor t_val = torch::empty({nnzA}, A_values.options());
  // (the one-workgroup-per-item plan of small items uses no workspace)
  const size_t ws_bytes = mi_csr_transpose_batched_in_lds(nnzA, a.batch, a.rows, a.cols) == 1
                              ? 0 : mi_csr_transpose_batched_workspace_bytes(a.batch, a.rows, a.cols, nnzA);
  torch::Tensor ws = byte_workspace(a.device, ws_bytes, 1);
  check_status(mi_csr_transpose_batched_f32(a.offsets, a.columns, a.f32(), nnzA, a.batch, a.rows, a.cols, t_off.data_ptr<int32_t>(),
                                            t_col.data_ptr<int32_t>(), t_val.data_ptr<float>(), ws.data_ptr(), ws_bytes,
                                            stream_of(A_values)),
               what);
  return std::make_tuple(t_val, t_col, t_off);
}

// The same on a batched CSR pattern (offsets [batch, rows + 1], global), dC [batch, A_rows, N], B [batch, A_cols, N] or
// [A_cols, N] (shared), into the caller's out [nnzA]; False (nothing launched) when the LDS-resident form does not take
// the problem: run sddmm on the block-diagonal matrix of the batch instead (same bits).
bool sddmm_batched(torch::Tensor A_columns, torch::Tensor A_offsets, int64_t nnzA, int64_t batch, int64_t A_rows,
                   int64_t A_cols, torch::Tensor dC, torch::Tensor B, torch::Tensor out) {
  const char* what = "sddmm_batched";
  value_dtype(what, {{"dC", &dC}, {"B", &B}, {"out", &out}});
  const Csr a = csr_arrays(what, nullptr, &A_columns, A_offsets, nnzA, A_rows, A_cols, batch);
  check_same_device(what, a.device, {&dC, &B, &out});
  TORCH_CHECK(out.is_contiguous() && out.numel() >= nnzA, what, ": out must be contiguous with nnzA entries");
  TORCH_CHECK(dC.dim() == 3 && dC.size(0) == batch && dC.size(1) == A_rows, what, ": dC must be [batch, A_rows, N]");
  const int64_t N = dC.size(2);
  check_sizes(what, {N});
  const auto b = batched_b(what, B, batch, A_cols, N);
  torch::Tensor dCc = dC.contiguous();
  c10::hip::HIPGuard guard(out.device().index());
  const int st = mi_sddmm_csr_batched_f32(a.offsets, a.columns, nnzA, a.batch, a.rows, a.cols, (int32_t)N, dCc.data_ptr<float>(),
                                          ld1(N), A_rows * N, b.first.data_ptr<float>(), ld1(N), b.second, out.data_ptr<float>(),
                                          stream_of(out));
  if (st == 1) return false;
  check_status(st, what);
  return true;
}

// out[p] = <dC[row(p), :], B[col[p], :]> on A's pattern: d(A·B)/d(A values).
torch::Tensor sddmm(torch::Tensor A_columns, torch::Tensor A_offsets, int64_t nnzA, int64_t A_rows,
                    int64_t A_cols, torch::Tensor dC, torch::Tensor B) {
  const char* what = "sddmm";
  const torch::ScalarType dt = value_dtype(what, {{"dC", &dC}, {"B", &B}}, true);
  const Csr a = csr_arrays(what, nullptr, &A_columns, A_offsets, nnzA, A_rows, A_cols);
  check_same_device(what, a.device, {&dC, &B});
  TORCH_CHECK(dC.dim() == 2 && B.dim() == 2 && dC.size(0) == A_rows && B.size(0) == A_cols &&
                  dC.size(1) == B.size(1),
              what, ": dC must be [A_rows, N] and B [A_cols, N]");
  const int64_t N = B.size(1);
  check_sizes(what, {N});
  torch::Tensor dCc = dC.contiguous(), Bc = B.contiguous();
  c10::hip::HIPGuard guard(dC.device().index());
  torch::Tensor out = torch::empty({nnzA}, dCc.options());
  const int st =
      dt == torch::kFloat32
          ? mi_sddmm_csr_f32(a.offsets, a.columns, nnzA, a.rows, a.cols, (int32_t)N, dCc.data_ptr<float>(), ld1(N),
                             Bc.data_ptr<float>(), ld1(N), out.data_ptr<float>(), stream_of(dCc))
          : (dt == torch::kBFloat16 ? mi_sddmm_csr_bf16 : mi_sddmm_csr_f16)(
                a.offsets, a.columns, nnzA, a.rows, a.cols, (int32_t)N, static_cast<const uint16_t*>(dCc.data_ptr()), ld1(N),
                static_cast<const uint16_t*>(Bc.data_ptr()), ld1(N), static_cast<uint16_t*>(out.data_ptr()), stream_of(dCc));
  check_status(st, what);
  return out;
}

// ---- peer mappings of an output buffer (multi-GPU exchange; mi_ipc_* of the C-ABI) -------------------------------
// (handle bytes, offset of the tensor in its allocation, size of that allocation): what a peer needs to map `t`.
py::tuple ipc_export(const torch::Tensor& t) {
  check_device_f32(t, "ipc_export: tensor");
  TORCH_CHECK(t.is_contiguous(), "ipc_export: the buffer must be contiguous");
  c10::hip::HIPGuard guard(t.device().index());
  char handle[MI_IPC_HANDLE_BYTES];
  int64_t offset = 0, alloc_bytes = 0;
  check_status(mi_ipc_export(t.data_ptr(), handle, &offset, &alloc_bytes), "ipc_export");
  return py::make_tuple(py::bytes(handle, MI_IPC_HANDLE_BYTES), offset, alloc_bytes);
}

// A peer's buffer as a float32 tensor of `shape` in this process.  The tensor does NOT own the mapping: it is valid until
// ipc_close(handle) — the caller (sharded.ShardedSpMM) drops it before closing.
torch::Tensor ipc_open(const std::string& handle, int64_t offset, std::vector<int64_t> shape, int64_t device_index) {
  TORCH_CHECK(handle.size() == MI_IPC_HANDLE_BYTES, "ipc_open: a handle is ", MI_IPC_HANDLE_BYTES, " bytes");
  TORCH_CHECK(offset >= 0 && offset % 4 == 0, "ipc_open: bad offset");
  c10::hip::HIPGuard guard(static_cast<c10::DeviceIndex>(device_index));
  void* base = nullptr;
  check_status(mi_ipc_open(handle.data(), &base), "ipc_open");
  auto opts = torch::TensorOptions().dtype(torch::kFloat32).device(torch::kCUDA, static_cast<c10::DeviceIndex>(device_index));
  return torch::from_blob(static_cast<char*>(base) + offset, shape, [](void*) {}, opts);
}

void ipc_close(const std::string& handle) {
  TORCH_CHECK(handle.size() == MI_IPC_HANDLE_BYTES, "ipc_close: a handle is ", MI_IPC_HANDLE_BYTES, " bytes");
  check_status(mi_ipc_close(handle.data()), "ipc_close");
}
