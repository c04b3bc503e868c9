// custom_mm — block-sparse (BSR) × dense products on the matrix cores: the product over a CSR block list and the sampled
// product on it.  Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace (one
// translation unit; the split is for readers).  Not compiled on its own.  Contract: include/mi_spmm.h, "Block-sparse
// (BSR) × dense products": every value operand in bfloat16 or every one in float16; offsets, columns, entry ids and
// entry rows int32; values [n, 64, 64] contiguous; the dense operands [batch, rows, N], taken with their own leading
// dimension and item stride where they are row-major views (a column-offset view included), copied otherwise.

// a [batch, rows, N] operand as pointer + leading dimension + item stride; `keep` owns what is pointed to
struct BsrDense {
  torch::Tensor keep;
  int64_t ld, stride;
  uint16_t* ptr() const { return static_cast<uint16_t*>(keep.data_ptr()); }
};

BsrDense bsr_dense(const char* what, const char* name, const torch::Tensor& t, int64_t batch, int64_t rows, int64_t N) {
  TORCH_CHECK(t.dim() == 3 && t.size(0) == batch && t.size(1) == rows && t.size(2) == N, what, ": ", name, " must be [", batch, ", ",
              rows, ", ", N, "], got ", t.sizes());
  const bool row_major = (t.stride(2) == 1 || N <= 1) && (rows <= 1 || t.stride(1) >= ld1(N)) && (batch <= 1 || t.stride(0) >= 0);
  torch::Tensor x = row_major ? t : t.contiguous();
  return {x, rows > 1 ? x.stride(1) : ld1(N), batch > 1 ? x.stride(0) : 0};
}

// values / dvalues [n, 64, 64], contiguous, blocks on 16-byte boundaries
void check_bsr_values(const char* what, const char* name, const torch::Tensor& v) {
  TORCH_CHECK(v.dim() == 3 && v.size(1) == 64 && v.size(2) == 64, what, ": ", name, " must be [n, 64, 64], got ", v.sizes());
  TORCH_CHECK(v.is_contiguous(), what, ": ", name, " must be contiguous");
  TORCH_CHECK(v.numel() == 0 || reinterpret_cast<uintptr_t>(v.data_ptr()) % 16 == 0, what, ": ", name, " must be 16-byte aligned");
}

const int32_t* entry_ids_of(const char* what, const c10::optional<torch::Tensor>& ids, int64_t nnz, const torch::Device& dev) {
  if (!ids.has_value() || !ids->defined()) return nullptr;
  check_device_i32(*ids, "entry_ids");
  check_same_device(what, dev, {&*ids});
  TORCH_CHECK(ids->is_contiguous() && ids->numel() >= nnz, what, ": entry_ids must be a contiguous int32 tensor of nnz entries");
  return ids->data_ptr<int32_t>();
}

// C[i] = op(A) · B[i]: offsets [C rows / 64 + 1] and columns [nnz] list, per 64-row block of C, the 64-blocks of B's rows
// it sums over; entry p uses values[entry_ids[p]] (None: values[p]), transposed when trans_a (the lists then being those
// of Aᵀ).  C [batch, rows, N] contiguous, rows a multiple of 64; B [batch, inner, N].
torch::Tensor bsr_mm(torch::Tensor offsets, torch::Tensor columns, c10::optional<torch::Tensor> entry_ids, int64_t nnz,
                     torch::Tensor values, torch::Tensor B, torch::Tensor C, bool trans_a) {
  const char* what = "bsr_mm";
  const torch::ScalarType dt = value_dtype(what, {{"values", &values}, {"B", &B}, {"C", &C}}, true);
  TORCH_CHECK(is_lowp(dt), what, ": values must be bfloat16 or float16, got ", dt);
  TORCH_CHECK(B.dim() == 3 && C.dim() == 3, what, ": B must be [batch, inner, N] and C [batch, rows, N]");
  const int64_t batch = C.size(0), rows = C.size(1), N = C.size(2), inner = B.size(1);
  TORCH_CHECK(rows % 64 == 0 && inner % 64 == 0, what, ": the rows of C and of B must be multiples of 64, got ", rows, " and ", inner);
  const Csr list = csr_arrays(what, nullptr, &columns, offsets, nnz, rows / 64, inner / 64, c10::nullopt, nullptr,
                              {"values", "columns", "offsets"});
  check_same_device(what, list.device, {&values, &B, &C});
  const int32_t* ids = entry_ids_of(what, entry_ids, nnz, list.device);
  check_bsr_values(what, "values", values);
  TORCH_CHECK(ids != nullptr || values.size(0) >= nnz, what, ": values holds ", values.size(0), " blocks for ", nnz, " entries");
  TORCH_CHECK(C.is_contiguous(), what, ": C must be contiguous");
  const BsrDense b = bsr_dense(what, "B", B, batch, inner, N);
  check_sizes(what, {batch, rows, inner, N, values.size(0)}, nnz);
  c10::hip::HIPGuard guard(C.device().index());
  const int st = (dt == torch::kBFloat16 ? mi_bsr_mm_bf16 : mi_bsr_mm_f16)(
      list.offsets, list.columns, ids, nnz, trans_a ? 1 : 0, (int32_t)rows, (int32_t)inner, (int32_t)N, (int32_t)batch,
      static_cast<const uint16_t*>(values.data_ptr()), values.size(0), b.ptr(), b.ld, b.stride,
      static_cast<uint16_t*>(C.data_ptr()), ld1(N), rows * N, stream_of(C));
  check_status(st, what);
  return C;
}

// the column tile (64 or 128) bsr_mm launches for C [batch, rows, N]: shape only
int64_t bsr_mm_tile_n(int64_t rows, int64_t N, int64_t batch) {
  check_sizes("bsr_mm_tile_n", {rows, N, batch});
  return mi_bsr_mm_tile_n((int32_t)rows, (int32_t)N, (int32_t)batch);
}

// dvalues[entry_ids[p]] (None: dvalues[p]) = Σ over the items of dC[64·entry_row[p] …, :] · B[64·columns[p] …, :]ᵀ
torch::Tensor bsr_sddmm(torch::Tensor entry_row, torch::Tensor columns, c10::optional<torch::Tensor> entry_ids, int64_t nnz,
                        torch::Tensor dC, torch::Tensor B, torch::Tensor dvalues) {
  const char* what = "bsr_sddmm";
  const torch::ScalarType dt = value_dtype(what, {{"dC", &dC}, {"B", &B}, {"dvalues", &dvalues}}, true);
  TORCH_CHECK(is_lowp(dt), what, ": dC must be bfloat16 or float16, got ", dt);
  TORCH_CHECK(dC.dim() == 3 && B.dim() == 3, what, ": dC must be [batch, M, N] and B [batch, K, N]");
  const int64_t batch = dC.size(0), M = dC.size(1), N = dC.size(2), K = B.size(1);
  TORCH_CHECK(M % 64 == 0 && K % 64 == 0, what, ": the rows of dC and of B must be multiples of 64, got ", M, " and ", K);
  check_device_i32(entry_row, "entry_row");
  check_device_i32(columns, "columns");
  const torch::Device dev = entry_row.device();
  check_same_device(what, dev, {&columns, &dC, &B, &dvalues});
  TORCH_CHECK(entry_row.is_contiguous() && columns.is_contiguous() && entry_row.numel() >= nnz && columns.numel() >= nnz, what,
              ": entry_row and columns must be contiguous int32 tensors of nnz entries");
  const int32_t* ids = entry_ids_of(what, entry_ids, nnz, dev);
  check_bsr_values(what, "dvalues", dvalues);
  TORCH_CHECK(ids != nullptr || dvalues.size(0) >= nnz, what, ": dvalues holds ", dvalues.size(0), " blocks for ", nnz, " entries");
  const BsrDense g = bsr_dense(what, "dC", dC, batch, M, N);
  const BsrDense b = bsr_dense(what, "B", B, batch, K, N);
  check_sizes(what, {batch, M, K, N, dvalues.size(0)}, nnz);
  c10::hip::HIPGuard guard(dvalues.device().index());
  const int st = (dt == torch::kBFloat16 ? mi_bsr_sddmm_bf16 : mi_bsr_sddmm_f16)(
      entry_row.data_ptr<int32_t>(), columns.data_ptr<int32_t>(), ids, nnz, (int32_t)M, (int32_t)K, (int32_t)N, (int32_t)batch,
      g.ptr(), g.ld, g.stride, b.ptr(), b.ld, b.stride, static_cast<uint16_t*>(dvalues.data_ptr()), dvalues.size(0),
      stream_of(dvalues));
  check_status(st, what);
  return dvalues;
}
