// custom_mm — softmax over the stored entries of every CSR row, and its backward
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace (one translation unit; the
// split is for readers).  Not compiled on its own.  Contract: include/mi_spmm.h, "CSR row softmax": float32, or every value
// operand in bfloat16 or every one in float16; offsets int32 [batch, rows + 1] with the items' bases (batch = 1: a 2-d CSR).

// the C-ABI call shared by both directions: `in2` is null for the forward
torch::Tensor csr_softmax_impl(const char* what, const torch::Tensor& in, const torch::Tensor* in2, const torch::Tensor& offsets,
                               int64_t nnz, int64_t batch, int64_t rows, double scale, torch::Tensor out) {
  const torch::ScalarType dt = in2 != nullptr ? value_dtype(what, {{"y", &in}, {"dy", in2}, {"out", &out}}, true)
                                              : value_dtype(what, {{"values", &in}, {"out", &out}}, true);
  const Csr a = csr_arrays(what, &in, nullptr, offsets, nnz, rows, 0, batch, nullptr, {"values", "columns", "offsets"});
  check_same_device(what, a.device, {&out});
  TORCH_CHECK(out.is_contiguous() && out.numel() >= nnz, what, ": out must be contiguous with nnz entries");
  if (in2 != nullptr) {
    check_same_device(what, a.device, {in2});
    TORCH_CHECK(in2->is_contiguous() && in2->numel() >= nnz, what, ": dy must be contiguous with nnz entries");
  }
  TORCH_CHECK(batch * (rows + 1) <= INT32_MAX, what, ": batch · (rows + 1) does not fit int32 offsets");
  c10::hip::HIPGuard guard(out.device().index());
  const size_t ws_bytes = mi_csr_softmax_workspace_bytes(nnz, a.batch, a.rows);
  torch::Tensor ws;
  if (ws_bytes > 0) ws = byte_workspace(a.device, ws_bytes);
  void* const ws_ptr = ws.defined() ? ws.data_ptr() : nullptr;
  const mi_stream_t stream = stream_of(out);
  const float s = (float)scale;
  int st;
  if (in2 == nullptr) {
    st = dt == torch::kFloat32
             ? mi_csr_softmax_f32(a.offsets, nnz, a.batch, a.rows, a.f32(), s, out.data_ptr<float>(), ws_ptr, ws_bytes, stream)
             : (dt == torch::kBFloat16 ? mi_csr_softmax_bf16 : mi_csr_softmax_f16)(
                   a.offsets, nnz, a.batch, a.rows, a.b16(), s, static_cast<uint16_t*>(out.data_ptr()), ws_ptr, ws_bytes, stream);
  } else {
    st = dt == torch::kFloat32
             ? mi_csr_softmax_backward_f32(a.offsets, nnz, a.batch, a.rows, a.f32(), in2->data_ptr<float>(), s,
                                           out.data_ptr<float>(), ws_ptr, ws_bytes, stream)
             : (dt == torch::kBFloat16 ? mi_csr_softmax_backward_bf16 : mi_csr_softmax_backward_f16)(
                   a.offsets, nnz, a.batch, a.rows, a.b16(), static_cast<const uint16_t*>(in2->data_ptr()), s,
                   static_cast<uint16_t*>(out.data_ptr()), ws_ptr, ws_bytes, stream);
  }
  check_status(st, what);
  return out;
}

// out[p] = softmax over the row of entry p of scale · values; out may be values (in place)
torch::Tensor csr_softmax(torch::Tensor values, torch::Tensor offsets, int64_t nnz, int64_t batch, int64_t rows, double scale,
                          torch::Tensor out) {
  return csr_softmax_impl("csr_softmax", values, nullptr, offsets, nnz, batch, rows, scale, out);
}

// out[p] = scale · y[p] · (dy[p] − Σ_q dy[q] y[q] over the row); out may be dy (in place)
torch::Tensor csr_softmax_backward(torch::Tensor y, torch::Tensor dy, torch::Tensor offsets, int64_t nnz, int64_t batch,
                                   int64_t rows, double scale, torch::Tensor out) {
  return csr_softmax_impl("csr_softmax_backward", y, &dy, offsets, nnz, batch, rows, scale, out);
}
