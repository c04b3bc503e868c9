// custom_mm — fused sparse attention on a CSR pattern: the one-launch forward and the row side of its backward
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace (one translation unit; the
// split is for readers).  Not compiled on its own.  Contract: include/mi_spmm.h, "Fused sparse attention": float32, or every
// value operand in bfloat16 or every one in float16; offsets int32 [batch, rows + 1] with the items' bases (batch = 1: a
// 2-d CSR), columns int32 item-local; q, out, dout, dq [batch, rows, D] and k, v [batch, cols, D] contiguous.

// a contiguous [batch, n, D] operand of the fused entries
void check_attention_dense(const char* what, const char* name, const torch::Tensor& t, int64_t batch, int64_t n, int64_t D) {
  TORCH_CHECK(t.dim() == 3 && t.size(0) == batch && t.size(1) == n && t.size(2) == D && t.is_contiguous(), what, ": ", name,
              " must be a contiguous [", batch, ", ", n, ", ", D, "] tensor");
}

// out[i] = softmax(scale · q[i]·k[i]ᵀ on item i's pattern) · v[i]; stats [batch · rows, 2] float32 receives (m, 1 / s) per row
torch::Tensor sparse_attention_fwd(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, int64_t batch, int64_t rows,
                                   int64_t cols, torch::Tensor q, torch::Tensor k, torch::Tensor v, double scale,
                                   torch::Tensor out, torch::Tensor stats) {
  const char* what = "sparse_attention_fwd";
  const torch::ScalarType dt = value_dtype(what, {{"q", &q}, {"k", &k}, {"v", &v}, {"out", &out}}, true);
  const Csr a = csr_arrays(what, nullptr, &columns, offsets, nnz, rows, cols, batch, nullptr, {"values", "columns", "offsets"});
  check_same_device(what, a.device, {&q, &k, &v, &out, &stats});
  check_device_f32(stats, "stats");
  TORCH_CHECK(q.dim() == 3, what, ": q must be [batch, rows, D]");
  const int64_t D = q.size(2);
  check_attention_dense(what, "q", q, batch, rows, D);
  check_attention_dense(what, "k", k, batch, cols, D);
  check_attention_dense(what, "v", v, batch, cols, D);
  check_attention_dense(what, "out", out, batch, rows, D);
  TORCH_CHECK(stats.is_contiguous() && stats.numel() == 2 * batch * rows, what, ": stats must be a contiguous [batch · rows, 2] tensor");
  check_sizes(what, {D});
  c10::hip::HIPGuard guard(out.device().index());
  const mi_stream_t stream = stream_of(out);
  const float s = (float)scale;
  const int32_t d = (int32_t)D;
  int st;
  if (dt == torch::kFloat32) {
    st = mi_sparse_attention_f32(a.offsets, a.columns, nnz, a.batch, a.rows, a.cols, d, q.data_ptr<float>(), D, rows * D,
                                 k.data_ptr<float>(), D, cols * D, v.data_ptr<float>(), D, cols * D, s, out.data_ptr<float>(), D,
                                 rows * D, stats.data_ptr<float>(), nullptr, 0, stream);
  } else {
    auto p = [](const torch::Tensor& t) { return static_cast<uint16_t*>(t.data_ptr()); };
    st = (dt == torch::kBFloat16 ? mi_sparse_attention_bf16 : mi_sparse_attention_f16)(
        a.offsets, a.columns, nnz, a.batch, a.rows, a.cols, d, p(q), D, rows * D, p(k), D, cols * D, p(v), D, cols * D, s, p(out),
        D, rows * D, stats.data_ptr<float>(), nullptr, 0, stream);
  }
  check_status(st, what);
  return out;
}

// dq (returned), and y [nnz], ds [nnz] in CSR order, from the forward's operands, its stats and the incoming dout
torch::Tensor sparse_attention_bwd(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, int64_t batch, int64_t rows,
                                   int64_t cols, torch::Tensor q, torch::Tensor k, torch::Tensor v, torch::Tensor dout,
                                   torch::Tensor stats, double scale, torch::Tensor dq, torch::Tensor y, torch::Tensor ds) {
  const char* what = "sparse_attention_bwd";
  const torch::ScalarType dt =
      value_dtype(what, {{"q", &q}, {"k", &k}, {"v", &v}, {"dout", &dout}, {"dq", &dq}, {"y", &y}, {"ds", &ds}}, true);
  const Csr a = csr_arrays(what, nullptr, &columns, offsets, nnz, rows, cols, batch, nullptr, {"values", "columns", "offsets"});
  check_same_device(what, a.device, {&q, &k, &v, &dout, &stats, &dq, &y, &ds});
  check_device_f32(stats, "stats");
  TORCH_CHECK(q.dim() == 3, what, ": q must be [batch, rows, D]");
  const int64_t D = q.size(2);
  check_attention_dense(what, "q", q, batch, rows, D);
  check_attention_dense(what, "k", k, batch, cols, D);
  check_attention_dense(what, "v", v, batch, cols, D);
  check_attention_dense(what, "dout", dout, batch, rows, D);
  check_attention_dense(what, "dq", dq, batch, rows, D);
  TORCH_CHECK(stats.is_contiguous() && stats.numel() == 2 * batch * rows, what, ": stats must be a contiguous [batch · rows, 2] tensor");
  TORCH_CHECK(y.is_contiguous() && y.numel() >= nnz && ds.is_contiguous() && ds.numel() >= nnz, what,
              ": y and ds must be contiguous with nnz entries");
  check_sizes(what, {D});
  c10::hip::HIPGuard guard(dq.device().index());
  const mi_stream_t stream = stream_of(dq);
  const float s = (float)scale;
  const int32_t d = (int32_t)D;
  int st;
  if (dt == torch::kFloat32) {
    st = mi_sparse_attention_backward_f32(a.offsets, a.columns, nnz, a.batch, a.rows, a.cols, d, q.data_ptr<float>(), D, rows * D,
                                          k.data_ptr<float>(), D, cols * D, v.data_ptr<float>(), D, cols * D,
                                          dout.data_ptr<float>(), D, rows * D, stats.data_ptr<float>(), s, dq.data_ptr<float>(), D,
                                          rows * D, y.data_ptr<float>(), ds.data_ptr<float>(), nullptr, 0, stream);
  } else {
    auto p = [](const torch::Tensor& t) { return static_cast<uint16_t*>(t.data_ptr()); };
    st = (dt == torch::kBFloat16 ? mi_sparse_attention_backward_bf16 : mi_sparse_attention_backward_f16)(
        a.offsets, a.columns, nnz, a.batch, a.rows, a.cols, d, p(q), D, rows * D, p(k), D, cols * D, p(v), D, cols * D, p(dout), D,
        rows * D, stats.data_ptr<float>(), s, p(dq), D, rows * D, p(y), p(ds), nullptr, 0, stream);
  }
  check_status(st, what);
  return dq;
}
