// custom_mm — block-sparse attention on the matrix cores: the forward and the backward over a CSR block layout
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace (one translation unit; the
// split is for readers).  Not compiled on its own.  Contract: include/mi_spmm.h, "Block-sparse attention": every value
// operand in bfloat16 or every one in float16; offsets int32 [layouts, blocks + 1] with the layouts' bases, columns int32
// layout-local, in 64-blocks; q, out, dout, dq [batch, Sq, D] and k, v, dk, dv [batch, Sk, D] contiguous; lse float32
// [batch, Sq].

struct BlockLayout {
  Csr list;
  int64_t layouts;
};

// the block lists of `layouts` layouts over rows × cols positions (both multiples of 64)
BlockLayout block_layout(const char* what, const torch::Tensor& offsets, const torch::Tensor& columns, int64_t nnz,
                         int64_t rows, int64_t cols) {
  TORCH_CHECK(rows >= 0 && cols >= 0 && rows % 64 == 0 && cols % 64 == 0, what, ": Sq and Sk must be multiples of 64, got ", rows,
              " and ", cols);
  const int64_t blocks = rows / 64;
  TORCH_CHECK(offsets.numel() > 0 && offsets.numel() % (blocks + 1) == 0, what, ": offsets must be [layouts, Sq/64 + 1] = [*, ",
              blocks + 1, "], got ", offsets.numel(), " entries");
  const int64_t layouts = offsets.numel() / (blocks + 1);
  return {csr_arrays(what, nullptr, &columns, offsets, nnz, blocks, cols / 64, layouts, nullptr, {"values", "columns", "offsets"}),
          layouts};
}

bool is_lowp_dtype(const char* what, torch::ScalarType dt) {
  TORCH_CHECK(is_lowp(dt), what, ": q must be bfloat16 or float16, got ", dt);
  return dt == torch::kBFloat16;
}

// out[i] = softmax(scale · q[i]·k[i]ᵀ + mask of layout i mod layouts) · v[i]; lse [batch, Sq] receives the rows' log-sum-exp
torch::Tensor block_attention_forward(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q, torch::Tensor k,
                                      torch::Tensor v, double scale, bool causal, torch::Tensor out, torch::Tensor lse) {
  const char* what = "block_attention_forward";
  const torch::ScalarType dt = value_dtype(what, {{"q", &q}, {"k", &k}, {"v", &v}, {"out", &out}}, true);
  const bool bf = is_lowp_dtype(what, dt);
  TORCH_CHECK(q.dim() == 3 && k.dim() == 3, what, ": q must be [batch, Sq, D] and k [batch, Sk, D]");
  const int64_t batch = q.size(0), Sq = q.size(1), D = q.size(2), Sk = k.size(1);
  const BlockLayout lay = block_layout(what, offsets, columns, nnz, Sq, Sk);
  check_same_device(what, lay.list.device, {&q, &k, &v, &out, &lse});
  check_device_f32(lse, "lse");
  check_attention_dense(what, "q", q, batch, Sq, D);
  check_attention_dense(what, "k", k, batch, Sk, D);
  check_attention_dense(what, "v", v, batch, Sk, D);
  check_attention_dense(what, "out", out, batch, Sq, D);
  TORCH_CHECK(lse.is_contiguous() && lse.numel() == batch * Sq, what, ": lse must be a contiguous [batch, Sq] tensor");
  TORCH_CHECK(!causal || Sq == Sk, what, ": causal needs Sq == Sk, got ", Sq, " and ", Sk);
  check_sizes(what, {batch, Sq, Sk, D});
  c10::hip::HIPGuard guard(out.device().index());
  auto p = [](const torch::Tensor& t) { return static_cast<uint16_t*>(t.data_ptr()); };
  const int st = (bf ? mi_block_attention_fwd_bf16 : mi_block_attention_fwd_f16)(
      lay.list.offsets, lay.list.columns, nnz, (int32_t)lay.layouts, (int32_t)batch, (int32_t)Sq, (int32_t)Sk, (int32_t)D,
      causal ? 1 : 0, p(q), D, Sq * D, p(k), D, Sk * D, p(v), D, Sk * D, (float)scale, p(out), D, Sq * D, lse.data_ptr<float>(),
      stream_of(out));
  check_status(st, what);
  return out;
}

// (dq, dk, dv) from the forward's operands, its out and lse, and the incoming dout; the transposed lists of the layouts
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> block_attention_backward(
    torch::Tensor offsets, torch::Tensor columns, torch::Tensor t_offsets, torch::Tensor t_columns, int64_t nnz, torch::Tensor q,
    torch::Tensor k, torch::Tensor v, torch::Tensor out, torch::Tensor dout, torch::Tensor lse, double scale, bool causal,
    torch::Tensor dq, torch::Tensor dk, torch::Tensor dv) {
  const char* what = "block_attention_backward";
  const torch::ScalarType dt = value_dtype(
      what, {{"q", &q}, {"k", &k}, {"v", &v}, {"out", &out}, {"dout", &dout}, {"dq", &dq}, {"dk", &dk}, {"dv", &dv}}, true);
  const bool bf = is_lowp_dtype(what, dt);
  TORCH_CHECK(q.dim() == 3 && k.dim() == 3, what, ": q must be [batch, Sq, D] and k [batch, Sk, D]");
  const int64_t batch = q.size(0), Sq = q.size(1), D = q.size(2), Sk = k.size(1);
  const BlockLayout lay = block_layout(what, offsets, columns, nnz, Sq, Sk);
  const BlockLayout tlay = block_layout(what, t_offsets, t_columns, nnz, Sk, Sq);
  TORCH_CHECK(lay.layouts == tlay.layouts, what, ": the layouts and their transposes differ in number");
  check_same_device(what, lay.list.device, {&t_offsets, &t_columns, &q, &k, &v, &out, &dout, &lse, &dq, &dk, &dv});
  check_device_f32(lse, "lse");
  check_attention_dense(what, "q", q, batch, Sq, D);
  check_attention_dense(what, "k", k, batch, Sk, D);
  check_attention_dense(what, "v", v, batch, Sk, D);
  check_attention_dense(what, "out", out, batch, Sq, D);
  check_attention_dense(what, "dout", dout, batch, Sq, D);
  check_attention_dense(what, "dq", dq, batch, Sq, D);
  check_attention_dense(what, "dk", dk, batch, Sk, D);
  check_attention_dense(what, "dv", dv, batch, Sk, D);
  TORCH_CHECK(lse.is_contiguous() && lse.numel() == batch * Sq, what, ": lse must be a contiguous [batch, Sq] tensor");
  TORCH_CHECK(!causal || Sq == Sk, what, ": causal needs Sq == Sk, got ", Sq, " and ", Sk);
  check_sizes(what, {batch, Sq, Sk, D});
  c10::hip::HIPGuard guard(dq.device().index());
  const size_t ws_bytes = mi_block_attention_workspace_bytes((int32_t)batch, (int32_t)Sq);
  torch::Tensor ws = byte_workspace(dq.device(), ws_bytes, 16);
  auto p = [](const torch::Tensor& t) { return static_cast<uint16_t*>(t.data_ptr()); };
  const int st = (bf ? mi_block_attention_bwd_bf16 : mi_block_attention_bwd_f16)(
      lay.list.offsets, lay.list.columns, tlay.list.offsets, tlay.list.columns, nnz, (int32_t)lay.layouts, (int32_t)batch,
      (int32_t)Sq, (int32_t)Sk, (int32_t)D, causal ? 1 : 0, p(q), D, Sq * D, p(k), D, Sk * D, p(v), D, Sk * D, p(out), D, Sq * D,
      p(dout), D, Sq * D, lse.data_ptr<float>(), (float)scale, p(dq), D, Sq * D, p(dk), D, Sk * D, p(dv), D, Sk * D, ws.data_ptr(),
      ws_bytes, stream_of(dq));
  check_status(st, what);
  return std::make_tuple(dq, dk, dv);
}
