// custom_mm — block-sparse attention on the matrix cores: the forward and the backward over a CSR block layout
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace (one translation unit; the
// split is for readers).  Not compiled on its own.  Contract: include/mi_spmm.h, "Block-sparse attention": every value
// operand in bfloat16 or every one in float16; offsets int32 [layouts, blocks + 1] with the layouts' bases, columns int32
// layout-local, in 64-blocks; q, out, dout, dq [batch, Sq, D] and k, v, dk, dv [batch / group, Sk, D] contiguous; lse
// float32 [batch, Sq] — batch counts QUERY items.
// One implementation per direction (block_forward, block_backward) behind the four registered names.  The plain pair
// fixes group = 1 and has no lengths; the _ex pair (DESIGN.md §3.17) infers the group from the two batch sizes and takes
// q_lens / k_lens, None or int32 device tensors of one count that divides batch / group.  Both call the _ex C entries:
// the plain C entries are those with 1, nullptr, nullptr, 0.

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

using OptTensor = c10::optional<torch::Tensor>;

struct BlockLens {
  const int32_t* q;
  const int32_t* k;
  int64_t count;
};

BlockLens block_lens(const char* what, const OptTensor& q_lens, const OptTensor& k_lens, int64_t batch, int64_t group,
                     const torch::Device& dev) {
  BlockLens r = {nullptr, nullptr, 0};
  const std::pair<const char*, const OptTensor*> both[] = {{"q_lens", &q_lens}, {"k_lens", &k_lens}};
  for (const auto& [name, t] : both) {
    if (!t->has_value() || !(*t)->defined()) continue;
    check_device_i32(**t, name);
    check_same_device(what, dev, {&**t});
    TORCH_CHECK((*t)->is_contiguous() && (*t)->numel() > 0, what, ": ", name, " must be a contiguous, non-empty int32 tensor");
    TORCH_CHECK(r.count == 0 || r.count == (*t)->numel(), what, ": q_lens and k_lens must have one count, got ", r.count, " and ",
                (*t)->numel());
    r.count = (*t)->numel();
    (name[0] == 'q' ? r.q : r.k) = (*t)->data_ptr<int32_t>();
  }
  TORCH_CHECK(r.count == 0 || (batch % r.count == 0 && (batch / r.count) % group == 0), what, ": ", r.count,
              " lengths do not divide ", batch, " query items in groups of ", group);
  return r;
}

// the query items per k / v item: 1 for the plain bindings (k of another item count fails its own check later), inferred
// from the two batch sizes where the binding is `grouped`
int64_t block_group(const char* what, bool grouped, const torch::Tensor& q, const torch::Tensor& k) {
  TORCH_CHECK(q.dim() == 3 && k.dim() == 3, what, ": q must be [batch, Sq, D] and k ",
              grouped ? "[batch / group, Sk, D]" : "[batch, Sk, D]");
  if (!grouped) return 1;
  TORCH_CHECK(k.size(0) > 0 ? q.size(0) % k.size(0) == 0 : q.size(0) == 0, what, ": ", q.size(0), " query items are not a multiple of ",
              k.size(0), " k / v items");
  return k.size(0) > 0 ? std::max<int64_t>(q.size(0) / k.size(0), 1) : 1;
}

struct BlockDense {
  const char* name;
  const torch::Tensor& t;
  int64_t items, S;
};

// out[i] = softmax(scale · q[i]·k[i / group]ᵀ + mask of layout i mod layouts) · v[i / group]; lse [batch, Sq] receives the
// rows' log-sum-exp
torch::Tensor block_forward(const char* what, bool grouped, const torch::Tensor& offsets, const torch::Tensor& columns, int64_t nnz,
                            const torch::Tensor& q, const torch::Tensor& k, const torch::Tensor& v, double scale, bool causal,
                            const torch::Tensor& out, const torch::Tensor& lse, const OptTensor& q_lens, const OptTensor& k_lens) {
  const torch::ScalarType dt = value_dtype(what, {{"q", &q}, {"k", &k}, {"v", &v}, {"out", &out}}, true);
  const bool bf = is_lowp_dtype(what, dt);
  const int64_t group = block_group(what, grouped, q, k);
  const int64_t batch = q.size(0), Sq = q.size(1), D = q.size(2), Sk = k.size(1), items = grouped ? k.size(0) : batch;
  const BlockLayout lay = block_layout(what, offsets, columns, nnz, Sq, Sk);
  check_same_device(what, lay.list.device, {&q, &k, &v, &out, &lse});
  check_device_f32(lse, "lse");
  for (const BlockDense& d : {BlockDense{"q", q, batch, Sq}, {"k", k, items, Sk}, {"v", v, items, Sk}, {"out", out, batch, Sq}})
    check_attention_dense(what, d.name, d.t, d.items, d.S, D);
  TORCH_CHECK(lse.is_contiguous() && lse.numel() == batch * Sq, what, ": lse must be a contiguous [batch, Sq] tensor");
  TORCH_CHECK(!causal || Sq == Sk, what, ": causal needs Sq == Sk, got ", Sq, " and ", Sk);
  check_sizes(what, {batch, Sq, Sk, D});
  const BlockLens lens = block_lens(what, q_lens, k_lens, batch, group, lay.list.device);
  c10::hip::HIPGuard guard(out.device().index());
  auto p = [](const torch::Tensor& t) { return static_cast<uint16_t*>(t.data_ptr()); };
  const int st = (bf ? mi_block_attention_fwd_ex_bf16 : mi_block_attention_fwd_ex_f16)(
      lay.list.offsets, lay.list.columns, nnz, (int32_t)lay.layouts, (int32_t)batch, (int32_t)Sq, (int32_t)Sk, (int32_t)D,
      causal ? 1 : 0, p(q), D, Sq * D, p(k), D, Sk * D, p(v), D, Sk * D, (float)scale, p(out), D, Sq * D, lse.data_ptr<float>(),
      (int32_t)group, lens.q, lens.k, (int32_t)lens.count, stream_of(out));
  check_status(st, what);
  return out;
}

// (dq, dk, dv) from the forward's operands, its out and lse, and the incoming dout; the transposed lists of the layouts;
// dk, dv [batch / group, Sk, D] summed over the group in one accumulator
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> block_backward(
    const char* what, bool grouped, const torch::Tensor& offsets, const torch::Tensor& columns, const torch::Tensor& t_offsets,
    const torch::Tensor& t_columns, int64_t nnz, const torch::Tensor& q, const torch::Tensor& k, const torch::Tensor& v,
    const torch::Tensor& out, const torch::Tensor& dout, const torch::Tensor& lse, double scale, bool causal, const torch::Tensor& dq,
    const torch::Tensor& dk, const torch::Tensor& dv, const OptTensor& q_lens, const OptTensor& k_lens) {
  const torch::ScalarType dt = value_dtype(
      what, {{"q", &q}, {"k", &k}, {"v", &v}, {"out", &out}, {"dout", &dout}, {"dq", &dq}, {"dk", &dk}, {"dv", &dv}}, true);
  const bool bf = is_lowp_dtype(what, dt);
  const int64_t group = block_group(what, grouped, q, k);
  const int64_t batch = q.size(0), Sq = q.size(1), D = q.size(2), Sk = k.size(1), items = grouped ? k.size(0) : batch;
  const BlockLayout lay = block_layout(what, offsets, columns, nnz, Sq, Sk);
  const BlockLayout tlay = block_layout(what, t_offsets, t_columns, nnz, Sk, Sq);
  TORCH_CHECK(lay.layouts == tlay.layouts, what, ": the layouts and their transposes differ in number");
  check_same_device(what, lay.list.device, {&t_offsets, &t_columns, &q, &k, &v, &out, &dout, &lse, &dq, &dk, &dv});
  check_device_f32(lse, "lse");
  for (const BlockDense& d : {BlockDense{"q", q, batch, Sq}, {"k", k, items, Sk}, {"v", v, items, Sk}, {"out", out, batch, Sq},
                              {"dout", dout, batch, Sq}, {"dq", dq, batch, Sq}, {"dk", dk, items, Sk}, {"dv", dv, items, Sk}})
    check_attention_dense(what, d.name, d.t, d.items, d.S, D);
  TORCH_CHECK(lse.is_contiguous() && lse.numel() == batch * Sq, what, ": lse must be a contiguous [batch, Sq] tensor");
  TORCH_CHECK(!causal || Sq == Sk, what, ": causal needs Sq == Sk, got ", Sq, " and ", Sk);
  check_sizes(what, {batch, Sq, Sk, D});
  const BlockLens lens = block_lens(what, q_lens, k_lens, batch, group, lay.list.device);
  c10::hip::HIPGuard guard(dq.device().index());
  const size_t ws_bytes = mi_block_attention_workspace_bytes((int32_t)batch, (int32_t)Sq);
  torch::Tensor ws = byte_workspace(dq.device(), ws_bytes, 16);
  auto p = [](const torch::Tensor& t) { return static_cast<uint16_t*>(t.data_ptr()); };
  const int st = (bf ? mi_block_attention_bwd_ex_bf16 : mi_block_attention_bwd_ex_f16)(
      lay.list.offsets, lay.list.columns, tlay.list.offsets, tlay.list.columns, nnz, (int32_t)lay.layouts, (int32_t)batch,
      (int32_t)Sq, (int32_t)Sk, (int32_t)D, causal ? 1 : 0, p(q), D, Sq * D, p(k), D, Sk * D, p(v), D, Sk * D, p(out), D, Sq * D,
      p(dout), D, Sq * D, lse.data_ptr<float>(), (float)scale, p(dq), D, Sq * D, p(dk), D, Sk * D, p(dv), D, Sk * D, ws.data_ptr(),
      ws_bytes, (int32_t)group, lens.q, lens.k, (int32_t)lens.count, stream_of(dq));
  check_status(st, what);
  return std::make_tuple(dq, dk, dv);
}

// ---- the registered names: their argument lists are the Python signatures ----------------------------------------------

torch::Tensor block_attention_forward(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q, torch::Tensor k,
                                      torch::Tensor v, double scale, bool causal, torch::Tensor out, torch::Tensor lse) {
  return block_forward("block_attention_forward", false, offsets, columns, nnz, q, k, v, scale, causal, out, lse, c10::nullopt,
                       c10::nullopt);
}

torch::Tensor block_attention_forward_ex(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q, torch::Tensor k,
                                         torch::Tensor v, double scale, bool causal, torch::Tensor out, torch::Tensor lse,
                                         OptTensor q_lens, OptTensor k_lens) {
  return block_forward("block_attention_forward_ex", true, offsets, columns, nnz, q, k, v, scale, causal, out, lse, q_lens, k_lens);
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> block_attention_backward(
    torch::Tensor offsets, torch::Tensor columns, torch::Tensor t_offsets, torch::Tensor t_columns, int64_t nnz, torch::Tensor q,
    torch::Tensor k, torch::Tensor v, torch::Tensor out, torch::Tensor dout, torch::Tensor lse, double scale, bool causal,
    torch::Tensor dq, torch::Tensor dk, torch::Tensor dv) {
  return block_backward("block_attention_backward", false, offsets, columns, t_offsets, t_columns, nnz, q, k, v, out, dout, lse, scale,
                        causal, dq, dk, dv, c10::nullopt, c10::nullopt);
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> block_attention_backward_ex(
    torch::Tensor offsets, torch::Tensor columns, torch::Tensor t_offsets, torch::Tensor t_columns, int64_t nnz, torch::Tensor q,
    torch::Tensor k, torch::Tensor v, torch::Tensor out, torch::Tensor dout, torch::Tensor lse, double scale, bool causal,
    torch::Tensor dq, torch::Tensor dk, torch::Tensor dv, OptTensor q_lens, OptTensor k_lens) {
  return block_backward("block_attention_backward_ex", true, offsets, columns, t_offsets, t_columns, nnz, q, k, v, out, dout, lse,
                        scale, causal, dq, dk, dv, q_lens, k_lens);
}
