// custom_mm — the block-sparse linear layer on the matrix cores: Y = X·Wᵀ (+ bias) and dX = dY·W over a CSR block list of
// the weight, and the weight gradient on the kept blocks.  Part of the `custom_mm` extension: included by custom_mm.cpp
// inside its anonymous namespace (one translation unit; the split is for readers).  Not compiled on its own.  Contract:
// include/mi_spmm.h, "Block-sparse linear layer": every value operand in bfloat16 or every one in float16; offsets,
// columns, entry ids and entry rows int32; values [n, 64, 64] contiguous; the token operands [T, width] 2-d, taken with
// their own leading dimension where they are row-major views (a column-offset view included), copied otherwise.

// a [T, width] operand as pointer + leading dimension; `keep` owns what is pointed to
struct BsrTokens {
  torch::Tensor keep;
  int64_t ld;
  uint16_t* ptr() const { return static_cast<uint16_t*>(keep.data_ptr()); }
};

BsrTokens bsr_tokens(const char* what, const char* name, const torch::Tensor& t, int64_t tokens, int64_t width) {
  TORCH_CHECK(t.dim() == 2 && t.size(0) == tokens && t.size(1) == width, what, ": ", name, " must be [", tokens, ", ", width,
              "], got ", t.sizes());
  const bool row_major = (t.stride(1) == 1 || width <= 1) && (tokens <= 1 || t.stride(0) >= ld1(width));
  torch::Tensor x = row_major ? t : t.contiguous();
  return {x, tokens > 1 ? x.stride(0) : ld1(width)};
}

// Y[:, 64·P …] = Σ over the entries of list row P of X[:, 64·columns[p] …] · op(values[entry_ids[p]])ᵀ (+ bias): offsets
// [Y columns / 64 + 1] and columns [nnz] list, per 64-column block of Y, the 64-column blocks of X it sums over.
// trans_w False: the block rows of W and their block columns (the forward); True: the transposed lists, every block used
// transposed (dX = dY·W, X being dY).  Y [T, outer] row-major, written in place.
torch::Tensor bsr_linear(torch::Tensor offsets, torch::Tensor columns, c10::optional<torch::Tensor> entry_ids, int64_t nnz,
                         torch::Tensor values, torch::Tensor X, c10::optional<torch::Tensor> bias, torch::Tensor Y, bool trans_w) {
  const char* what = "bsr_linear";
  const bool has_bias = bias.has_value() && bias->defined();
  const torch::ScalarType dt = has_bias ? value_dtype(what, {{"values", &values}, {"X", &X}, {"Y", &Y}, {"bias", &*bias}}, true)
                                        : value_dtype(what, {{"values", &values}, {"X", &X}, {"Y", &Y}}, true);
  TORCH_CHECK(is_lowp(dt), what, ": values must be bfloat16 or float16, got ", dt);
  TORCH_CHECK(X.dim() == 2 && Y.dim() == 2 && X.size(0) == Y.size(0), what, ": X must be [T, inner] and Y [T, outer]");
  const int64_t tokens = Y.size(0), outer = Y.size(1), inner = X.size(1);
  TORCH_CHECK(outer % 64 == 0 && inner % 64 == 0, what, ": the columns of Y and of X must be multiples of 64, got ", outer, " and ",
              inner);
  const Csr list = csr_arrays(what, nullptr, &columns, offsets, nnz, outer / 64, inner / 64, c10::nullopt, nullptr,
                              {"values", "columns", "offsets"});
  check_same_device(what, list.device, {&values, &X, &Y});
  const int32_t* ids = entry_ids_of(what, entry_ids, nnz, list.device);
  check_bsr_values(what, "values", values);
  TORCH_CHECK(ids != nullptr || values.size(0) >= nnz, what, ": values holds ", values.size(0), " blocks for ", nnz, " entries");
  torch::Tensor b;
  if (has_bias) {
    check_same_device(what, list.device, {&*bias});
    TORCH_CHECK(bias->dim() == 1 && bias->size(0) == outer, what, ": bias must have ", outer, " entries");
    b = bias->contiguous();
  }
  const BsrTokens x = bsr_tokens(what, "X", X, tokens, inner);
  const BsrTokens y = bsr_tokens(what, "Y", Y, tokens, outer);
  TORCH_CHECK(y.keep.is_same(Y), what, ": Y must be a row-major [T, outer] tensor (it is written in place)");
  check_sizes(what, {tokens, inner, outer, values.size(0)}, nnz);
  c10::hip::HIPGuard guard(Y.device().index());
  const int st = (dt == torch::kBFloat16 ? mi_bsr_linear_bf16 : mi_bsr_linear_f16)(
      list.offsets, list.columns, ids, nnz, trans_w ? 1 : 0, (int32_t)tokens, (int32_t)inner, (int32_t)outer,
      static_cast<const uint16_t*>(values.data_ptr()), values.size(0), x.ptr(), x.ld, b16_or_null(b), y.ptr(), y.ld, stream_of(Y));
  check_status(st, what);
  return Y;
}

int64_t bsr_wgrad_split_count(int64_t nnz, int64_t tokens) {
  check_sizes("bsr_wgrad_split_count", {tokens}, nnz);
  return mi_bsr_wgrad_split_count(nnz, tokens);
}

// the token tile (64 or 128) bsr_linear launches for Y [tokens, outer]: shape only
int64_t bsr_linear_tile_tokens(int64_t outer, int64_t tokens) {
  check_sizes("bsr_linear_tile_tokens", {outer, tokens});
  return mi_bsr_linear_tile_tokens((int32_t)outer, (int32_t)tokens);
}

// dvalues[entry_ids[p]] (None: dvalues[p]) = dY[:, 64·entry_row[p] …]ᵀ · X[:, 64·columns[p] …], the tokens cut into `splits`
// ranges (0: the rule of bsr_wgrad_split_count); the fp32 workspace of a split lives until the stream has used it (the
// caching allocator's stream order).
torch::Tensor bsr_wgrad(torch::Tensor entry_row, torch::Tensor columns, c10::optional<torch::Tensor> entry_ids, int64_t nnz,
                        torch::Tensor dY, torch::Tensor X, torch::Tensor dvalues, int64_t splits) {
  const char* what = "bsr_wgrad";
  const torch::ScalarType dt = value_dtype(what, {{"dY", &dY}, {"X", &X}, {"dvalues", &dvalues}}, true);
  TORCH_CHECK(is_lowp(dt), what, ": dY must be bfloat16 or float16, got ", dt);
  TORCH_CHECK(dY.dim() == 2 && X.dim() == 2 && dY.size(0) == X.size(0), what, ": dY must be [T, out] and X [T, in]");
  const int64_t tokens = dY.size(0), out = dY.size(1), in = X.size(1);
  TORCH_CHECK(out % 64 == 0 && in % 64 == 0, what, ": the columns of dY and of X must be multiples of 64, got ", out, " and ", in);
  check_device_i32(entry_row, "entry_row");
  check_device_i32(columns, "columns");
  const torch::Device dev = entry_row.device();
  check_same_device(what, dev, {&columns, &dY, &X, &dvalues});
  TORCH_CHECK(entry_row.is_contiguous() && columns.is_contiguous() && entry_row.numel() >= nnz && columns.numel() >= nnz, what,
              ": entry_row and columns must be contiguous int32 tensors of nnz entries");
  const int32_t* ids = entry_ids_of(what, entry_ids, nnz, dev);
  check_bsr_values(what, "dvalues", dvalues);
  TORCH_CHECK(ids != nullptr || dvalues.size(0) >= nnz, what, ": dvalues holds ", dvalues.size(0), " blocks for ", nnz, " entries");
  check_sizes(what, {tokens, out, in, dvalues.size(0), splits}, nnz);
  const BsrTokens g = bsr_tokens(what, "dY", dY, tokens, out);
  const BsrTokens x = bsr_tokens(what, "X", X, tokens, in);
  const int32_t S = splits > 0 ? (int32_t)splits : mi_bsr_wgrad_split_count(nnz, tokens);
  c10::hip::HIPGuard guard(dvalues.device().index());
  const size_t bytes = mi_bsr_wgrad_workspace_bytes(nnz, S);
  torch::Tensor ws = bytes > 0 ? byte_workspace(dev, bytes) : torch::Tensor();
  const int st = (dt == torch::kBFloat16 ? mi_bsr_wgrad_bf16 : mi_bsr_wgrad_f16)(
      entry_row.data_ptr<int32_t>(), columns.data_ptr<int32_t>(), ids, nnz, (int32_t)tokens, (int32_t)out, (int32_t)in, g.ptr(), g.ld,
      x.ptr(), x.ld, static_cast<uint16_t*>(dvalues.data_ptr()), dvalues.size(0), S, ws.defined() ? ws.data_ptr() : nullptr, bytes,
      stream_of(dvalues));
  check_status(st, what);
  return dvalues;
}
