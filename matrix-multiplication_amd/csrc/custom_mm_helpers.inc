// custom_mm — argument checks, operand descriptors, stream helpers, the dense-product body
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace (one translation unit; the
// split is for readers).  Not compiled on its own.

void check_status(int st, const char* what) {
  if (st == MI_OK) return;
  if (st == MI_EHIP)
    TORCH_CHECK(false, what, ": HIP error: ", mi_last_hip_error_string());
  if (st == MI_EINVAL) throw std::invalid_argument(std::string(what) + ": " + mi_status_string(st));
  TORCH_CHECK(false, what, ": ", mi_status_string(st));
}

void check_device_f32(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a device (HIP) tensor; custom_mm has no CPU path");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be float32, got ", t.scalar_type());
}

void check_device_i32(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a device (HIP) tensor; custom_mm has no CPU path");
  TORCH_CHECK(t.scalar_type() == torch::kInt32, name, " must be int32, got ", t.scalar_type());
}

void check_same_device(const char* what, const torch::Device& dev, std::initializer_list<const torch::Tensor*> ts) {
  for (const torch::Tensor* t : ts)
    TORCH_CHECK(t->device() == dev, what, ": tensors are on different devices (", t->device(), " vs ", dev, ")");
}

// Sizes the C-ABI takes as int32_t; nnz (an int64_t there) only has to be non-negative.
void check_sizes(const char* what, std::initializer_list<int64_t> int32_sizes, int64_t nnz = 0) {
  bool negative = nnz < 0, too_large = false;
  for (const int64_t v : int32_sizes) {
    negative = negative || v < 0;
    too_large = too_large || v > INT32_MAX;
  }
  TORCH_CHECK(!negative, what, ": negative size");
  TORCH_CHECK(!too_large, what, ": dimension too large for the int32 sizes of the C-ABI");
}

int64_t ld1(int64_t n) { return std::max<int64_t>(n, 1); }

bool is_lowp(torch::ScalarType t) { return t == torch::kBFloat16 || t == torch::kHalf; }

// The dtype of an entry point's value operands: one dtype for all of them (checked first, so that mixed dtypes are named
// even for host tensors), then the device (no CPU path), then the dtype itself — float32, or with `lowp` also bfloat16 /
// float16.
using Named = std::pair<const char*, const torch::Tensor*>;
torch::ScalarType value_dtype(const char* what, std::initializer_list<Named> ts, bool lowp = false) {
  const Named& first = *ts.begin();
  const torch::ScalarType dt = first.second->scalar_type();
  for (const Named& nt : ts)
    TORCH_CHECK(nt.second->scalar_type() == dt, what, ": ", first.first, " is ", dt, " but ", nt.first, " is ",
                nt.second->scalar_type(), ": all operands must share one dtype (",
                lowp ? "float32, bfloat16 or float16" : "float32", ")");
  for (const Named& nt : ts)
    TORCH_CHECK(nt.second->is_cuda(), nt.first, " must be a device (HIP) tensor; custom_mm has no CPU path");
  TORCH_CHECK(dt == torch::kFloat32 || (lowp && is_lowp(dt)), first.first, " must be float32",
              lowp ? ", bfloat16 or float16" : "", ", got ", dt);
  return dt;
}

// A CSR matrix (or, given `batch`, that many: offsets [batch, rows + 1], global over the batch) as the C-ABI takes it:
// pointers, int32 sizes, the device.  `values` may be null (a pattern) and has passed value_dtype; `columns` may be null
// where the callee reads the offsets only; `perm` (int32) indexes the values.  One check order, one set of messages.
struct CsrNames {
  const char *values = "A_values", *columns = "A_columns", *offsets = "A_offsets";
};
struct Csr {
  const int32_t* offsets;
  const int32_t* columns;
  const void* values;
  const int32_t* perm;
  int64_t nnz;
  int32_t rows, cols, batch;
  torch::Device device;
  const float* f32() const { return static_cast<const float*>(values); }
  const uint16_t* b16() const { return static_cast<const uint16_t*>(values); }
};
Csr csr_arrays(const char* what, const torch::Tensor* values, const torch::Tensor* columns, const torch::Tensor& offsets,
               int64_t nnz, int64_t rows, int64_t cols, c10::optional<int64_t> batch = c10::nullopt,
               const torch::Tensor* perm = nullptr,
               const CsrNames& names = CsrNames()) {
  if (columns != nullptr) check_device_i32(*columns, names.columns);
  check_device_i32(offsets, names.offsets);
  if (perm != nullptr) check_device_i32(*perm, "perm");
  const torch::Device dev = offsets.device();
  for (const torch::Tensor* t : {values, columns, perm})
    if (t != nullptr) check_same_device(what, dev, {t});
  check_sizes(what, {rows, cols, batch.value_or(0)}, nnz);
  bool contiguous = offsets.is_contiguous(), holds_nnz = true;
  for (const torch::Tensor* t : {values, columns, perm})
    if (t != nullptr) {
      contiguous = contiguous && t->is_contiguous();
      holds_nnz = holds_nnz && t->numel() >= nnz;
    }
  TORCH_CHECK(contiguous, what, ": CSR arrays must be contiguous");
  TORCH_CHECK(holds_nnz, what, ": nnzA exceeds the CSR arrays");
  const int64_t entries = batch.value_or(1) * (rows + 1);
  TORCH_CHECK(offsets.numel() == entries, what, ": ", names.offsets, " must have ", batch ? "batch · " : "",
              "(A_rows + 1) = ", entries, " entries, got ", offsets.numel());
  return Csr{offsets.data_ptr<int32_t>(), columns != nullptr ? columns->data_ptr<int32_t>() : nullptr,
             values != nullptr ? values->data_ptr() : nullptr, perm != nullptr ? perm->data_ptr<int32_t>() : nullptr,
             nnz, (int32_t)rows, (int32_t)cols, (int32_t)batch.value_or(1), dev};
}

// B [K, N] of a row-major product: a row-major view with any leading dimension (column-offset views included) is taken
// as it is, anything else copied.
struct RowMajorB {
  torch::Tensor keep;
  int64_t ld;
};
RowMajorB row_major_b(const torch::Tensor& B) {
  const int64_t N = B.size(1);
  torch::Tensor Bc = (B.stride(1) == 1 || N == 1) && (B.stride(0) >= N || B.size(0) <= 1) ? B : B.contiguous();
  return {Bc, Bc.size(0) > 1 ? Bc.stride(0) : ld1(N)};
}

// B of a batched product: [batch, K, N] (one per item) or [K, N] (shared by every item), contiguous, and its item stride.
std::pair<torch::Tensor, int64_t> batched_b(const char* what, const torch::Tensor& B, int64_t batch, int64_t K, int64_t N) {
  if (B.dim() == 3) {
    TORCH_CHECK(B.size(0) == batch && B.size(1) == K && B.size(2) == N, what, ": B must be [batch, A_cols, N]");
    return {B.contiguous(), K * N};
  }
  TORCH_CHECK(B.dim() == 2 && B.size(0) == K && B.size(1) == N, what, ": B must be [A_cols, N]");
  return {B.contiguous(), 0};
}

// The bias [N] of a fused epilogue, contiguous (undefined when there is none): float32, or — where the entry's operands
// are bfloat16 / float16 (`dt`, the dense epilogue only) — of the operands' dtype.
torch::Tensor bias_of(const char* what, const torch::Tensor* bias, int64_t N, const torch::Tensor& C,
                      torch::ScalarType dt = torch::kFloat32) {
  if (bias == nullptr || !bias->defined()) return torch::Tensor();
  if (is_lowp(dt)) {
    TORCH_CHECK(bias->scalar_type() == dt, what, ": C is ", dt, " but bias is ", bias->scalar_type(),
                ": the bias must share the operands' dtype");
    TORCH_CHECK(bias->is_cuda(), "bias must be a device (HIP) tensor; custom_mm has no CPU path");
  } else {
    check_device_f32(*bias, "bias");
  }
  check_same_device(what, C.device(), {bias});
  TORCH_CHECK(bias->dim() == 1 && bias->size(0) == N, what, ": bias must have ", N, " entries");
  return bias->contiguous();
}
const float* f32_or_null(const torch::Tensor& t) { return t.defined() ? t.data_ptr<float>() : nullptr; }
const uint16_t* b16_or_null(const torch::Tensor& t) { return t.defined() ? static_cast<const uint16_t*>(t.data_ptr()) : nullptr; }

// A device byte buffer of at least `min_bytes` (C-ABI workspaces; some entries want a non-null pointer even for 0 bytes).
torch::Tensor byte_workspace(const torch::Device& dev, size_t bytes, size_t min_bytes = 0) {
  return torch::empty({(int64_t)std::max(bytes, min_bytes)}, torch::dtype(torch::kUInt8).device(dev));
}

mi_stream_t stream_of(const torch::Tensor& t) {
  return static_cast<mi_stream_t>(c10::hip::getCurrentHIPStream(t.device().index()).stream());
}

// A dense operand as the C-ABI wants it: pointer (of the tensor's own dtype), leading dimension, batch
// stride, and whether the stored matrix is the transpose of the logical one.
struct Operand {
  torch::Tensor keep;  // owns the memory for the duration of the call
  const void* ptr;
  int64_t ld;
  int64_t batch_stride;
  bool stored_transposed;
  int64_t rows, cols;  // logical (before `stored_transposed`)
};

// View the last two dims of `t` (after flattening the leading `nbatch` dims to
// one) as row-major-with-ld, or as a transposed row-major matrix; copy only
// when the strides fit neither.
Operand as_operand(const torch::Tensor& t, int nbatch_dims) {
  Operand o;
  const int64_t d = t.dim();
  TORCH_CHECK(d == nbatch_dims + 2, "expected a ", nbatch_dims + 2, "-d tensor, got ", d, "-d");
  o.rows = t.size(d - 2);
  o.cols = t.size(d - 1);
  // Leading dims must flatten to ONE batch stride (nbatch_dims ≤ 2 here).
  auto batch_stride_of = [&](const torch::Tensor& y, int64_t& stride) {
    stride = 0;
    if (nbatch_dims == 0) return true;
    if (nbatch_dims == 1) {
      stride = y.size(0) > 1 ? y.stride(0) : 0;
      return stride >= 0;
    }
    const int64_t b0 = y.size(0), b1 = y.size(1), s0 = y.stride(0), s1 = y.stride(1);
    if (b0 <= 1) stride = b1 > 1 ? s1 : 0;
    else if (b1 <= 1) stride = s0;
    else if (s0 == s1 * b1) stride = s1;
    else return false;
    return stride >= 0;
  };
  // Row-major with a leading dimension, or the transpose of one.
  auto layout_of = [&](const torch::Tensor& y, bool& transposed, int64_t& ld) {
    const int64_t sr = y.stride(d - 2), sc = y.stride(d - 1);
    if ((sc == 1 || o.cols <= 1) && (o.rows <= 1 || sr >= std::max<int64_t>(o.cols, 1))) {
      transposed = false;
      ld = o.rows > 1 ? sr : std::max<int64_t>(o.cols, 1);
      return true;
    }
    if ((sr == 1 || o.rows <= 1) && (o.cols <= 1 || sc >= std::max<int64_t>(o.rows, 1))) {
      transposed = true;
      ld = o.cols > 1 ? sc : std::max<int64_t>(o.rows, 1);
      return true;
    }
    return false;
  };
  torch::Tensor x = t;
  bool transposed = false;
  int64_t ld = 0, bstride = 0;
  if (!layout_of(x, transposed, ld) || !batch_stride_of(x, bstride)) {
    x = t.contiguous();
    TORCH_INTERNAL_ASSERT(layout_of(x, transposed, ld) && batch_stride_of(x, bstride));
  }
  o.keep = x;
  o.ptr = x.data_ptr();
  o.stored_transposed = transposed;
  o.ld = ld;
  o.batch_stride = bstride;
  return o;
}

int64_t batch_count(const torch::Tensor& t, int nbatch_dims) {
  int64_t b = 1;
  for (int i = 0; i < nbatch_dims; ++i) b *= t.size(i);
  return b;
}

// C = op(A)·op(B) (+ bias) for `nbatch_dims` leading batch dims.  float32, or A, B, C (and the bias) all bfloat16 or all
// float16: the C-ABI's low-precision dense entries (fp32 sums, one rounding per element).
// `lowp_splits` (low precision, one product): < 0 never splits k — cublas_mmul / cublas_bmm / cublas_mmul_bias, whose bits
// do not depend on m and n; 0 splits by the rule of mi_gemm_lowp_split_count; > 0 into that many ranges.
torch::Tensor gemm_impl(const torch::Tensor& A, const torch::Tensor& B, torch::Tensor C,
                        int nbatch_dims, bool transa, bool transb, const char* what,
                        const torch::Tensor* bias = nullptr, int64_t lowp_splits = -1) {
  // (a bias beside low-precision operands is one of them: a mismatch names both dtypes, before the device check; beside
  // float32 operands it keeps the messages of bias_of, which the sparse bias entries share)
  const bool lowp_bias = bias != nullptr && bias->defined() && is_lowp(A.scalar_type());
  const torch::ScalarType dt = lowp_bias ? value_dtype(what, {{"A", &A}, {"B", &B}, {"C", &C}, {"bias", bias}}, true)
                                         : value_dtype(what, {{"A", &A}, {"B", &B}, {"C", &C}}, true);
  check_same_device(what, C.device(), {&A, &B});
  TORCH_CHECK(C.is_contiguous(), what, ": C must be contiguous");
  TORCH_CHECK(C.dim() == nbatch_dims + 2, what, ": C has the wrong rank");
  for (int i = 0; i < nbatch_dims; ++i)
    TORCH_CHECK(A.size(i) == B.size(i) && A.size(i) == C.size(i), what,
                ": batch dimensions of A, B and C differ");
  Operand a = as_operand(A, nbatch_dims);
  Operand b = as_operand(B, nbatch_dims);
  const int64_t m = transa ? a.cols : a.rows, ka = transa ? a.rows : a.cols;
  const int64_t kb = transb ? b.cols : b.rows, n = transb ? b.rows : b.cols;
  TORCH_CHECK(ka == kb, what, ": inner dimensions differ (", ka, " vs ", kb, ")");
  TORCH_CHECK(C.size(-2) == m && C.size(-1) == n, what, ": C must be ", m, "x", n, ", got ",
              C.size(-2), "x", C.size(-1));
  const int64_t batch = batch_count(C, nbatch_dims);
  check_sizes(what, {m, n, ka, batch});
  const torch::Tensor bias_keep = bias_of(what, bias, n, C, dt);
  c10::hip::HIPGuard guard(C.device().index());
  const int ta = transa != a.stored_transposed, tb = transb != b.stored_transposed;
  if (is_lowp(dt)) {
    const bool bf = dt == torch::kBFloat16;
    const uint16_t* pa = static_cast<const uint16_t*>(a.ptr);
    const uint16_t* pb = static_cast<const uint16_t*>(b.ptr);
    uint16_t* pc = static_cast<uint16_t*>(C.data_ptr());
    int st;
    if (lowp_splits >= 0) {  // one product (nbatch_dims == 0), k cut into a fixed number of ranges
      const int64_t S = lowp_splits > 0 ? lowp_splits : mi_gemm_lowp_split_count((int32_t)m, (int32_t)n, (int32_t)ka, 1);
      TORCH_CHECK(S <= 1024, what, ": at most 1024 ranges");
      const size_t ws_bytes = S > 1 ? (size_t)S * m * n * sizeof(float) : 0;
      torch::Tensor ws;
      if (ws_bytes > 0) ws = byte_workspace(C.device(), ws_bytes);
      st = (bf ? mi_gemm_split_bf16 : mi_gemm_split_f16)(ta, tb, (int32_t)m, (int32_t)n, (int32_t)ka, pa, a.ld, pb, b.ld,
                                                         b16_or_null(bias_keep), pc, ld1(n), (int32_t)S,
                                                         ws_bytes > 0 ? ws.data_ptr() : nullptr, ws_bytes, stream_of(C));
    } else if (bias_keep.defined()) {
      st = (bf ? mi_gemm_bias_bf16 : mi_gemm_bias_f16)(ta, tb, (int32_t)m, (int32_t)n, (int32_t)ka, pa, a.ld, a.batch_stride, pb,
                                                       b.ld, b.batch_stride, b16_or_null(bias_keep), pc, ld1(n), m * n,
                                                       (int32_t)batch, stream_of(C));
    } else {  // no split-k here: one kernel family, one order (include/mi_spmm.h)
      st = (bf ? mi_gemm_bf16 : mi_gemm_f16)(ta, tb, (int32_t)m, (int32_t)n, (int32_t)ka, pa, a.ld, a.batch_stride, pb, b.ld,
                                             b.batch_stride, pc, ld1(n), m * n, (int32_t)batch, stream_of(C));
    }
    check_status(st, what);
    return C;
  }
  // few output tiles and a long k: the fixed split of include/mi_spmm.h ("Deterministic split-k") needs room for its partial sums
  const size_t ws_bytes = mi_gemm_workspace_bytes((int32_t)m, (int32_t)n, (int32_t)ka, (int32_t)batch);
  torch::Tensor ws;
  if (ws_bytes > 0) ws = byte_workspace(C.device(), ws_bytes);
  const int st = mi_gemm_ws_f32(ta, tb,
                                (int32_t)m, (int32_t)n, (int32_t)ka, static_cast<const float*>(a.ptr), a.ld, a.batch_stride,
                                static_cast<const float*>(b.ptr), b.ld, b.batch_stride, f32_or_null(bias_keep), C.data_ptr<float>(),
                                ld1(n), m * n, (int32_t)batch, ws_bytes > 0 ? ws.data_ptr() : nullptr, ws_bytes,
                                stream_of(C));
  check_status(st, what);
  return C;
}
