// custom_mm — bfloat16 / float16 forms of naive_spmm, cusparse_mmul, naive_spmm_ex, sddmm and gather_perm
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace (one translation unit; the
// split is for readers).  Not compiled on its own.
//
// The entry points of custom_mm_reference.inc / custom_mm_extras.inc hand their call here when any operand is bf16 or
// fp16 (lowp_operands); everything else keeps the fp32 path untouched.  The C-ABI (include/mi_spmm.h, low-precision
// section) sums in fp32 and rounds once at the store: C = rne_T(the fp32 product of the widened operands, long rows
// split).  No automatic row schedules here (custom_mm_reference.inc: auto_schedule*); the long-row workspace is the
// per-stream one the fp32 products use (zero header kept between products, MI_LONG_ROWS_AUTO_ZEROED).

bool is_lowp(const torch::Tensor& t) {
  return t.scalar_type() == torch::kBFloat16 || t.scalar_type() == torch::kHalf;
}

bool lowp_operands(std::initializer_list<const torch::Tensor*> ts) {
  for (const torch::Tensor* t : ts)
    if (is_lowp(*t)) return true;
  return false;
}

// One dtype for every value operand (checked first, so that mixed dtypes are named even for host tensors), then the
// device: no CPU path.
void check_lowp_operands(const char* what, std::initializer_list<std::pair<const char*, const torch::Tensor*>> ts) {
  const auto& first = *ts.begin();
  for (const auto& nt : ts)
    TORCH_CHECK(nt.second->scalar_type() == first.second->scalar_type(), what, ": ", first.first, " is ",
                first.second->scalar_type(), " but ", nt.first, " is ", nt.second->scalar_type(),
                ": all operands must share one dtype (float32, bfloat16 or float16)");
  for (const auto& nt : ts)
    TORCH_CHECK(nt.second->is_cuda(), nt.first, " must be a device (HIP) tensor; custom_mm has no CPU path");
}

const uint16_t* b16_ptr(const torch::Tensor& t) { return static_cast<const uint16_t*>(t.data_ptr()); }
uint16_t* b16_mut(torch::Tensor& t) { return static_cast<uint16_t*>(t.data_ptr()); }

torch::Tensor spmm_lowp(const torch::Tensor& A_values, const torch::Tensor& A_columns, const torch::Tensor& A_offsets,
                        int64_t nnzA, int64_t A_rows, int64_t A_cols, const torch::Tensor& B, torch::Tensor C,
                        const char* what, int long_rows) {
  check_lowp_operands(what, {{"A_values", &A_values}, {"B", &B}, {"C", &C}});
  check_device_i32(A_columns, "A_columns");
  check_device_i32(A_offsets, "A_offsets");
  check_same_device(A_values, C, what);
  check_same_device(A_columns, C, what);
  check_same_device(A_offsets, C, what);
  check_same_device(B, C, what);
  TORCH_CHECK(A_rows >= 0 && A_cols >= 0 && nnzA >= 0, what, ": negative size");
  TORCH_CHECK(A_rows <= INT32_MAX && A_cols <= INT32_MAX, what, ": dimension too large");
  TORCH_CHECK(A_values.is_contiguous() && A_columns.is_contiguous() && A_offsets.is_contiguous(), what,
              ": CSR arrays must be contiguous");
  TORCH_CHECK(A_values.numel() >= nnzA && A_columns.numel() >= nnzA, what, ": nnzA exceeds the CSR arrays");
  TORCH_CHECK(A_offsets.numel() == A_rows + 1, what, ": A_offsets must have A_rows + 1 entries");
  TORCH_CHECK(B.dim() == 2 && C.dim() == 2, what, ": B and C must be 2-d");
  TORCH_CHECK(B.size(0) == A_cols, what, ": B must have A_cols = ", A_cols, " rows, got ", B.size(0));
  TORCH_CHECK(C.size(0) == A_rows && C.size(1) == B.size(1), what, ": C must be ", A_rows, "x", B.size(1));
  TORCH_CHECK(C.is_contiguous(), what, ": C must be contiguous");
  // row-major with any leading dimension (column-offset views included) is taken as it is
  torch::Tensor Bc = (B.stride(1) == 1 || B.size(1) == 1) && (B.stride(0) >= B.size(1) || B.size(0) <= 1) ? B : B.contiguous();
  const int64_t N = B.size(1);
  TORCH_CHECK(N <= INT32_MAX, what, ": dimension too large");
  const int64_t ldb = Bc.size(0) > 1 ? Bc.stride(0) : std::max<int64_t>(N, 1);
  c10::hip::HIPGuard guard(C.device().index());
  const mi_stream_t stream = stream_of(C);
  // a workspace only where a row may be split (N < 4 keeps the narrow order: never split)
  const bool may_split = long_rows != MI_LONG_ROWS_NONE && N >= 4 && nnzA > mi_spmm_long_row_threshold();
  const size_t ws_bytes = may_split ? mi_spmm_csr_workspace_bytes(nnzA, (int32_t)N) : 0;
  torch::Tensor ws;
  int mode = long_rows;
  if (ws_bytes > 0) {
    if (long_rows == MI_LONG_ROWS_AUTO && !stream_is_capturing(stream)) {
      ws = zeroed_stream_workspace(C.device(), stream, ws_bytes);  // shared with the fp32 products on this stream
      mode = MI_LONG_ROWS_AUTO_ZEROED;
    } else {
      ws = torch::empty({(int64_t)ws_bytes}, torch::dtype(torch::kUInt8).device(C.device()));
    }
  }
  const auto entry = A_values.scalar_type() == torch::kBFloat16 ? mi_spmm_csr_ex_bf16 : mi_spmm_csr_ex_f16;
  const int st = entry(A_offsets.data_ptr<int32_t>(), A_columns.data_ptr<int32_t>(), b16_ptr(A_values), nnzA,
                       (int32_t)A_rows, (int32_t)A_cols, (int32_t)N, b16_ptr(Bc), ldb, b16_mut(C), std::max<int64_t>(N, 1),
                       mode, ws.defined() ? ws.data_ptr() : nullptr, ws.defined() ? (size_t)ws.numel() : 0, stream);
  if (st != MI_OK && mode == MI_LONG_ROWS_AUTO_ZEROED) drop_stream_workspace(C.device(), stream);  // its header may be dirty
  check_status(st, what);
  return C;
}

torch::Tensor sddmm_lowp(const torch::Tensor& A_columns, const torch::Tensor& A_offsets, int64_t nnzA, int64_t A_rows,
                         int64_t A_cols, const torch::Tensor& dC, const torch::Tensor& B) {
  const char* what = "sddmm";
  check_lowp_operands(what, {{"dC", &dC}, {"B", &B}});
  check_device_i32(A_columns, "A_columns");
  check_device_i32(A_offsets, "A_offsets");
  check_same_device(A_columns, dC, what);
  check_same_device(A_offsets, dC, what);
  check_same_device(B, dC, what);
  TORCH_CHECK(A_columns.is_contiguous() && A_offsets.is_contiguous(), what, ": CSR arrays must be contiguous");
  TORCH_CHECK(A_offsets.numel() == A_rows + 1 && A_columns.numel() >= nnzA, what, ": CSR array sizes do not match");
  TORCH_CHECK(dC.dim() == 2 && B.dim() == 2 && dC.size(0) == A_rows && B.size(0) == A_cols && dC.size(1) == B.size(1),
              what, ": dC must be [A_rows, N] and B [A_cols, N]");
  TORCH_CHECK(A_rows <= INT32_MAX && A_cols <= INT32_MAX && B.size(1) <= INT32_MAX, what, ": dimension too large");
  torch::Tensor dCc = dC.contiguous(), Bc = B.contiguous();
  const int64_t N = Bc.size(1);
  c10::hip::HIPGuard guard(dC.device().index());
  torch::Tensor out = torch::empty({nnzA}, dCc.options());
  const auto entry = dC.scalar_type() == torch::kBFloat16 ? mi_sddmm_csr_bf16 : mi_sddmm_csr_f16;
  check_status(entry(A_offsets.data_ptr<int32_t>(), A_columns.data_ptr<int32_t>(), nnzA, (int32_t)A_rows, (int32_t)A_cols,
                     (int32_t)N, b16_ptr(dCc), std::max<int64_t>(N, 1), b16_ptr(Bc), std::max<int64_t>(N, 1), b16_mut(out),
                     stream_of(dCc)),
               what);
  return out;
}

torch::Tensor gather_perm_lowp(const torch::Tensor& values, const torch::Tensor& perm) {
  TORCH_CHECK(values.is_cuda(), "values must be a device (HIP) tensor; custom_mm has no CPU path");
  check_device_i32(perm, "perm");
  check_same_device(values, perm, "gather_perm");
  TORCH_CHECK(values.dim() == 1 && perm.dim() == 1 && values.is_contiguous() && perm.is_contiguous(),
              "gather_perm: expected contiguous 1-d tensors");
  c10::hip::HIPGuard guard(values.device().index());
  torch::Tensor out = torch::empty({perm.numel()}, values.options());
  check_status(mi_gather_b16(b16_ptr(values), perm.data_ptr<int32_t>(), perm.numel(), b16_mut(out), stream_of(values)),
               "gather_perm");
  return out;
}
