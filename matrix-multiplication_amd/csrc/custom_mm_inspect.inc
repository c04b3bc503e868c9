// custom_mm — inspector–executor handles: cusparse_inspect / cusparse_mmul_opt / tiledspmm_* (column-major executor)
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace (one translation unit; the
// split is for readers).  Not compiled on its own.
// ---- inspector–executor registries -----------------------------------------
// What `*_inspect` amortises here (reference: TiledSpMM_inspect builds its tiled-ELL image once,
// src/sparse_mm.cu:137-368; cusparse_inspect caches descriptors, src/custom_mm.cpp:236-257):
//   * the CSR arrays, owned (tensor references) and VALIDATED once (offsets monotone, columns in range);
//   * Aᵀ in CSR — the backward product of a sparse-weight layer (`*_mmul_opt_t`) and any Aᵀ·G need it,
//     and a transpose costs about a sixth of a product at the C3 shape;
//   * the longest row of A and of Aᵀ, and — only when a row exceeds the split threshold — the prepared
//     list of long rows (MI_LONG_ROWS_PREPARED: no per-call memset + list-building launch); without
//     long rows every product is ONE kernel launch between the two operand transposes;
//   * the executor's transposed-operand buffers (no allocation per call).
// Calls on one handle must be ordered on one stream (they share those buffers), as with a cuSPARSE handle.

struct CsrSide {
  int64_t rows = 0, cols = 0;      // this side's matrix is rows × cols
  torch::Tensor rowptr, col, val;  // device, int32 / int32 / float32 — owned references
  int64_t max_row = 0;             // longest row (host-known since inspect)
  torch::Tensor long_ws;           // prepared long-row list + partial rows (defined iff max_row > threshold)
  std::shared_ptr<PySchedule> sched;  // the row schedule (include/mi_spmm.h "Row schedules"): active on degree-skewed matrices
};

struct CsrHandle {
  int64_t M = 0, K = 0, N = 0;  // A is M×K, dense width N
  int64_t nnz = 0;
  CsrSide a, at;                // A and Aᵀ
  torch::Tensor ws;             // executor workspace: Bt [K,N] | Ct [M,N] (either orientation)
};

std::mutex g_registry_mutex;
std::unordered_map<std::string, CsrHandle> g_cusparse_layers;  // cusparse_inspect / _mmul_opt
std::unordered_map<std::string, CsrHandle> g_tiled_layers;     // tiledspmm_*

int64_t longest_row(const torch::Tensor& rowptr) {
  if (rowptr.numel() < 2) return 0;
  return (rowptr.slice(0, 1) - rowptr.slice(0, 0, rowptr.numel() - 1)).max().item<int32_t>();
}

void prepare_side(CsrSide& side, int64_t nnz, int64_t N, const char* what) {
  side.max_row = longest_row(side.rowptr);
  // what an inspector is for (reference: TiledSpMM_inspect restructures A once, src/sparse_mm.cu:137-368): the order in which
  // this matrix's rows go to waves — longest first, like lengths together, heavy rows apart; inactive (and free) for a matrix
  // of short, alike rows
  if (side.rows > 1 && nnz > 0 && N > 0) side.sched = make_schedule(side.rowptr, nnz, side.rows, N, false, what, &side.col, side.cols);
  if (side.max_row > mi_spmm_long_row_threshold() && N > 0) {
    const size_t bytes = mi_spmm_csr_workspace_bytes(nnz, (int32_t)N);
    side.long_ws = byte_workspace(side.val.device(), bytes);
    check_status(mi_spmm_long_rows_prepare(side.rowptr.data_ptr<int32_t>(), (int32_t)side.rows, nnz, (int32_t)N,
                                           side.long_ws.data_ptr(), bytes, stream_of(side.val)),
                 what);
  }
}

// Shared inspector: device CSR → a complete handle.
CsrHandle build_handle(int64_t M, int64_t K, int64_t N, int64_t nnz, torch::Tensor rowptr, torch::Tensor col,
                       torch::Tensor val, const char* what) {
  value_dtype(what, {{"value", &val}});
  const Csr a = csr_arrays(what, &val, &col, rowptr, nnz, M, K, c10::nullopt, nullptr, {"value", "colindex", "displ"});
  check_sizes(what, {N});
  c10::hip::HIPGuard guard(val.device().index());
  // validate once what every later product trusts (the kernels index B with these columns)
  if (M > 0) {
    TORCH_CHECK(rowptr[0].item<int32_t>() == 0 && rowptr[M].item<int32_t>() == nnz, what,
                ": offsets must start at 0 and end at nnz");
    TORCH_CHECK((rowptr.slice(0, 1) - rowptr.slice(0, 0, M)).min().item<int32_t>() >= 0, what,
                ": offsets must not decrease");
  }
  if (nnz > 0) {
    torch::Tensor c = col.slice(0, 0, nnz);
    TORCH_CHECK(c.min().item<int32_t>() >= 0 && c.max().item<int32_t>() < K, what, ": column index out of range");
  }
  CsrHandle h;
  h.M = M;
  h.K = K;
  h.N = N;
  h.nnz = nnz;
  h.a.rows = M;
  h.a.cols = K;
  h.a.rowptr = rowptr;
  h.a.col = col.slice(0, 0, nnz);
  h.a.val = val.slice(0, 0, nnz);
  // Aᵀ
  auto iopt = torch::dtype(torch::kInt32).device(val.device());
  h.at.rows = K;
  h.at.cols = M;
  h.at.rowptr = torch::empty({K + 1}, iopt);
  h.at.col = torch::empty({nnz}, iopt);
  h.at.val = torch::empty({nnz}, val.options());
  {
    const size_t bytes = mi_csr_transpose_workspace_bytes(a.rows, a.cols, nnz);
    torch::Tensor tws = byte_workspace(a.device, bytes, 1);
    check_status(mi_csr_transpose_f32(a.offsets, a.columns, a.f32(), nnz, a.rows, a.cols, h.at.rowptr.data_ptr<int32_t>(),
                                      h.at.col.data_ptr<int32_t>(), h.at.val.data_ptr<float>(), tws.data_ptr(), bytes,
                                      stream_of(val)),
                 what);
  }
  prepare_side(h.a, nnz, N, what);
  prepare_side(h.at, nnz, N, what);
  h.ws = byte_workspace(a.device, mi_spmm_colmajor_workspace_bytes(a.rows, a.cols, (int32_t)N), 16);
  return h;
}

// Column-major executor shared by cusparse_mmul_opt and tiledspmm_mm (and their `_t` forms on Aᵀ):
// C (rows×N col-major) = S · B (cols×N col-major), S = A or Aᵀ; tensors of any shape with the
// right element count are accepted, as in the reference (raw data_ptr()).
void colmajor_mm(const CsrHandle& h, bool transposed, const torch::Tensor& B, torch::Tensor& C, const char* what) {
  const CsrSide& s = transposed ? h.at : h.a;
  value_dtype(what, {{"B", &B}, {"C", &C}});
  check_same_device(what, s.val.device(), {&B, &C});
  TORCH_CHECK(B.is_contiguous() && C.is_contiguous(), what, ": B and C must be contiguous");
  TORCH_CHECK(B.numel() == s.cols * h.N, what, ": B must hold ", s.cols * h.N, " elements, got ", B.numel());
  TORCH_CHECK(C.numel() == s.rows * h.N, what, ": C must hold ", s.rows * h.N, " elements, got ", C.numel());
  c10::hip::HIPGuard guard(C.device().index());
  const size_t ws_bytes = mi_spmm_colmajor_workspace_bytes((int32_t)s.rows, (int32_t)s.cols, (int32_t)h.N);
  TORCH_INTERNAL_ASSERT((size_t)h.ws.numel() >= ws_bytes);
  // the same summation rule as cusparse_mmul / naive_spmm on this matrix: long rows are split iff the
  // AUTO plan of the (row-major) product would split them — with the list prepared at inspect time
  int mode = MI_LONG_ROWS_NONE;
  if (s.long_ws.defined()) {
    const float* bt = static_cast<const float*>(h.ws.data_ptr());
    if (mi_spmm_auto_splits_long_rows(h.nnz, (int32_t)s.rows, (int32_t)s.cols, (int32_t)h.N, bt, h.N, bt, h.N) == 1)
      mode = MI_LONG_ROWS_PREPARED;
  }
  const int st = mi_spmm_csr_colmajor_sched_f32(
      s.sched ? s.sched->sc : nullptr, s.rowptr.data_ptr<int32_t>(), s.col.data_ptr<int32_t>(), s.val.data_ptr<float>(), h.nnz, (int32_t)s.rows,
      (int32_t)s.cols, (int32_t)h.N, B.data_ptr<float>(), s.cols, C.data_ptr<float>(), s.rows, mode,
      mode == MI_LONG_ROWS_NONE ? nullptr : s.long_ws.data_ptr(), mode == MI_LONG_ROWS_NONE ? 0 : (size_t)s.long_ws.numel(),
      h.ws.data_ptr(), (size_t)h.ws.numel(), stream_of(C));
  check_status(st, what);
}

const CsrHandle& lookup(const std::unordered_map<std::string, CsrHandle>& reg,
                        const std::string& layer, const char* what) {
  auto it = reg.find(layer);
  if (it == reg.end()) throw std::runtime_error(std::string(what) + ": Invalid handle_id! (unknown layer '" + layer + "')");
  return it->second;
}

// reference custom_mm.cpp:236-257: (displ, colindex, value, nnz, M, N, K, layer);
// A is M×K, dense operand width N (custom_mm.cpp:266-267 passes M, K, then K, N).
void cusparse_inspect(torch::Tensor displ, torch::Tensor colindex, torch::Tensor value, int nnz,
                      int M, int N, int K, std::string layer) {
  CsrHandle h = build_handle(M, K, N, nnz, displ.contiguous(), colindex.contiguous(), value.contiguous(), "cusparse_inspect");
  std::lock_guard<std::mutex> lock(g_registry_mutex);
  g_cusparse_layers[layer] = std::move(h);
}

torch::Tensor cusparse_mmul_opt(torch::Tensor B, torch::Tensor C, std::string layer) {
  CsrHandle h;
  {
    std::lock_guard<std::mutex> lock(g_registry_mutex);
    h = lookup(g_cusparse_layers, layer, "cusparse_mmul_opt");
  }
  colmajor_mm(h, false, B, C, "cusparse_mmul_opt");
  return C;
}

// Addition: C (K×N col-major) = Aᵀ · B (M×N col-major) with the Aᵀ cached by cusparse_inspect — the
// input gradient of a sparse-weight layer (Y = X·Aᵀ  ⇒  dX = dY·A, i.e. dXᵀ = Aᵀ·dYᵀ).
torch::Tensor cusparse_mmul_opt_t(torch::Tensor B, torch::Tensor C, std::string layer) {
  CsrHandle h;
  {
    std::lock_guard<std::mutex> lock(g_registry_mutex);
    h = lookup(g_cusparse_layers, layer, "cusparse_mmul_opt_t");
  }
  colmajor_mm(h, true, B, C, "cusparse_mmul_opt_t");
  return C;
}

// What a handle holds (tests / diagnostics): sizes, longest rows, whether long-row lists were prepared.
pybind11::dict inspect_info(const std::string& layer, bool tiled) {
  CsrHandle h;
  {
    std::lock_guard<std::mutex> lock(g_registry_mutex);
    h = lookup(tiled ? g_tiled_layers : g_cusparse_layers, layer, "inspect_info");
  }
  pybind11::dict d;
  d["M"] = h.M;
  d["K"] = h.K;
  d["N"] = h.N;
  d["nnz"] = h.nnz;
  d["max_row"] = h.a.max_row;
  d["max_row_transposed"] = h.at.max_row;
  d["long_rows_prepared"] = h.a.long_ws.defined();
  d["schedule_active"] = h.a.sched ? py::cast<bool>(h.a.sched->info()["active"]) : false;
  d["schedule_active_transposed"] = h.at.sched ? py::cast<bool>(h.at.sched->info()["active"]) : false;
  d["long_rows_prepared_transposed"] = h.at.long_ws.defined();
  d["transpose"] = std::make_tuple(h.at.val, h.at.col, h.at.rowptr);
  d["workspace_bytes"] = (int64_t)h.ws.numel();
  return d;
}

void cusparse_clean() {
  std::lock_guard<std::mutex> lock(g_registry_mutex);
  g_cusparse_layers.clear();
}

// TiledSpMM convention (reference custom_mm.cpp:283-290): C[M×K] = A[M×N]·B[N×K],
// B and C column-major.  In CsrHandle terms: inner dim = N, dense width = K.
void register_tiled(int64_t M, int64_t N, int64_t K, torch::Tensor rowptr_cpu_i32,
                    torch::Tensor col_cpu_i32, torch::Tensor val_cpu, const std::string& layer) {
  const auto dev = torch::Device(torch::kCUDA, c10::hip::current_device());
  // TiledSpMM convention: inner dimension = N, dense width = K (CsrHandle: K = inner, N = width)
  CsrHandle h = build_handle(M, /*inner=*/N, /*width=*/K, val_cpu.numel(), rowptr_cpu_i32.to(dev), col_cpu_i32.to(dev),
                             val_cpu.to(dev), "tiledspmm_inspect");
  std::lock_guard<std::mutex> lock(g_registry_mutex);
  g_tiled_layers[layer] = std::move(h);
}

void check_host(const torch::Tensor& t, torch::ScalarType ty, const char* name) {
  TORCH_CHECK(t.device().is_cpu(), name, " must be a CPU tensor (host inspector input)");
  TORCH_CHECK(t.scalar_type() == ty, name, " must be ", ty, ", got ", t.scalar_type());
}

// reference custom_mm.cpp:321-335: CSR with int64 displ / colindex on the host.
void tiledspmm_inspect_csr(int M, int N, int K, torch::Tensor displ, torch::Tensor colindex,
                           torch::Tensor value, std::string layer) {
  check_host(displ, torch::kInt64, "displ");
  check_host(colindex, torch::kInt64, "colindex");
  check_host(value, torch::kFloat32, "value");
  check_sizes("tiledspmm_inspect_csr", {M, N, K});
  TORCH_CHECK(displ.numel() == (int64_t)M + 1, "tiledspmm_inspect_csr: displ must have M + 1 entries");
  torch::Tensor d = displ.contiguous(), c = colindex.contiguous(), v = value.contiguous();
  const int64_t nnz = M > 0 ? d.data_ptr<int64_t>()[M] : 0;
  TORCH_CHECK(nnz >= 0 && nnz <= INT32_MAX, "tiledspmm_inspect_csr: nnz does not fit int32");
  TORCH_CHECK(c.numel() >= nnz && v.numel() >= nnz, "tiledspmm_inspect_csr: nnz exceeds the CSR arrays");
  if (nnz > 0) {
    TORCH_CHECK(c.slice(0, 0, nnz).min().item<int64_t>() >= 0 &&
                    c.slice(0, 0, nnz).max().item<int64_t>() < N,
                "tiledspmm_inspect_csr: column index out of range");
  }
  register_tiled(M, N, K, d.to(torch::kInt32), c.slice(0, 0, nnz).to(torch::kInt32),
                 v.slice(0, 0, nnz).contiguous(), layer);
}

// reference custom_mm.cpp:293-319: COO with int32 indices on the host, sorted by row.
void tiledspmm_inspect_coo(int M, int N, int K, int64_t nnz, torch::Tensor rowidx,
                           torch::Tensor colidx, torch::Tensor value, std::string layer) {
  check_host(rowidx, torch::kInt32, "rowidx");
  check_host(colidx, torch::kInt32, "colidx");
  check_host(value, torch::kFloat32, "value");
  check_sizes("tiledspmm_inspect_coo", {M, N, K}, nnz);
  TORCH_CHECK(rowidx.numel() >= nnz && colidx.numel() >= nnz && value.numel() >= nnz,
              "tiledspmm_inspect_coo: nnz exceeds the COO arrays");
  torch::Tensor r = rowidx.contiguous(), c = colidx.contiguous(), v = value.contiguous();
  if (nnz > 0) {
    TORCH_CHECK(c.slice(0, 0, nnz).min().item<int32_t>() >= 0 &&
                    c.slice(0, 0, nnz).max().item<int32_t>() < N,
                "tiledspmm_inspect_coo: column index out of range");
  }
  torch::Tensor rowptr = torch::empty({(int64_t)M + 1}, torch::kInt32);
  torch::Tensor col = torch::empty({nnz}, torch::kInt32);
  torch::Tensor val = torch::empty({nnz}, torch::kFloat32);
  int st;
  {
    pybind11::gil_scoped_release nogil;  // host inspector pass
    st = mi_coo_to_csr_host(M, nnz, r.data_ptr<int32_t>(), c.data_ptr<int32_t>(), v.data_ptr<float>(),
                            rowptr.data_ptr<int32_t>(), col.data_ptr<int32_t>(), val.data_ptr<float>());
  }
  check_status(st, "tiledspmm_inspect_coo");
  register_tiled(M, N, K, rowptr, col, val, layer);
}

void tiledspmm_mm(torch::Tensor B, torch::Tensor C, std::string layer) {
  CsrHandle h;
  {
    std::lock_guard<std::mutex> lock(g_registry_mutex);
    h = lookup(g_tiled_layers, layer, "tiledspmm_mm");
  }
  colmajor_mm(h, false, B, C, "tiledspmm_mm");
}

void tiledspmm_mm_t(torch::Tensor B, torch::Tensor C, std::string layer) {
  CsrHandle h;
  {
    std::lock_guard<std::mutex> lock(g_registry_mutex);
    h = lookup(g_tiled_layers, layer, "tiledspmm_mm_t");
  }
  colmajor_mm(h, true, B, C, "tiledspmm_mm_t");
}

void tiledspmm_clean() {
  std::lock_guard<std::mutex> lock(g_registry_mutex);
  g_tiled_layers.clear();
}
