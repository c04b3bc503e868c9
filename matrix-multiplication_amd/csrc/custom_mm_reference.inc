// custom_mm — the reference's row-major entry points: cublas_mmul / cublas_bmm, naive_spmm / cusparse_mmul (+ bias / long-row forms)
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace (one translation unit; the
// split is for readers).  Not compiled on its own.
// ---- cuBLAS-named entry points (reference custom_mm.cpp:104-164) ------------

torch::Tensor cublas_mmul(torch::Tensor A, torch::Tensor B, torch::Tensor C, bool transa,
                          bool transb) {
  return gemm_impl(A, B, C, 0, transa, transb, "cublas_mmul");
}

torch::Tensor cublas_bmm(torch::Tensor A, torch::Tensor B, torch::Tensor C, int dim, bool transa,
                         bool transb) {
  if (dim == 3) return gemm_impl(A, B, C, 1, transa, transb, "cublas_bmm");
  if (dim == 4) return gemm_impl(A, B, C, 2, transa, transb, "cublas_bmm");
  if (dim == 2) return cublas_mmul(A, B, C, transa, transb);
  throw std::invalid_argument("Invalid dim argument.");  // reference custom_mm.cpp:162
}

// ---- CSR × dense, row-major (reference custom_mm.cpp:166-179, :203-217) -----

// One long-row workspace per (device, stream), reused by every plain naive_spmm / cusparse_mmul on that stream
// (products on one stream are ordered, so they can share it).  Invariant (MI_LONG_ROWS_AUTO_ZEROED, include/mi_spmm.h):
// its first 16 bytes are zero whenever no product is in flight — zeroed once here, restored by each product's
// follow-up kernel.  Not used under stream capture (the buffer would belong to the graph's pool).
struct StreamWorkspace {
  torch::Tensor buf;
};
std::mutex g_stream_ws_mutex;
std::map<std::pair<int, mi_stream_t>, StreamWorkspace> g_stream_ws;

bool stream_is_capturing(mi_stream_t stream) {
  hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(static_cast<hipStream_t>(stream), &status) != hipSuccess) {
    (void)hipGetLastError();
    return true;  // be conservative: the per-call path is always valid
  }
  return status != hipStreamCaptureStatusNone;
}

torch::Tensor zeroed_stream_workspace(const torch::Device& dev, mi_stream_t stream, size_t bytes) {
  std::lock_guard<std::mutex> lock(g_stream_ws_mutex);
  const auto key = std::make_pair((int)dev.index(), stream);
  if (g_stream_ws.size() >= 64 && g_stream_ws.find(key) == g_stream_ws.end())
    g_stream_ws.clear();  // a program that keeps creating streams: start over (the allocator keeps freed blocks stream-ordered)
  StreamWorkspace& w = g_stream_ws[key];
  if (!w.buf.defined() || (size_t)w.buf.numel() < bytes) {
    const int64_t cap = (int64_t)(bytes + bytes / 2 + 4096);
    w.buf = torch::empty({cap}, torch::dtype(torch::kUInt8).device(dev));
    w.buf.narrow(0, 0, 16).zero_();  // once per (re)allocation, on the current stream
  }
  return w.buf;
}

void drop_stream_workspace(const torch::Device& dev, mi_stream_t stream) {
  std::lock_guard<std::mutex> lock(g_stream_ws_mutex);
  g_stream_ws.erase(std::make_pair((int)dev.index(), stream));
}

// mi_spmm_schedule_info (include/mi_spmm.h) as an array
std::array<int64_t, MI_SPMM_SCHEDULE_INFO_LEN> schedule_info(const mi_spmm_schedule_t* sc, const char* what) {
  std::array<int64_t, MI_SPMM_SCHEDULE_INFO_LEN> v{};
  check_status(mi_spmm_schedule_info(sc, v.data()), what);
  return v;
}

// ---- row schedules (include/mi_spmm.h "Row schedules": the inspector's format for degree-skewed matrices) --------------------
// One per matrix (per CSR pattern): the order in which rows are handed to waves — longest first, like lengths together,
// the heavy rows in a launch of their own.  Same bits as the unscheduled entry points.  Products on one schedule must be
// ordered on one stream.
struct PySchedule {
  torch::Tensor order;  // device int32 [rows]: slot → row
  torch::Tensor order_keep;  // the buffer `order` is a view of (the class-only order and, when columns were given, the locality order)
  mi_spmm_schedule_t* sc = nullptr;
  int64_t rows = 0, nnz = 0;
  // the rows beyond the long-row threshold, listed once for the width the schedule was made for (defined iff there may be
  // such rows): a scheduled product then runs their kernel FIRST, beside its other launches, instead of last
  torch::Tensor long_ws;
  int64_t long_ws_width = -1;
  int64_t long_rows = -1;  // rows beyond the long-row threshold (counted when the list was prepared; -1: not looked at)
  ~PySchedule() { mi_spmm_schedule_destroy(sc); }
  py::dict info() const {
    const auto v = schedule_info(sc, "SpmmSchedule.info");
    py::dict d;
    d["rows"] = v[0];
    d["heavy_rows"] = v[1];
    d["heavy_length"] = v[2];
    d["classes"] = v[3];
    d["longest_at_least"] = v[4];
    d["side_stream"] = (v[5] & 1) != 0;
    d["active"] = (v[5] & 2) != 0;
    d["locality_order"] = (v[5] & 4) != 0;
    d["window_span_natural"] = v[8] < 0 ? -1.0 : v[8] / 1000.0;   // share of B's rows a window of 2048 consecutive rows touches
    d["window_span_scheduled"] = v[9] < 0 ? -1.0 : v[9] / 1000.0; // … a window of 2048 consecutive slots of this order
    d["row_span"] = v[10] < 0 ? -1.0 : v[10] / 1000.0;
    d["long_rows"] = long_rows;
    d["nnz"] = v[6];
    d["width"] = v[7];
    d["long_rows_prepared"] = long_ws.defined();
    return d;
  }
  void set_heavy(int64_t heavy_len, bool side_stream) {
    check_status(mi_spmm_schedule_set_heavy(sc, (int32_t)heavy_len, side_stream ? 1 : 0), "SpmmSchedule.set_heavy");
  }
};

// ---- automatic row schedules for the plain entry points (naive_spmm / cusparse_mmul / naive_spmm_bias) --------------------------
// The reference's API has no inspector for these calls, and its tests and benchmarks call them in loops on one matrix.  The
// extension therefore remembers the CSR arrays it has seen (device, stream, offsets pointer, columns pointer, rows, nnz): on the
// SECOND product of a key it enqueues the schedule's build behind that product (mi_spmm_schedule_begin: device kernels + copies
// of the class table and the window statistics to pinned memory, an event behind them), and the first later product that finds
// the event done finishes the schedule on the host and runs on it from then on — no synchronisation at any point, nothing under
// stream capture.  A key is loose on purpose: a stale schedule (the arrays were rewritten in place, or freed and their addresses
// handed to another matrix of the same size) is still a PERMUTATION of the rows, so it can cost time, never bits — which is also
// why no prepared long-row list is kept here (that would be a correctness risk).  Inactive schedules (no skew, no hidden
// locality) cost a map lookup per product.  MI_AUTO_SCHEDULE=0 turns the whole thing off.
struct AutoEntry {
  int seen = 0;
  bool pending = false, failed = false, active = false;  // active: the finished schedule is worth running on (read once)
  std::shared_ptr<PySchedule> sched;
  torch::Tensor order_buf, ws, host;  // the pending build's buffers (host: pinned)
  hipEvent_t ev = nullptr;
  uint64_t stamp = 0;
};
using AutoKey = std::tuple<int, mi_stream_t, const void*, const void*, int64_t, int64_t>;
std::mutex g_auto_mutex;
std::map<AutoKey, AutoEntry> g_auto;
uint64_t g_auto_clock = 0;
int64_t g_auto_built = 0;

bool auto_schedule_enabled() {
  static const bool on = []() {
    const char* e = std::getenv("MI_AUTO_SCHEDULE");
    return !(e != nullptr && e[0] == '0');
  }();
  return on;
}

void auto_drop(AutoEntry& e) {
  if (e.ev != nullptr) (void)hipEventDestroy(e.ev);
  e.ev = nullptr;
}

std::shared_ptr<PySchedule> auto_schedule(const torch::Tensor& A_offsets, const torch::Tensor& A_columns, int64_t nnzA,
                                          int64_t A_rows, int64_t A_cols, int64_t N, mi_stream_t stream) {
  // worth it only where rows can matter: ≥ 16 Ki entries in ≥ 1024 rows (a thousand rows of 38 entries with one of 3 500 among
  // them take 0.29 ms unscheduled, 1 500 rows with one of 8 000 0.7 ms: tools/plan_grid.py --pattern degskew; an inactive schedule
  // costs the lookup below per product)
  if (!auto_schedule_enabled() || nnzA < (1 << 14) || A_rows < 1024 || A_cols > INT32_MAX || stream_is_capturing(stream)) return nullptr;
  std::lock_guard<std::mutex> lock(g_auto_mutex);
  const AutoKey key{(int)A_offsets.device().index(), stream, A_offsets.data_ptr(), A_columns.data_ptr(), A_rows, nnzA};
  AutoEntry& e = g_auto[key];
  e.seen++;
  e.stamp = ++g_auto_clock;
  if (e.sched) return e.active ? e.sched : nullptr;
  if (e.failed) return nullptr;
  if (e.pending) {
    if (e.ev == nullptr) return nullptr;  // (the product that was to launch the build raised: the next one launches it)
    const hipError_t q = hipEventQuery(e.ev);
    if (q == hipErrorNotReady) {
      (void)hipGetLastError();
      return nullptr;
    }
    e.pending = false;
    auto_drop(e);
    if (q != hipSuccess) {
      e.failed = true;
      return nullptr;
    }
    auto out = std::make_shared<PySchedule>();
    int32_t* order = e.order_buf.data_ptr<int32_t>();
    if (mi_spmm_schedule_finish(e.host.data_ptr<int32_t>(), order, order + A_rows, (int32_t)A_rows, (int32_t)A_cols, nnzA, (int32_t)N,
                                &out->sc) != MI_OK) {
      e.failed = true;
      return nullptr;
    }
    const auto v = schedule_info(out->sc, "auto_schedule");
    out->rows = A_rows;
    out->nnz = nnzA;
    out->order_keep = e.order_buf;
    out->order = (v[5] & 4) ? e.order_buf.narrow(0, A_rows, A_rows) : e.order_buf.narrow(0, 0, A_rows);
    if (!(v[5] & 2)) out->order_keep = out->order = torch::Tensor();  // inactive: nothing will ever read the orders
    e.order_buf = e.ws = e.host = torch::Tensor();
    e.sched = out;
    e.active = (v[5] & 2) != 0;
    g_auto_built++;
    return e.active ? e.sched : nullptr;
  }
  if (e.seen == 2) {
    // the build goes BEHIND this product on its stream (the caller's product is not delayed by it; the arrays are alive: they are
    // this call's arguments, and the stream orders the build before anything that could free them is allowed to run)
    try {
      auto iopt = torch::dtype(torch::kInt32).device(A_offsets.device());
      e.order_buf = torch::empty({2 * A_rows}, iopt);
      e.ws = byte_workspace(A_offsets.device(), mi_spmm_schedule_workspace_bytes((int32_t)A_rows));
      e.host = torch::empty({MI_SCHEDULE_HOST_INTS}, torch::dtype(torch::kInt32).pinned_memory(true));
      e.pending = true;  // (the launch itself happens in auto_schedule_launch, after the product)
    } catch (...) {
      e.failed = true;
      e.order_buf = e.ws = e.host = torch::Tensor();
    }
  }
  // bounded: drop the entry that has been idle longest (never one whose build is in flight)
  if (g_auto.size() > 16) {
    auto victim = g_auto.end();
    for (auto it = g_auto.begin(); it != g_auto.end(); ++it)
      if (!it->second.pending && &it->second != &e && (victim == g_auto.end() || it->second.stamp < victim->second.stamp)) victim = it;
    if (victim != g_auto.end()) {
      auto_drop(victim->second);
      g_auto.erase(victim);
    }
  }
  return nullptr;
}

// second product of a key: enqueue the build behind it
void auto_schedule_launch(const torch::Tensor& A_offsets, const torch::Tensor& A_columns, int64_t nnzA, int64_t A_rows,
                          int64_t A_cols, int64_t N, mi_stream_t stream) {
  if (!auto_schedule_enabled()) return;
  std::lock_guard<std::mutex> lock(g_auto_mutex);
  auto it = g_auto.find(AutoKey{(int)A_offsets.device().index(), stream, A_offsets.data_ptr(), A_columns.data_ptr(), A_rows, nnzA});
  if (it == g_auto.end()) return;
  AutoEntry& e = it->second;
  if (!e.pending || e.ev != nullptr || !e.order_buf.defined()) return;
  int32_t* order = e.order_buf.data_ptr<int32_t>();
  const int st = mi_spmm_schedule_begin(A_offsets.data_ptr<int32_t>(), A_columns.data_ptr<int32_t>(), (int32_t)A_rows, (int32_t)A_cols,
                                        nnzA, (int32_t)N, order, order + A_rows, e.ws.data_ptr(), (size_t)e.ws.numel(),
                                        e.host.data_ptr<int32_t>(), stream);
  bool ok = st == MI_OK && hipEventCreateWithFlags(&e.ev, hipEventDisableTiming) == hipSuccess &&
            hipEventRecord(e.ev, static_cast<hipStream_t>(stream)) == hipSuccess;
  if (!ok) {
    auto_drop(e);
    e.pending = false;
    e.failed = true;
    e.order_buf = e.ws = e.host = torch::Tensor();
  }
}

py::dict auto_schedule_stats() {
  std::lock_guard<std::mutex> lock(g_auto_mutex);
  int64_t pending = 0, active = 0, inactive = 0;
  for (auto& kv : g_auto) {
    if (kv.second.pending) pending++;
    if (kv.second.sched) (py::cast<bool>(kv.second.sched->info()["active"]) ? active : inactive)++;
  }
  py::dict d;
  d["enabled"] = auto_schedule_enabled();
  d["entries"] = (int64_t)g_auto.size();
  d["pending"] = pending;
  d["active"] = active;
  d["inactive"] = inactive;
  d["built"] = g_auto_built;
  return d;
}

void auto_schedule_clear() {
  std::lock_guard<std::mutex> lock(g_auto_mutex);
  for (auto& kv : g_auto) auto_drop(kv.second);
  g_auto.clear();
}

// C = A·B (+ bias) for A in CSR.  float32, or with `lowp` bfloat16 / float16 (C-ABI low-precision section: fp32 sums,
// one rounding at the store; no bias, row schedules or variants there).
torch::Tensor spmm_impl(const torch::Tensor& A_values, const torch::Tensor& A_columns,
                        const torch::Tensor& A_offsets, int64_t nnzA, int64_t A_rows,
                        int64_t A_cols, const torch::Tensor& B, torch::Tensor C, const char* what,
                        const torch::Tensor* bias = nullptr, int long_rows = MI_LONG_ROWS_AUTO,
                        const PySchedule* schedule = nullptr, int variant = MI_SPMM_AUTO, bool allow_auto = false,
                        bool lowp = false) {
  const torch::ScalarType dt = value_dtype(what, {{"A_values", &A_values}, {"B", &B}, {"C", &C}}, lowp);
  const Csr a = csr_arrays(what, &A_values, &A_columns, A_offsets, nnzA, A_rows, A_cols);
  check_same_device(what, a.device, {&B, &C});
  TORCH_CHECK(B.dim() == 2 && C.dim() == 2, what, ": B and C must be 2-d");
  TORCH_CHECK(B.size(0) == A_cols, what, ": B must have A_cols = ", A_cols, " rows, got ", B.size(0));
  TORCH_CHECK(C.size(0) == A_rows && C.size(1) == B.size(1), what, ": C must be ", A_rows, "x",
              B.size(1));
  TORCH_CHECK(C.is_contiguous(), what, ": C must be contiguous");
  const int64_t N = B.size(1);
  check_sizes(what, {N});
  const RowMajorB b = row_major_b(B);
  const torch::Tensor bias_keep = bias_of(what, bias, N, C);
  const bool f32 = dt == torch::kFloat32;
  c10::hip::HIPGuard guard(C.device().index());
  // workspace for the over-long rows (list + partial rows of the split ones); none when the caller pins "no row is split"
  // (MI_LONG_ROWS_NONE: one launch, nothing else).  bf16 / fp16: only where a row may be split (N < 4 keeps the narrow
  // order: never split).
  const bool may_split = long_rows != MI_LONG_ROWS_NONE && (f32 || (N >= 4 && nnzA > mi_spmm_long_row_threshold()));
  const size_t ws_bytes = may_split ? mi_spmm_csr_workspace_bytes(nnzA, (int32_t)N) : 0;
  torch::Tensor ws;
  int mode = long_rows;
  const mi_stream_t stream = stream_of(C);
  std::shared_ptr<PySchedule> auto_keep;  // a schedule the extension built by itself for arrays it has seen before (see auto_schedule)
  if (f32 && allow_auto && schedule == nullptr && long_rows == MI_LONG_ROWS_AUTO) {
    auto_keep = auto_schedule(A_offsets, A_columns, nnzA, A_rows, A_cols, N, stream);
    schedule = auto_keep.get();
  }
  if (ws_bytes > 0 && schedule != nullptr && long_rows == MI_LONG_ROWS_AUTO && schedule->long_ws.defined() &&
      schedule->long_ws_width == N && schedule->nnz == nnzA &&
      mi_spmm_auto_splits_long_rows(nnzA, a.rows, a.cols, (int32_t)N, b.keep.data_ptr<float>(), b.ld,
                                    C.data_ptr<float>(), ld1(N)) == 1) {
    ws = schedule->long_ws;  // the prepared list: the same split rule, its kernel launched first, beside the rest
    mode = MI_LONG_ROWS_PREPARED;
  } else if (ws_bytes > 0 && schedule != nullptr && schedule->long_rows == 0 && schedule->nnz == nnzA && long_rows == MI_LONG_ROWS_AUTO) {
    mode = MI_LONG_ROWS_NONE;  // the inspector counted: no row is beyond the threshold — nothing to list, nothing to follow up
  } else if (ws_bytes > 0) {
    if (long_rows == MI_LONG_ROWS_AUTO && !stream_is_capturing(stream)) {
      // the plain entry points (every dtype): one workspace per (device, stream), kept with a zero header between products,
      // so a product is the main kernel (which lists the rows it skips) + one follow-up launch — no memset, no scan
      ws = zeroed_stream_workspace(C.device(), stream, ws_bytes);
      mode = MI_LONG_ROWS_AUTO_ZEROED;
    } else {
      ws = byte_workspace(C.device(), ws_bytes);  // caching allocator
    }
  }
  void* const ws_ptr = ws.defined() ? ws.data_ptr() : nullptr;
  const size_t ws_size = ws.defined() ? (size_t)ws.numel() : 0;
  int st;
  if (schedule != nullptr)
    st = mi_spmm_csr_scheduled_f32(schedule->sc, variant, a.offsets, a.columns, a.f32(), nnzA, a.rows, a.cols, (int32_t)N,
                                   b.keep.data_ptr<float>(), b.ld, f32_or_null(bias_keep), C.data_ptr<float>(), ld1(N), mode,
                                   ws_ptr, ws_size, stream);
  else if (f32)
    st = mi_spmm_csr_ex_f32(a.offsets, a.columns, a.f32(), nnzA, a.rows, a.cols, (int32_t)N, b.keep.data_ptr<float>(), b.ld,
                            f32_or_null(bias_keep), C.data_ptr<float>(), ld1(N), mode, ws_ptr, ws_size, stream);
  else
    st = (dt == torch::kBFloat16 ? mi_spmm_csr_ex_bf16 : mi_spmm_csr_ex_f16)(
        a.offsets, a.columns, a.b16(), nnzA, a.rows, a.cols, (int32_t)N, static_cast<const uint16_t*>(b.keep.data_ptr()),
        b.ld, static_cast<uint16_t*>(C.data_ptr()), ld1(N), mode, ws_ptr, ws_size, stream);
  if (st != MI_OK && mode == MI_LONG_ROWS_AUTO_ZEROED) drop_stream_workspace(C.device(), stream);  // its header may be dirty
  check_status(st, what);
  if (f32 && allow_auto && long_rows == MI_LONG_ROWS_AUTO && auto_keep == nullptr)
    auto_schedule_launch(A_offsets, A_columns, nnzA, A_rows, A_cols, N, stream);  // (does something on the second product of a key only)
  return C;
}

torch::Tensor naive_spmm(torch::Tensor A_values, torch::Tensor A_columns, torch::Tensor A_offsets,
                         int nnzA, int A_rows, int A_cols, torch::Tensor B, torch::Tensor C) {
  return spmm_impl(A_values, A_columns, A_offsets, nnzA, A_rows, A_cols, B, C, "naive_spmm", nullptr, MI_LONG_ROWS_AUTO, nullptr,
                   MI_SPMM_AUTO, true, true);
}

torch::Tensor cusparse_mmul(torch::Tensor A_values, torch::Tensor A_columns, torch::Tensor A_offsets,
                            int nnzA, int A_rows, int A_cols, torch::Tensor B, torch::Tensor C) {
  return spmm_impl(A_values, A_columns, A_offsets, nnzA, A_rows, A_cols, B, C, "cusparse_mmul", nullptr, MI_LONG_ROWS_AUTO,
                   nullptr, MI_SPMM_AUTO, true, true);
}

// Fused FC-layer forms (additions): C = op(A)·op(B) + bias and C = A_csr·B + bias, bias[n]
// added to every row in the kernel epilogue — what cublasLinear / cusparseLinear.forward
// compute with a clone and an in-place add (reference benchmarks/cublas_fc_layer.py:41-45).
torch::Tensor cublas_mmul_bias(torch::Tensor A, torch::Tensor B, torch::Tensor bias, torch::Tensor C,
                               bool transa, bool transb) {
  return gemm_impl(A, B, C, 0, transa, transb, "cublas_mmul_bias", &bias);
}

// The deterministic split-k of the low-precision dense product (include/mi_spmm.h, mi_gemm_ws_bf16 / _f16): one 2-d product
// of bfloat16 / float16 operands, k cut by the rule of gemm_lowp_split_count (or into `splits` ranges), an optional bias of
// the same dtype in the combine.  cublas_mmul never takes this path; float32 products split inside cublas_mmul itself.
torch::Tensor cublas_mmul_splitk(torch::Tensor A, torch::Tensor B, torch::Tensor C, bool transa, bool transb,
                                 c10::optional<torch::Tensor> bias, int64_t splits) {
  const char* what = "cublas_mmul_splitk";
  const bool all_f32 = A.scalar_type() == torch::kFloat32 && B.scalar_type() == torch::kFloat32 && C.scalar_type() == torch::kFloat32;
  TORCH_CHECK(!all_f32, what, ": bfloat16 / float16 operands only; float32 products go through cublas_mmul, which splits k by "
              "its own rule");
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2 && C.dim() == 2, what, ": 2-d operands only");
  TORCH_CHECK(splits >= 0, what, ": splits must be 0 (the rule) or the number of ranges");
  const torch::Tensor* bp = bias.has_value() && bias->defined() ? &*bias : nullptr;
  return gemm_impl(A, B, C, 0, transa, transb, what, bp, splits);
}

int64_t gemm_lowp_split_count(int64_t m, int64_t n, int64_t k) {
  check_sizes("gemm_lowp_split_count", {m, n, k});
  return mi_gemm_lowp_split_count((int32_t)m, (int32_t)n, (int32_t)k, 1);
}

// the width (64 or 128) of the output tile a bfloat16 / float16 product of `batch` items of m × n launches: shape only
int64_t gemm_lowp_tile_n(int64_t m, int64_t n, int64_t batch) {
  check_sizes("gemm_lowp_tile_n", {m, n, batch});
  return mi_gemm_lowp_tile_n((int32_t)m, (int32_t)n, (int32_t)batch);
}

torch::Tensor naive_spmm_bias(torch::Tensor A_values, torch::Tensor A_columns, torch::Tensor A_offsets,
                              int64_t nnzA, int64_t A_rows, int64_t A_cols, torch::Tensor B,
                              torch::Tensor bias, torch::Tensor C) {
  return spmm_impl(A_values, A_columns, A_offsets, nnzA, A_rows, A_cols, B, C, "naive_spmm_bias", &bias, MI_LONG_ROWS_AUTO, nullptr, MI_SPMM_AUTO, true);
}

// naive_spmm with the long-row rule pinned (include/mi_spmm.h, MI_LONG_ROWS_*): -1 = as naive_spmm,
// 0 = plain CSR-order chain for every row, ONE launch and no workspace (also right when the caller
// knows no row exceeds long_row_threshold() non-zeros), 1 = always split the long rows.  Used by
// sharded.py so a row shard sums exactly as the whole matrix would.
torch::Tensor naive_spmm_ex(torch::Tensor A_values, torch::Tensor A_columns, torch::Tensor A_offsets,
                            int64_t nnzA, int64_t A_rows, int64_t A_cols, torch::Tensor B, torch::Tensor C,
                            int long_rows) {
  if (long_rows < MI_LONG_ROWS_AUTO || long_rows > MI_LONG_ROWS_SPLIT)
    throw std::invalid_argument("naive_spmm_ex: long_rows must be -1, 0 or 1");
  // (bf16 / fp16: -1 and 1 are the same rule, long rows split)
  return spmm_impl(A_values, A_columns, A_offsets, nnzA, A_rows, A_cols, B, C, "naive_spmm_ex", nullptr, long_rows, nullptr,
                   MI_SPMM_AUTO, false, true);
}

// … and with the fused bias (fc_layers: activations converted from a dense matrix have no row longer than
// the layer is wide, so a layer of ≤ long_row_threshold() inputs needs neither workspace nor helper launches).
torch::Tensor naive_spmm_bias_ex(torch::Tensor A_values, torch::Tensor A_columns, torch::Tensor A_offsets,
                                 int64_t nnzA, int64_t A_rows, int64_t A_cols, torch::Tensor B, torch::Tensor bias,
                                 torch::Tensor C, int long_rows) {
  if (long_rows < MI_LONG_ROWS_AUTO || long_rows > MI_LONG_ROWS_SPLIT)
    throw std::invalid_argument("naive_spmm_bias_ex: long_rows must be -1, 0 or 1");
  return spmm_impl(A_values, A_columns, A_offsets, nnzA, A_rows, A_cols, B, C, "naive_spmm_bias_ex", &bias, long_rows);
}

// (variant id, kernel name, launches per product, splits_long_rows) of the AUTO plan for
// C[M,N] = A[M,K]·B with nnz non-zeros and these operand buffers — no GPU work.
std::tuple<int, std::string, int, bool> spmm_plan(int64_t nnz, int64_t M, int64_t K, torch::Tensor B, torch::Tensor C) {
  value_dtype("spmm_plan", {{"B", &B}, {"C", &C}});
  TORCH_CHECK(B.dim() == 2 && C.dim() == 2 && B.size(1) == C.size(1), "spmm_plan: B [K,N] and C [M,N] expected");
  const int64_t N = B.size(1);
  check_sizes("spmm_plan", {M, K, N}, nnz);
  const int64_t ldb = B.size(0) > 1 ? B.stride(0) : ld1(N);
  const int64_t ldc = C.size(0) > 1 ? C.stride(0) : ld1(N);
  const int v = mi_spmm_csr_f32_plan(nnz, (int32_t)M, (int32_t)K, (int32_t)N, B.data_ptr<float>(), ldb,
                                     C.data_ptr<float>(), ldc);
  check_status(v < 0 ? v : MI_OK, "spmm_plan");
  const int sp = mi_spmm_auto_splits_long_rows(nnz, (int32_t)M, (int32_t)K, (int32_t)N, B.data_ptr<float>(), ldb,
                                               C.data_ptr<float>(), ldc);
  return std::make_tuple(v, std::string(mi_spmm_variant_name(v)), mi_spmm_variant_launches(v), sp == 1);
}

int long_row_threshold() { return mi_spmm_long_row_threshold(); }

// Opt-in check of a CSR's CONTENTS (the hot-path entry points validate sizes, dtypes, devices and
// layout, but trust the indices like the reference does, src/naive_sparse_mm.cu:60-92: a column
// outside [0, A_cols) or decreasing offsets read B out of bounds).  Raises on the first violation;
// costs a few reductions and one host read-back, so call it where the matrix is built, not per product.
// The inspector entry points (cusparse_inspect / tiledspmm_inspect_*) run the same checks once.
void validate_csr(torch::Tensor A_values, torch::Tensor A_columns, torch::Tensor A_offsets, int64_t nnzA,
                  int64_t A_rows, int64_t A_cols) {
  const char* what = "validate_csr";
  value_dtype(what, {{"A_values", &A_values}});
  csr_arrays(what, &A_values, &A_columns, A_offsets, nnzA, A_rows, A_cols);
  torch::Tensor off = A_offsets.reshape({-1});
  if (A_rows > 0) {
    TORCH_CHECK(off[0].item<int32_t>() == 0 && off[A_rows].item<int32_t>() == nnzA, what,
                ": offsets must start at 0 and end at nnz");
    TORCH_CHECK((off.slice(0, 1) - off.slice(0, 0, A_rows)).min().item<int32_t>() >= 0, what,
                ": offsets must not decrease");
  } else {
    TORCH_CHECK(nnzA == 0, what, ": a matrix without rows has no non-zeros");
  }
  if (nnzA > 0) {
    torch::Tensor c = A_columns.reshape({-1}).slice(0, 0, nnzA);
    TORCH_CHECK(c.min().item<int32_t>() >= 0 && c.max().item<int32_t>() < A_cols, what, ": column index out of range");
  }
}

// Column sums of a 2-d tensor (bias gradient of the FC layers): returns a [n] tensor of src's dtype (float32, or bfloat16 /
// float16: fp32 sums in the float32 order, rounded once).
torch::Tensor column_sums(torch::Tensor src) {
  const torch::ScalarType dt = value_dtype("column_sums", {{"src", &src}}, true);
  TORCH_CHECK(src.dim() == 2, "column_sums: expected a 2-d tensor");
  const int64_t rows = src.size(0), n = src.size(1);
  check_sizes("column_sums", {rows, n});
  torch::Tensor x = src.stride(1) == 1 && src.stride(0) >= n ? src : src.contiguous();
  c10::hip::HIPGuard guard(x.device().index());
  torch::Tensor out = torch::empty({n}, x.options());
  const size_t ws_bytes = mi_colsum_workspace_bytes((int32_t)rows, (int32_t)n);
  torch::Tensor ws = byte_workspace(x.device(), ws_bytes, 4);
  const int64_t ld = rows > 1 ? x.stride(0) : ld1(n);
  int st;
  if (is_lowp(dt))
    st = (dt == torch::kBFloat16 ? mi_colsum_bf16 : mi_colsum_f16)(static_cast<const uint16_t*>(x.data_ptr()), (int32_t)rows,
                                                                    (int32_t)n, ld, static_cast<uint16_t*>(out.data_ptr()),
                                                                    ws.data_ptr(), ws_bytes, stream_of(x));
  else
    st = mi_colsum_f32(x.data_ptr<float>(), (int32_t)rows, (int32_t)n, ld, out.data_ptr<float>(), ws.data_ptr(), ws_bytes,
                       stream_of(x));
  check_status(st, "column_sums");
  return out;
}

// values[perm] as a new tensor (perm int32, values f32 / bf16 / fp16, both contiguous and on one device); what torch's
// index_select does, without its index conversion (bound by one line request per value either way: tools/probes/gather_bench.py)
torch::Tensor gather_perm(torch::Tensor values, torch::Tensor perm) {
  const char* what = "gather_perm";
  const torch::ScalarType dt = value_dtype(what, {{"values", &values}}, true);
  check_device_i32(perm, "perm");
  check_same_device(what, values.device(), {&perm});
  TORCH_CHECK(values.dim() == 1 && perm.dim() == 1 && values.is_contiguous() && perm.is_contiguous(),
              "gather_perm: expected contiguous 1-d tensors");
  c10::hip::HIPGuard guard(values.device().index());
  torch::Tensor out = torch::empty({perm.numel()}, values.options());
  const int st = dt == torch::kFloat32
                     ? mi_gather_f32(values.data_ptr<float>(), perm.data_ptr<int32_t>(), perm.numel(), out.data_ptr<float>(),
                                     stream_of(values))
                     : mi_gather_b16(static_cast<const uint16_t*>(values.data_ptr()), perm.data_ptr<int32_t>(), perm.numel(),
                                     static_cast<uint16_t*>(out.data_ptr()), stream_of(values));
  check_status(st, what);
  return out;
}

std::shared_ptr<PySchedule> make_schedule(torch::Tensor A_offsets, int64_t nnzA, int64_t A_rows, int64_t N, bool list_long_rows,
                                          const char* what, const torch::Tensor* A_columns = nullptr, int64_t A_cols = 0) {
  if (A_columns != nullptr && !A_columns->defined()) A_columns = nullptr;
  const Csr a = csr_arrays(what, nullptr, A_columns, A_offsets, nnzA, A_rows, A_cols);
  check_sizes(what, {N});
  c10::hip::HIPGuard guard(A_offsets.device().index());
  auto out = std::make_shared<PySchedule>();
  out->rows = A_rows;
  out->nnz = nnzA;
  torch::Tensor order_buf = torch::empty({(A_columns != nullptr ? 2 : 1) * A_rows}, A_offsets.options());
  const size_t ws_bytes = mi_spmm_schedule_workspace_bytes(a.rows);
  torch::Tensor ws = byte_workspace(a.device, ws_bytes);
  check_status(mi_spmm_schedule_create(a.offsets, a.columns, a.rows, a.cols, nnzA, (int32_t)N, order_buf.data_ptr<int32_t>(),
                                       ws.data_ptr(), ws_bytes, stream_of(A_offsets), &out->sc),
               what);
  const auto v = schedule_info(out->sc, what);
  out->order_keep = order_buf;  // both candidate orders; `order` is the half the schedule points at
  out->order = (v[5] & 4) ? order_buf.narrow(0, A_rows, A_rows) : order_buf.narrow(0, 0, A_rows);
  // the longest class starts at v[4] entries and is ≈ 12 % wide: list the long rows when it may reach beyond the threshold
  // (and nnz does: below that, mi_spmm_long_rows_prepare writes no list)
  const int64_t threshold = mi_spmm_long_row_threshold();
  if (list_long_rows && N > 0 && nnzA > threshold && v[4] + v[4] / 8 + 1 > threshold) {
    const size_t lbytes = mi_spmm_csr_workspace_bytes(nnzA, (int32_t)N);
    out->long_ws = byte_workspace(a.device, lbytes, 16);
    check_status(mi_spmm_long_rows_prepare(a.offsets, a.rows, nnzA, (int32_t)N, out->long_ws.data_ptr(), lbytes,
                                           stream_of(A_offsets)),
                 what);
    out->long_ws_width = N;
    out->long_rows = out->long_ws.view(torch::kInt32)[0].item<int32_t>();  // (inspection time: one more read-back)
    if (out->long_rows == 0) out->long_ws = torch::Tensor();
  } else if (list_long_rows) {
    out->long_rows = 0;
  }
  return out;
}

std::shared_ptr<PySchedule> spmm_schedule(torch::Tensor A_offsets, int64_t nnzA, int64_t A_rows, int64_t N,
                                          c10::optional<torch::Tensor> A_columns, int64_t A_cols) {
  const torch::Tensor* c = A_columns.has_value() && A_columns->defined() ? &*A_columns : nullptr;
  return make_schedule(A_offsets, nnzA, A_rows, N, true, "spmm_schedule", c, A_cols);
}

torch::Tensor naive_spmm_scheduled(std::shared_ptr<PySchedule> schedule, torch::Tensor A_values, torch::Tensor A_columns,
                                   torch::Tensor A_offsets, int64_t nnzA, int64_t A_rows, int64_t A_cols, torch::Tensor B,
                                   torch::Tensor C, c10::optional<torch::Tensor> bias, int long_rows, int variant) {
  const char* what = "naive_spmm_scheduled";
  TORCH_CHECK(schedule && schedule->sc, what, ": no schedule");
  TORCH_CHECK(schedule->rows == A_rows, what, ": the schedule was built for ", schedule->rows, " rows, A has ", A_rows);
  check_same_device(what, C.device(), {&schedule->order});
  if (long_rows < MI_LONG_ROWS_AUTO || long_rows > MI_LONG_ROWS_SPLIT)
    throw std::invalid_argument("naive_spmm_scheduled: long_rows must be -1, 0 or 1");
  const torch::Tensor* b = bias.has_value() && bias->defined() ? &*bias : nullptr;
  return spmm_impl(A_values, A_columns, A_offsets, nnzA, A_rows, A_cols, B, C, what, b, long_rows, schedule.get(), variant);
}
