// custom_mm — what the bindings of the KV-cache family (block_attention_decode*, block_attention_prefill*, kv_append*,
// rope_kv_append*) say about the cache operands, said once (DESIGN.md §3.23), and what the reading ones say alike about the
// whole call (§3.31)
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace, ahead of those bindings.
// Not compiled on its own.  The cache is k, v [B, Hkv, Smax, D] or a pool k_pages, v_pages [P, Hkv, page, D] with block_table
// int32 [B, W] (Smax = W · page), READ AND WRITTEN THROUGH ITS OWN STRIDES (last stride 1, the others multiples of 16 bytes —
// 8 two-byte elements, 16 float8_e4m3fn bytes —, a 16-byte aligned data pointer — never copied); k_lens int32 [B] or [1] on
// the device; k_scale, v_scale: None (= 1) or float32 device tensors of 1 or Hkv entries, handed over as pointers and never
// read back.  Each rule is one function, so that every binding keeps the order in which it refuses; a message that differs
// between the callers by a word (the tensors' names, "batch" | "page", "keys" | "rows") takes that word as an argument.

// a cache operand's strides as the kernel takes them; the message names the stride that does not fit (`outer`: the first
// one, the batch stride of a cache or the page stride of a pool; `unit`: the elements of 16 bytes — 8, or 16 of an fp8 cache)
void check_cache_strides(const char* what, const char* name, const torch::Tensor& t, int64_t D, const char* outer = "batch",
                         int64_t unit = 8) {
  TORCH_CHECK(t.stride(3) == 1 || D == 1, what, ": ", name, " must have a last stride of 1, got ", t.stride(3));
  TORCH_CHECK(t.size(2) <= 1 || (t.stride(2) >= D && t.stride(2) % unit == 0), what, ": ", name,
              "'s row stride must be a multiple of ", unit, " elements and at least D = ", D, ", got ", t.stride(2));
  TORCH_CHECK(t.size(1) <= 1 || (t.stride(1) >= 0 && t.stride(1) % unit == 0), what, ": ", name,
              "'s head stride must be a multiple of ", unit, " elements, got ", t.stride(1));
  TORCH_CHECK(t.size(0) <= 1 || (t.stride(0) >= 0 && t.stride(0) % unit == 0), what, ": ", name,
              "'s ", outer, " stride must be a multiple of ", unit, " elements, got ", t.stride(0));
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, what, ": ", name, "'s data pointer must be 16-byte aligned");
}

// a stride the kernel never multiplies by anything but 0 (a dimension of one entry) is handed over as a harmless 0 / D
int64_t cache_stride(const torch::Tensor& t, int dim, int64_t fallback) { return t.size(dim) > 1 ? t.stride(dim) : fallback; }

// a source operand's strides (k_new, v_new, q of the rope call and its outputs) as the kernel takes them
void check_source_strides(const char* what, const char* name, const torch::Tensor& t) {
  static const char* const dims[] = {"batch", "head", "token"};
  TORCH_CHECK(t.stride(3) == 1 || t.size(3) <= 1, what, ": ", name, " must have a last stride of 1, got ", t.stride(3));
  for (int d = 2; d >= 0; --d)
    TORCH_CHECK(t.size(d) <= 1 || (t.stride(d) >= 0 && t.stride(d) % 8 == 0), what, ": ", name, "'s ", dims[d],
                " stride must be a multiple of 8 elements, got ", t.stride(d));
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, what, ": ", name, "'s data pointer must be 16-byte aligned");
}

// a scale operand as the C ABI takes it: (pointer or null, count)
std::pair<const float*, int32_t> fp8_scale(const char* what, const char* name, const c10::optional<torch::Tensor>& s, int64_t Hkv,
                                           const torch::Tensor& q) {
  if (!s.has_value()) return {nullptr, 1};
  const torch::Tensor& t = *s;
  TORCH_CHECK(t.scalar_type() == torch::kFloat32 && t.device() == q.device() && t.is_contiguous() && t.dim() <= 1 &&
                  (t.numel() == 1 || t.numel() == Hkv),
              what, ": ", name, " must be None or a contiguous float32 tensor on q's device of 1 or Hkv = ", Hkv, " entries");
  return {t.data_ptr<float>(), (int32_t)t.numel()};
}

// the page rule; `noun`: what a page holds for the caller — "keys" for the reading calls, "rows" for the writing ones
void check_page(const char* what, const char* noun, int64_t page) {
  TORCH_CHECK(page >= 16 && (page & (page - 1)) == 0, what, ": a page must hold a power of two >= 16 ", noun, ", got ", page);
}

// the block table's shape [B, W]: returns W, the logical pages of an item
int64_t table_width(const char* what, const torch::Tensor& table, int64_t B) {
  TORCH_CHECK(table.dim() == 2 && table.size(0) == B, what, ": block_table must be [B, W] = [", B, ", W]");
  return table.size(1);
}

// … its dtype and strides: it is handed over as it is
void check_table(const char* what, const torch::Tensor& table) {
  const int64_t B = table.size(0), W = table.size(1);
  check_device_i32(table, "block_table");
  TORCH_CHECK((W <= 1 || table.stride(1) == 1) && (B <= 1 || table.stride(0) >= W), what,
              ": block_table must have a last stride of 1 and a row stride of at least W = ", W, ", got strides (", table.stride(0),
              ", ", table.stride(1), ")");
}

void check_k_lens(const char* what, const torch::Tensor& k_lens, int64_t B) {
  TORCH_CHECK(k_lens.is_contiguous() && (k_lens.numel() == B || k_lens.numel() == 1), what,
              ": k_lens must be a contiguous int32 tensor of B = ", B, " entries or of one, got ", k_lens.numel());
}

// The cache operands as the C entries take them, gathered after the checks: `table` null — the contiguous cache — or the
// block table of a pool, for which k, v are k_pages, v_pages and the outer strides the page strides.
struct CacheOperands {
  bool paged;
  int64_t Smax, P, page;  // rows of an item; pool pages and rows of a page (0, 0: contiguous)
  const int32_t* table;
  int64_t table_ld;
  void *k, *v;
  int64_t ldk, headK, outerK, ldv, headV, outerV;
};

CacheOperands cache_operands(const torch::Tensor& k, const torch::Tensor& v, const torch::Tensor* table, int64_t D) {
  CacheOperands c = {table != nullptr, k.size(2), 0, 0, nullptr, 0, k.data_ptr(), v.data_ptr(),
                     cache_stride(k, 2, D), cache_stride(k, 1, 0), cache_stride(k, 0, 0),
                     cache_stride(v, 2, D), cache_stride(v, 1, 0), cache_stride(v, 0, 0)};
  if (table) {
    const int64_t B = table->size(0), W = table->size(1);
    c.P = k.size(0), c.page = k.size(2), c.Smax = W * c.page;
    c.table = table->data_ptr<int32_t>(), c.table_ld = B > 1 ? table->stride(0) : W;
  }
  return c;
}

// ---- a reading call: block_attention_decode*, block_attention_prefill*, block_attention_decode_lists* (DESIGN.md §3.31) --------
// q and out [B, Hq, T, D] bfloat16 or float16, the cache of q's type or (`fp8`) float8_e4m3fn with the two scales, `table` null
// or the block table of a pool, lse float32 [B, Hq, T].  Four pieces, between which every binding makes the checks of its own:
// read_shape, read_smax, check_read_operands and read_cache.

// q's and out's type of an fp8 call, the cache's checked on the way
bool fp8_decode_dtypes(const char* what, const torch::Tensor& q, const torch::Tensor& out, const char* kname, const torch::Tensor& k,
                       const char* vname, const torch::Tensor& v) {
  TORCH_CHECK(k.scalar_type() == torch::kFloat8_e4m3fn && v.scalar_type() == torch::kFloat8_e4m3fn, what, ": ", kname, " and ", vname,
              " must be float8_e4m3fn (the OCP e4m3fn encoding is what is read), got ", k.scalar_type(), " and ", v.scalar_type());
  return is_lowp_dtype(what, value_dtype(what, {{"q", &q}, {"out", &out}}, true));
}

struct ReadShape {
  bool bf;  // bfloat16, else float16
  int64_t B, Hq, T, D, Hkv, group;
};

// the dtype rule, the 4-d shapes, the pool or the cache against q's shape, the page and the heads / group rule
ReadShape read_shape(const char* what, const char* kname, const char* vname, bool fp8, const torch::Tensor& q, const torch::Tensor& k,
                     const torch::Tensor& v, const torch::Tensor* table, const torch::Tensor& out) {
  const bool bf = fp8 ? fp8_decode_dtypes(what, q, out, kname, k, vname, v)
                      : is_lowp_dtype(what, value_dtype(what, {{"q", &q}, {kname, &k}, {vname, &v}, {"out", &out}}, true));
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4, what, ": q must be [B, Hq, T, D], ", kname, " and ", vname,
              table ? " [P, Hkv, page, D]" : " [B, Hkv, Smax, D]");
  const int64_t B = q.size(0), Hq = q.size(1), T = q.size(2), D = q.size(3), Hkv = k.size(1);
  if (table) {
    TORCH_CHECK(k.size(3) == D && v.sizes() == k.sizes(), what, ": ", kname, " and ", vname,
                " must be [P, Hkv, page, D] = [P, Hkv, page, ", D, "]");
    check_page(what, "keys", k.size(2));
  } else {
    TORCH_CHECK(k.size(0) == B && k.size(3) == D && v.sizes() == k.sizes(), what, ": k and v must be [B, Hkv, Smax, D] = [", B,
                ", Hkv, Smax, ", D, "]");
  }
  TORCH_CHECK(Hkv > 0 ? Hq % Hkv == 0 : Hq == 0, what, ": ", Hq, " query heads are not a multiple of ", Hkv, " k / v heads");
  return {bf, B, Hq, T, D, Hkv, Hkv > 0 ? std::max<int64_t>(Hq / Hkv, 1) : 1};
}

// the rows of an item: the table's logical pages · page, or the cache's own
int64_t read_smax(const char* what, const torch::Tensor& k, const torch::Tensor* table, int64_t B) {
  return table ? table_width(what, *table, B) * k.size(2) : k.size(2);
}

// the devices (`dev`: the device of the call's lists, which the binding has checked q, k and v against), lse, k_lens and the
// table as they are handed over, out's and lse's shapes; `q_contiguous`: q is taken contiguous (the decode calls) — else it is
// read through its own strides, which the binding checks
void check_read_operands(const char* what, const torch::Device& dev, bool q_contiguous, const torch::Tensor& q,
                         const torch::Tensor* table, const torch::Tensor& k_lens, const torch::Tensor& out, const torch::Tensor& lse,
                         const ReadShape& s) {
  if (table) check_same_device(what, dev, {table});
  check_same_device(what, dev, {&out, &lse, &k_lens});
  check_device_f32(lse, "lse");
  check_device_i32(k_lens, "k_lens");
  if (table) check_table(what, *table);
  TORCH_CHECK(!q_contiguous || (q.is_contiguous() && out.is_contiguous() && out.sizes() == q.sizes()), what,
              ": q and out must be contiguous [B, Hq, T, D] tensors of one shape");
  TORCH_CHECK(out.is_contiguous() && out.sizes() == q.sizes(), what, ": out must be a contiguous [B, Hq, T, D] tensor of q's shape");
  TORCH_CHECK(lse.is_contiguous() && lse.numel() == s.B * s.Hq * s.T, what, ": lse must be a contiguous [B, Hq, T] tensor");
  check_k_lens(what, k_lens, s.B);
}

// the cache's strides, the scales of an fp8 cache, the operands gathered, and the sizes the C ABI takes as int32
struct ReadCache {
  CacheOperands c;
  std::pair<const float*, int32_t> ks, vs;
};

ReadCache read_cache(const char* what, const char* kname, const char* vname, bool fp8, const torch::Tensor& q, const torch::Tensor& k,
                     const torch::Tensor& v, const torch::Tensor* table, const c10::optional<torch::Tensor>& k_scale,
                     const c10::optional<torch::Tensor>& v_scale, const ReadShape& s) {
  const char* outer = table ? "page" : "batch";
  check_cache_strides(what, kname, k, s.D, outer, fp8 ? 16 : 8);
  check_cache_strides(what, vname, v, s.D, outer, fp8 ? 16 : 8);
  ReadCache r = {{}, {nullptr, 1}, {nullptr, 1}};
  if (fp8) r.ks = fp8_scale(what, "k_scale", k_scale, s.Hkv, q), r.vs = fp8_scale(what, "v_scale", v_scale, s.Hkv, q);
  r.c = cache_operands(k, v, table, s.D);
  check_sizes(what, {s.B * s.Hkv, s.B * s.Hq, s.T, r.c.Smax, s.D, r.c.P});  // (P: 0 without a pool)
  return r;
}

uint16_t* bits16(const torch::Tensor& t) { return static_cast<uint16_t*>(t.data_ptr()); }

// The argument lists of the 32 C entries (§3.31's 28 and the four list entries over an fp8 cache of §3.32) in the pieces they
// share (`s`: the ReadShape, `r`: the ReadCache, CT: the cache's element at the C ABI): the sizes, what the paged entries add, the cache with the lengths, what the fp8 entries add, out and lse.
#define MI_READ_SIZES (int32_t)(s.B * s.Hkv), (int32_t)s.Hkv, (int32_t)s.T, (int32_t)r.c.Smax
#define MI_READ_TABLE r.c.table, r.c.table_ld, (int32_t)r.c.P, (int32_t)r.c.page
#define MI_READ_CACHE(CT)                                                                                                   \
  static_cast<const CT*>(r.c.k), r.c.ldk, r.c.headK, r.c.outerK, static_cast<const CT*>(r.c.v), r.c.ldv, r.c.headV, r.c.outerV, \
      k_lens.data_ptr<int32_t>(), (int32_t)k_lens.numel()
#define MI_READ_SCALES r.ks.first, r.ks.second, r.vs.first, r.vs.second
#define MI_READ_OUT bits16(out), s.D, s.T* s.D, lse.data_ptr<float>()

// The tree mask of the block_attention_tree_… bindings (DESIGN.md §3.34) as the C ABI takes it: (pointer, rows) — contiguous int64 words [B, T], or
// [T] for the whole batch, on `dev`, T <= 64; handed over as it is and never read back
std::pair<const int64_t*, int32_t> tree_mask_operand(const char* what, const torch::Tensor& mask, int64_t B, int64_t T,
                                                     const torch::Device& dev) {
  TORCH_CHECK(mask.is_cuda(), "tree_mask must be a device (HIP) tensor; custom_mm has no CPU path");
  TORCH_CHECK(mask.scalar_type() == torch::kInt64, "tree_mask must be int64, got ", mask.scalar_type());
  check_same_device(what, dev, {&mask});
  const bool shared = mask.dim() == 1;
  TORCH_CHECK(mask.is_contiguous() && ((shared && mask.size(0) == T) || (mask.dim() == 2 && mask.size(0) == B && mask.size(1) == T)),
              what, ": tree_mask must be a contiguous [B, T] = [", B, ", ", T, "] or [T] tensor");
  TORCH_CHECK(T <= 64, what, ": a tree mask needs T <= 64, got T = ", T);
  return {mask.data_ptr<int64_t>(), shared ? 1 : (int32_t)B};
}

// The window of the block_attention_window_… bindings (DESIGN.md §3.35): the token sees its last `window` keys, itself included, and
// the first `sink` keys of the cache — two int32s, 1 <= window, 0 <= sink
struct WindowOperand {
  int64_t window, sink;
};
void check_window(const char* what, const WindowOperand& w) {
  TORCH_CHECK(w.window >= 1 && w.window <= INT32_MAX, what, ": window must be a positive int32, got ", w.window);
  TORCH_CHECK(w.sink >= 0 && w.sink <= INT32_MAX, what, ": sink must be an int32 >= 0, got ", w.sink);
}

// the writing calls' cache: of the source's dtype `dt` (a bit copy) or float8_e4m3fn; returns whether it is fp8
bool written_cache_is_fp8(const char* what, const char* kname, const char* vname, torch::ScalarType dt, const torch::Tensor& k,
                          const torch::Tensor& v, const c10::optional<torch::Tensor>& k_scale,
                          const c10::optional<torch::Tensor>& v_scale) {
  const bool fp8 = k.scalar_type() != dt || v.scalar_type() != dt;
  TORCH_CHECK(!fp8 || (k.scalar_type() == torch::kFloat8_e4m3fn && v.scalar_type() == torch::kFloat8_e4m3fn), what, ": ", kname,
              " and ", vname, " must have k_new's dtype ", dt, " or be float8_e4m3fn (the OCP e4m3fn encoding is what is written), got ",
              k.scalar_type(), " and ", v.scalar_type());
  TORCH_CHECK(fp8 || (!k_scale.has_value() && !v_scale.has_value()), what, ": k_scale and v_scale go with a float8_e4m3fn cache only");
  return fp8;
}

// … its shape against the source's B, Hkv and D
void check_written_cache_shape(const char* what, const char* kname, const char* vname, const torch::Tensor& k, const torch::Tensor& v,
                               bool paged, int64_t B, int64_t Hkv, int64_t D) {
  TORCH_CHECK((paged || k.size(0) == B) && k.size(1) == Hkv && k.size(3) == D && v.sizes() == k.sizes(), what, ": ", kname, " and ",
              vname, " must be ", paged ? "[P, Hkv, page, D]" : "[B, Hkv, Smax, D]", " with k_new's B = ", B, ", Hkv = ", Hkv,
              " and D = ", D);
}

// … and its page and table, in the writing calls' order of refusals (the reading calls make the same checks between others of
// their own); `dev`: the device of the call's first operand
void check_written_cache_table(const char* what, const torch::Tensor& k, const torch::Tensor* table, int64_t B,
                               const torch::Device& dev) {
  if (!table) return;
  check_page(what, "rows", k.size(2));
  table_width(what, *table, B);
  check_table(what, *table);
  check_same_device(what, dev, {table});
}
