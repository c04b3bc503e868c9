// custom_mm — query-aware key-block selection: the K best 64-key blocks of every new token, from the per-block key bounds
// (DESIGN.md §3.29)
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace, after custom_mm_kv_cache.inc
// (check_source_strides, check_k_lens).  Not compiled on its own.  Contract: include/mi_spmm.h, "Query-aware key-block
// selection": q [B, Hq, T, D] bfloat16 or float16 READ THROUGH ITS OWN STRIDES, bounds [B, Hkv, Smax/64, 2, D] contiguous of
// q's dtype, k_lens int32; block_ids int32 [B, Hkv, T, K], block_counts int32 [B, Hkv, T] and, optionally, scores float32
// [B, Hkv, T, Smax/64] are written in place.  Nothing is returned.
void block_select(torch::Tensor q, torch::Tensor bounds, torch::Tensor k_lens, int64_t K, int64_t sink, int64_t local,
                  torch::Tensor block_ids, torch::Tensor block_counts, c10::optional<torch::Tensor> scores) {
  const char* what = "block_select";
  const bool bf = is_lowp_dtype(what, value_dtype(what, {{"q", &q}, {"bounds", &bounds}}, true));
  TORCH_CHECK(q.dim() == 4 && bounds.dim() == 5, what, ": q must be [B, Hq, T, D] and bounds [B, Hkv, Smax/64, 2, D]");
  const int64_t B = q.size(0), Hq = q.size(1), T = q.size(2), D = q.size(3), Hkv = bounds.size(1), blocks = bounds.size(2);
  TORCH_CHECK(bounds.is_contiguous() && bounds.size(0) == B && bounds.size(3) == 2 && bounds.size(4) == D, what,
              ": bounds must be a contiguous [B, Hkv, Smax/64, 2, D] = [", B, ", Hkv, Smax/64, 2, ", D, "] tensor");
  TORCH_CHECK(Hkv > 0 ? Hq % Hkv == 0 : Hq == 0, what, ": ", Hq, " query heads are not a multiple of ", Hkv, " k / v heads");
  const int64_t group = Hkv > 0 ? std::max<int64_t>(Hq / Hkv, 1) : 1;
  TORCH_CHECK(K >= 1 && K <= INT32_MAX && sink >= 0 && local >= 1 && sink + local <= K, what,
              ": K >= 1, sink >= 0, local >= 1 and sink + local <= K are required, got K = ", K, ", sink = ", sink, ", local = ", local);
  TORCH_CHECK(blocks <= mi_block_select_max_blocks(), what, ": ", blocks, " blocks exceed the ", mi_block_select_max_blocks(),
              " one workgroup's LDS holds the scores of");
  check_same_device(what, q.device(), {&bounds, &k_lens, &block_ids, &block_counts});
  check_device_i32(k_lens, "k_lens");
  check_device_i32(block_ids, "block_ids");
  check_device_i32(block_counts, "block_counts");
  check_k_lens(what, k_lens, B);
  check_source_strides(what, "q", q);
  TORCH_CHECK(block_ids.is_contiguous() && block_ids.numel() == B * Hkv * T * K && block_counts.is_contiguous() &&
                  block_counts.numel() == B * Hkv * T,
              what, ": block_ids must be a contiguous [B, Hkv, T, K] and block_counts a contiguous [B, Hkv, T] tensor");
  float* sc = nullptr;
  if (scores.has_value()) {
    check_device_f32(*scores, "scores");
    check_same_device(what, q.device(), {&*scores});
    TORCH_CHECK(scores->is_contiguous() && scores->numel() == B * Hkv * T * blocks, what,
                ": scores must be a contiguous [B, Hkv, T, Smax/64] tensor");
    sc = scores->data_ptr<float>();
  }
  check_sizes(what, {B * Hkv, B * Hq, T, blocks * 64, D, B * Hkv * T});
  TORCH_CHECK(B * Hkv * T * K <= INT64_MAX / 4, what, ": block_ids too large");
  if (block_counts.numel() == 0) return;
  c10::hip::HIPGuard guard(q.device().index());
  const int st = (bf ? mi_block_select_bf16 : mi_block_select_f16)(
      (int32_t)(B * Hkv), (int32_t)Hkv, (int32_t)T, (int32_t)(blocks * 64), (int32_t)D, (int32_t)group,
      static_cast<const uint16_t*>(q.data_ptr()), cache_stride(q, 2, D), cache_stride(q, 1, 0), cache_stride(q, 0, 0),
      static_cast<const uint16_t*>(bounds.data_ptr()), k_lens.data_ptr<int32_t>(), (int32_t)k_lens.numel(), (int32_t)K, (int32_t)sink,
      (int32_t)local, block_ids.data_ptr<int32_t>(), block_counts.data_ptr<int32_t>(), sc, stream_of(q));
  check_status(st, what);
}

// … per POSITION TILE of a prefill chunk (DESIGN.md §3.33; include/mi_spmm.h, "Key-block selection per position tile"): the
// operands of block_select with new_lens — None or int32 [B] / [1] — after k_lens; block_ids int32 [B, Hkv, X, K], block_counts
// int32 [B, Hkv, X] and, optionally, scores float32 [B, Hkv, X, Smax/64] with X = ceil(T / 64) + 1 are written in place.
void block_select_tiles(torch::Tensor q, torch::Tensor bounds, torch::Tensor k_lens, c10::optional<torch::Tensor> new_lens, int64_t K,
                        int64_t sink, int64_t local, torch::Tensor block_ids, torch::Tensor block_counts,
                        c10::optional<torch::Tensor> scores) {
  const char* what = "block_select_tiles";
  const bool bf = is_lowp_dtype(what, value_dtype(what, {{"q", &q}, {"bounds", &bounds}}, true));
  TORCH_CHECK(q.dim() == 4 && bounds.dim() == 5, what, ": q must be [B, Hq, T, D] and bounds [B, Hkv, Smax/64, 2, D]");
  const int64_t B = q.size(0), Hq = q.size(1), T = q.size(2), D = q.size(3), Hkv = bounds.size(1), blocks = bounds.size(2);
  const int64_t X = (T + 63) / 64 + 1;
  TORCH_CHECK(bounds.is_contiguous() && bounds.size(0) == B && bounds.size(3) == 2 && bounds.size(4) == D, what,
              ": bounds must be a contiguous [B, Hkv, Smax/64, 2, D] = [", B, ", Hkv, Smax/64, 2, ", D, "] tensor");
  TORCH_CHECK(Hkv > 0 ? Hq % Hkv == 0 : Hq == 0, what, ": ", Hq, " query heads are not a multiple of ", Hkv, " k / v heads");
  const int64_t group = Hkv > 0 ? std::max<int64_t>(Hq / Hkv, 1) : 1;
  TORCH_CHECK(K >= 1 && K <= INT32_MAX && sink >= 0 && local >= 1 && sink + local <= K, what,
              ": K >= 1, sink >= 0, local >= 1 and sink + local <= K are required, got K = ", K, ", sink = ", sink, ", local = ", local);
  TORCH_CHECK(blocks <= mi_block_select_max_blocks(), what, ": ", blocks, " blocks exceed the ", mi_block_select_max_blocks(),
              " one workgroup's LDS holds the scores of");
  check_same_device(what, q.device(), {&bounds, &k_lens, &block_ids, &block_counts});
  check_device_i32(k_lens, "k_lens");
  check_device_i32(block_ids, "block_ids");
  check_device_i32(block_counts, "block_counts");
  check_k_lens(what, k_lens, B);
  const int32_t* nl = nullptr;
  int32_t nl_count = 0;
  if (new_lens.has_value()) {
    check_same_device(what, q.device(), {&*new_lens});
    check_device_i32(*new_lens, "new_lens");
    TORCH_CHECK(new_lens->is_contiguous() && (new_lens->numel() == B || new_lens->numel() == 1), what,
                ": new_lens must be None or a contiguous int32 tensor of B = ", B, " entries or of one, got ", new_lens->numel());
    nl = new_lens->data_ptr<int32_t>(), nl_count = (int32_t)new_lens->numel();
  }
  check_source_strides(what, "q", q);
  TORCH_CHECK(block_ids.is_contiguous() && block_ids.numel() == B * Hkv * X * K && block_counts.is_contiguous() &&
                  block_counts.numel() == B * Hkv * X,
              what, ": block_ids must be a contiguous [B, Hkv, ceil(T/64) + 1, K] and block_counts a contiguous [B, Hkv, ceil(T/64) + 1] tensor");
  float* sc = nullptr;
  if (scores.has_value()) {
    check_device_f32(*scores, "scores");
    check_same_device(what, q.device(), {&*scores});
    TORCH_CHECK(scores->is_contiguous() && scores->numel() == B * Hkv * X * blocks, what,
                ": scores must be a contiguous [B, Hkv, ceil(T/64) + 1, Smax/64] tensor");
    sc = scores->data_ptr<float>();
  }
  check_sizes(what, {B * Hkv, B * Hq, T, blocks * 64, D, B * Hkv * X});
  TORCH_CHECK(B * Hkv * X * K <= INT64_MAX / 4, what, ": block_ids too large");
  if (block_counts.numel() == 0) return;
  c10::hip::HIPGuard guard(q.device().index());
  const int st = (bf ? mi_block_select_tiles_bf16 : mi_block_select_tiles_f16)(
      (int32_t)(B * Hkv), (int32_t)Hkv, (int32_t)T, (int32_t)(blocks * 64), (int32_t)D, (int32_t)group,
      static_cast<const uint16_t*>(q.data_ptr()), cache_stride(q, 2, D), cache_stride(q, 1, 0), cache_stride(q, 0, 0),
      static_cast<const uint16_t*>(bounds.data_ptr()), k_lens.data_ptr<int32_t>(), (int32_t)k_lens.numel(), nl, nl_count, (int32_t)K,
      (int32_t)sink, (int32_t)local, block_ids.data_ptr<int32_t>(), block_counts.data_ptr<int32_t>(), sc, stream_of(q));
  check_status(st, what);
}
