"""matmuls.block_sparse_attention_decode on the MI355X: the T newest tokens of every item against a
strided key / value cache, the list of the token's layout row cut into chunks that are merged in order.  Accuracy is the
project's rule e_dev ≤ 8 · e_ref (sparse_attention_helpers) against dense masked attention in float64 under the mask built
here from the visibility rule, the yardstick the same in fp32 narrowed as dense_step narrows it; everything else is bit
for bit: a strided cache against its contiguous clone, an item of a batch against the call on it alone, a shared layout
against a repeated one, block = 128 against the 64-block layout expanded here, a graph replay against the eager call.

Smax = 512 (8 blocks), B · Hkv ≤ 8; chunk=2 wherever the split matters: several chunks, chunks with fewer entries than
waves, empty trailing chunks.  Long lists (16 and 64 entries: three and more turns per wave, up to 64 partials) live in
tests/test_gpu_block_attention_decode_long.py."""
import ctypes

import pytest
import torch

from gpu_helpers import SENTINEL, assert_outside_untouched, assert_same_bits, padded
from sparse_attention_helpers import assert_tensor_under_rule, dense_step, rel_err

pytestmark = pytest.mark.gpu

SMAX = 512
NAN = float("nan")
# The 64-block lists of the 8 layout rows: unsorted, the diagonal block never last where there is another, and entries
# above the diagonal (wholly beyond every pos of the row: skipped inside their chunk, they do not move the cut).
# Adjacent rows see different keys at their crossing (row 0 sees block 0, row 1 does not; row 2 sees blocks 0 and 1), so a
# token with k_len = 64 or 128 tells the layout row of pos from the row of k_len.
ROWS = [[3, 0], [1, 4], [2, 5, 0, 1], [1, 3, 0], [4, 0, 7, 2, 3], [5, 1, 0, 4, 3], [2, 6, 0, 5], [3, 7, 0, 5, 1, 6, 2, 4]]
ROWS_B = [[0, 5], [0, 1], [1, 2, 0, 6], [3, 2, 1], [0, 4, 3, 1, 2], [2, 5, 3, 0, 1], [6, 1, 5, 4], [7, 6, 5, 4, 3, 2, 1, 0]]


def layout_from_rows(rows_cols, dev):
    """A 2-d CSR block layout (values 1) from per-block-row column lists, kept in the order given."""
    crow = [0]
    for c in rows_cols:
        crow.append(crow[-1] + len(c))
    col = [j for c in rows_cols for j in c]
    n = len(rows_cols)
    return torch.sparse_csr_tensor(torch.tensor(crow, device=dev), torch.tensor(col, device=dev), torch.ones(len(col), device=dev),
                                   size=(n, n))


def stack_layouts(items, lead, dev):
    """2-d layouts of equal entry counts as one batched layout [*lead, rows, cols]."""
    crow = torch.stack([l.crow_indices() for l in items]).reshape(lead + (-1,))
    col = torch.stack([l.col_indices() for l in items]).reshape(lead + (-1,))
    return torch.sparse_csr_tensor(crow, col, torch.ones(col.shape, device=dev), size=lead + tuple(items[0].shape))


def visible(rows_per_item, B, Hkv, T, k_lens, block=64, smax=SMAX):
    """Boolean CPU mask [B, Hkv, T, Smax] from the rule alone: token t of item b stands at pos = k_len − T + t and sees key
    j iff j ≤ pos and the list of block row pos // block of its k / v item's layout holds j // block."""
    vis = torch.zeros(B, Hkv, T, smax, dtype=torch.bool)
    for b in range(B):
        for h in range(Hkv):
            rows = rows_per_item[(b * Hkv + h) % len(rows_per_item)]
            for t in range(T):
                pos = min(max(k_lens[b], 0), smax) - T + t
                if pos < 0:
                    continue
                for J in rows[pos // block]:
                    lo, hi = J * block, min((J + 1) * block, pos + 1)
                    if lo < hi:
                        vis[b, h, t, lo:hi] = True
    return vis


def operands(dev, B, Hkv, G, T, D, dtype, seed, smax=SMAX):
    g = torch.Generator(device=dev).manual_seed(seed)
    q = torch.randn((B, Hkv * G, T, D), device=dev, generator=g).to(dtype)
    k, v = (torch.randn((B, Hkv, smax, D), device=dev, generator=g).to(dtype) for _ in range(2))
    return q, k, v


def poison_unseen(x, vis):
    """A copy of the cache tensor x [B, Hkv, Smax, D] with NaN in every key no token of its item sees: the never-listed
    blocks, the positions beyond pos (so everything at or beyond k_len)."""
    x = x.clone()
    x[~vis.any(2).to(x.device)] = NAN
    return x


def references(q, k, v, vis, G):
    """(float64 reference, fp32 yardstick narrowed to q's dtype, float64 lse) of dense masked attention, rows that see
    nothing zero (lse −inf); k and v clean."""
    mask = vis.repeat_interleave(G, 1)
    scale = 1.0 / q.shape[-1] ** 0.5
    kr, vr = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
    w = torch.zeros_like(q)
    ref = dense_step(q, kr, vr, w, mask, scale, torch.float64)[0]
    yard = dense_step(q, kr, vr, w, mask, scale, torch.float32, narrow=q.dtype)[0]
    s = (scale * (q.cpu().double() @ kr.cpu().double().transpose(-1, -2))).masked_fill(~mask, -float("inf"))
    empty = ~mask.any(-1)
    lse = torch.logsumexp(s.masked_fill(empty[..., None], 0.0), -1).masked_fill(empty, -float("inf"))
    return ref, yard, lse


def check_rule(what, out, q, k, v, vis, G, lse=None):
    ref, yard, lse64 = references(q, k, v, vis, G)
    assert out.dtype == q.dtype and out.shape == q.shape, what
    assert torch.isfinite(out.float()).all(), what
    assert_tensor_under_rule(f"block attention decode {what} out", out, yard, ref)
    seen = vis.any(-1).repeat_interleave(G, 1)
    assert (out.cpu()[~seen] == 0).all(), f"{what}: a token that sees nothing is a zero row"
    if lse is not None:
        lse = lse.cpu()
        assert lse.dtype == torch.float32 and (lse[~seen] == -float("inf")).all(), what
        e = rel_err(lse[seen].double().numpy(), lse64[seen].numpy())
        print(f"block attention decode {what} lse: max rel err {e:.3e}")
        assert e <= 1e-5, f"{what}: lse differs from float64 by {e:.3e} relative"
    return ref, yard


def lens_tensor(k_lens, dev, dtype=torch.int32):
    return torch.tensor(k_lens, device=dev, dtype=dtype)


# ---- 1. all 8 forms ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [32, 64, 96, 128])
def test_1_all_forms_on_unsorted_lists_in_chunks_of_two(mm, dev, dtype, D):
    """pos = 511: the 8-entry list in four chunks of two entries (fewer than waves); pos = 199: three entries, of which
    the second chunk holds one, and two empty trailing chunks."""
    B, Hkv, G, T, k_lens = 2, 2, 4, 1, [512, 200]
    layout = layout_from_rows(ROWS, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 500 + D)
    vis = visible([ROWS], B, Hkv, T, k_lens)
    out, lse = mm.block_sparse_attention_decode(q, k, v, layout, lens_tensor(k_lens, dev), chunk=2, return_lse=True)
    assert not out.requires_grad
    check_rule(f"form {dtype} D={D}", out, q, k, v, vis, G, lse)


# ---- 2. group sizes, T = 3 across a block boundary ----------------------------------------------------------------------

@pytest.mark.parametrize("G", [1, 5, 16])
def test_2_group_sizes_and_three_tokens_across_a_block_boundary(mm, dev, G):
    """k_lens 1, 64, 65, 130, 512, 0 with T = 3: tokens that do not exist (pos < 0), the tokens of one call in two layout
    rows (65: pos 62, 63, 64; 130: 127, 128, 129), a whole zero item.  The keys of the later new tokens point along the
    first token's query (scores near +2·√D above the rest) with values near 30: a token that saw a later one would show."""
    B, Hkv, T, D, dtype, k_lens = 6, 1, 3, 64, torch.bfloat16, [1, 64, 65, 130, 512, 0]
    layout = layout_from_rows(ROWS, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 520 + G)
    for b, n in enumerate(k_lens):
        for t in range(1, T):
            if n - T + t >= 1:
                k[b, 0, n - T + t] = 2.0 * q[b, 0, 0]
                v[b, 0, n - T + t] = 30.0 + t
    vis = visible([ROWS], B, Hkv, T, k_lens)
    out, lse = mm.block_sparse_attention_decode(q, k, v, layout, lens_tensor(k_lens, dev, torch.int64), chunk=2, return_lse=True)
    check_rule(f"G={G} T=3", out, q, k, v, vis, G, lse)
    assert (out[5] == 0).all() and (lse[5] == -float("inf")).all()           # k_len = 0
    assert (out[0, :, :2] == 0).all() and (lse[0, :, :2] == -float("inf")).all()  # k_len = 1 < T: tokens 0 and 1 do not exist
    assert torch.isfinite(lse[0, :, 2]).all() and torch.isfinite(lse[1:5]).all()
    assert_same_bits(out[0, :, 2], v[0, 0, 0].expand(G, D), "one visible key: its value row")


# ---- 3. nothing outside is read -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["BHSD", "BSHD"])
def test_3_nothing_outside_is_read(mm, dev, form):
    """NaN in every key no token sees (never-listed blocks, positions beyond pos and so at or beyond k_len) and between
    the rows of the cache (row stride D + 8 in a buffer of NaN), for [B, Hkv, Smax, D] and the transposed view of
    [B, Smax, Hkv, D]: out is finite, under the rule, and has the bits of the call on a contiguous clone."""
    B, Hkv, G, T, D, dtype, k_lens = 2, 2, 4, 2, 64, torch.float16, [130, 449]
    layout = layout_from_rows(ROWS, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 541)
    vis = visible([ROWS], B, Hkv, T, k_lens)

    def strided(x):
        shape = (B, Hkv, SMAX, D + 8) if form == "BHSD" else (B, SMAX, Hkv, D + 8)
        buf = torch.full(shape, NAN, device=dev, dtype=dtype)
        view = buf[..., :D] if form == "BHSD" else buf[..., :D].transpose(1, 2)
        view.copy_(poison_unseen(x, vis))
        return view

    ks, vs = strided(k), strided(v)
    assert not ks.is_contiguous() and ks.stride(2) > D and ks.shape == k.shape
    lens = lens_tensor(k_lens, dev)
    ptrs = (ks.data_ptr(), vs.data_ptr())
    out, lse = mm.block_sparse_attention_decode(q, ks, vs, layout, lens, chunk=2, return_lse=True)
    assert (ks.data_ptr(), vs.data_ptr()) == ptrs
    check_rule(f"poisoned {form} cache", out, q, k, v, vis, G, lse)
    clone = mm.block_sparse_attention_decode(q, ks.contiguous(), vs.contiguous(), layout, lens, chunk=2, return_lse=True)
    assert_same_bits(out, clone[0], f"{form}: the strided cache against its contiguous clone")
    assert_same_bits(lse, clone[1], f"{form}: lse")


# ---- 4. batch and layout independence, bit for bit ---------------------------------------------------------------------------

def test_4_an_item_of_a_batch_is_the_call_on_it_alone(mm, dev):
    B, Hkv, G, T, D, dtype, k_lens = 6, 1, 4, 2, 128, torch.bfloat16, [512, 65, 300, 1, 129, 448]
    layout = layout_from_rows(ROWS, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 557)
    lens = lens_tensor(k_lens, dev)
    out, lse = mm.block_sparse_attention_decode(q, k, v, layout, lens, chunk=2, return_lse=True)
    check_rule("batch of 6", out, q, k, v, visible([ROWS], B, Hkv, T, k_lens), G, lse)
    for b in range(B):
        one = mm.block_sparse_attention_decode(q[b:b + 1], k[b:b + 1], v[b:b + 1], layout, lens[b:b + 1], chunk=2, return_lse=True)
        assert_same_bits(out[b:b + 1], one[0], f"item {b} alone")
        assert_same_bits(lse[b:b + 1], one[1], f"item {b} alone: lse")
        zero_d = mm.block_sparse_attention_decode(q[b:b + 1], k[b:b + 1], v[b:b + 1], layout, lens[b], chunk=2)
        assert_same_bits(out[b:b + 1], zero_d, f"item {b} alone, its length 0-d")


def test_4_shared_layout_against_per_item_layouts(mm, dev):
    B, Hkv, G, T, D, dtype, k_lens = 3, 2, 2, 1, 96, torch.float16, [512, 200, 333]
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 563)
    lens = lens_tensor(k_lens, dev)
    a, b = layout_from_rows(ROWS, dev), layout_from_rows(ROWS_B, dev)
    shared = mm.block_sparse_attention_decode(q, k, v, a, lens, chunk=2)
    repeated = mm.block_sparse_attention_decode(q, k, v, stack_layouts([a] * 6, (B, Hkv), dev), lens, chunk=2)
    assert_same_bits(repeated, shared, "the layout repeated per item")
    # per k / v head: the query heads of a group share their k / v head's layout
    per_head = mm.block_sparse_attention_decode(q, k, v, stack_layouts([a, b], (Hkv,), dev), lens, chunk=2)
    check_rule("a layout per k / v head", per_head, q, k, v, visible([ROWS, ROWS_B], B, Hkv, T, k_lens), G)
    assert_same_bits(per_head[:, :G], shared[:, :G], "k / v head 0 keeps layout a")
    only_b = mm.block_sparse_attention_decode(q, k, v, b, lens, chunk=2)
    assert_same_bits(per_head[:, G:], only_b[:, G:], "k / v head 1 has layout b")
    # per item, indexed by the k / v item b · Hkv + h
    mixed = [ROWS, ROWS_B, ROWS_B, ROWS, ROWS, ROWS_B]
    per_item = mm.block_sparse_attention_decode(
        q, k, v, stack_layouts([layout_from_rows(r, dev) for r in mixed], (B, Hkv), dev), lens, chunk=2)
    check_rule("a layout per k / v item", per_item, q, k, v, visible(mixed, B, Hkv, T, k_lens), G)


def test_4_block_128_is_the_expanded_64_block_layout(mm, dev):
    B, Hkv, G, T, D, dtype, k_lens = 2, 2, 4, 3, 64, torch.bfloat16, [258, 512]
    rows128 = [[0], [1, 0], [0, 2, 1], [2, 3, 0]]
    expanded = [[x for c in rows128[i // 2] for x in (2 * c, 2 * c + 1)] for i in range(8)]  # sub-block order
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 569)
    lens = lens_tensor(k_lens, dev)
    coarse = mm.block_sparse_attention_decode(q, k, v, layout_from_rows(rows128, dev), lens, block=128, chunk=2, return_lse=True)
    fine = mm.block_sparse_attention_decode(q, k, v, layout_from_rows(expanded, dev), lens, block=64, chunk=2, return_lse=True)
    assert_same_bits(coarse[0], fine[0], "block = 128 against the expanded layout")
    assert_same_bits(coarse[1], fine[1], "block = 128 against the expanded layout: lse")
    check_rule("block = 128", coarse[0], q, k, v, visible([rows128], B, Hkv, T, k_lens, block=128), G, coarse[1])


# ---- 5. the split -----------------------------------------------------------------------------------------------------

def test_5_every_chunk_size_and_the_prefill_rows(mm, dev):
    """One 8-entry list (layout row 7, pos 509 … 511) under chunk 1, 2, 3, 8 and 64 — 8 and 64 are one chunk: the walk
    stores out itself, no combine launch — each under the rule, lse to 1e-5 of float64; and the same rows of the causal
    block_sparse_attention call on the full sequence under the rule against the same reference."""
    B, Hkv, G, T, D, dtype, k_lens = 2, 2, 4, 3, 128, torch.bfloat16, [512, 512]
    layout = layout_from_rows(ROWS, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 577)
    lens = lens_tensor(k_lens, dev)
    vis = visible([ROWS], B, Hkv, T, k_lens)
    ref, yard, _ = references(q, k, v, vis, G)
    results = {}
    for chunk in (1, 2, 3, 8, 64):
        out, lse = mm.block_sparse_attention_decode(q, k, v, layout, lens, chunk=chunk, return_lse=True)
        check_rule(f"chunk={chunk}", out, q, k, v, vis, G, lse)
        results[chunk] = out
    assert_same_bits(results[8], results[64], "one chunk either way")
    default = mm.block_sparse_attention_decode(q, k, v, layout, lens)
    assert_same_bits(default, mm.block_sparse_attention_decode(q, k, v, layout, lens, chunk=mm._decode_chunk(SMAX, D)), "chunk=None")
    full = torch.randn((B, Hkv * G, SMAX, D), device=dev, generator=torch.Generator(device=dev).manual_seed(578)).to(dtype)
    full[:, :, SMAX - T:] = q
    prefill = mm.block_sparse_attention(full, k, v, layout, causal=True, k_lens=lens)[:, :, SMAX - T:]
    assert_tensor_under_rule("block attention decode: the prefill call's last rows", prefill, yard, ref)


# ---- 6. graph capture -------------------------------------------------------------------------------------------------

def test_6_one_graph_replayed_while_the_cache_grows(mm, dev):
    """One capture; before every replay k_lens is incremented in place, the new token's key / value row is written into
    the cache and its query into q: the replay gives the bits of the eager call on the new state, through the step where
    pos crosses into the next layout row (63 → 64 for item 0, 127 → 128 for item 1)."""
    B, Hkv, G, T, D, dtype = 2, 2, 4, 1, 64, torch.float16
    layout = layout_from_rows(ROWS, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 587)
    lens = lens_tensor([63, 127], dev, torch.int64)
    g = torch.Generator(device=dev).manual_seed(588)
    run = lambda: mm.block_sparse_attention_decode(q, k, v, layout, lens, chunk=2, return_lse=True)  # noqa: E731
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()  # warm-up on the side stream: the layout's lists are built here
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # a host synchronisation in here would fail the capture
        out, lse = run()
    previous = None
    for step, host_lens in enumerate(([64, 128], [65, 129], [66, 130])):
        with torch.no_grad():
            lens += 1
            for b, n in enumerate(host_lens):
                k[b, :, n - 1] = torch.randn((Hkv, D), device=dev, generator=g).to(dtype)
                v[b, :, n - 1] = torch.randn((Hkv, D), device=dev, generator=g).to(dtype)
            q.copy_(torch.randn(q.shape, device=dev, generator=g).to(dtype))
        assert lens.tolist() == host_lens
        want = run()
        out.fill_(NAN)
        lse.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert_same_bits(out, want[0], f"replay {step}, k_lens {host_lens}")
        assert_same_bits(lse, want[1], f"replay {step}: lse")
        check_rule(f"replay {step}", out, q, k, v, visible([ROWS], B, Hkv, T, host_lens), G)  # (lse: its bits, above)
        assert previous is None or not torch.equal(previous, out)
        previous = out.clone()


# ---- 7. the C ABI -------------------------------------------------------------------------------------------------------

def _decode_entry(capi, dtype):
    vp, i64, i32, f32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_size_t
    fn = getattr(capi, "mi_block_attention_decode_" + {torch.bfloat16: "bf16", torch.float16: "f16"}[dtype])
    fn.argtypes = [vp, vp, i64] + 6 * [i32] + [vp, i64, i64] + 2 * [vp, i64, i64, i64] + [vp, i32, i32, i32, f32] + \
        [vp, i64, i64, vp, vp, sz, vp]
    fn.restype = ctypes.c_int
    capi.mi_block_attention_decode_workspace_bytes.argtypes = 6 * [i32]
    capi.mi_block_attention_decode_workspace_bytes.restype = sz
    return fn


@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 96), (torch.float16, 32)])
def test_7_c_abi_refusals_and_one_padded_call(mm, capi, dev, dtype, D):
    """MI_EINVAL / MI_ENOMEM without a launch (the outputs keep their sentinel), then one call on operands with leading
    dimensions and strides of their own — NaN around the inputs, SENTINEL around out, lse and the workspace —: the bits of
    the call through matmuls, nothing outside touched."""
    B, Hkv, G, T, k_lens, chunk = 2, 2, 5, 2, [130, 512], 2
    items, Hq = B * Hkv, Hkv * G
    layout = layout_from_rows(ROWS, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 593 + D)
    vis = visible([ROWS], B, Hkv, T, k_lens)
    lens = lens_tensor(k_lens, dev)
    want = mm.block_sparse_attention_decode(q, k, v, layout, lens, chunk=chunk, return_lse=True)
    offsets, columns, nnz, L = mm._block_layout(layout, dev, 1, mm._csr_state(layout))["fwd"]
    fn = _decode_entry(capi, dtype)
    pq = padded(q.reshape(items * G, T, D), 0, NAN)
    pk, pv = (padded(poison_unseen(x, vis).reshape(items, SMAX, D), i, NAN) for i, x in ((1, k), (2, v)))
    pout = padded(torch.full((items * G, T, D), SENTINEL, device=dev, dtype=dtype), 3, SENTINEL)
    lse_buf = torch.full((B * Hq * T + 16,), SENTINEL, device=dev)
    lse = lse_buf[8:8 + B * Hq * T]
    ws_bytes = capi.mi_block_attention_decode_workspace_bytes(items, T, G, D, SMAX, chunk)
    assert ws_bytes == items * T * 4 * G * (D + 2) * 4
    ws_buf = torch.full((ws_bytes + 32,), 0xAB, device=dev, dtype=torch.uint8)
    stream = torch.cuda.current_stream().cuda_stream
    scale = 1.0 / D ** 0.5

    def call(group=G, chunk=chunk, items=items, T=T, D=D, q_ptr=pq.buf.data_ptr(), ldk=pk.ld, ws_bytes=ws_bytes):
        return fn(offsets.data_ptr(), columns.data_ptr(), nnz, L, items, Hkv, T, SMAX, D, q_ptr, pq.ld, pq.stride,
                  pk.buf.data_ptr(), ldk, pk.stride, Hkv * pk.stride, pv.buf.data_ptr(), pv.ld, pv.stride, Hkv * pv.stride,
                  lens.data_ptr(), B, group, chunk, scale, pout.buf.data_ptr(), pout.ld, pout.stride, lse.data_ptr(),
                  ws_buf.data_ptr() + 16, ws_bytes, stream)

    for kw in ({"group": 0}, {"group": 17}, {"D": 48}, {"chunk": 0}, {"items": 65536}, {"T": 65536}, {"q_ptr": pq.buf.data_ptr() + 2},
               {"ldk": pk.ld + 4}):
        assert call(**kw) == -1, kw   # MI_EINVAL
    assert call(ws_bytes=ws_bytes - 1) == -4  # MI_ENOMEM
    torch.cuda.synchronize()
    assert_same_bits(pout.buf, torch.full_like(pout.buf, SENTINEL), "a refused call launches nothing")
    assert call() == 0
    torch.cuda.synchronize()
    assert_outside_untouched(pout, "out")
    assert_same_bits(pout.x.reshape(B, Hq, T, D), want[0], f"{dtype} D={D} through the C ABI: out")
    assert_same_bits(lse.reshape(B, Hq, T), want[1], "through the C ABI: lse")
    rest = torch.cat([lse_buf[:8], lse_buf[8 + B * Hq * T:]])
    assert_same_bits(rest, torch.full_like(rest, SENTINEL), "around lse")
    guard = torch.cat([ws_buf[:16], ws_buf[16 + ws_bytes:]])
    assert (guard == 0xAB).all(), "around the workspace"
    assert torch.isfinite(pout.x.float()).all()
