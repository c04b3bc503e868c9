"""matmuls.block_sparse_attention_prefill and its paged / fp8 forms on the MI355X: the T newest tokens of
every item — a whole prompt or a chunk of it — against the KV cache, in 64-row position tiles that walk the list of their
layout row as the causal training forward walks it.

The contract is bit for bit: the out and lse rows of existing tokens are those of custom_mm.block_attention_forward_ex with
causal=True and q_lens = k_lens = lens on the (gathered, widened) cache, q scattered to its positions in a [B·Hq, Smax, D]
tensor and the layout repeated per query head.  From it: a paged call equals the contiguous call on the gathered cache, an
fp8 call without scales the 2-byte call on the widened cache, a strided cache its contiguous clone; a row's bits depend on its
item's operands, its list and pos — never on T, new_lens, B, the neighbours or the launch.  Accuracy is the project's rule
e_dev ≤ 8 · e_ref (sparse_attention_helpers) against dense masked attention in float64 under the mask built from the rule, and
lse within 1e-5 of float64: no new tolerance.  Smax = 512, Smax / 64 = 8 blocks; the lists (ROWS) are the decode tests'.
The ratios are printed (MI_SOFTMAX_LOG collects them: profiles/r26_block_attention_prefill_forms.log)."""
import ctypes

import pytest
import torch

from gpu_helpers import SENTINEL, assert_outside_untouched, assert_same_bits, padded
from sparse_attention_helpers import FACTOR, rel_err, scaled_err
from test_gpu_block_attention_decode import (ROWS, ROWS_B, SMAX, check_rule, layout_from_rows, lens_tensor, operands, poison_unseen,
                                             references, stack_layouts, visible)
from test_gpu_block_attention_decode_fp8 import codes, fp8, pools, wide
from test_gpu_block_attention_decode_paged import gathered, paged

pytestmark = pytest.mark.gpu

NAN = float("nan")
KB = 64
LSE_BOUND = 1e-5  # check_rule's bound on lse, relative to float64
WIDTHS = [32, 64, 96, 128]
DTYPES = [torch.bfloat16, torch.float16]


def clamp(n, lo, hi):
    return min(max(int(n), lo), hi)


def visible_new(rows_per_item, B, Hkv, T, k_lens, new_lens=None, block=64):
    """`visible` with new_lens: slot t of item b holds a token iff t ≥ T − clamp(new_lens[b], 0, T) (and pos ≥ 0)."""
    vis = visible(rows_per_item, B, Hkv, T, k_lens, block)
    if new_lens is not None:
        for b in range(B):
            vis[b, :, :T - clamp(new_lens[b], 0, T)] = False
    return vis


def tokens(T, k_len, new_len=None):
    """(first slot, first position, count) of the existing tokens of an item."""
    n = clamp(k_len, 0, SMAX)
    lo = max(n - (T if new_len is None else clamp(new_len, 0, T)), 0)
    return T - (n - lo), lo, n - lo


def training_forward(mm, q, k, v, rows_per_item, k_lens, new_lens=None, scale=None):
    """(out, lse) [B, Hq, T, …] of custom_mm.block_attention_forward_ex, causal, q_lens = k_lens = lens, on the cache k, v
    [B, Hkv, Smax, D], q scattered to its positions in [B·Hq, Smax, D], the layout repeated per query head; rows of slots
    without a token: zero and −inf, as the prefill call gives them."""
    B, Hq, T, D = q.shape
    Hkv = k.shape[1]
    G, dev = Hq // Hkv, q.device
    full = torch.zeros((B, Hq, SMAX, D), device=dev, dtype=q.dtype)
    for b in range(B):
        t0, lo, n = tokens(T, k_lens[b], None if new_lens is None else new_lens[b])
        full[b, :, lo:lo + n] = q[b, :, t0:t0 + n]
    if len(rows_per_item) == 1:
        layout = layout_from_rows(rows_per_item[0], dev)
    else:  # indexed by the query item b · Hq + h · G + g
        per_q = [layout_from_rows(rows_per_item[(b * Hkv + h) % len(rows_per_item)], dev) for b in range(B) for h in range(Hkv) for _ in range(G)]
        layout = stack_layouts(per_q, (B * Hq,), dev)
    offsets, columns, nnz, _ = mm._block_layout(layout, dev, 1, mm._csr_state(layout))["fwd"]
    lens = torch.tensor([clamp(n, 0, SMAX) for n in k_lens], device=dev, dtype=torch.int32)
    o3 = torch.empty((B * Hq, SMAX, D), device=dev, dtype=q.dtype)
    l3 = torch.empty((B * Hq, SMAX), device=dev, dtype=torch.float32)
    mm.custom_mm.block_attention_forward_ex(offsets, columns, nnz, full.reshape(B * Hq, SMAX, D), k.reshape(B * Hkv, SMAX, D).contiguous(),
                                            v.reshape(B * Hkv, SMAX, D).contiguous(), float(scale or 1.0 / D ** 0.5), True, o3, l3, lens, lens)
    out = torch.zeros_like(q)
    lse = torch.full((B, Hq, T), -float("inf"), device=dev)
    o4, l4 = o3.reshape(B, Hq, SMAX, D), l3.reshape(B, Hq, SMAX)
    for b in range(B):
        t0, lo, n = tokens(T, k_lens[b], None if new_lens is None else new_lens[b])
        out[b, :, t0:t0 + n] = o4[b, :, lo:lo + n]
        lse[b, :, t0:t0 + n] = l4[b, :, lo:lo + n]
    return out, lse


def same(got, want, what):
    assert_same_bits(got[0], want[0], f"{what}: out")
    assert_same_bits(got[1], want[1], f"{what}: lse")


# ---- the classes of a call and the CPU proofs ------------------------------------------------------------------------------

def tile_classes(B, Hq, T, k_lens):
    """{name: Boolean [B, Hq, T]}: the rows of one (item, query head, position tile) that hold a token."""
    classes = {}
    for b in range(B):
        t0, lo, n = tokens(T, k_lens[b])
        pos = torch.arange(T) + (clamp(k_lens[b], 0, SMAX) - T)
        for h in range(Hq):
            for r in range(lo // KB, (lo + n - 1) // KB + 1 if n else 0):
                m = torch.zeros(B, Hq, T, dtype=torch.bool)
                m[b, h] = (pos >= max(lo, r * KB)) & (pos < (r + 1) * KB)
                classes[f"item {b} head {h} tile {r}"] = m
    return classes


def dense64(q, k, v, mask, G, scale):
    """float64 dense masked attention on the CPU: (out, lse); mask Boolean [B, Hkv, T, Smax]; rows that see nothing: 0, −inf."""
    m = mask.repeat_interleave(G, 1)
    qd, kd, vd = q.cpu().double(), k.cpu().double().repeat_interleave(G, 1), v.cpu().double().repeat_interleave(G, 1)
    s = (scale * (qd @ kd.transpose(-1, -2))).masked_fill(~m, -float("inf"))
    empty = ~m.any(-1)
    lse = torch.logsumexp(s.masked_fill(empty[..., None], 0.0), -1).masked_fill(empty, -float("inf"))
    p = torch.softmax(s.masked_fill(empty[..., None], 0.0), -1).masked_fill(empty[..., None], 0.0)
    return p @ vd, lse


def mistaken_masks(rows, B, Hkv, T, k_lens):
    """The masks three mistaken kernels would apply, by name."""
    masks = {name: torch.zeros(B, Hkv, T, SMAX, dtype=torch.bool) for name in ("diagonal mask from t", "row of the first token", "dropped entry")}
    for b in range(B):
        n = clamp(k_lens[b], 0, SMAX)
        start = n - T
        for t in range(T):
            pos = start + t
            if pos < 0:
                continue
            r = pos // KB
            for name, m in masks.items():
                row = r
                if name == "row of the first token":  # tiles cut by t, not by pos: the row of the tile's first token
                    row = max(start, 0) // KB + (t // KB) if start >= 0 else r
                lst = [J for J in rows[row] if J <= row]
                if name == "dropped entry":
                    lst = lst[:-1]
                for J in lst:
                    hi = min((J + 1) * KB, pos + 1)
                    if name == "diagonal mask from t" and J == r:  # own row t % 64 of the tile instead of pos % 64
                        hi = min(J * KB + (t % KB) + 1, n)
                    if J * KB < hi:
                        m[b, :, t, J * KB:hi] = True
    return masks


def prove_the_checks_see_three_mistakes(what, q, k, v, rows, k_lens, G, ref, yard, lse64):
    """On the test's own inputs, in float64: each mistake moves out beyond FACTOR · e_ref of some class, or lse beyond its
    bound there.  Prints the margins (in bounds)."""
    B, Hq, T, D = q.shape
    classes = tile_classes(B, Hq, T, k_lens)
    ref, yard = ref.numpy(), yard.double().numpy()
    for name, mask in mistaken_masks(rows, B, q.shape[1] // G, T, k_lens).items():
        wrong, wrong_lse = dense64(q, k, v, mask, G, 1.0 / D ** 0.5)
        best_out, best_lse = 0.0, 0.0
        for rows_of in classes.values():
            m = rows_of.numpy()
            e_ref = scaled_err(yard[m], ref[m])
            best_out = max(best_out, scaled_err(wrong.numpy()[m], ref[m]) / (FACTOR * e_ref))
            best_lse = max(best_lse, rel_err(wrong_lse.numpy()[m], lse64.numpy()[m]) / LSE_BOUND)
        print(f"block attention prefill {what} proof '{name}': out {best_out:.1f} bounds, lse {best_lse:.1f} bounds")
        assert max(best_out, best_lse) > 1.0, f"{what}: the checks would not see '{name}'"


def check_classes(what, out, lse, ref, yard, lse64, k_lens):
    """The rule per class — the rows of one (item, query head, position tile) —, each against its OWN e_ref: no other class
    sets the floor."""
    B, Hq, T, _ = out.shape
    got, ref, yard = out.cpu().double().numpy(), ref.numpy(), yard.double().numpy()
    worst = 0.0
    for name, rows_of in tile_classes(B, Hq, T, k_lens).items():
        m = rows_of.numpy()
        e_ref, e_dev = scaled_err(yard[m], ref[m]), scaled_err(got[m], ref[m])
        worst = max(worst, e_dev / e_ref)
        assert e_dev <= FACTOR * e_ref, f"{what}, {name}: e_dev {e_dev:.3e} > {FACTOR:g} · e_ref {e_ref:.3e}"
        e = rel_err(lse.cpu().double().numpy()[m], lse64.numpy()[m])
        assert e <= LSE_BOUND, f"{what}, {name}: lse differs from float64 by {e:.3e} relative"
    print(f"block attention prefill {what}: worst class ratio {worst:.2f}")


# ---- 1. the bits of the training forward ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", WIDTHS)
def test_1_the_bits_of_the_training_forward(mm, dev, dtype, D):
    """T = 100 at k_lens [333, 512]: item 0 covers positions 233 … 332 — tiles 3 (rows 41 … 63), 4 (whole; its list holds
    block 7, above the diagonal) and 5 (rows 0 … 12) —, item 1 positions 412 … 511.  Before the device call the CPU proves
    in float64 that the checks see a diagonal mask taken from t (off by 41 rows), the layout row of a tile's first token used
    for its neighbour, and a dropped list entry.  Then T = 128 at [256, 512] (aligned), T = 512 (a whole prompt), T = 1."""
    B, Hkv, G = 2, 2, 2
    layout = layout_from_rows(ROWS, dev)
    assert 7 in ROWS[4]
    for T, k_lens in ((100, [333, 512]), (128, [256, 512]), (512, [512, 512]), (1, [333, 512])):
        what = f"{dtype} D={D} T={T}"
        q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 2600 + D + T)
        vis = visible([ROWS], B, Hkv, T, k_lens)
        if T == 100:
            ref, yard, lse64 = references(q, k, v, vis, G)
            prove_the_checks_see_three_mistakes(what, q, k, v, ROWS, k_lens, G, ref, yard, lse64)
        out, lse = mm.block_sparse_attention_prefill(q, k, v, layout, lens_tensor(k_lens, dev), return_lse=True)
        assert not out.requires_grad and out.is_contiguous()
        same((out, lse), training_forward(mm, q, k, v, [ROWS], k_lens), what + " against block_attention_forward_ex")
        check_rule("prefill " + what, out, q, k, v, vis, G, lse)
        if T == 100:
            check_classes(what, out, lse, ref, yard, lse64, k_lens)


# ---- 2. forms -----------------------------------------------------------------------------------------------------------

PAGED = [(page, WIDTHS[i % 4], DTYPES[i % 2]) for i, page in enumerate([16, 32, 64, 128, 256])]


@pytest.mark.parametrize("page,D,dtype", PAGED)
def test_2_paged_has_the_bits_of_the_contiguous_call_on_the_gathered_cache(mm, dev, page, D, dtype):
    B, Hkv, G, T, k_lens = 2, 2, 2, 100, [333, 512]
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 2700 + page)
    kp, vp, table = paged(k, v, page, 2701 + page)
    got = mm.block_sparse_attention_prefill_paged(q, kp, vp, table, layout, lens, return_lse=True)
    same(got, mm.block_sparse_attention_prefill(q, gathered(kp, table), gathered(vp, table), layout, lens, return_lse=True),
         f"page {page} D={D} {dtype}")
    check_rule(f"prefill paged {page} D={D} {dtype}", got[0], q, k, v, visible([ROWS], B, Hkv, T, k_lens), G, got[1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", WIDTHS)
def test_2_fp8_without_scales_has_the_bits_of_the_call_on_the_widened_cache(mm, dev, dtype, D):
    B, Hkv, G, T, k_lens = 2, 2, 2, 100, [333, 512]
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q = operands(dev, B, Hkv, G, T, D, dtype, 2710 + D)[0]
    kc, vc = codes(2711 + D, B, Hkv, SMAX, D), codes(2712 + D, B, Hkv, SMAX, D)
    want = mm.block_sparse_attention_prefill(q, wide(kc, dtype, dev), wide(vc, dtype, dev), layout, lens, return_lse=True)
    same(mm.block_sparse_attention_prefill_fp8(q, fp8(kc, dev), fp8(vc, dev), layout, lens, return_lse=True), want, f"fp8 D={D} {dtype}")
    page = [16, 64, 32, 256][WIDTHS.index(D)]
    kp, vp, table = pools(kc, vc, page, 2713 + D)
    same(mm.block_sparse_attention_prefill_paged_fp8(q, fp8(kp, dev), fp8(vp, dev), table.to(dev), layout, lens, return_lse=True), want,
         f"paged fp8 page {page} D={D} {dtype}")


@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 128), (torch.float16, 64)])
def test_2_fp8_with_per_head_scales_under_the_rule_on_the_scaled_cache(mm, dev, dtype, D):
    B, Hkv, G, T, k_lens = 2, 2, 2, 100, [333, 512]
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 2720 + D)
    k8, ks = mm.kv_to_fp8(k)
    v8, vs = mm.kv_to_fp8(v)
    real_k = k8.float() * ks.reshape(1, Hkv, 1, 1)  # float32: exact products of an e4m3fn value and a float32 scale are not T
    real_v = v8.float() * vs.reshape(1, Hkv, 1, 1)
    out, lse = mm.block_sparse_attention_prefill_fp8(q, k8, v8, layout, lens, k_scale=ks, v_scale=vs, return_lse=True)
    check_rule(f"prefill fp8 per-head scales D={D} {dtype}", out, q, real_k, real_v, visible([ROWS], B, Hkv, T, k_lens), G, lse)
    kp, vp, table = pools(k8.view(torch.uint8).cpu(), v8.view(torch.uint8).cpu(), 32, 2721)
    same(mm.block_sparse_attention_prefill_paged_fp8(q, fp8(kp, dev), fp8(vp, dev), table.to(dev), layout, lens, k_scale=ks, v_scale=vs,
                                                     return_lse=True), (out, lse),
         "paged fp8 with scales against the contiguous fp8 call")


# ---- 3. nothing outside is read or written -----------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["BHSD", "BSHD"])
def test_3_nothing_outside_the_cache_or_q_is_read(mm, dev, form):
    """NaN in every key no token sees and between the rows (row stride D + 8 in NaN buffers), [B, Hkv, Smax, D] and the
    [B, Smax, Hkv, D].transpose(1, 2) view; q as the slice of a fused projection full of NaN elsewhere: finite, under the
    rule, the bits of the call on the contiguous clones, data_ptrs unchanged."""
    B, Hkv, G, T, D, dtype, k_lens = 2, 2, 2, 100, 64, torch.float16, [333, 449]
    Hq = Hkv * G
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 2730)
    vis = visible([ROWS], B, Hkv, T, k_lens)

    def strided(x):
        shape = (B, Hkv, SMAX, D + 8) if form == "BHSD" else (B, SMAX, Hkv, D + 8)
        buf = torch.full(shape, NAN, device=dev, dtype=dtype)
        view = buf[..., :D] if form == "BHSD" else buf[..., :D].transpose(1, 2)
        view.copy_(poison_unseen(x, vis))
        return view

    ks, vs = strided(k), strided(v)
    fused = torch.full((B, T, Hq + 2 * Hkv, D), NAN, device=dev, dtype=dtype)
    fused[:, :, :Hq] = q.transpose(1, 2)
    qs = fused[:, :, :Hq].transpose(1, 2)
    assert not ks.is_contiguous() and not qs.is_contiguous() and qs.stride(2) == (Hq + 2 * Hkv) * D
    ptrs = (qs.data_ptr(), ks.data_ptr(), vs.data_ptr())
    out, lse = mm.block_sparse_attention_prefill(qs, ks, vs, layout, lens, return_lse=True)
    assert (qs.data_ptr(), ks.data_ptr(), vs.data_ptr()) == ptrs and out.is_contiguous()
    check_rule(f"prefill poisoned {form} cache", out, q, k, v, vis, G, lse)
    same((out, lse), mm.block_sparse_attention_prefill(qs.contiguous(), ks.contiguous(), vs.contiguous(), layout, lens, return_lse=True),
         f"{form}: strided operands against their contiguous clones")


@pytest.mark.parametrize("page", [16, 64])
def test_3_nothing_outside_the_pool_is_read(mm, dev, page):
    """Unreferenced pages NaN, the pages wholly beyond the largest pos behind −1 and P + 5 entries, [P, page, Hkv, D] with a
    row stride of D + 8 in a NaN buffer."""
    B, Hkv, G, T, D, dtype, k_lens = 2, 2, 2, 100, 96, torch.bfloat16, [333, 449]
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 2740 + page)
    vis = visible([ROWS], B, Hkv, T, k_lens)
    kp, vp, table = paged(poison_unseen(k, vis), poison_unseen(v, vis), page, 2741 + page)
    P = kp.shape[0]
    for b, n in enumerate(k_lens):
        beyond = torch.arange((n + page - 1) // page, SMAX // page, device=dev)
        kp[table[b, beyond].long()] = NAN
        vp[table[b, beyond].long()] = NAN
        table[b, beyond] = torch.where(beyond % 2 == 0, -1, P + 5).to(torch.int32)

    def strided(pool):
        buf = torch.full((P, page, Hkv, D + 8), NAN, device=dev, dtype=dtype)
        view = buf[..., :D].transpose(1, 2)
        view.copy_(pool)
        return view

    ks, vs = strided(kp), strided(vp)
    out, lse = mm.block_sparse_attention_prefill_paged(q, ks, vs, table, layout, lens, return_lse=True)
    check_rule(f"prefill poisoned pool, page {page}", out, q, k, v, vis, G, lse)
    same((out, lse), mm.block_sparse_attention_prefill(q, k, v, layout, lens, return_lse=True), f"page {page}: against the clean cache")


@pytest.mark.parametrize("page,fp8_cache", [(16, False), (64, False), (32, True), (128, True)])
def test_3_invalid_entries_hide_their_keys(mm, dev, page, fp8_cache):
    """−1 and P + 5 at SEEN logical pages — inside a diagonal block, inside a whole block of a list, in both items —: the keys of
    those pages are invisible (the rule on the mask without them) and nothing of the NaN pages they pointed to is loaded."""
    B, Hkv, G, T, D, dtype, k_lens = 2, 2, 2, 100, 64, torch.bfloat16, [333, 512]
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 2745 + page)
    if fp8_cache:
        k, v = (codes(2746 + i + page, B, Hkv, SMAX, D).view(torch.float8_e4m3fn).to(dtype).to(dev) for i in range(2))
    vis = visible([ROWS], B, Hkv, T, k_lens)
    # item 0: a page of tile 4's diagonal block and one of tile 5's (page 128 holds both: then the page of blocks 0 and 1);
    # item 1: a page of block 7, the diagonal of its last tile, and the page of block 0
    hidden = {0: [256 // page, 320 // page if page < 128 else 0], 1: [448 // page, 0]}
    assert all(len(set(ws)) == 2 for ws in hidden.values())
    kp, vp, table = paged(k, v, page, 2747 + page)
    P = kp.shape[0]
    for b, ws in hidden.items():
        for i, w in enumerate(ws):
            kp[table[b, w].long()] = NAN
            vp[table[b, w].long()] = NAN
            table[b, w] = (-1, P + 5)[i]
            vis[b, :, :, w * page:(w + 1) * page] = False
    if fp8_cache:
        kp8, vp8 = (x.nan_to_num(0.0).to(torch.float8_e4m3fn).view(torch.uint8) for x in (kp, vp))
        bad = torch.isnan(kp.float())
        kp8[bad], vp8[bad] = 0x7F, 0x7F
        out, lse = mm.block_sparse_attention_prefill_paged_fp8(q, kp8.view(torch.float8_e4m3fn), vp8.view(torch.float8_e4m3fn), table,
                                                               layout, lens, return_lse=True)
    else:
        out, lse = mm.block_sparse_attention_prefill_paged(q, kp, vp, table, layout, lens, return_lse=True)
    check_rule(f"prefill hidden pages, page {page}, fp8 {fp8_cache}", out, q, k, v, vis, G, lse)


def _prefill_entry(capi, dtype):
    vp, i64, i32, f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float
    fn = getattr(capi, "mi_block_attention_prefill_" + {torch.bfloat16: "bf16", torch.float16: "f16"}[dtype])
    fn.argtypes = [vp, vp, i64] + 6 * [i32] + 3 * [vp, i64, i64, i64] + [vp, i32, vp, i32, i32, f32] + [vp, i64, i64, vp, vp]
    fn.restype = ctypes.c_int
    return fn


@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 96), (torch.float16, 32)])
def test_3_nothing_outside_out_is_written_through_the_c_abi(mm, capi, dev, dtype, D):
    """out and lse inside sentinel buffers, the inputs inside NaN: a refused call launches nothing; one call writes every row
    of out and lse — the slots without a token too — and nothing else; the bits of the call through matmuls."""
    B, Hkv, G, T, k_lens, new_lens = 2, 2, 3, 100, [70, 512], [100, 37]
    items, Hq = B * Hkv, Hkv * G
    layout = layout_from_rows(ROWS, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 2750 + D)
    vis = visible_new([ROWS], B, Hkv, T, k_lens, new_lens)
    lens, news = lens_tensor(k_lens, dev), lens_tensor(new_lens, dev)
    want = mm.block_sparse_attention_prefill(q, k, v, layout, lens, new_lens=news, return_lse=True)
    offsets, columns, nnz, L = mm._block_layout(layout, dev, 1, mm._csr_state(layout))["fwd"]
    fn = _prefill_entry(capi, dtype)
    pq = padded(q.reshape(items * G, T, D), 0, NAN)
    pk, pv = (padded(poison_unseen(x, vis).reshape(items, SMAX, D), i, NAN) for i, x in ((1, k), (2, v)))
    pout = padded(torch.full((items * G, T, D), SENTINEL, device=dev, dtype=dtype), 3, SENTINEL)
    lse_buf = torch.full((B * Hq * T + 16,), SENTINEL, device=dev)
    lse = lse_buf[8:8 + B * Hq * T]
    stream = torch.cuda.current_stream().cuda_stream

    def call(group=G, D=D, q_ptr=pq.buf.data_ptr(), ldk=pk.ld, news_count=B):
        return fn(offsets.data_ptr(), columns.data_ptr(), nnz, L, items, Hkv, T, SMAX, D, q_ptr, pq.ld, pq.stride, Hq * pq.stride,
                  pk.buf.data_ptr(), ldk, pk.stride, Hkv * pk.stride, pv.buf.data_ptr(), pv.ld, pv.stride, Hkv * pv.stride,
                  lens.data_ptr(), B, news.data_ptr(), news_count, group, 1.0 / D ** 0.5, pout.buf.data_ptr(), pout.ld, pout.stride,
                  lse.data_ptr(), stream)

    for kw in ({"group": 0}, {"D": 48}, {"q_ptr": pq.buf.data_ptr() + 2}, {"ldk": pk.ld + 4}, {"news_count": 3}):
        assert call(**kw) == -1, kw   # MI_EINVAL
    torch.cuda.synchronize()
    assert_same_bits(pout.buf, torch.full_like(pout.buf, SENTINEL), "a refused call launches nothing")
    assert call() == 0
    torch.cuda.synchronize()
    assert_outside_untouched(pout, "out")
    assert (pout.x != SENTINEL).all() and (lse != SENTINEL).all(), "every row of out and lse is written"
    assert_same_bits(pout.x.reshape(B, Hq, T, D), want[0], f"{dtype} D={D} through the C ABI: out")
    assert_same_bits(lse.reshape(B, Hq, T), want[1], "through the C ABI: lse")
    rest = torch.cat([lse_buf[:8], lse_buf[8 + B * Hq * T:]])
    assert_same_bits(rest, torch.full_like(rest, SENTINEL), "around lse")


# ---- 4. tokens that do not exist -----------------------------------------------------------------------------------------

def test_4_slots_with_a_negative_position(mm, dev):
    """T = 200 at k_lens [130, 512]: the first 70 slots of item 0 have pos < 0 — zero rows, lse −inf —, the rest are bit for
    bit the call with T = 130 on the sliced q."""
    B, Hkv, G, T, D, dtype, k_lens = 2, 2, 2, 200, 64, torch.bfloat16, [130, 512]
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 2760)
    out, lse = mm.block_sparse_attention_prefill(q, k, v, layout, lens, return_lse=True)
    check_rule("prefill T=200, 70 slots with pos < 0", out, q, k, v, visible([ROWS], B, Hkv, T, k_lens), G, lse)
    assert (out[0, :, :70] == 0).all() and (lse[0, :, :70] == -float("inf")).all() and torch.isfinite(lse[0, :, 70:]).all()
    same((out[:1, :, 70:], lse[:1, :, 70:]),
         mm.block_sparse_attention_prefill(q[:1, :, 70:], k[:1], v[:1], layout, lens[:1], return_lse=True), "item 0 with T = 130")
    same((out, lse), training_forward(mm, q, k, v, [ROWS], k_lens), "against block_attention_forward_ex")


@pytest.mark.parametrize("dtype", DTYPES)
def test_4_new_lens(mm, dev, dtype):
    """new_lens = [0, 37, 100] with T = 100: zero rows and −inf in the slots ahead of the new tokens, the rows of existing
    tokens bit for bit those of the call with T = new_len on the sliced q; int64 and out-of-range entries are clamped."""
    B, Hkv, G, T, D, k_lens, new_lens = 3, 2, 2, 100, 128, [200, 333, 512], [0, 37, 100]
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 2770)
    out, lse = mm.block_sparse_attention_prefill(q, k, v, layout, lens, new_lens=lens_tensor(new_lens, dev), return_lse=True)
    vis = visible_new([ROWS], B, Hkv, T, k_lens, new_lens)
    check_rule(f"prefill new_lens {dtype}", out, q, k, v, vis, G, lse)
    same((out, lse), training_forward(mm, q, k, v, [ROWS], k_lens, new_lens), "against block_attention_forward_ex")
    for b, n in enumerate(new_lens):
        assert (out[b, :, :T - n] == 0).all() and (lse[b, :, :T - n] == -float("inf")).all()
        if n:
            same((out[b:b + 1, :, T - n:], lse[b:b + 1, :, T - n:]),
                 mm.block_sparse_attention_prefill(q[b:b + 1, :, T - n:], k[b:b + 1], v[b:b + 1], layout, lens[b:b + 1], return_lse=True),
                 f"item {b} with T = {n}")
    wild = mm.block_sparse_attention_prefill(q, k, v, layout, lens, new_lens=lens_tensor([-5, 37, 1000], dev, torch.int64), return_lse=True)
    same(wild, (out, lse), "new_lens clamped to [0, T]")


# ---- 5. independence -----------------------------------------------------------------------------------------------------

def test_5_an_item_alone_layouts_block_128_and_chunks(mm, dev):
    B, Hkv, G, T, D, dtype, k_lens = 3, 2, 2, 100, 96, torch.float16, [333, 512, 100]
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 2780)
    lens = lens_tensor(k_lens, dev)
    a, b_ = layout_from_rows(ROWS, dev), layout_from_rows(ROWS_B, dev)
    run = lambda *args, **kw: mm.block_sparse_attention_prefill(*args, return_lse=True, **kw)  # noqa: E731
    shared = run(q, k, v, a, lens)
    for b in range(B):
        same(run(q[b:b + 1], k[b:b + 1], v[b:b + 1], a, lens[b:b + 1]), (shared[0][b:b + 1], shared[1][b:b + 1]), f"item {b} alone")
        same(run(q[b:b + 1], k[b:b + 1], v[b:b + 1], a, lens[b]), (shared[0][b:b + 1], shared[1][b:b + 1]), f"item {b} alone, its length 0-d")
    same(run(q, k, v, stack_layouts([a] * 6, (B, Hkv), dev), lens), shared, "the layout repeated per item")
    per_head = run(q, k, v, stack_layouts([a, b_], (Hkv,), dev), lens)
    check_rule("prefill, a layout per k / v head", per_head[0], q, k, v, visible([ROWS, ROWS_B], B, Hkv, T, k_lens), G, per_head[1])
    same((per_head[0][:, :G], per_head[1][:, :G]), (shared[0][:, :G], shared[1][:, :G]), "k / v head 0 keeps layout a")
    same(per_head, training_forward(mm, q, k, v, [ROWS, ROWS_B], k_lens), "a layout per k / v head against block_attention_forward_ex")
    # block = 128 against the expanded layout
    rows128 = [[0], [1, 0], [0, 2, 1], [2, 3, 0]]
    expanded = [[x for c in rows128[i // 2] for x in (2 * c, 2 * c + 1)] for i in range(8)]  # sub-block order
    same(run(q, k, v, layout_from_rows(rows128, dev), lens, block=128), run(q, k, v, layout_from_rows(expanded, dev), lens, block=64),
         "block = 128 against the expanded layout")
    # T = 100 against the same tokens as two calls of 60 and 40, k_lens stepped
    first = run(q[:, :, :60], k, v, a, lens - 40)
    second = run(q[:, :, 60:], k, v, a, lens)
    same((torch.cat([first[0], second[0]], 2), torch.cat([first[1], second[1]], 2)), shared, "chunks of 60 and 40 against one of 100")
    # the decode call with the same T: under the rule, NOT bit for bit — that call cuts the list into chunks dealt to four
    # waves and merges partials, this one walks the list in order in one accumulator: the order of summation differs
    T2 = 5
    dec = mm.block_sparse_attention_decode(q[:, :, -T2:], k, v, a, lens, return_lse=True)
    check_rule("decode call, the same 5 tokens", dec[0], q[:, :, -T2:], k, v, visible([ROWS], B, Hkv, T2, k_lens), G, dec[1])
    check_rule("prefill call, the same 5 tokens", shared[0][:, :, -T2:], q[:, :, -T2:], k, v, visible([ROWS], B, Hkv, T2, k_lens), G,
               shared[1][:, :, -T2:])


def test_5_groups_and_an_item_loop_beyond_the_grid(mm, dev):
    """G = 1, 5 and 17 (beyond the decode calls' 16); and more work units than the launch has workgroups: B·Hkv·2·G > 65536
    with T = 1, Smax = 64, so that the item loop runs — every item against the call on it alone for a sample."""
    D, dtype = 32, torch.bfloat16
    for G in (1, 5, 17):
        B, Hkv, T, k_lens = 2, 2, 70, [333, 512]
        q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 2790 + G)
        out, lse = mm.block_sparse_attention_prefill(q, k, v, layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev), return_lse=True)
        same((out, lse), training_forward(mm, q, k, v, [ROWS], k_lens), f"G={G}")
    B, Hkv, G, T, smax = 2100, 4, 4, 1, 64
    assert B * Hkv * 2 * G > 65536
    g = torch.Generator(device=dev).manual_seed(2795)
    q = torch.randn((B, Hkv * G, T, D), device=dev, generator=g).to(dtype)
    k, v = (torch.randn((B, Hkv, smax, D), device=dev, generator=g).to(dtype) for _ in range(2))
    lens = torch.randint(1, smax + 1, (B,), device=dev, generator=g, dtype=torch.int32)
    layout = layout_from_rows([[0]], dev)
    out, lse = mm.block_sparse_attention_prefill(q, k, v, layout, lens, return_lse=True)
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    for b in (0, 1, 1023, 1024, 2047, 2048, 2099):
        same(mm.block_sparse_attention_prefill(q[b:b + 1], k[b:b + 1], v[b:b + 1], layout, lens[b:b + 1], return_lse=True),
             (out[b:b + 1], lse[b:b + 1]), f"item {b} of {B} alone")
    sample = slice(2040, 2056)  # (across the first work unit of the loop: slot 16384 is item 2048)
    check_rule("prefill, items in the loop", out[sample], q[sample], k[sample], v[sample],
               visible([[[0]]], 16, Hkv, T, lens[sample].tolist(), smax=smax), G, lse[sample])


# ---- 6. one graph -------------------------------------------------------------------------------------------------------

def test_6_one_graph_of_lens_rope_append_and_prefill(mm, dev):
    """`lens += new; rope_kv_cache_append(…, new_lens); prefill` captured once and replayed three times while the cache grows
    across a block boundary (item 0: 50 → 67 → 84 → 101 crosses 64; item 1 takes 3 of the 17 slots each time): each replay is
    bit for bit the eager calls on a copy of the state."""
    B, Hkv, G, T, D, dtype = 2, 2, 2, 17, 64, torch.float16
    Hq = Hkv * G
    layout = layout_from_rows(ROWS, dev)
    g = torch.Generator(device=dev).manual_seed(2800)
    k, v = (torch.randn((B, Hkv, SMAX, D), device=dev, generator=g).to(dtype) for _ in range(2))
    lens = lens_tensor([50, 120], dev, torch.int64)
    news = lens_tensor([T, 3], dev, torch.int64)
    ang = torch.arange(SMAX, device=dev, dtype=torch.float32)[:, None] * torch.exp(-torch.arange(D // 2, device=dev) * 0.2)[None]
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    fused = torch.randn((B, T, Hq + 2 * Hkv, D), device=dev, generator=g).to(dtype)
    qv, knew, vnew = (fused[:, :, a:b].transpose(1, 2) for a, b in ((0, Hq), (Hq, Hq + Hkv), (Hq + Hkv, Hq + 2 * Hkv)))

    def step(lens, k, v):
        lens += news
        qr = mm.rope_kv_cache_append(qv, knew, vnew, cos, sin, k, v, lens, new_lens=news)
        return mm.block_sparse_attention_prefill(qr, k, v, layout, lens, new_lens=news, return_lse=True)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(lens.clone(), k.clone(), v.clone())  # warm-up on the side stream: the layout's lists are built here
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    state = (lens.clone(), k.clone(), v.clone())  # the capture itself does not run: the state is as before
    with torch.cuda.graph(graph):  # a host synchronisation in here would fail the capture
        out, lse = step(lens, k, v)
    lens.copy_(state[0]), k.copy_(state[1]), v.copy_(state[2])
    previous = None
    for replay in range(3):
        fused.copy_(torch.randn(fused.shape, device=dev, generator=g).to(dtype))
        eager = (lens.clone(), k.clone(), v.clone())
        want = step(*eager)
        out.fill_(NAN)
        lse.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert lens.tolist() == eager[0].tolist() == [50 + 17 * (replay + 1), 120 + 3 * (replay + 1)]
        same((out, lse), want, f"replay {replay}")
        assert_same_bits(k, eager[1], f"replay {replay}: the cache")
        assert (out[1, :, :T - 3] == 0).all() and torch.isfinite(lse[0]).all()
        assert previous is None or not torch.equal(previous, out)
        previous = out.clone()
