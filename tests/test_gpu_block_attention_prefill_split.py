"""The split key walks of matmuls.block_sparse_attention_prefill and its paged / fp8 forms on the MI355X:
`split=s` cuts the list of a tile's layout row by list position into parts of s entries, one workgroup per (tile, query head,
part), and a second launch merges the parts in ascending order.

The contract: a row whose list holds at most s entries has the bits of the unsplit call, also inside a call where other rows
have many parts; a row's bits are a function of its item's operands, its list, pos and s — so paged equals contiguous on the
gathered cache, fp8 without scales the 2-byte call on the widened cache, a strided cache its clone, an item alone the item in
its batch, 100 tokens the chunks of 60 and 40 —; rows of more than one part agree with float64 under the project's rule
e_dev ≤ 8 · e_ref per class (the rows of one (item, query head, tile)) and lse within 1e-5: no new tolerance.  Two shapes: the
decode tests' ROWS at Smax = 512 with k_lens [333, 512], T = 100, and Smax = 2048 (32 blocks), B = Hkv = G = 2, T = 200 at
k_lens [2000, 1030] under a lower-triangle layout with entries above the diagonal inside the parts of one row."""
import ctypes

import pytest
import torch

from gpu_helpers import SENTINEL, assert_outside_untouched, assert_same_bits, padded
from sparse_attention_helpers import FACTOR, rel_err, scaled_err
from test_gpu_block_attention_decode import (ROWS, SMAX, check_rule, layout_from_rows, lens_tensor, operands, poison_unseen, references,
                                             visible)
from test_gpu_block_attention_decode_fp8 import codes, fp8, pools, wide
from test_gpu_block_attention_decode_paged import gathered, paged
from test_gpu_block_attention_prefill import DTYPES, KB, LSE_BOUND, NAN, WIDTHS, clamp, same, visible_new

pytestmark = pytest.mark.gpu

# the longer shape: the lower triangle in ascending order, but row 13 — a row of item 1's tokens — with entries above the
# diagonal (≥ 14) inside its parts.  At split = 5 its parts are [0, 1, 2, 4, 5], [20, 25, 3, 7, 30] (the walk skips its first
# entry, two in a row, and its last), [6, 8, 9, 10, 11], [12, 13, 16, 17, 18] and [19, 21, 22] (a part that computes nothing).
LONG = 2048
LONG_ROWS = [list(range(r + 1)) for r in range(LONG // KB)]
LONG_ROWS[13] = [0, 1, 2, 4, 5, 20, 25, 3, 7, 30, 6, 8, 9, 10, 11, 12, 13, 16, 17, 18, 19, 21, 22]
LONG_LENS, LONG_T = [2000, 1030], 200
assert sorted(j for j in LONG_ROWS[13] if j <= 13) == list(range(14))


def parts_of(rows, r, split):
    return -(-len(rows[r]) // split)


def token_rows(T, k_len, smax):
    """The layout rows that hold a token of an item with all T slots new."""
    n = clamp(k_len, 0, smax)
    lo = max(n - T, 0)
    return list(range(lo // KB, (n - 1) // KB + 1)) if n > lo else []


def tile_classes(B, Hq, T, k_lens, smax):
    """{name: Boolean [B, Hq, T]}: the rows of one (item, query head, position tile) that hold a token."""
    classes = {}
    for b in range(B):
        n = clamp(k_lens[b], 0, smax)
        pos = torch.arange(T) + (n - T)
        for h in range(Hq):
            for r in token_rows(T, k_lens[b], smax):
                m = torch.zeros(B, Hq, T, dtype=torch.bool)
                m[b, h] = (pos >= max(r * KB, 0)) & (pos < (r + 1) * KB) & (pos >= 0)
                classes[f"item {b} head {h} tile {r}"] = m
    return classes


def check_classes(what, out, lse, ref, yard, lse64, classes):
    """The rule per class, each against its OWN e_ref; prints the worst ratio."""
    got, ref, yard = out.cpu().double().numpy(), ref.numpy(), yard.double().numpy()
    lse, lse64 = lse.cpu().double().numpy(), lse64.numpy()
    worst = 0.0
    for name, rows_of in classes.items():
        m = rows_of.numpy()
        e_ref, e_dev = scaled_err(yard[m], ref[m]), scaled_err(got[m], ref[m])
        worst = max(worst, e_dev / e_ref)
        assert e_dev <= FACTOR * e_ref, f"{what}, {name}: e_dev {e_dev:.3e} > {FACTOR:g} · e_ref {e_ref:.3e}"
        e = rel_err(lse[m], lse64[m])
        assert e <= LSE_BOUND, f"{what}, {name}: lse differs from float64 by {e:.3e} relative"
    print(f"block attention prefill split {what}: worst class ratio {worst:.2f}")


def part_index(rows, B, Hkv, T, k_lens, split, smax):
    """int [B, Hkv, T, smax]: the part (by list position) of the entry through which a token sees a key, −1 where it does not;
    and int [B, T]: the parts of the token's list."""
    part = torch.full((B, Hkv, T, smax), -1, dtype=torch.int64)
    count = torch.zeros(B, T, dtype=torch.int64)
    for b in range(B):
        n = clamp(k_lens[b], 0, smax)
        for t in range(T):
            pos = n - T + t
            if pos < 0:
                continue
            r = pos // KB
            count[b, t] = parts_of(rows, r, split)
            for p, J in enumerate(rows[r]):
                if J <= r:
                    part[b, :, t, J * KB:min((J + 1) * KB, pos + 1)] = p // split
    return part, count


def mistaken_results(q, k, v, rows, k_lens, G, split, smax):
    """float64 (out, lse) of three mistaken split kernels, by name: the combine dropping the last part of a list of several;
    the weights all taken as 1 (no rescale to the common maximum); the entry at a cut taken by both parts."""
    B, Hq, T, D = q.shape
    Hkv, scale = Hq // G, 1.0 / D ** 0.5
    part, count = part_index(rows, B, Hkv, T, k_lens, split, smax)
    qd, kd, vd = q.cpu().double(), k.cpu().double().repeat_interleave(G, 1), v.cpu().double().repeat_interleave(G, 1)
    s = scale * (qd @ kd.transpose(-1, -2))
    partq = part.repeat_interleave(G, 1)
    ninf = -float("inf")

    def finish(weights_log):  # scores + log of a key's weight (−inf: unseen) → (out, lse)
        x = s + weights_log
        empty = ~torch.isfinite(x).any(-1)
        lse = torch.logsumexp(x.masked_fill(empty[..., None], 0.0), -1).masked_fill(empty, ninf)
        p = torch.softmax(x.masked_fill(empty[..., None], 0.0), -1).masked_fill(empty[..., None], 0.0)
        return p @ vd, lse

    seen = partq >= 0
    results = {}
    last = (count - 1)[:, None, :, None]
    keep = seen & ~((partq == last) & (last > 0))
    results["the combine drops the last part"] = finish(torch.zeros_like(s).masked_fill(~keep, ninf))
    # no rescale: part i contributes exp(s − mᵢ) with its own maximum, so key j weighs exp(−m_part(j)) times too much / little
    logw = torch.zeros_like(s).masked_fill(~seen, ninf)
    top = torch.full(s.shape[:-1], ninf, dtype=torch.float64)
    for i in range(int(count.max())):
        mine = partq == i
        m_i = s.masked_fill(~mine, ninf).amax(-1)
        logw = torch.where(mine, -m_i[..., None].expand_as(s), logw)
        top = torch.maximum(top, m_i)
    out, lse = finish(logw)  # lse = log Σ lᵢ; the mistaken kernel adds the common maximum
    results["the weights all taken as 1"] = (out, lse + top.masked_fill(~torch.isfinite(top), 0.0))
    twice = torch.zeros(B, Hkv, T, smax, dtype=torch.bool)
    for b in range(B):
        n = clamp(k_lens[b], 0, smax)
        for t in range(T):
            pos = n - T + t
            if pos < 0:
                continue
            r = pos // KB
            for p, J in enumerate(rows[r]):
                if p % split == 0 and p > 0 and J <= r:
                    twice[b, :, t, J * KB:min((J + 1) * KB, pos + 1)] = True
    two = torch.tensor(2.0, dtype=torch.float64).log()
    results["an entry at a cut taken by both parts"] = finish(torch.where(twice.repeat_interleave(G, 1), two, 0.0).masked_fill(~seen, ninf))
    return results


def prove_the_checks_see_three_mistakes(what, q, k, v, rows, k_lens, G, split, smax, ref, yard, lse64, classes):
    """On the test's own inputs, in float64, before the device call: each mistake moves out beyond FACTOR · e_ref of some
    class, or lse beyond its bound there.  Prints the margins (in bounds)."""
    ref, yard, lse64 = ref.numpy(), yard.double().numpy(), lse64.numpy()
    for name, (wrong, wrong_lse) in mistaken_results(q, k, v, rows, k_lens, G, split, smax).items():
        best_out, best_lse = 0.0, 0.0
        for rows_of in classes.values():
            m = rows_of.numpy()
            e_ref = scaled_err(yard[m], ref[m])
            best_out = max(best_out, scaled_err(wrong.numpy()[m], ref[m]) / (FACTOR * e_ref))
            best_lse = max(best_lse, rel_err(wrong_lse.numpy()[m], lse64[m]) / LSE_BOUND)
        print(f"block attention prefill split {what} proof '{name}': out {best_out:.1f} bounds, lse {best_lse:.1f} bounds")
        assert max(best_out, best_lse) > 1.0, f"{what}: the checks would not see '{name}'"


def run(mm, *args, **kw):
    return mm.block_sparse_attention_prefill(*args, return_lse=True, **kw)


def rows_mask(B, Hq, T, k_lens, smax, rows, keep):
    """Boolean [B, Hq, T]: the slots whose token stands in a layout row r with keep(r)."""
    m = torch.zeros(B, Hq, T, dtype=torch.bool)
    for b in range(B):
        pos = torch.arange(T) + (clamp(k_lens[b], 0, smax) - T)
        for r in token_rows(T, k_lens[b], smax):
            if keep(r):
                m[b, :, (pos >= r * KB) & (pos < (r + 1) * KB) & (pos >= 0)] = True
    return m


# ---- 1. the rule per class ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", WIDTHS)
def test_1_the_rule_per_class_on_the_decode_tests_lists(mm, dev, dtype, D):
    """T = 100 at k_lens [333, 512] (tiles 3, 4, 5 of item 0 and 6, 7 of item 1; lists of 3, 5, 5, 4 and 8 entries) at
    split 1, 2 and 3: up to 8, 4 and 3 partials a row."""
    B, Hkv, G, T, k_lens = 2, 2, 2, 100, [333, 512]
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 2900 + D)
    vis = visible([ROWS], B, Hkv, T, k_lens)
    ref, yard, lse64 = references(q, k, v, vis, G)
    classes = tile_classes(B, Hkv * G, T, k_lens, SMAX)
    assert len(classes) == 5 * Hkv * G
    for split in (1, 2, 3):
        what = f"{dtype} D={D} split={split}"
        assert max(parts_of(ROWS, r, split) for r in (3, 4, 5, 6, 7)) == -(-8 // split)
        prove_the_checks_see_three_mistakes(what, q, k, v, ROWS, k_lens, G, split, SMAX, ref, yard, lse64, classes)
        out, lse = run(mm, q, k, v, layout, lens, split=split)
        assert not out.requires_grad and out.is_contiguous() and out.dtype == dtype
        check_rule("prefill split " + what, out, q, k, v, vis, G, lse)
        check_classes(what, out, lse, ref, yard, lse64, classes)


@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 128), (torch.float16, 64)])
def test_1_the_rule_per_class_on_the_longer_shape(mm, dev, dtype, D):
    """Smax = 2048, T = 200 at k_lens [2000, 1030]: rows 28 … 31 and 12 … 16; split 5 and 1 give up to 7 and 32 partials."""
    B, Hkv, G, T, k_lens = 2, 2, 2, LONG_T, LONG_LENS
    assert token_rows(T, 2000, LONG) == [28, 29, 30, 31] and token_rows(T, 1030, LONG) == [12, 13, 14, 15, 16]
    used = token_rows(T, 2000, LONG) + token_rows(T, 1030, LONG)
    assert max(parts_of(LONG_ROWS, r, 5) for r in used) == 7 and max(parts_of(LONG_ROWS, r, 1) for r in used) == 32
    assert parts_of(LONG_ROWS, 13, 5) == 5 and all(j > 13 for j in LONG_ROWS[13][20:]) and LONG_ROWS[13][5] > 13 < LONG_ROWS[13][9]
    layout, lens = layout_from_rows(LONG_ROWS, dev), lens_tensor(k_lens, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 2910 + D, smax=LONG)
    vis = visible([LONG_ROWS], B, Hkv, T, k_lens, smax=LONG)
    ref, yard, lse64 = references(q, k, v, vis, G)
    classes = tile_classes(B, Hkv * G, T, k_lens, LONG)
    for split in (5, 1):
        what = f"long {dtype} D={D} split={split}"
        prove_the_checks_see_three_mistakes(what, q, k, v, LONG_ROWS, k_lens, G, split, LONG, ref, yard, lse64, classes)
        out, lse = run(mm, q, poison_unseen(k, vis), poison_unseen(v, vis), layout, lens, split=split)
        check_rule("prefill split " + what, out, q, k, v, vis, G, lse)
        check_classes(what, out, lse, ref, yard, lse64, classes)


# ---- 2. bits -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_2_a_row_whose_list_fits_in_one_part_has_the_unsplit_bits(mm, dev, dtype):
    """split = 5 on ROWS: the lists of rows 3 … 6 fit, row 7 (8 entries) has two parts — in one call.  split ≥ 8: every list
    fits (the unsplit launch).  The longer shape at split 16: rows 12, 14 and 15 fit beside rows of two and three parts."""
    B, Hkv, G, T, D, k_lens = 2, 2, 2, 100, 128, [333, 512]
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 2920)
    whole = run(mm, q, k, v, layout, lens)
    got = run(mm, q, k, v, layout, lens, split=5)
    fits = rows_mask(B, Hkv * G, T, k_lens, SMAX, ROWS, lambda r: len(ROWS[r]) <= 5)
    assert fits.any() and not fits.all()
    same((got[0][fits], got[1][fits]), (whole[0][fits], whole[1][fits]), f"{dtype} split 5, the rows of one part")
    for split in (8, 9, 100, 2 ** 31 - 1):
        same(run(mm, q, k, v, layout, lens, split=split), whole, f"{dtype} split {split}: every list fits")
    T, k_lens = LONG_T, LONG_LENS
    layout, lens = layout_from_rows(LONG_ROWS, dev), lens_tensor(k_lens, dev)
    q, k, v = operands(dev, B, Hkv, G, T, 64, dtype, 2921, smax=LONG)
    whole, got = run(mm, q, k, v, layout, lens), run(mm, q, k, v, layout, lens, split=16)
    fits = rows_mask(B, Hkv * G, T, k_lens, LONG, LONG_ROWS, lambda r: len(LONG_ROWS[r]) <= 16)
    assert fits[1].any() and not fits[0].any() and not fits[1].all()
    same((got[0][fits], got[1][fits]), (whole[0][fits], whole[1][fits]), f"{dtype} long split 16, the rows of one part")


@pytest.mark.parametrize("page,D,dtype", [(16, 32, torch.bfloat16), (64, 96, torch.float16), (256, 128, torch.bfloat16)])
def test_2_paged_has_the_bits_of_the_contiguous_split_call_on_the_gathered_cache(mm, dev, page, D, dtype):
    B, Hkv, G, T, k_lens = 2, 2, 2, 100, [333, 512]
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 2930 + page)
    kp, vp, table = paged(k, v, page, 2931 + page)
    for split in (1, 3):
        got = mm.block_sparse_attention_prefill_paged(q, kp, vp, table, layout, lens, return_lse=True, split=split)
        same(got, run(mm, q, gathered(kp, table), gathered(vp, table), layout, lens, split=split), f"page {page} D={D} {dtype} split {split}")


@pytest.mark.parametrize("dtype,D,page", [(torch.bfloat16, 32, 16), (torch.float16, 64, 64), (torch.bfloat16, 96, 32), (torch.float16, 128, 256)])
def test_2_fp8_without_scales_has_the_bits_of_the_split_call_on_the_widened_cache(mm, dev, dtype, D, page):
    B, Hkv, G, T, k_lens, split = 2, 2, 2, 100, [333, 512], 2
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q = operands(dev, B, Hkv, G, T, D, dtype, 2940 + D)[0]
    kc, vc = codes(2941 + D, B, Hkv, SMAX, D), codes(2942 + D, B, Hkv, SMAX, D)
    want = run(mm, q, wide(kc, dtype, dev), wide(vc, dtype, dev), layout, lens, split=split)
    same(mm.block_sparse_attention_prefill_fp8(q, fp8(kc, dev), fp8(vc, dev), layout, lens, return_lse=True, split=split), want,
         f"fp8 D={D} {dtype}")
    kp, vp, table = pools(kc, vc, page, 2943 + D)
    same(mm.block_sparse_attention_prefill_paged_fp8(q, fp8(kp, dev), fp8(vp, dev), table.to(dev), layout, lens, return_lse=True, split=split),
         want, f"paged fp8 page {page} D={D} {dtype} against the contiguous 2-byte split call")


def test_2_strided_cache_item_alone_chunks_and_swapped_entries(mm, dev):
    B, Hkv, G, T, D, dtype, k_lens, split = 2, 2, 2, 100, 64, torch.float16, [333, 512], 2
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 2950)
    shared = run(mm, q, k, v, layout, lens, split=split)
    # a strided (BSHD) cache inside NaN against its clone
    def bshd(x):
        buf = torch.full((B, SMAX, Hkv, D + 8), NAN, device=dev, dtype=dtype)
        view = buf[..., :D].transpose(1, 2)
        view.copy_(x)
        return view
    ks, vs = bshd(k), bshd(v)
    assert not ks.is_contiguous()
    same(run(mm, q, ks, vs, layout, lens, split=split), shared, "a strided cache against its clone")
    # an item alone
    for b in range(B):
        same(run(mm, q[b:b + 1], k[b:b + 1], v[b:b + 1], layout, lens[b:b + 1], split=split), (shared[0][b:b + 1], shared[1][b:b + 1]),
             f"item {b} alone")
    # 100 = 60 + 40 at the same split
    first = run(mm, q[:, :, :60], k, v, layout, lens - 40, split=split)
    second = run(mm, q[:, :, 60:], k, v, layout, lens, split=split)
    same((torch.cat([first[0], second[0]], 2), torch.cat([first[1], second[1]], 2)), shared, "chunks of 60 and 40 against one of 100")
    # one above-diagonal entry of a list swapped for another: the same cut, the same bits
    assert 7 in ROWS[4] and 6 not in ROWS[4]
    swapped = [list(r) for r in ROWS]
    swapped[4][swapped[4].index(7)] = 6
    same(run(mm, q, k, v, layout_from_rows(swapped, dev), lens, split=split), shared, "block 7 of row 4's list swapped for block 6")
    T2, lens2 = LONG_T, lens_tensor(LONG_LENS, dev)
    q, k, v = operands(dev, B, Hkv, G, T2, D, dtype, 2951, smax=LONG)
    swapped = [list(r) for r in LONG_ROWS]
    swapped[13][5], swapped[13][9], swapped[13][21] = 14, 31, 27
    same(run(mm, q, k, v, layout_from_rows(swapped, dev), lens2, split=5), run(mm, q, k, v, layout_from_rows(LONG_ROWS, dev), lens2, split=5),
         "the above-diagonal entries of row 13 swapped for others")


# ---- 3. per-head fp8 scales ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 128), (torch.float16, 64)])
def test_3_fp8_with_per_head_scales_under_the_rule(mm, dev, dtype, D):
    B, Hkv, G, T, k_lens, split = 2, 2, 2, 100, [333, 512], 2
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 2960 + D)
    k8, ks = mm.kv_to_fp8(k)
    v8, vs = mm.kv_to_fp8(v)
    real_k, real_v = k8.float() * ks.reshape(1, Hkv, 1, 1), v8.float() * vs.reshape(1, Hkv, 1, 1)
    out, lse = mm.block_sparse_attention_prefill_fp8(q, k8, v8, layout, lens, k_scale=ks, v_scale=vs, return_lse=True, split=split)
    check_rule(f"prefill split fp8 per-head scales D={D} {dtype}", out, q, real_k, real_v, visible([ROWS], B, Hkv, T, k_lens), G, lse)
    kp, vp, table = pools(k8.view(torch.uint8).cpu(), v8.view(torch.uint8).cpu(), 32, 2961)
    same(mm.block_sparse_attention_prefill_paged_fp8(q, fp8(kp, dev), fp8(vp, dev), table.to(dev), layout, lens, k_scale=ks, v_scale=vs,
                                                     return_lse=True, split=split), (out, lse), "paged fp8 with scales against the contiguous")
    # a v_scale takes the scaled statement: the rows of one part have the unsplit fp8 call's bits
    whole = mm.block_sparse_attention_prefill_fp8(q, k8, v8, layout, lens, k_scale=ks, v_scale=vs, return_lse=True)
    fits = rows_mask(B, Hkv * G, T, k_lens, SMAX, ROWS, lambda r: len(ROWS[r]) <= 5)
    got = mm.block_sparse_attention_prefill_fp8(q, k8, v8, layout, lens, k_scale=ks, v_scale=vs, return_lse=True, split=5)
    same((got[0][fits], got[1][fits]), (whole[0][fits], whole[1][fits]), "the scaled store of a row of one part")


# ---- 4. new_lens ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_4_new_lens_and_slots_at_negative_positions(mm, dev, dtype):
    """new_lens = [0, 37, 100], T = 200 over k_len = 130 (70 slots at negative positions): zero rows and −inf wherever no
    token stands, each row written once (NaN in out and lse cannot survive: they are fresh tensors — the C entry test looks
    at pre-filled ones); the rows of existing tokens are the call with T = new_len on the sliced q."""
    B, Hkv, G, T, D, k_lens, new_lens, split = 3, 2, 2, 200, 64, [130, 130, 130], [0, 37, 100], 1
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 2970)
    out, lse = run(mm, q, k, v, layout, lens, new_lens=lens_tensor(new_lens, dev), split=split)
    vis = visible_new([ROWS], B, Hkv, T, k_lens, new_lens)
    check_rule(f"prefill split new_lens {dtype}", out, q, k, v, vis, G, lse)
    for b, n in enumerate(new_lens):
        assert (out[b, :, :T - n] == 0).all() and (lse[b, :, :T - n] == -float("inf")).all()
        if n:
            assert torch.isfinite(lse[b, :, T - n:]).all()
            same((out[b:b + 1, :, T - n:], lse[b:b + 1, :, T - n:]),
                 run(mm, q[b:b + 1, :, T - n:], k[b:b + 1], v[b:b + 1], layout, lens[b:b + 1], split=split), f"item {b} with T = {n}")
    full = run(mm, q, k, v, layout, lens, split=split)  # no new_lens: the first 70 slots stand at negative positions
    assert (full[0][:, :, :70] == 0).all() and (full[1][:, :, :70] == -float("inf")).all() and torch.isfinite(full[1][:, :, 70:]).all()
    same((full[0][2:, :, 100:], full[1][2:, :, 100:]), (out[2:, :, 100:], lse[2:, :, 100:]), "the tokens both calls hold: the same rows")


# ---- 5. through the C entry ---------------------------------------------------------------------------------------------

def _split_entry(capi, dtype):
    vp, i64, i32, f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float
    fn = getattr(capi, "mi_block_attention_prefill_split_" + {torch.bfloat16: "bf16", torch.float16: "f16"}[dtype])
    fn.argtypes = [vp, vp, i64] + 6 * [i32] + 3 * [vp, i64, i64, i64] + [vp, i32, vp, i32, i32, f32] + \
        [vp, i64, i64, vp, i32, vp, ctypes.c_size_t, vp]
    fn.restype = ctypes.c_int
    capi.mi_block_attention_prefill_split_workspace_bytes.argtypes = 6 * [i32]
    capi.mi_block_attention_prefill_split_workspace_bytes.restype = i64
    return fn


@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 96), (torch.float16, 32)])
def test_5_through_the_c_entry_nothing_else_is_written(mm, capi, dev, dtype, D):
    """The workspace full of NaN inside sentinels, out and lse inside sentinels: the python call's bits; every row written;
    nothing outside out, lse and the workspace's own bytes touched; a short workspace launches nothing."""
    B, Hkv, G, T, k_lens, new_lens, split = 2, 2, 3, 100, [70, 512], [100, 37], 3
    items, Hq = B * Hkv, Hkv * G
    layout = layout_from_rows(ROWS, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 2980 + D)
    lens, news = lens_tensor(k_lens, dev), lens_tensor(new_lens, dev)
    want = run(mm, q, k, v, layout, lens, new_lens=news, split=split)
    offsets, columns, nnz, L = mm._block_layout(layout, dev, 1, mm._csr_state(layout))["fwd"]
    fn = _split_entry(capi, dtype)
    need = capi.mi_block_attention_prefill_split_workspace_bytes(items, G, T, D, SMAX, split)
    assert need == items * G * 3 * 3 * 64 * (D + 2) * 4
    pq = padded(q.reshape(items * G, T, D), 0, NAN)
    pk, pv = (padded(x.reshape(items, SMAX, D), i, NAN) for i, x in ((1, k), (2, v)))
    pout = padded(torch.full((items * G, T, D), SENTINEL, device=dev, dtype=dtype), 3, SENTINEL)
    lse_buf = torch.full((B * Hq * T + 16,), SENTINEL, device=dev)
    lse = lse_buf[8:8 + B * Hq * T]
    ws_buf = torch.full((need // 4 + 64,), SENTINEL, device=dev)
    ws = ws_buf[32:32 + need // 4]
    ws.fill_(NAN)
    assert ws.data_ptr() % 16 == 0
    stream = torch.cuda.current_stream().cuda_stream

    def call(ws_ptr=ws.data_ptr(), ws_bytes=need, split=split):
        return fn(offsets.data_ptr(), columns.data_ptr(), nnz, L, items, Hkv, T, SMAX, D, pq.buf.data_ptr(), pq.ld, pq.stride, Hq * pq.stride,
                  pk.buf.data_ptr(), pk.ld, pk.stride, Hkv * pk.stride, pv.buf.data_ptr(), pv.ld, pv.stride, Hkv * pv.stride,
                  lens.data_ptr(), B, news.data_ptr(), B, G, 1.0 / D ** 0.5, pout.buf.data_ptr(), pout.ld, pout.stride,
                  lse.data_ptr(), split, ws_ptr, ws_bytes, stream)

    assert call(ws_bytes=need - 1) == -4 and call(ws_ptr=ws.data_ptr() + 4) == -1 and call(ws_ptr=None) == -1 and call(split=0) == -1
    torch.cuda.synchronize()
    assert_same_bits(pout.buf, torch.full_like(pout.buf, SENTINEL), "a refused call launches nothing")
    assert torch.isnan(ws).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert_outside_untouched(pout, "out")
    assert (pout.x != SENTINEL).all() and (lse != SENTINEL).all(), "every row of out and lse is written"
    assert_same_bits(pout.x.reshape(B, Hq, T, D), want[0], f"{dtype} D={D} through the C entry: out")
    assert_same_bits(lse.reshape(B, Hq, T), want[1], "through the C entry: lse")
    rest = torch.cat([lse_buf[:8], lse_buf[8 + B * Hq * T:], ws_buf[:32], ws_buf[32 + need // 4:]])
    assert_same_bits(rest, torch.full_like(rest, SENTINEL), "around lse and around the workspace")
    assert torch.isnan(ws).any() and not torch.isnan(ws).all()  # (the partials of tiles without a token are never written)


# ---- 6. more work units × parts than the launch has workgroups ------------------------------------------------------------

def test_6_an_item_loop_beyond_the_grid_in_both_launches(mm, dev):
    """B·Hkv·2·G = 67 200 tiles, two parts each: the walk's and the combine's item loops run — every sampled item against
    the call on it alone."""
    D, dtype, B, Hkv, G, T, smax = 32, torch.bfloat16, 2100, 4, 4, 1, 128
    assert B * Hkv * 2 * G > 65536
    g = torch.Generator(device=dev).manual_seed(2990)
    q = torch.randn((B, Hkv * G, T, D), device=dev, generator=g).to(dtype)
    k, v = (torch.randn((B, Hkv, smax, D), device=dev, generator=g).to(dtype) for _ in range(2))
    lens = torch.randint(1, smax + 1, (B,), device=dev, generator=g, dtype=torch.int32)
    rows = [[0], [1, 0]]
    layout = layout_from_rows(rows, dev)
    out, lse = run(mm, q, k, v, layout, lens, split=1)
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    for b in (0, 1, 1023, 1024, 2047, 2048, 2099):
        same(run(mm, q[b:b + 1], k[b:b + 1], v[b:b + 1], layout, lens[b:b + 1], split=1), (out[b:b + 1], lse[b:b + 1]), f"item {b} of {B} alone")
    sample = slice(2040, 2056)
    check_rule("prefill split, items in the loop", out[sample], q[sample], k[sample], v[sample],
               visible([rows], 16, Hkv, T, lens[sample].tolist(), smax=smax), G, lse[sample])


# ---- 7. one graph -------------------------------------------------------------------------------------------------------

def test_7_one_graph_of_lens_rope_append_and_split_prefill(mm, dev):
    """`lens += new; rope_kv_cache_append(…, new_lens); prefill(split=2)` captured once and replayed three times while item 0
    grows 100 → 117 → 134 → 151 across the block boundary at 128: the list of row 1 has two entries — one part —, that of
    row 2 four: the tile's list gains its second part on the way.  Each replay is bit for bit the eager calls on a copy."""
    B, Hkv, G, T, D, dtype = 2, 2, 2, 17, 64, torch.float16
    Hq = Hkv * G
    assert len(ROWS[1]) == 2 and len(ROWS[2]) == 4
    layout = layout_from_rows(ROWS, dev)
    g = torch.Generator(device=dev).manual_seed(2995)
    k, v = (torch.randn((B, Hkv, SMAX, D), device=dev, generator=g).to(dtype) for _ in range(2))
    lens = lens_tensor([100, 120], dev, torch.int64)
    news = lens_tensor([T, 3], dev, torch.int64)
    ang = torch.arange(SMAX, device=dev, dtype=torch.float32)[:, None] * torch.exp(-torch.arange(D // 2, device=dev) * 0.2)[None]
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    fused = torch.randn((B, T, Hq + 2 * Hkv, D), device=dev, generator=g).to(dtype)
    qv, knew, vnew = (fused[:, :, a:b].transpose(1, 2) for a, b in ((0, Hq), (Hq, Hq + Hkv), (Hq + Hkv, Hq + 2 * Hkv)))

    def step(lens, k, v):
        lens += news
        qr = mm.rope_kv_cache_append(qv, knew, vnew, cos, sin, k, v, lens, new_lens=news)
        return mm.block_sparse_attention_prefill(qr, k, v, layout, lens, new_lens=news, return_lse=True, split=2)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(lens.clone(), k.clone(), v.clone())  # warm-up on the side stream: the layout's lists are built here
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    state = (lens.clone(), k.clone(), v.clone())
    with torch.cuda.graph(graph):  # a host synchronisation or a memset in here would fail the capture
        out, lse = step(lens, k, v)
    lens.copy_(state[0]), k.copy_(state[1]), v.copy_(state[2])
    for replay in range(3):
        fused.copy_(torch.randn(fused.shape, device=dev, generator=g).to(dtype))
        eager = (lens.clone(), k.clone(), v.clone())
        want = step(*eager)
        out.fill_(NAN)
        lse.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert lens.tolist() == eager[0].tolist() == [100 + 17 * (replay + 1), 120 + 3 * (replay + 1)]
        same((out, lse), want, f"replay {replay}")
        assert_same_bits(k, eager[1], f"replay {replay}: the cache")
        assert (out[1, :, :T - 3] == 0).all() and torch.isfinite(lse[0]).all()
