"""The parts of matmuls.block_sparse_attention_prefill(split=s) and the forms that meet `split` on the MI355X:
what tests/test_gpu_block_attention_prefill_split.py leaves to a max-norm per class is pinned here element by element.

1. The merge against the parts' own calls.  The unsplit call on the layout PART_i — row r lists entries [i·s, (i + 1)·s) of the
   row's list — returns round_T(oᵢ / lᵢ) and mᵢ + log lᵢ of part i, so in float64 lse* = logsumexp lseᵢ, wᵢ = exp(lseᵢ − lse*),
   want = Σ wᵢ·outᵢ and A = Σ wᵢ·|outᵢ| are the merged row up to the roundings that are known: one to T in every outᵢ and one
   in out — |out − want| ≤ u_T · (|want| + A) to first order —, and an lse that is off by LSE_BOUND relative, which moves a
   weight by at most the factor exp(LSE_BOUND · |lse|) − 1 ≤ 2 · LSE_BOUND · max(1, |lse|):
       |out − want| ≤ u_T · (|want| + A) + 2 · LSE_BOUND · max(1, max |lseᵢ|) · A     and     |lse − lse*| ≤ LSE_BOUND · |lse*|.
   The terms are derived, none is fitted: u_T is test_gpu_gemm_lowp's U, LSE_BOUND the prefill tests' 1e-5.  Before the
   device call the CPU proves in float64, on the test's inputs, that the bound holds for the right merge and sees four
   mistaken ones; a weight ROUNDED TO T stands at 0.9 … 1.1 of the bound and is not claimed as detectable.
2. Exact identities: a row of which only one part computes has the unsplit call's bits wherever that part stands; rows whose
   tokens see nothing, or whose list is empty, are zero rows with lse −inf in every call.
3. The forms crossed with split: a layout per k / v head and per item (the part count of a layout row differs between the
   heads), block = 128, G ∈ {1, 5, 17}, a 0-d k_lens, a scale of its own, k_lens outside [0, Smax], T = 1 and T = 512, the
   one-entry k_lens / new_lens of the C entries, poisoned pools and hidden table entries.

Smax = 512 (8 blocks), B = Hkv = G = 2, T = 100 at k_lens [333, 512] unless a test says otherwise.  The ratios are printed
(MI_SOFTMAX_LOG collects them: profiles/r31_block_attention_prefill_parts.log)."""
import numpy as np
import pytest
import torch

from gpu_helpers import SENTINEL, assert_outside_untouched, assert_same_bits, padded
from sparse_attention_helpers import FACTOR, dense_step, record, rel_err, scaled_err
from test_gpu_block_attention_decode import (ROWS, ROWS_B, SMAX, check_rule, layout_from_rows, lens_tensor, operands, poison_unseen,
                                             references, stack_layouts, visible)
from test_gpu_block_attention_decode_fp8 import NANB, codes, fp8, poisoned, pools, wide
from test_gpu_block_attention_decode_paged import paged
from test_gpu_block_attention_prefill import DTYPES, KB, LSE_BOUND, NAN, WIDTHS, _prefill_entry, same, training_forward
from test_gpu_block_attention_prefill_split import (_split_entry, check_classes, part_index, parts_of, rows_mask, run, tile_classes,
                                                    token_rows)
from test_gpu_gemm_lowp import U

pytestmark = pytest.mark.gpu

NINF = -float("inf")
# rows 3 … 7 hold the tokens of T = 100 at k_lens [333, 512]; the entries above a row's diagonal are skipped inside their part
EDGE_ROWS = ROWS[:3] + [[7, 6, 5, 4, 3, 0, 1, 2], [5, 6, 4, 0, 7], [0, 5, 6, 7], [7], []]
ROWS128 = [[0], [1, 0], [0, 2, 1], [2, 3, 0]]  # the block = 128 lists of the decode and prefill tests
EXPANDED = [[x for c in ROWS128[i // 2] for x in (2 * c, 2 * c + 1)] for i in range(8)]  # sub-block order


def swapped_rows(rows, *pairs):
    rows = [list(r) for r in rows]
    for a, b in pairs:
        rows[a], rows[b] = rows[b], rows[a]
    return rows


# four distinct assignments of the two files' lists to the layout rows: equal entry counts, different part counts per row
PERMUTED = [swapped_rows(ROWS, (3, 7)), swapped_rows(ROWS_B, (4, 6), (3, 5)), swapped_rows(ROWS, (5, 6), (3, 4)),
            swapped_rows(ROWS_B, (3, 4), (4, 5), (5, 6), (6, 7))]


def part_rows(rows, i, split):
    """PART_i: row r lists entries [i·split, (i + 1)·split) of rows[r] in their order; a row with fewer parts an empty list."""
    return [row[i * split:(i + 1) * split] for row in rows]


def seen_rows(vis, G):
    return vis.any(-1).repeat_interleave(G, 1)


def references_scaled(q, k, v, vis, G, scale):
    """test_gpu_block_attention_decode.references with a scale of the caller's."""
    mask = vis.repeat_interleave(G, 1)
    kr, vr = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
    w = torch.zeros_like(q)
    ref = dense_step(q, kr, vr, w, mask, scale, torch.float64)[0]
    yard = dense_step(q, kr, vr, w, mask, scale, torch.float32, narrow=q.dtype)[0]
    s = (scale * (q.cpu().double() @ kr.cpu().double().transpose(-1, -2))).masked_fill(~mask, NINF)
    empty = ~mask.any(-1)
    lse = torch.logsumexp(s.masked_fill(empty[..., None], 0.0), -1).masked_fill(empty, NINF)
    return ref, yard, lse


# ---- the merge of the parts' own calls, and the float64 parts of the proofs --------------------------------------------------

def merged(outs, lses, dtype):
    """float64 (want, bound, lse*) of the parts' (outᵢ, lseᵢ) [n][B, Hq, T(, D)]: the module docstring's statements."""
    O = torch.stack([o.cpu().double() for o in outs])
    Ls = torch.stack([x.cpu().double() for x in lses])
    top = Ls.amax(0)
    safe = top.masked_fill(~torch.isfinite(top), 0.0)
    log_sum = torch.exp(Ls - safe).sum(0).clamp(min=1e-300).log()  # (the clamp acts where every lseᵢ is −inf)
    star = (safe + log_sum).masked_fill(~torch.isfinite(top), NINF)
    w = torch.exp(Ls - safe - log_sum)  # (0 where lseᵢ = −inf)
    want, A = (w[..., None] * O).sum(0), (w[..., None] * O.abs()).sum(0)
    big = Ls.abs().masked_fill(~torch.isfinite(Ls), 0.0).amax(0).clamp(min=1.0)
    return want, U[dtype] * (want.abs() + A) + 2 * LSE_BOUND * big[..., None] * A, star


def element_ratios(out, lse, want, bound, star, rows_of):
    """(worst |out − want| / bound, the bound and the error there, worst |lse − lse*| / (LSE_BOUND · |lse*|)) over the rows
    of the Boolean [B, Hq, T] rows_of; an element with a zero bound counts as inf unless it is exact."""
    err = (out.cpu().double() - want).abs()[rows_of]
    bnd = bound[rows_of]
    ratio = torch.where(bnd > 0, err / bnd.clamp(min=1e-300), torch.where(err == 0, 0.0, float("inf")))
    at = int(ratio.argmax())
    e = rel_err(lse.cpu().double()[rows_of].numpy(), star[rows_of].numpy())
    return float(ratio.flatten()[at]), float(bnd.flatten()[at]), float(err.flatten()[at]), e / LSE_BOUND


def parts64(q, k, v, rows, k_lens, G, split):
    """float64 (o [n, B, Hq, T, D], m, l [n, B, Hq, T], count [B, T]) of the parts: the running maximum, the row sum and the
    unnormalised accumulator over the keys a token sees through the entries of part i of its list."""
    B, Hq, T, D = q.shape
    part, count = part_index(rows, B, Hq // G, T, k_lens, split, SMAX)
    qd, kd, vd = q.cpu().double(), k.cpu().double().repeat_interleave(G, 1), v.cpu().double().repeat_interleave(G, 1)
    s = (qd @ kd.transpose(-1, -2)) / D ** 0.5
    partq = part.repeat_interleave(G, 1)
    o, m, l = [], [], []
    for i in range(int(count.max())):
        x = s.masked_fill(partq != i, NINF)
        mi = x.amax(-1)
        e = torch.exp(x - mi.masked_fill(~torch.isfinite(mi), 0.0)[..., None])
        o.append(e @ vd), m.append(mi), l.append(e.sum(-1))
    return torch.stack(o), torch.stack(m), torch.stack(l), count


def combine64(o, m, l, count, mistake=None):
    """float64 (out, lse) of the combine — M = max mᵢ, wᵢ = exp(mᵢ − M), L = Σ lᵢ·wᵢ, O = Σ oᵢ·wᵢ — or of a mistaken one."""
    n, D = o.shape[0], o.shape[-1]
    M = m.amax(0)
    w = torch.exp(m - M.masked_fill(~torch.isfinite(M), 0.0))
    index = torch.arange(n)[:, None, None, None]
    last = (index == (count - 1).clamp(min=0)[None, :, None, :]).expand_as(w)  # [n, B, Hq, T]: the last part of the token's list
    wo, wl = w.clone(), w.clone()
    if mistake == "the first part's weight taken as 1":
        wo[0], wl[0] = 1.0, 1.0
    elif mistake == "the last part's l added unweighted":
        wl = torch.where(last, 1.0, wl)
    elif mistake == "the last part's weight wrong by 1 + 2^-6 in the O sum only":
        wo = torch.where(last, wo * (1 + 2.0 ** -6), wo)
    L, O = (l * wl).sum(0), (o * wo[..., None]).sum(0)
    if mistake == "one half of the columns weighted with the previous part's weight":
        O[..., D // 2:] = (o * torch.cat([w[:1], w[:-1]])[..., None]).sum(0)[..., D // 2:]
    empty = L == 0
    out = (O / L.masked_fill(empty, 1.0)[..., None]).masked_fill(empty[..., None], 0.0)
    return out, (M + L.masked_fill(empty, 1.0).log()).masked_fill(empty, NINF)


MISTAKES = ("the first part's weight taken as 1", "the last part's l added unweighted",
            "one half of the columns weighted with the previous part's weight",
            "the last part's weight wrong by 1 + 2^-6 in the O sum only")


def prove_the_element_bound_sees_four_mistakes(what, q, k, v, k_lens, G, split, ref, yard, lse64, classes):
    """On the test's own inputs, in float64, before the device call: the parts' own statements rounded as the device rounds
    them (outᵢ to T, lseᵢ to float32), the right combine rounded to T inside the bound, each mistaken combine — rounded to T
    as well — outside it in out or in lse on some row of several parts.  Prints the margins (in bounds); for the fourth
    mistake also the class rule's, which it does not reach in bfloat16: what check_classes alone would have missed."""
    dtype = q.dtype
    o, m, l, count = parts64(q, k, v, ROWS, k_lens, G, split)
    multi = (count > 1)[:, None, :].expand(m.shape[1:]).clone()
    lsafe = l.masked_fill(l == 0, 1.0)
    outs = (o / lsafe[..., None]).to(dtype)
    lses = (m + lsafe.log()).masked_fill(l == 0, NINF).float()
    want, bound, star = merged(list(outs), list(lses), dtype)
    right = combine64(o, m, l, count)
    r_out, _, _, r_lse = element_ratios(right[0].to(dtype), right[1].float(), want, bound, star, multi)
    print(f"block attention prefill parts {what} proof: the right combine at {r_out:.2f} of the bound, lse {r_lse:.2f}")
    assert r_out <= 1.0 and r_lse <= 1.0, f"{what}: the bound does not hold for the right combine in float64"
    margins = {}
    for name in MISTAKES:
        wrong, wrong_lse = combine64(o, m, l, count, name)
        e_out, _, _, e_lse = element_ratios(wrong.to(dtype), wrong_lse.float(), want, bound, star, multi)
        line = f"block attention prefill parts {what} proof '{name}': out {e_out:.1f} bounds, lse {e_lse:.1f} bounds"
        if name == MISTAKES[3]:
            old = 0.0
            for rows_of in classes.values():
                c = rows_of.numpy() & multi.numpy()  # (the rows of one part keep their bit test)
                if not c.any():
                    continue
                old = max(old, scaled_err(wrong.to(dtype).double().numpy()[c], ref.numpy()[c]) /
                          (FACTOR * scaled_err(yard.double().numpy()[c], ref.numpy()[c])),
                          rel_err(wrong_lse.numpy()[c], lse64.numpy()[c]) / LSE_BOUND)
            line += f"; the class rule alone {old:.2f} bounds"
        print(line)
        margins[name] = max(e_out, e_lse)
        assert margins[name] > 1.0, f"{what}: the element bound would not see '{name}'"
    return margins


# ---- 1. parts against their own calls --------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 128])
def test_1_the_merge_against_the_parts_own_calls(mm, dev, dtype, D):
    """ROWS at split 1, 2 and 3 (up to 8, 4 and 3 parts a row): every row of several parts inside the element bound against
    the merge of the unsplit calls on PART_0 … PART_n−1, lse within LSE_BOUND of their logsumexp; rows of one part keep the
    unsplit call's bits; outᵢ, lseᵢ of a row without part i — an empty list under a tile that holds tokens — are zero and −inf.
    The CPU emulation of the walk and the combine in float32 stayed at ≤ 0.89 of the bound on inputs of this shape."""
    B, Hkv, G, T, k_lens = 2, 2, 2, 100, [333, 512]
    Hq = Hkv * G
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 3100 + D)
    ref, yard, lse64 = references(q, k, v, visible([ROWS], B, Hkv, T, k_lens), G)
    classes = tile_classes(B, Hq, T, k_lens, SMAX)
    whole = run(mm, q, k, v, layout, lens)
    for split in (1, 2, 3):
        what = f"{dtype} D={D} split={split}"
        n = max(parts_of(ROWS, r, split) for r in (3, 4, 5, 6, 7))
        assert n == -(-8 // split)
        prove_the_element_bound_sees_four_mistakes(what, q, k, v, k_lens, G, split, ref, yard, lse64, classes)
        outs, lses = [], []
        for i in range(n):
            out_i, lse_i = run(mm, q, k, v, layout_from_rows(part_rows(ROWS, i, split), dev), lens)
            without = rows_mask(B, Hq, T, k_lens, SMAX, ROWS, lambda r: parts_of(ROWS, r, split) <= i)
            assert (out_i.cpu()[without] == 0).all() and (lse_i.cpu()[without] == NINF).all(), f"{what}: rows without part {i}"
            assert bool(without.any()) == (i >= min(parts_of(ROWS, r, split) for r in (3, 4, 5, 6, 7)))
            outs.append(out_i), lses.append(lse_i)
        want, bound, star = merged(outs, lses, dtype)
        out, lse = run(mm, q, k, v, layout, lens, split=split)
        one = rows_mask(B, Hq, T, k_lens, SMAX, ROWS, lambda r: parts_of(ROWS, r, split) == 1)
        multi = rows_mask(B, Hq, T, k_lens, SMAX, ROWS, lambda r: parts_of(ROWS, r, split) > 1)
        assert multi.any() and (one.any() or split < 3) and int(one.sum() + multi.sum()) == 2 * Hq * T
        same((out[one], lse[one]), (whole[0][one], whole[1][one]), f"{what}: the rows of one part")
        assert torch.isfinite(lse.cpu()[multi]).all()
        r_out, bnd, err, r_lse = element_ratios(out, lse, want, bound, star, multi)
        record(f"block attention prefill parts {what} out against the merge of the parts' own calls (bound, error)", bnd, err)
        print(f"block attention prefill parts {what}: lse at {r_lse:.2f} of its bound")
        assert r_out <= 1.0, f"{what}: an element of out at {r_out:.2f} of the element bound (error {err:.3e}, bound {bnd:.3e})"
        assert r_lse <= 1.0, f"{what}: lse differs from the logsumexp of the parts' lse by {r_lse:.2f} bounds"


# ---- 2. exact identities ---------------------------------------------------------------------------------------------------

def computing_parts(rows, r, split):
    """The parts of rows[r] that hold an entry at or below the diagonal."""
    return [i for i in range(parts_of(rows, r, split)) if any(j <= r for j in rows[r][i * split:(i + 1) * split])]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", WIDTHS)
def test_2_a_row_of_which_one_part_computes_has_the_unsplit_bits(mm, dev, dtype, D):
    """EDGE_ROWS: at split 4 part 0 of row 3 computes nothing and part 1 everything; at split 2 only the middle part of row 4
    and only the first of row 5 compute; the tokens of row 6 see nothing ([7]) and row 7 is an empty list.  One finite m
    makes the merge exact (0 · 0, then + o · 1): the unsplit call's bits, wherever the part stands.  (Row 3 at split 2 has
    two computing parts — [3, 0] and [1, 2] — and stays under the rule.)"""
    B, Hkv, G, T, k_lens = 2, 2, 2, 100, [333, 512]
    Hq = Hkv * G
    exact = {(r, s) for r in (3, 4, 5) for s in (2, 4) if len(computing_parts(EDGE_ROWS, r, s)) == 1}
    assert exact == {(3, 4), (4, 2), (4, 4), (5, 2), (5, 4)}
    assert computing_parts(EDGE_ROWS, 3, 4) == [1] and computing_parts(EDGE_ROWS, 4, 2) == [1] and parts_of(EDGE_ROWS, 4, 2) == 3
    assert computing_parts(EDGE_ROWS, 5, 2) == [0] and parts_of(EDGE_ROWS, 5, 2) == 2 and computing_parts(EDGE_ROWS, 6, 1) == []
    layout, lens = layout_from_rows(EDGE_ROWS, dev), lens_tensor(k_lens, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 3200 + D)
    vis = visible([EDGE_ROWS], B, Hkv, T, k_lens)
    assert not vis[1].any() and vis[0].any(-1).all()
    ref, yard, lse64 = references(q, k, v, vis, G)
    classes = {name: c for name, c in tile_classes(B, Hq, T, k_lens, SMAX).items() if name.startswith("item 0")}
    whole = run(mm, q, poison_unseen(k, vis), poison_unseen(v, vis), layout, lens)
    same(whole, training_forward(mm, q, k, v, [EDGE_ROWS], k_lens), f"{dtype} D={D}: the unsplit call against block_attention_forward_ex")
    check_rule(f"prefill parts edge rows {dtype} D={D}", whole[0], q, k, v, vis, G, whole[1])
    for split in (1, 2, 4):
        got = run(mm, q, poison_unseen(k, vis), poison_unseen(v, vis), layout, lens, split=split)
        for res in (whole, got):  # rows 6 and 7: item 1
            assert (res[0][1] == 0).all() and (res[1][1] == NINF).all() and not torch.isfinite(res[1][1]).any()
            assert torch.isfinite(res[0].float()).all() and torch.isfinite(res[1][0]).all()
        rows_of = rows_mask(B, Hq, T, k_lens, SMAX, EDGE_ROWS, lambda r: (r, split) in exact)
        if split > 1:
            assert rows_of[0].any() and not rows_of[1].any()
            same((got[0][rows_of], got[1][rows_of]), (whole[0][rows_of], whole[1][rows_of]), f"{dtype} D={D} split {split}: one computing part")
        check_classes(f"edge rows {dtype} D={D} split={split}", got[0], got[1], ref, yard, lse64, classes)


@pytest.mark.parametrize("fp8_cache,page,dtype,D", [(False, 16, torch.bfloat16, 64), (True, 32, torch.float16, 128)])
def test_2_hidden_pages_leave_one_computing_part(mm, dev, fp8_cache, page, dtype, D):
    """Row 7 of ROWS at split 3 — parts [3, 7, 0], [5, 1, 6], [2, 4] — with −1 / P + 5 at every page of blocks 3, 7, 0, 2 and 4
    of item 1 and NaN in the pool pages they named: the first and the last part see hidden keys only, the rows of tile 7 have
    the bits of the unsplit paged call with the same table, and the call is under the rule on the mask without those keys."""
    B, Hkv, G, T, k_lens, split = 2, 2, 2, 100, [333, 512], 3
    assert [ROWS[7][i:i + 3] for i in (0, 3, 6)] == [[3, 7, 0], [5, 1, 6], [2, 4]]
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 3250 + page)
    if fp8_cache:
        kc, vc = codes(3251, B, Hkv, SMAX, D), codes(3252, B, Hkv, SMAX, D)
        k, v = wide(kc, dtype, dev), wide(vc, dtype, dev)
        kp, vp, table = pools(kc, vc, page, 3253)
    else:
        kp, vp, table = paged(k, v, page, 3253)
    P = kp.shape[0]
    vis = visible([ROWS], B, Hkv, T, k_lens)
    for J in (3, 7, 0, 2, 4):
        for w in range(J * KB // page, (J + 1) * KB // page):
            kp[table[1, w].long()] = NANB if fp8_cache else NAN
            vp[table[1, w].long()] = NANB if fp8_cache else NAN
            table[1, w] = -1 if w % 2 == 0 else P + 5
        vis[1, :, :, J * KB:(J + 1) * KB] = False
    if fp8_cache:
        call = lambda **kw: mm.block_sparse_attention_prefill_paged_fp8(q, fp8(kp, dev), fp8(vp, dev), table.to(dev), layout, lens,  # noqa: E731
                                                                        return_lse=True, **kw)
    else:
        call = lambda **kw: mm.block_sparse_attention_prefill_paged(q, kp, vp, table, layout, lens, return_lse=True, **kw)  # noqa: E731
    whole, got = call(), call(split=split)
    tile7 = rows_mask(B, Hkv * G, T, k_lens, SMAX, ROWS, lambda r: r == 7)
    assert int(tile7.sum()) == Hkv * G * 64 and not tile7[0].any()
    same((got[0][tile7], got[1][tile7]), (whole[0][tile7], whole[1][tile7]), f"page {page} fp8 {fp8_cache}: tile 7 against the unsplit paged call")
    assert torch.isfinite(got[1][1]).all()
    for name, res in (("unsplit", whole), ("split 3", got)):
        check_rule(f"prefill parts hidden pages, page {page}, fp8 {fp8_cache}, {name}", res[0], q, k, v, vis, G, res[1])


# ---- 3. forms crossed with split -------------------------------------------------------------------------------------------

def through_the_c_entry(mm, capi, dev, layout, q, k, v, lens, news, G, split=None, scale=None):
    """(out, lse) of mi_block_attention_prefill[_split]_T on contiguous operands: lens / news int32 device tensors of any
    entry count (news None: no new_lens), out and lse inside sentinels, the workspace full of NaN inside sentinels; asserts
    status 0, every row written and nothing else touched."""
    B, Hq, T, D = q.shape
    Hkv, items, dtype = k.shape[1], B * k.shape[1], q.dtype
    offsets, columns, nnz, L = mm._block_layout(layout, dev, 1, mm._csr_state(layout))["fwd"]
    qc, kc, vc = q.contiguous(), k.contiguous(), v.contiguous()
    pout = padded(torch.full((B * Hq, T, D), SENTINEL, device=dev, dtype=dtype), 3, SENTINEL)
    lse_buf = torch.full((B * Hq * T + 16,), SENTINEL, device=dev)
    lse = lse_buf[8:8 + B * Hq * T]
    args = [offsets.data_ptr(), columns.data_ptr(), nnz, L, items, Hkv, T, SMAX, D, qc.data_ptr(), D, T * D, Hq * T * D,
            kc.data_ptr(), D, SMAX * D, Hkv * SMAX * D, vc.data_ptr(), D, SMAX * D, Hkv * SMAX * D, lens.data_ptr(), lens.numel(),
            None if news is None else news.data_ptr(), 0 if news is None else news.numel(), G,
            float(scale or 1.0 / D ** 0.5), pout.buf.data_ptr(), pout.ld, pout.stride, lse.data_ptr()]
    stream = torch.cuda.current_stream().cuda_stream
    rest = [lse_buf[:8], lse_buf[8 + B * Hq * T:]]
    if split is None:
        status = _prefill_entry(capi, dtype)(*args, stream)
    else:
        fn = _split_entry(capi, dtype)
        need = capi.mi_block_attention_prefill_split_workspace_bytes(items, G, T, D, SMAX, split)
        assert need > 0 and need % 4 == 0
        ws_buf = torch.full((need // 4 + 64,), SENTINEL, device=dev)
        ws = ws_buf[32:32 + need // 4]
        ws.fill_(NAN)
        assert ws.data_ptr() % 16 == 0
        status = fn(*args, split, ws.data_ptr(), need, stream)
        rest += [ws_buf[:32], ws_buf[32 + need // 4:]]
    torch.cuda.synchronize()
    assert status == 0, status
    assert_outside_untouched(pout, "out")
    assert (pout.x != SENTINEL).all() and (lse != SENTINEL).all(), "every row of out and lse is written"
    rest = torch.cat(rest)
    assert_same_bits(rest, torch.full_like(rest, SENTINEL), "around lse and around the workspace")
    return pout.x.reshape(B, Hq, T, D).contiguous(), lse.reshape(B, Hq, T).clone()


@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 64), (torch.float16, 128)])
def test_3_a_layout_per_head_and_per_item_under_split(mm, capi, dev, dtype, D):
    """A layout per k / v head ([ROWS, ROWS_B]) and per (item, head) (four assignments of their lists to the rows: a layout
    row has a different number of parts from head to head) at split 2: every (item, head) is bit for bit the call on it alone
    with its own 2-d layout — the walk and the combine agree on c % layouts and on the part count —, through matmuls and
    through the C entry with the workspace full of NaN (a combine that merged a part nobody wrote would not be finite)."""
    B, Hkv, G, T, k_lens, split = 2, 2, 2, 100, [333, 512], 2
    Hq = Hkv * G
    lens = lens_tensor(k_lens, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 3300 + D)
    assert len({sum(len(r) for r in rows) for rows in [ROWS, ROWS_B] + PERMUTED}) == 1, "stack_layouts needs equal entry counts"
    assert len({repr(rows) for rows in PERMUTED}) == 4
    differ = [(b, r) for b in range(B) for r in token_rows(T, k_lens[b], SMAX)
              if parts_of(PERMUTED[b * Hkv], r, split) != parts_of(PERMUTED[b * Hkv + 1], r, split)]
    assert differ, "no layout row differs in its number of parts between two heads"
    # against layout 0's count an (item, head) has fewer parts in one row and more in another: a combine that took the list of
    # another layout would merge a part nobody wrote here and leave one out there
    counts = [(parts_of(PERMUTED[0], r, split), parts_of(PERMUTED[b * Hkv + h], r, split))
              for b in range(B) for h in range(Hkv) for r in token_rows(T, k_lens[b], SMAX)]
    assert any(zero > own for zero, own in counts) and any(zero < own for zero, own in counts)
    classes = tile_classes(B, Hq, T, k_lens, SMAX)
    for name, per_item, lead in (("per k / v head", [ROWS, ROWS_B], (Hkv,)), ("per item and head", PERMUTED, (B, Hkv))):
        what = f"{name} {dtype} D={D} split={split}"
        layouts = [layout_from_rows(rows, dev) for rows in per_item]
        stacked = stack_layouts(layouts, lead, dev)
        vis = visible(per_item, B, Hkv, T, k_lens)
        ref, yard, lse64 = references(q, k, v, vis, G)
        got = run(mm, q, k, v, stacked, lens, split=split)
        entry = through_the_c_entry(mm, capi, dev, stacked, q, k, v, lens, None, G, split=split)
        assert torch.isfinite(entry[0].float()).all(), f"{what}: out is not finite over a workspace of NaN: a part nobody wrote was merged"
        assert torch.isfinite(entry[1][seen_rows(vis, G)]).all(), f"{what}: lse is not finite over a workspace of NaN"
        same(entry, got, f"{what}: through the C entry over a workspace of NaN")
        for b in range(B):
            for h in range(Hkv):
                hs = slice(h * G, (h + 1) * G)
                alone = run(mm, q[b:b + 1, hs], k[b:b + 1, h:h + 1], v[b:b + 1, h:h + 1], layouts[(b * Hkv + h) % len(layouts)],
                            lens[b:b + 1], split=split)
                same((got[0][b:b + 1, hs], got[1][b:b + 1, hs]), alone, f"{what}: item {b} head {h} alone with its own layout")
        check_rule(f"prefill parts, a layout {what}", got[0], q, k, v, vis, G, got[1])
        check_classes(what, got[0], got[1], ref, yard, lse64, classes)
        unsplit = run(mm, q, k, v, stacked, lens)
        same(unsplit, training_forward(mm, q, k, v, per_item, k_lens), f"{what}: the unsplit call against block_attention_forward_ex")


@pytest.mark.parametrize("dtype", DTYPES)
def test_3_block_128_is_the_expanded_layout_at_the_same_split(mm, dev, dtype):
    """The cut is made on the expanded 64-list: block = 128 at split 1 and 3 against the layout expanded here, bit for bit."""
    B, Hkv, G, T, D, k_lens = 2, 2, 2, 100, 96, [333, 512]
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 3310)
    lens = lens_tensor(k_lens, dev)
    coarse, fine = layout_from_rows(ROWS128, dev), layout_from_rows(EXPANDED, dev)
    assert max(len(r) for r in EXPANDED) == 6
    for split in (1, 3):
        got = run(mm, q, k, v, coarse, lens, block=128, split=split)
        same(got, run(mm, q, k, v, fine, lens, block=64, split=split), f"{dtype} block = 128 against the expanded layout, split {split}")
        check_rule(f"prefill parts block = 128 {dtype} split={split}", got[0], q, k, v, visible([ROWS128], B, Hkv, T, k_lens, block=128), G, got[1])


@pytest.mark.parametrize("G", [1, 5, 17])
def test_3_groups_under_split(mm, dev, G):
    """B · Hkv · tiles = 12 slots, no multiple of 8 (the last eight of u = 8G·a + 8g + s are padded), times two parts: T = 100
    at k_lens [100, 512] — the lists of rows 0 and 1 hold two entries, one part at split 2: the bits of the training forward —,
    rows 6 and 7 two and four parts: the rule per class."""
    B, Hkv, T, D, dtype, k_lens, split = 2, 2, 100, 32, torch.bfloat16, [100, 512], 2
    Hq = Hkv * G
    assert (B * Hkv * (-(-T // KB) + 1)) % 8 != 0 and token_rows(T, 100, SMAX) == [0, 1] and len(ROWS[0]) == len(ROWS[1]) == 2
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 3320 + G)
    vis = visible([ROWS], B, Hkv, T, k_lens)
    ref, yard, lse64 = references(q, k, v, vis, G)
    got = run(mm, q, k, v, layout, lens, split=split)
    want = training_forward(mm, q, k, v, [ROWS], k_lens)
    one = rows_mask(B, Hq, T, k_lens, SMAX, ROWS, lambda r: parts_of(ROWS, r, split) == 1)
    assert one[0].all() and not one[1].any()
    same((got[0][one], got[1][one]), (want[0][one], want[1][one]), f"G={G}: the rows of one part against block_attention_forward_ex")
    check_rule(f"prefill parts G={G} split={split}", got[0], q, k, v, vis, G, got[1])
    check_classes(f"G={G} split={split}", got[0], got[1], ref, yard, lse64, tile_classes(B, Hq, T, k_lens, SMAX))


@pytest.mark.parametrize("dtype", DTYPES)
def test_3_k_lens_of_one_entry_and_outside_the_cache(mm, dev, dtype):
    """B = 3.  A 0-d k_lens (the kernels' lens_div = items) against the [B] tensor of equal entries, and k_lens [−3, 0, 700]
    — clamped to [0, Smax] where read: zero rows and −inf for the first two items, the third the call with 512 —, unsplit
    and split, bit for bit."""
    B, Hkv, G, T, D = 3, 2, 2, 100, 64
    layout = layout_from_rows(ROWS, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 3330)
    for split in (None, 2):
        one = run(mm, q, k, v, layout, torch.tensor(333, device=dev, dtype=torch.int32), split=split)
        same(one, run(mm, q, k, v, layout, lens_tensor([333] * B, dev), split=split), f"{dtype} split {split}: a 0-d k_lens")
        assert torch.isfinite(one[1]).all()
        wild = run(mm, q, k, v, layout, lens_tensor([-3, 0, 700], dev), split=split)
        assert (wild[0][:2] == 0).all() and (wild[1][:2] == NINF).all()
        full = run(mm, q, k, v, layout, lens_tensor([512] * B, dev), split=split)
        same((wild[0][2:], wild[1][2:]), (full[0][2:], full[1][2:]), f"{dtype} split {split}: k_lens 700 against 512")
        wild64 = run(mm, q, k, v, layout, lens_tensor([-3, 0, 700], dev, torch.int64), split=split)
        same(wild64, wild, f"{dtype} split {split}: int64 k_lens")


@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 96), (torch.float16, 64)])
def test_3_a_scale_of_the_callers(mm, dev, dtype, D):
    """scale = 0.37: the unsplit contiguous call has the bits of block_attention_forward_ex with that scale; the fp8 call with
    k_scale = 0.8125 those of the forward on the widened cache with the float32 product 0.37 · 0.8125 (one product, taken
    once); both, and their split 2 calls, under the rule against references that take the scale."""
    B, Hkv, G, T, k_lens, scale, ks = 2, 2, 2, 100, [333, 512], 0.37, 0.8125
    Hq = Hkv * G
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 3340 + D)
    vis = visible([ROWS], B, Hkv, T, k_lens)
    classes = tile_classes(B, Hq, T, k_lens, SMAX)
    ref, yard, lse64 = references_scaled(q, k, v, vis, G, scale)
    assert not np.allclose(ref.numpy(), references(q, k, v, vis, G)[0].numpy(), atol=1e-3), "the scale must matter"
    whole = run(mm, q, k, v, layout, lens, scale=scale)
    same(whole, training_forward(mm, q, k, v, [ROWS], k_lens, scale=scale), f"{dtype} D={D} scale {scale}: against block_attention_forward_ex")
    for name, res in (("unsplit", whole), ("split 2", run(mm, q, k, v, layout, lens, scale=scale, split=2))):
        check_classes(f"scale {scale} {dtype} D={D} {name}", res[0], res[1], ref, yard, lse64, classes)
    kc, vc = codes(3341 + D, B, Hkv, SMAX, D), codes(3342 + D, B, Hkv, SMAX, D)
    k8, v8 = wide(kc, dtype, dev), wide(vc, dtype, dev)
    product = float(np.float32(scale) * np.float32(ks))
    ref, yard, lse64 = references_scaled(q, k8.float() * ks, v8, vis, G, scale)
    for k_scale in (ks, torch.tensor([ks] * Hkv, device=dev)):
        whole = mm.block_sparse_attention_prefill_fp8(q, fp8(kc, dev), fp8(vc, dev), layout, lens, scale=scale, k_scale=k_scale, return_lse=True)
        same(whole, training_forward(mm, q, k8, v8, [ROWS], k_lens, scale=product), f"{dtype} D={D} fp8 scale {scale} · k_scale {ks}")
    got = mm.block_sparse_attention_prefill_fp8(q, fp8(kc, dev), fp8(vc, dev), layout, lens, scale=scale, k_scale=ks, return_lse=True, split=2)
    for name, res in (("unsplit", whole), ("split 2", got)):
        check_classes(f"fp8 scale {scale} k_scale {ks} {dtype} D={D} {name}", res[0], res[1], ref, yard, lse64, classes)


@pytest.mark.parametrize("T,dtype,D", [(1, torch.bfloat16, 96), (512, torch.float16, 64), (512, torch.bfloat16, 128)])
def test_3_one_token_and_a_whole_prompt_at_split_3(mm, dev, T, dtype, D):
    """T = 1 (two tiles an item, one row each) and T = 512 (nine tiles; item 0, at k_len 333, with 179 slots at negative
    positions): the rows of one part — lists of at most three entries — have the unsplit bits, the rule per class holds
    everywhere."""
    B, Hkv, G, k_lens, split = 2, 2, 2, [333, 512], 3
    Hq = Hkv * G
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 3350 + T)
    vis = visible([ROWS], B, Hkv, T, k_lens)
    ref, yard, lse64 = references(q, k, v, vis, G)
    whole, got = run(mm, q, k, v, layout, lens), run(mm, q, k, v, layout, lens, split=split)
    one = rows_mask(B, Hq, T, k_lens, SMAX, ROWS, lambda r: len(ROWS[r]) <= split)
    assert one.any() == (T > 1)
    same((got[0][one], got[1][one]), (whole[0][one], whole[1][one]), f"T={T} {dtype}: the rows of one part")
    check_rule(f"prefill parts T={T} {dtype} D={D} split={split}", got[0], q, k, v, vis, G, got[1])
    check_classes(f"T={T} {dtype} D={D} split={split}", got[0], got[1], ref, yard, lse64, tile_classes(B, Hq, T, k_lens, SMAX))
    if T == 512:
        assert (got[0][0, :, :179] == 0).all() and (got[1][0, :, :179] == NINF).all() and torch.isfinite(got[1][0, :, 179:]).all()


@pytest.mark.parametrize("dtype,D,split", [(torch.bfloat16, 64, None), (torch.float16, 96, 2)])
def test_3_one_entry_lens_through_the_c_entries(mm, capi, dev, dtype, D, split):
    """lens_count = 1 and new_lens_count = 1 with B = 2 (reachable through the C entries only: lens_div = items and
    new_lens_one in the walk and in the combine): the python call with the entries repeated, bit for bit; out and lse inside
    sentinels."""
    B, Hkv, G, T, k_len, new_len = 2, 2, 3, 100, 333, 37
    layout = layout_from_rows(ROWS, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 3360 + D)
    want = run(mm, q, k, v, layout, lens_tensor([k_len] * B, dev), new_lens=lens_tensor([new_len] * B, dev), split=split)
    assert (want[0][:, :, :T - new_len] == 0).all() and torch.isfinite(want[1][:, :, T - new_len:]).all()
    got = through_the_c_entry(mm, capi, dev, layout, q, k, v, lens_tensor([k_len], dev), lens_tensor([new_len], dev), G, split=split)
    same(got, want, f"{dtype} D={D} split {split}: one k_lens entry and one new_lens entry for two items")
    mixed = through_the_c_entry(mm, capi, dev, layout, q, k, v, lens_tensor([k_len, 512], dev), lens_tensor([new_len], dev), G, split=split)
    same(mixed, run(mm, q, k, v, layout, lens_tensor([k_len, 512], dev), new_lens=lens_tensor([new_len] * B, dev), split=split),
         f"{dtype} D={D} split {split}: one new_lens entry beside two k_lens")


def strided_pool(pool, fill):
    """The pool [P, Hkv, page, D] as the transposed view of [P, page, Hkv, D + 16] full of `fill`."""
    P, Hkv, page, D = pool.shape
    buf = torch.full((P, page, Hkv, D + 16), fill, device=pool.device, dtype=pool.dtype)
    view = buf[..., :D].transpose(1, 2)
    view.copy_(pool)
    return view


@pytest.mark.parametrize("fp8_cache,page", [(False, 16), (True, 32)])
def test_3_nothing_outside_the_pool_is_read_under_split(mm, dev, fp8_cache, page):
    """The prefill file's poisoned pool at split 2: NaN in every key no token sees, in the unreferenced pages and between the
    rows of a strided pool, −1 and P + 5 at the pages wholly beyond k_len: under the rule, and the bits of the contiguous split
    call on the clean cache."""
    B, Hkv, G, T, D, dtype, k_lens, split = 2, 2, 2, 100, 96, torch.bfloat16, [333, 449], 2
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 3370 + page)
    vis = visible([ROWS], B, Hkv, T, k_lens)
    if fp8_cache:
        kc, vc = codes(3371, B, Hkv, SMAX, D), codes(3372, B, Hkv, SMAX, D)
        k, v = wide(kc, dtype, dev), wide(vc, dtype, dev)
        kp, vp, table = pools(poisoned(kc, vis), poisoned(vc, vis), page, 3373)
        clean = mm.block_sparse_attention_prefill_fp8(q, fp8(kc, dev), fp8(vc, dev), layout, lens, return_lse=True, split=split)
    else:
        kp, vp, table = paged(poison_unseen(k, vis), poison_unseen(v, vis), page, 3373)
        clean = run(mm, q, k, v, layout, lens, split=split)
    P, bad = kp.shape[0], NANB if fp8_cache else NAN
    for b, n in enumerate(k_lens):
        beyond = torch.arange((n + page - 1) // page, SMAX // page, device=table.device)
        kp[table[b, beyond].long()] = bad
        vp[table[b, beyond].long()] = bad
        table[b, beyond] = torch.where(beyond % 2 == 0, -1, P + 5).to(torch.int32)
    if fp8_cache:
        ks, vs = strided_pool(kp.to(dev), NANB).view(torch.float8_e4m3fn), strided_pool(vp.to(dev), NANB).view(torch.float8_e4m3fn)
        got = mm.block_sparse_attention_prefill_paged_fp8(q, ks, vs, table.to(dev), layout, lens, return_lse=True, split=split)
    else:
        ks, vs = strided_pool(kp, NAN), strided_pool(vp, NAN)
        got = mm.block_sparse_attention_prefill_paged(q, ks, vs, table, layout, lens, return_lse=True, split=split)
    assert not ks.is_contiguous()
    check_rule(f"prefill parts poisoned pool, page {page}, fp8 {fp8_cache}, split {split}", got[0], q, k, v, vis, G, got[1])
    same(got, clean, f"page {page} fp8 {fp8_cache} split {split}: against the clean contiguous cache")


@pytest.mark.parametrize("fp8_cache,page", [(False, 16), (True, 32)])
def test_3_invalid_entries_hide_their_keys_under_split(mm, dev, fp8_cache, page):
    """The prefill file's hidden pages at split 2: −1 and P + 5 at seen logical pages — inside the diagonal blocks of tiles 4, 5
    and 7 and in block 0 — over NaN pages: the rule on the mask without their keys; tile 3 of item 0, whose list names none
    of them, has the bits of the contiguous split call on the clean cache."""
    B, Hkv, G, T, D, dtype, k_lens, split = 2, 2, 2, 100, 64, torch.bfloat16, [333, 512], 2
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 3380 + page)
    vis = visible([ROWS], B, Hkv, T, k_lens)
    hidden = {0: [256 // page, 320 // page], 1: [448 // page, 0]}
    if fp8_cache:
        kc, vc = codes(3381, B, Hkv, SMAX, D), codes(3382, B, Hkv, SMAX, D)
        k, v = wide(kc, dtype, dev), wide(vc, dtype, dev)
        kp, vp, table = pools(kc, vc, page, 3383)
        clean = mm.block_sparse_attention_prefill_fp8(q, fp8(kc, dev), fp8(vc, dev), layout, lens, return_lse=True, split=split)
    else:
        kp, vp, table = paged(k, v, page, 3383)
        clean = run(mm, q, k, v, layout, lens, split=split)
    P, bad = kp.shape[0], NANB if fp8_cache else NAN
    for b, ws in hidden.items():
        for i, w in enumerate(ws):
            kp[table[b, w].long()] = bad
            vp[table[b, w].long()] = bad
            table[b, w] = (-1, P + 5)[i]
            vis[b, :, :, w * page:(w + 1) * page] = False
    if fp8_cache:
        got = mm.block_sparse_attention_prefill_paged_fp8(q, fp8(kp, dev), fp8(vp, dev), table.to(dev), layout, lens, return_lse=True, split=split)
    else:
        got = mm.block_sparse_attention_prefill_paged(q, kp, vp, table, layout, lens, return_lse=True, split=split)
    check_rule(f"prefill parts hidden pages, page {page}, fp8 {fp8_cache}, split {split}", got[0], q, k, v, vis, G, got[1])
    untouched = torch.zeros(B, Hkv * G, T, dtype=torch.bool)
    for b, ws in hidden.items():
        blocks = {w * page // KB for w in ws}
        one = rows_mask(B, Hkv * G, T, k_lens, SMAX, ROWS, lambda r: not any(j in blocks and j <= r for j in ROWS[r]))
        untouched[b] = one[b]
    assert untouched[0, :, :23].all() and int(untouched.sum()) == Hkv * G * 23, "tile 3 of item 0 alone names no hidden page"
    same((got[0][untouched], got[1][untouched]), (clean[0][untouched], clean[1][untouched]), f"page {page} fp8 {fp8_cache}: tile 3 of item 0")
