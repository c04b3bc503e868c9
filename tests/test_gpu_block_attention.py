"""matmuls.block_sparse_attention on the MI355X: forward and the three gradients against dense masked attention on the CPU
in float64 (the mask is the block layout expanded by `block`, and-ed with the lower triangle when causal; rows that see
nothing are zero), held to the project's rule e_dev ≤ 8 · e_ref on scaled_err, where e_ref is the error of the same
computation with every stage in fp32 on widened inputs, narrowed to T after the scores, after the softmax and after the
product, with autograd through it.  Beside the rule: exact zeros for rows that see nothing and keys nobody sees, bits
that do not depend on the batch or the layout's form, causal skipping, NaN outside the kept blocks, block = 128 as its
expansion, determinism, and the memory autograd keeps.  A rectangular batch (Sq ≠ Sk: q's item stride differs from k's)
under the rule and item by item; and through the C ABI every dense operand with a leading dimension and an item stride of
its own, NaN around the inputs and a sentinel around the outputs, and k, v shared by the batch (item stride 0)."""
import pytest
import torch

from gpu_helpers import (SENTINEL, assert_outside_untouched, assert_same_bits, padded, _block_attention_bwd_through_the_c_abi,
                         _block_attention_fwd_through_the_c_abi)
from sparse_attention_helpers import assert_tensor_under_rule, dense_step, device_pattern

pytestmark = pytest.mark.gpu

NAMES = ("out", "dq", "dk", "dv")


def layout_from_rows(rows_cols, cols, dev, index_dtype=torch.int64):
    """A 2-d CSR block layout (values 1) from per-block-row column lists, kept in the order given (unsorted allowed)."""
    crow = [0]
    for c in rows_cols:
        crow.append(crow[-1] + len(c))
    col = [j for c in rows_cols for j in c]
    return torch.sparse_csr_tensor(torch.tensor(crow, dtype=index_dtype, device=dev), torch.tensor(col, dtype=index_dtype, device=dev),
                                   torch.ones(len(col), device=dev), size=(len(rows_cols), cols))


def block_mask(layout, block, causal=False):
    """Boolean CPU mask [*l_lead, Sq, Sk] of a block layout."""
    vals = torch.ones_like(torch.Tensor.values(layout), dtype=torch.float32)
    m = torch.sparse_csr_tensor(torch.Tensor.crow_indices(layout), torch.Tensor.col_indices(layout), vals, size=layout.shape)
    m = (m.cpu().to_dense() != 0).repeat_interleave(block, -2).repeat_interleave(block, -1)
    if causal:
        m = m & torch.ones(m.shape[-2:], dtype=torch.bool).tril()
    return m


def operands(dev, lead, Sq, Sk, D, dtype, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    q = torch.randn(lead + (Sq, D), device=dev, generator=g).to(dtype)
    k, v = (torch.randn(lead + (Sk, D), device=dev, generator=g).to(dtype) for _ in range(2))
    w = torch.randn(lead + (Sq, D), device=dev, generator=g).to(dtype)
    return q, k, v, w


def step(mm, q, k, v, layout, w, **kw):
    """(out, dq, dk, dv) of one forward + backward on fresh leaves."""
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = mm.block_sparse_attention(q, k, v, layout, **kw)
    return (out.detach(),) + torch.autograd.grad(out, (q, k, v), grad_outputs=w)


def check_rule(what, got, q, k, v, w, mask, scale=None):
    scale = 1.0 / q.shape[-1] ** 0.5 if scale is None else scale
    ref = dense_step(q, k, v, w, mask, scale, torch.float64)
    yard = dense_step(q, k, v, w, mask, scale, torch.float32, narrow=q.dtype)
    for name, g, r, y in zip(NAMES, got, ref, yard):
        assert g.dtype == q.dtype and g.shape == r.shape, (what, name)
        assert_tensor_under_rule(f"block attention {what} {name}", g, y, r)


def assert_same_step(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert_same_bits(g, w, f"{what}: {name}")


FULL = [[0, 1, 2, 3]] * 4
DIAGONAL = [[0], [1], [2], [3]]
BAND_GLOBAL = [[0], [1, 0], [], [0, 2]]  # band + global first column; block row 2 empty, block column 3 never kept


@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 32), (torch.bfloat16, 128), (torch.float16, 64)])
@pytest.mark.parametrize("name,rows", [("full", FULL), ("diagonal", DIAGONAL), ("band+global", BAND_GLOBAL)])
def test_1_small_layouts(mm, dev, dtype, D, name, rows):
    S = 256
    assert mm.block_attention_takes(dtype, D, 64)
    layout = layout_from_rows(rows, 4, dev)
    q, k, v, w = operands(dev, (), S, S, D, dtype, 7 + D)
    got = step(mm, q, k, v, layout, w)
    check_rule(f"{name} {dtype} D={D}", got, q, k, v, w, block_mask(layout, 64))
    if rows is BAND_GLOBAL:
        assert (got[0][128:192] == 0).all() and (got[1][128:192] == 0).all()  # the empty block row
        assert (got[2][192:] == 0).all() and (got[3][192:] == 0).all()        # the block column nobody keeps
        assert got[2][:192].abs().sum() > 0 and got[3][:192].abs().sum() > 0


@pytest.mark.parametrize("index_dtype", [torch.int64, torch.int32])
def test_1_rectangular_layout(mm, dev, index_dtype):
    Sq, Sk, D = 128, 320, 96
    layout = layout_from_rows([[4, 1, 0], [2, 3]], 5, dev, index_dtype)
    q, k, v, w = operands(dev, (), Sq, Sk, D, torch.bfloat16, 11)
    got = step(mm, q, k, v, layout, w, scale=0.2)
    check_rule("2 x 5, D=96", got, q, k, v, w, block_mask(layout, 64), scale=0.2)


def test_2_long_block_row_with_a_moving_maximum(mm, dev):
    Sq, Sk, D = 64, 2560, 64
    layout = layout_from_rows([list(range(40))], 40, dev)
    q, k, v, w = operands(dev, (), Sq, Sk, D, torch.bfloat16, 13)
    q = (q.float() * 4).to(q.dtype)
    k = k.clone()
    k[-64:] = (k[-64:].float() * 3).to(k.dtype)  # the row maximum arrives in the LAST block
    got = step(mm, q, k, v, layout, w)
    check_rule("1 x 40", got, q, k, v, w, block_mask(layout, 64))


def batch_case(mm, dev, form, seed=17):
    lead, S, D = (2, 3), 256, 64
    l_lead = {"per item": (2, 3), "per head": (3,), "shared": ()}[form]
    layout = device_pattern(dev, l_lead, 4, 0.5, seed)  # exactly 2 of 4 blocks per block row, built on the device
    q, k, v, w = operands(dev, lead, S, S, D, torch.bfloat16, seed + 1)
    return layout, q, k, v, w, step(mm, q, k, v, layout, w)


def item_layout(layout, i):
    if layout.dim() == 2:
        return layout
    crow = layout.crow_indices().reshape(-1, layout.shape[-2] + 1)
    col = layout.col_indices().reshape(crow.shape[0], -1)
    n = crow.shape[0]
    return torch.sparse_csr_tensor(crow[i % n].contiguous(), col[i % n].contiguous(), torch.ones(col.shape[1], device=col.device),
                                   size=tuple(layout.shape[-2:]))


@pytest.mark.parametrize("form", ["per item", "per head", "shared"])
def test_3_batch_and_broadcast(mm, dev, form):
    layout, q, k, v, w, got = batch_case(mm, dev, form)
    S, D = q.shape[-2:]
    flat = [t.reshape(-1, S, D) for t in (q, k, v, w)]
    for i in range(6):
        want = step(mm, flat[0][i], flat[1][i], flat[2][i], item_layout(layout, i), flat[3][i])
        assert_same_step([g.reshape(-1, S, D)[i] for g in got], want, f"{form}, item {i}")
    i = 1  # item (0, 1) under the rule
    check_rule(f"batch ({form}) item (0, 1)", [g[0, 1] for g in got], q[0, 1], k[0, 1], v[0, 1], w[0, 1],
               block_mask(item_layout(layout, i), 64))


def test_4_causal(mm, dev):
    S, D = 256, 64
    q, k, v, w = operands(dev, (), S, S, D, torch.bfloat16, 19)
    tril = [[0], [0, 1], [0, 1, 2], [0, 1, 2, 3]]
    lay = layout_from_rows(tril, 4, dev)
    got = step(mm, q, k, v, lay, w, causal=True)
    check_rule("causal", got, q, k, v, w, block_mask(lay, 64, causal=True))
    above = layout_from_rows([[0, 2], [0, 1], [0, 1, 2], [0, 1, 2, 3]], 4, dev)  # one kept block above the diagonal
    assert_same_step(step(mm, q, k, v, above, w, causal=True), got, "a kept block above the diagonal")
    no_diag1 = layout_from_rows([[0], [0], [0, 1, 2], [0, 1, 2, 3]], 4, dev)  # block row 1 sees block 0 only
    check_rule("causal, row 1 without its diagonal", step(mm, q, k, v, no_diag1, w, causal=True), q, k, v, w,
               block_mask(no_diag1, 64, causal=True))
    no_diag0 = layout_from_rows([[1], [0, 1], [0, 1, 2], [0, 1, 2, 3]], 4, dev)  # block row 0 sees nothing
    got0 = step(mm, q, k, v, no_diag0, w, causal=True)
    check_rule("causal, row 0 without its diagonal", got0, q, k, v, w, block_mask(no_diag0, 64, causal=True))
    assert (got0[0][:64] == 0).all() and (got0[1][:64] == 0).all()
    with pytest.raises(ValueError, match="causal=True needs Sq == Sk"):
        mm.block_sparse_attention(q[:128], k, v, layout_from_rows([[0], [1]], 4, dev), causal=True)


def test_5_never_kept_positions_are_not_read(mm, dev):
    S, D = 256, 64
    layout = layout_from_rows(BAND_GLOBAL, 4, dev)
    q, k, v, w = operands(dev, (), S, S, D, torch.bfloat16, 23)
    k0, v0 = k.clone(), v.clone()
    k0[192:], v0[192:] = 0, 0
    kn, vn = k0.clone(), v0.clone()
    kn[192:], vn[192:] = float("nan"), float("nan")
    want = step(mm, q, k0, v0, layout, w)
    got = step(mm, q, kn, vn, layout, w)
    for g in got[:2]:
        assert torch.isfinite(g.float()).all()
    assert_same_bits(got[0], want[0], "out beside NaN keys")
    assert_same_bits(got[1], want[1], "dq beside NaN keys")
    assert (got[2][192:] == 0).all() and (got[3][192:] == 0).all()
    assert_same_bits(got[2], want[2], "dk beside NaN keys")
    assert_same_bits(got[3], want[3], "dv beside NaN keys")


def test_6_block_128_is_its_expansion(mm, dev):
    S, D = 256, 64
    q, k, v, w = operands(dev, (), S, S, D, torch.float16, 29)
    coarse = layout_from_rows([[1], [1, 0]], 2, dev)
    fine = layout_from_rows([[2, 3], [2, 3], [2, 3, 0, 1], [2, 3, 0, 1]], 4, dev)  # sub-block order
    got = step(mm, q, k, v, coarse, w, block=128)
    assert_same_step(got, step(mm, q, k, v, fine, w, block=64), "block = 128")
    check_rule("block = 128", got, q, k, v, w, block_mask(coarse, 128))


def test_7_determinism(mm, dev):
    for form in ("per item", "shared"):
        first = batch_case(mm, dev, form)[-1]
        second = batch_case(mm, dev, form)[-1]
        assert_same_step(second, first, f"run to run ({form})")


def test_8_memory(mm, dev):
    items, S, D, nb = 8, 2048, 64, 32
    rows = [[j for j in (i - 1, i, i + 1) if 0 <= j < nb] for i in range(nb)]  # a band 3 blocks wide
    layout = layout_from_rows(rows, nb, dev)
    q, k, v, w = operands(dev, (items,), S, S, D, torch.bfloat16, 31)
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = mm.block_sparse_attention(q, k, v, layout)
    grads = torch.autograd.grad(out, (q, k, v), grad_outputs=w)
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated() - before
    print(f"block attention memory: forward + backward peak {used} bytes over the operands "
          f"(dense scores {items * S * S * 2}, design {4 * items * S * D * 2 + 2 * items * S * 4})")
    assert used < items * S * S * 2
    assert all(torch.isfinite(g.float()).all() for g in grads)


# Sq = 128, Sk = 192: 2 × 3 blocks.  Per item: equal entry counts, as torch builds a batch; item 1 has an empty block row
# and a block column nobody keeps.
RECT_PER_ITEM = [[[1], [2]], [[], [2, 0]], [[2], [0]]]
RECT_SHARED = [[2, 0], [0, 1, 2]]


def rect_layouts(dev, form):
    """(layout, the items' 2-d layouts) of the rectangular batch of 3."""
    items = [layout_from_rows(r, 3, dev) for r in (RECT_PER_ITEM if form == "per item" else [RECT_SHARED] * 3)]
    if form == "shared":
        return items[0], items
    crow = torch.stack([l.crow_indices() for l in items])
    col = torch.stack([l.col_indices() for l in items])
    return torch.sparse_csr_tensor(crow, col, torch.ones(col.shape, device=dev), size=(3, 2, 3)), items


@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 32), (torch.float16, 96)])
@pytest.mark.parametrize("form", ["per item", "shared"])
def test_9_rectangular_batch(mm, dev, dtype, D, form):
    nb, Sq, Sk = 3, 128, 192
    layout, items = rect_layouts(dev, form)
    q, k, v, w = operands(dev, (nb,), Sq, Sk, D, dtype, 41 + D)
    got = step(mm, q, k, v, layout, w)
    mask = torch.stack([block_mask(l, 64) for l in items])
    check_rule(f"rectangular batch ({form}) {dtype} D={D}", got, q, k, v, w, mask)
    for i in range(nb):
        assert_same_step([g[i] for g in got], step(mm, q[i], k[i], v[i], items[i], w[i]), f"rectangular batch ({form}), item {i}")
    if form == "per item":
        assert (got[0][1, :64] == 0).all() and (got[1][1, :64] == 0).all()        # item 1's empty block row
        assert (got[2][1, 64:128] == 0).all() and (got[3][1, 64:128] == 0).all()  # item 1's block column nobody keeps
        assert got[2][1, :64].abs().sum() > 0 and got[3][1, 128:].abs().sum() > 0


@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 32), (torch.float16, 96)])
def test_10_leading_dimensions_and_strides(mm, cmm, capi, dev, dtype, D):
    """The per-item rectangular batch through the C ABI: each of the eight dense operands in a buffer of its own with its
    own leading dimension and item stride (operand number i: ld = D + 8(i + 1), stride = rows · ld + 8(i + 1)), NaN around
    the inputs, a sentinel around the outputs; every logical output has the bits of the packed call through custom_mm.
    Then k, v shared by the batch: item stride 0 on one item equals the packed call on that item expanded."""
    nb, Sq, Sk = 3, 128, 192
    nan = float("nan")
    layout, _ = rect_layouts(dev, "per item")
    rec = mm._block_layout(layout, dev, 1, mm._csr_state(layout))
    offsets, columns, nnz, L = rec["fwd"]
    t_off, t_col = mm._block_layout_transposed(rec, Sq // 64, Sk // 64)
    assert L == nb and nnz == 6
    q, k, v, w = operands(dev, (nb,), Sq, Sk, D, dtype, 51 + D)
    scale = 1.0 / D ** 0.5

    def packed(k3, v3):
        out, dq = torch.full_like(q, nan), torch.full_like(q, nan)
        dk, dv = torch.full_like(k3, nan), torch.full_like(k3, nan)
        lse = torch.full((nb, Sq), nan, device=dev)
        cmm.block_attention_forward(offsets, columns, nnz, q, k3, v3, scale, False, out, lse)
        cmm.block_attention_backward(offsets, columns, t_off, t_col, nnz, q, k3, v3, out, w, lse, scale, False, dq, dk, dv)
        return out, lse, dq, dk, dv

    def strided(k3, v3, kv_stride, what):
        pq, pk, pv, pw = padded(q, 0, nan), padded(k3, 1, nan), padded(v3, 2, nan), padded(w, 4, nan)
        pout = padded(torch.full_like(q, SENTINEL), 3, SENTINEL)
        lse = torch.full((nb, Sq), nan, device=dev)
        st = _block_attention_fwd_through_the_c_abi(capi, dtype, offsets, columns, nnz, L, nb, Sq, Sk, D, 0, pq, pk, pv, scale, pout,
                                                    lse, kv_stride)
        assert st == 0, (what, st)
        torch.cuda.synchronize()
        assert_outside_untouched(pout, f"{what}: out")
        pout_in = padded(pout.x.contiguous(), 3, nan)  # the backward reads out
        outs = [padded(torch.full((nb, rows, D), SENTINEL, device=dev, dtype=dtype), i, SENTINEL)
                for i, rows in ((5, Sq), (6, Sk), (7, Sk))]
        st = _block_attention_bwd_through_the_c_abi(capi, dtype, offsets, columns, t_off, t_col, nnz, L, nb, Sq, Sk, D, 0, pq, pk, pv,
                                                    pout_in, pw, lse, scale, *outs, kv_stride)
        assert st == 0, (what, st)
        torch.cuda.synchronize()
        for name, p in zip(("dq", "dk", "dv"), outs):
            assert_outside_untouched(p, f"{what}: {name}")
        return (pout.x, lse) + tuple(p.x for p in outs)

    def compare(got, want, what):
        for name, g, x in zip(("out", "lse", "dq", "dk", "dv"), got, want):
            assert_same_bits(g, x, f"{what}: {name}")
            assert not torch.isnan(g.float()).any(), (what, name)

    compare(strided(k, v, None, "own ld and strides"), packed(k, v), f"{dtype} D={D}, own ld and strides")
    k1, v1 = k[1:2], v[1:2]  # one k, v for the whole batch
    compare(strided(k1, v1, 0, "shared k, v"), packed(k1.expand(nb, Sk, D).contiguous(), v1.expand(nb, Sk, D).contiguous()),
            f"{dtype} D={D}, strideK = strideV = 0")
