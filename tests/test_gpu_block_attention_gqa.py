"""Grouped-query heads and per-item lengths of matmuls.block_sparse_attention on the MI355X.  Grouped:
out and dq are the bits of the call on repeated k / v, dk and dv are under the project's rule e_dev ≤ 8 · e_ref against
float64 (dense_step on the repeated k / v, the group's gradients summed in float64; the yardstick the same in fp32,
narrowed), and the head mapping is pinned bit for bit with one-head gradients.  Lengths: lengths that change nothing give
the bits of the call without them, lengths on block boundaries the bits of the call on the cut layout, lengths inside a
block — with NaN in every padded row of q, k, v and the incoming gradient — finite outputs, exact zeros on the padding,
the rule on the rest, and each item the bits of the 2-d call on it alone.  Everything at once, twice, for determinism; and
the _ex entries of the C ABI on operands with leading dimensions and item strides of their own."""
import pytest
import torch

from block_attention_gqa_helpers import bwd_ex_through_the_c_abi, fill_padding, fwd_ex_through_the_c_abi, length_mask
from gpu_helpers import SENTINEL, assert_outside_untouched, assert_same_bits, padded
from sparse_attention_helpers import assert_tensor_under_rule, dense_step

pytestmark = pytest.mark.gpu

NAMES = ("out", "dq", "dk", "dv")
CONFIGS = [(torch.bfloat16, 32), (torch.bfloat16, 128), (torch.float16, 64)]
S = 256
NAN = float("nan")


def layout_from_rows(rows_cols, cols, dev):
    """A 2-d CSR block layout (values 1) from per-block-row column lists, kept in the order given."""
    crow = [0]
    for c in rows_cols:
        crow.append(crow[-1] + len(c))
    col = [j for c in rows_cols for j in c]
    return torch.sparse_csr_tensor(torch.tensor(crow, device=dev), torch.tensor(col, device=dev), torch.ones(len(col), device=dev),
                                   size=(len(rows_cols), cols))


def stack_layouts(items, dev):
    """2-d layouts of equal entry counts as one batched layout [len(items), rows, cols]."""
    crow = torch.stack([l.crow_indices() for l in items])
    col = torch.stack([l.col_indices() for l in items])
    return torch.sparse_csr_tensor(crow, col, torch.ones(col.shape, device=dev), size=(len(items),) + tuple(items[0].shape))


def block_mask(layout, causal=False):
    """Boolean CPU mask [*l_lead, Sq, Sk] of a layout in 64-blocks."""
    vals = torch.ones_like(torch.Tensor.values(layout), dtype=torch.float32)
    m = torch.sparse_csr_tensor(torch.Tensor.crow_indices(layout), torch.Tensor.col_indices(layout), vals, size=layout.shape)
    m = (m.cpu().to_dense() != 0).repeat_interleave(64, -2).repeat_interleave(64, -1)
    return m & torch.ones(m.shape[-2:], dtype=torch.bool).tril() if causal else m


def operands(dev, lead, kv_lead, Sq, Sk, D, dtype, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    q = torch.randn(lead + (Sq, D), device=dev, generator=g).to(dtype)
    k, v = (torch.randn(kv_lead + (Sk, D), device=dev, generator=g).to(dtype) for _ in range(2))
    w = torch.randn(lead + (Sq, D), device=dev, generator=g).to(dtype)
    return q, k, v, w


def step(mm, q, k, v, layout, w, **kw):
    """(out, dq, dk, dv) of one forward + backward on fresh leaves."""
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = mm.block_sparse_attention(q, k, v, layout, **kw)
    return (out.detach(),) + torch.autograd.grad(out, (q, k, v), grad_outputs=w)


def grouped_reference(q, k, v, w, mask, G, wide, narrow=None):
    """dense_step on k, v repeated G times along the head dimension, dk and dv summed over each group in `wide`."""
    scale = 1.0 / q.shape[-1] ** 0.5
    out, dq, dk, dv = dense_step(q, k.repeat_interleave(G, -3), v.repeat_interleave(G, -3), w, mask, scale, wide, narrow=narrow)
    fold = lambda t: t.reshape(t.shape[:-3] + (t.shape[-3] // G, G) + t.shape[-2:]).sum(-3)  # noqa: E731
    return out, dq, fold(dk), fold(dv)


def check_rule(what, got, q, k, v, w, mask, G=1, names=NAMES):
    ref = grouped_reference(q, k, v, w, mask, G, torch.float64)
    yard = grouped_reference(q, k, v, w, mask, G, torch.float32, narrow=q.dtype)
    for name, g, r, y in zip(NAMES, got, ref, yard):
        assert g.dtype == q.dtype and g.shape == r.shape, (what, name)
        if name in names:
            assert_tensor_under_rule(f"block attention gqa {what} {name}", g, y, r)


def assert_same_step(got, want, what, names=NAMES):
    for name, g, x in zip(NAMES, got, want):
        if name in names:
            assert_same_bits(g, x, f"{what}: {name}")


# equal entry counts per head, as torch builds a batch: 16 would not stack with 4, so every head keeps 2 blocks per row
PER_HEAD = [[[0, 1], [1, 0], [2, 3], [3, 2]], [[0, 3], [1, 2], [2, 1], [3, 0]], [[1, 0], [1, 2], [3, 2], [0, 3]],
            [[3, 2], [0, 1], [1, 2], [2, 3]]]
SHARED = [[0, 1], [0, 1, 2], [1, 2, 3], [3, 0]]
BAND_GLOBAL = [[0], [1, 0], [], [0, 2]]  # band + global first column; block row 2 empty, block column 3 never kept


def the_layout(dev, form):
    if form == "per head":
        return stack_layouts([layout_from_rows(r, 4, dev) for r in PER_HEAD], dev)
    return layout_from_rows(SHARED if form == "shared" else BAND_GLOBAL, 4, dev)


# ---- 1. grouped = the repeated call ------------------------------------------------------------------------------------

def grouped_against_repeated(mm, dev, dtype, D, Hkv, form, causal, seed):
    G = 4 // Hkv
    layout = the_layout(dev, form)
    q, k, v, w = operands(dev, (2, 4), (2, Hkv), S, S, D, dtype, seed)
    got = step(mm, q, k, v, layout, w, causal=causal)
    assert got[2].shape == k.shape and got[3].shape == v.shape
    want = step(mm, q, k.repeat_interleave(G, -3), v.repeat_interleave(G, -3), layout, w, causal=causal)
    what = f"{dtype} D={D} G={G} {form} causal={causal}"
    assert_same_step(got, want, what, names=("out", "dq"))
    check_rule(what, got, q, k, v, w, block_mask(layout, causal).expand(2, 4, S, S), G, names=("dk", "dv"))
    return got


@pytest.mark.parametrize("dtype,D", CONFIGS)
@pytest.mark.parametrize("Hkv", [2, 1])
@pytest.mark.parametrize("form", ["per head", "shared"])
@pytest.mark.parametrize("causal", [False, True])
def test_1_grouped_is_the_repeated_call(mm, dev, dtype, D, Hkv, form, causal):
    grouped_against_repeated(mm, dev, dtype, D, Hkv, form, causal, 3 + D + Hkv)


def test_1_grouped_band_global_causal_d96(mm, dev):
    got = grouped_against_repeated(mm, dev, torch.bfloat16, 96, 2, "band+global", True, 5)
    assert (got[0][..., 128:192, :] == 0).all() and (got[1][..., 128:192, :] == 0).all()  # the empty block row
    assert (got[2][..., 192:, :] == 0).all() and (got[3][..., 192:, :] == 0).all()        # the block column nobody keeps
    assert got[2][..., :192, :].abs().sum() > 0


# ---- 2. the head mapping, exactly ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,D", CONFIGS)
@pytest.mark.parametrize("Hkv", [2, 1])
def test_2_head_mapping_is_pinned_by_one_head_gradients(mm, dev, dtype, D, Hkv):
    G = 4 // Hkv
    layout = the_layout(dev, "per head")
    q, k, v, w = operands(dev, (2, 4), (2, Hkv), S, S, D, dtype, 11 + D)
    for g in range(G):
        w1 = torch.zeros_like(w)
        w1[:, g::G] = w[:, g::G]  # query heads h·G + g only
        got = step(mm, q, k, v, layout, w1)
        for h in range(Hkv):
            head = h * G + g
            lay = layout_from_rows(PER_HEAD[head], 4, dev)
            want = step(mm, q[:, head], k[:, h], v[:, h], lay, w[:, head])
            assert_same_bits(got[2][:, h], want[2], f"dk of kv head {h} from query head {head}")
            assert_same_bits(got[3][:, h], want[3], f"dv of kv head {h} from query head {head}")


# ---- 3. lengths that change nothing ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,D", CONFIGS)
def test_3_full_lengths_change_no_bit(mm, dev, dtype, D):
    layout = the_layout(dev, "shared")
    q, k, v, w = operands(dev, (2, 2), (2, 2), S, S, D, dtype, 13 + D)
    want = step(mm, q, k, v, layout, w, causal=True)
    for lens in (torch.tensor([S, S], device=dev), torch.tensor([S + 1, 2 ** 31 - 1], device=dev, dtype=torch.int32),
                 torch.tensor([[S, S + 7], [S, S]], device=dev)):
        assert_same_step(step(mm, q, k, v, layout, w, causal=True, q_lens=lens, k_lens=lens), want, f"lengths {lens.tolist()}")


# ---- 4. lengths on block boundaries ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,D", CONFIGS)
def test_4_lengths_on_block_boundaries(mm, dev, dtype, D):
    q, k, v, w = operands(dev, (2,), (2,), S, S, D, dtype, 17 + D)
    layout = layout_from_rows(SHARED, 4, dev)
    lens = torch.tensor([128, 128], device=dev)
    cut_cols = layout_from_rows([[j for j in r if j < 2] for r in SHARED], 4, dev)
    got = step(mm, q, k, v, layout, w, k_lens=lens)
    assert_same_step(got, step(mm, q, k, v, cut_cols, w), "k_len = 128")
    assert (got[2][:, 128:] == 0).all() and (got[3][:, 128:] == 0).all()
    cut_rows = layout_from_rows([r if i < 2 else [] for i, r in enumerate(SHARED)], 4, dev)
    got = step(mm, q, k, v, layout, w, q_lens=lens)
    assert_same_step(got, step(mm, q, k, v, cut_rows, w), "q_len = 128")
    assert (got[0][:, 128:] == 0).all() and (got[1][:, 128:] == 0).all()
    for kw in ({"k_lens": torch.tensor([0, -5], device=dev)}, {"q_lens": torch.tensor([-1, 0], device=dev)}):
        for name, g in zip(NAMES, step(mm, q, k, v, layout, w, **kw)):
            assert (g == 0).all(), (kw, name)


# ---- 5. lengths inside a block, poisoned padding ------------------------------------------------------------------------------

def poisoned_case(mm, dev, dtype, D, Sq, Sk, layout, q_lens, k_lens, seed, Hkv=2, causal=False):
    """One item per length, lens [B] against lead [B, 2]: the call on poisoned operands; returns (got, clean operands)."""
    B = len(q_lens if q_lens is not None else k_lens)
    q, k, v, w = operands(dev, (B, 2), (B, Hkv), Sq, Sk, D, dtype, seed)
    q, w = (fill_padding(t, q_lens, 0) for t in (q, w))
    k, v = (fill_padding(t, k_lens, 0) for t in (k, v))
    dev_lens = {n: None if l is None else torch.tensor(l, device=dev) for n, l in (("q_lens", q_lens), ("k_lens", k_lens))}
    got = step(mm, fill_padding(q, q_lens, NAN), fill_padding(k, k_lens, NAN), fill_padding(v, k_lens, NAN), layout,
               fill_padding(w, q_lens, NAN), causal=causal, **dev_lens)
    for name, g in zip(NAMES, got):
        assert torch.isfinite(g.float()).all(), name
    for b in range(B):
        if q_lens is not None:
            assert (got[0][b, :, q_lens[b]:] == 0).all() and (got[1][b, :, q_lens[b]:] == 0).all(), b
        if k_lens is not None:
            assert (got[2][b, :, k_lens[b]:] == 0).all() and (got[3][b, :, k_lens[b]:] == 0).all(), b
    return got, (q, k, v, w), dev_lens


@pytest.mark.parametrize("dtype,D", CONFIGS)
def test_5_lengths_inside_a_block_with_poisoned_padding(mm, dev, dtype, D):
    # Every length on each side, crossed, with two precautions about rows that see ONE existing key.  Such a row has P ≡ 1,
    # so that key's dv row is the plain sum of those rows' dout: the yardstick (whose gradients stay in fp32) has it exact, a
    # result in T rounds it once at the store, and summed over many query rows it is the tensor's largest element — the
    # whole-tensor figure would then measure the output format's half-ulp (2⁻⁹ in bfloat16, 2⁻¹¹ in float16) against an
    # e_ref without any rounding in it, which no result in T can meet.  So k_len = 1 goes with q_len = 1 (that dv row is one
    # dout row, exact in T as well), and every block row of the layout keeps block 0, so that k_len = 65 leaves no block
    # row with key 64 alone.
    layout = layout_from_rows([[0, 1], [0, 1, 2], [0, 2, 3], [3, 0]], 4, dev)
    q_lens, k_lens = [1, 63, 65, 200], [1, 200, 63, 65]
    got, (q, k, v, w), _ = poisoned_case(mm, dev, dtype, D, S, S, layout, q_lens, k_lens, 19 + D)
    mask = length_mask(block_mask(layout).expand(4, 2, S, S), q_lens, k_lens)
    check_rule(f"lengths {dtype} D={D}", got, q, k, v, w, mask)
    for b in range(4):  # batch independence: the 2-d call on the item alone, its own lengths as 0-d tensors
        for h in range(2):
            want = step(mm, q[b, h], k[b, h], v[b, h], layout, w[b, h], q_lens=torch.tensor(q_lens[b], device=dev),
                        k_lens=torch.tensor(k_lens[b], device=dev))
            assert_same_step([g[b, h] for g in got], want, f"item {b}, head {h} alone")


def test_5_rectangular_with_a_key_length(mm, dev):
    Sq, Sk, D = 128, 320, 96
    layout = layout_from_rows([[4, 1, 0], [2, 3]], 5, dev)
    got, (q, k, v, w), _ = poisoned_case(mm, dev, torch.bfloat16, D, Sq, Sk, layout, None, [257, 320], 23)
    check_rule("rectangular, k_lens = 257", got, q, k, v, w, length_mask(block_mask(layout).expand(2, 2, Sq, Sk), None, [257, 320]))


# ---- 6. everything at once ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,D", CONFIGS)
def test_6_grouped_causal_per_head_lengths_poison(mm, dev, dtype, D):
    layout = stack_layouts([layout_from_rows(r, 4, dev) for r in PER_HEAD[:2]], dev)
    lens = [65, 200, 256, 1]
    runs = [poisoned_case(mm, dev, dtype, D, S, S, layout, lens, lens, 29 + D, Hkv=1, causal=True) for _ in range(2)]
    got, (q, k, v, w), _ = runs[0]
    mask = length_mask(block_mask(layout, causal=True).expand(4, 2, S, S), lens, lens)
    check_rule(f"everything {dtype} D={D}", got, q, k, v, w, mask, G=2)
    assert_same_step(runs[1][0], got, "run to run")


# ---- 7. through the C ABI ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 32), (torch.float16, 96)])
def test_7_ex_entries_with_leading_dimensions_and_strides(mm, cmm, capi, dev, dtype, D):
    """G = 2 with lengths [B] against lead [B, 2]: each of the eight dense operands in a buffer of its own (operand number i:
    ld = D + 8(i + 1), stride = rows · ld + 8(i + 1)), NaN around the inputs and in their padding, a sentinel around the
    outputs; every logical output has the bits of the call through matmuls."""
    B, Sq, Sk = 2, 128, 192
    layout = stack_layouts([layout_from_rows(r, 3, dev) for r in ([[2, 0], [1, 2]], [[1, 0], [0, 2]])], dev)
    q_lens, k_lens = [100, 128], [192, 70]
    q, k, v, w = operands(dev, (B, 2), (B, 1), Sq, Sk, D, dtype, 31 + D)
    q, w = (fill_padding(t, q_lens, NAN) for t in (q, w))
    k, v = (fill_padding(t, k_lens, NAN) for t in (k, v))
    ql, kl = (torch.tensor(l, device=dev, dtype=torch.int32) for l in (q_lens, k_lens))
    want = step(mm, q, k, v, layout, w, q_lens=ql, k_lens=kl)
    rec = mm._block_layout(layout, dev, 1, mm._csr_state(layout))
    offsets, columns, nnz, L = rec["fwd"]
    t_off, t_col = mm._block_layout_transposed(rec, Sq // 64, Sk // 64)
    scale = 1.0 / D ** 0.5
    q3, k3, v3, w3 = q.reshape(-1, Sq, D), k.reshape(-1, Sk, D), v.reshape(-1, Sk, D), w.reshape(-1, Sq, D)
    nq, nk = q3.shape[0], k3.shape[0]
    pq, pk, pv, pw = padded(q3, 0, NAN), padded(k3, 1, NAN), padded(v3, 2, NAN), padded(w3, 4, NAN)
    pout = padded(torch.full_like(q3, SENTINEL), 3, SENTINEL)
    lse = torch.full((nq, Sq), NAN, device=dev)
    st = fwd_ex_through_the_c_abi(capi, dtype, offsets, columns, nnz, L, nq, Sq, Sk, D, 0, pq, pk, pv, scale, pout, lse, 2, ql, kl, B)
    assert st == 0
    torch.cuda.synchronize()
    assert_outside_untouched(pout, "out")
    pout_in = padded(pout.x.contiguous(), 3, NAN)
    outs = [padded(torch.full((n, rows, D), SENTINEL, device=dev, dtype=dtype), i, SENTINEL)
            for i, n, rows in ((5, nq, Sq), (6, nk, Sk), (7, nk, Sk))]
    st = bwd_ex_through_the_c_abi(capi, dtype, offsets, columns, t_off, t_col, nnz, L, nq, Sq, Sk, D, 0, pq, pk, pv, pout_in, pw, lse,
                                  scale, *outs, 2, ql, kl, B)
    assert st == 0
    torch.cuda.synchronize()
    for name, p in zip(("dq", "dk", "dv"), outs):
        assert_outside_untouched(p, name)
    for name, g, x in zip(NAMES, (pout.x,) + tuple(p.x for p in outs), want):
        assert_same_bits(g, x.reshape(g.shape), f"{dtype} D={D} through the C ABI: {name}")
        assert torch.isfinite(g.float()).all(), name
    assert (lse.reshape(B, 2, Sq)[0, :, 100:] == float("-inf")).all() and torch.isfinite(lse.reshape(B, 2, Sq)[0, :, :100]).all()
