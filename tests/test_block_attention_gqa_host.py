"""Grouped-query heads and per-item lengths of matmuls.block_sparse_attention without a GPU: every new
refusal with its exception type and text, the old refusals still first for old inputs, the routing (equal leads without
lengths reach the OLD binding, anything else the _ex one — tests/fake_custom_mm_block_attention_gqa.py records which),
the lengths handed over as contiguous int32 of one count, the autograd wiring against torch autograd of dense masked
attention in float64 on repeated k / v, what autograd saves, and the _ex entries of the C ABI: declared, exported, and
MI_EINVAL for every invalid group / lengths combination before any HIP call."""
import ctypes
import importlib
import re
import sys
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "mi_spmm.h"
SUFFIXES = ("bf16", "f16")
ENTRIES = tuple(f"mi_block_attention_{d}_ex_{s}" for d in ("fwd", "bwd") for s in SUFFIXES)
OK, EINVAL = 0, -1
FAKE = 0x1000  # a non-null, 16-byte aligned address that is never dereferenced: every call below returns before the device


# ---- the C ABI -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(built):
    import torch  # noqa: F401  (torch's HIP runtime first, as in the product)
    lib = ctypes.CDLL(str(built / "libmi_spmm.so"))
    vp, i64, i32, f32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_size_t
    dense, ex = [vp, i64, i64], [i32, vp, vp, i32, vp]
    for s in SUFFIXES:
        getattr(lib, f"mi_block_attention_fwd_ex_{s}").argtypes = [vp, vp, i64] + 6 * [i32] + 3 * dense + [f32] + dense + [vp] + ex
        getattr(lib, f"mi_block_attention_bwd_ex_{s}").argtypes = [vp, vp, vp, vp, i64] + 6 * [i32] + 5 * dense + [vp, f32] + \
            3 * dense + [vp, sz] + ex
    return lib


def test_header_declares_and_library_exports_the_ex_entries(lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(lib, name), name


DEFAULTS = dict(nnz=4, layouts=1, batch=8, Sq=128, Sk=192, D=64, q=FAKE, group=1, q_lens=None, k_lens=None, lens_count=0)


def fwd(lib, s, **kw):
    a = {**DEFAULTS, **kw}
    ld = a["D"]
    return getattr(lib, f"mi_block_attention_fwd_ex_{s}")(
        FAKE, FAKE, a["nnz"], a["layouts"], a["batch"], a["Sq"], a["Sk"], a["D"], 0, a["q"], ld, a["Sq"] * ld, FAKE, ld, a["Sk"] * ld,
        FAKE, ld, a["Sk"] * ld, 1.0, FAKE, ld, a["Sq"] * ld, FAKE, a["group"], a["q_lens"], a["k_lens"], a["lens_count"], None)


def bwd(lib, s, **kw):
    a = {**DEFAULTS, **kw}
    ld = a["D"]
    return getattr(lib, f"mi_block_attention_bwd_ex_{s}")(
        FAKE, FAKE, FAKE, FAKE, a["nnz"], a["layouts"], a["batch"], a["Sq"], a["Sk"], a["D"], 0, a["q"], ld, a["Sq"] * ld, FAKE, ld,
        a["Sk"] * ld, FAKE, ld, a["Sk"] * ld, FAKE, ld, a["Sq"] * ld, FAKE, ld, a["Sq"] * ld, FAKE, 1.0, FAKE, ld, a["Sq"] * ld, FAKE,
        ld, a["Sk"] * ld, FAKE, ld, a["Sk"] * ld, FAKE, 1 << 20, a["group"], a["q_lens"], a["k_lens"], a["lens_count"], None)


@pytest.mark.parametrize("s", SUFFIXES)
def test_ex_entries_validate_group_and_lengths_before_any_hip_call(lib, s):
    """Each invalid combination alone gives MI_EINVAL; the same call made valid goes on to the pointer checks (q = NULL:
    MI_EINVAL too, so a valid combination is told apart by the empty problem, batch = 0 → MI_OK, and by what follows)."""
    for call in (fwd, bwd):
        for kw in ({"group": 0}, {"group": -1}, {"group": 3},                                   # batch % group
                   {"q_lens": FAKE, "lens_count": 0}, {"k_lens": FAKE, "lens_count": -2},       # a lens pointer without a count
                   {"q_lens": FAKE, "lens_count": 3}, {"k_lens": FAKE, "lens_count": 16},       # batch % lens_count
                   {"q_lens": FAKE, "lens_count": 4, "group": 4},                               # (batch / lens_count) % group
                   {"k_lens": FAKE, "lens_count": 8, "group": 2},
                   {"q_lens": FAKE + 2, "lens_count": 2}, {"q_lens": FAKE, "k_lens": FAKE + 1, "lens_count": 2}):  # misaligned
            assert call(lib, s, **kw) == EINVAL, (call.__name__, kw)
        # group < 1 is refused even for an empty problem; everything else about an empty problem is not looked at
        assert call(lib, s, batch=0, group=0) == EINVAL
        assert call(lib, s, batch=0, group=4, q_lens=FAKE + 2, lens_count=0) == OK
        # the plain entries' refusals hold for the _ex ones
        for kw in ({"nnz": -1}, {"D": 48}, {"Sq": 100}, {"layouts": 0}, {"q": None}):
            assert call(lib, s, **kw, group=2, q_lens=FAKE, lens_count=2) == EINVAL, (call.__name__, kw)
        # a lens_count without pointers is ignored: the plain call
        assert call(lib, s, lens_count=3, q=None) == EINVAL and call(lib, s, lens_count=3, batch=0) == OK


# ---- matmuls on the real extension: refusals before the device ---------------------------------------------------

@pytest.fixture()
def real(built):
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import matmuls
    yield matmuls
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)


def _layout(rows, cols, lead=()):
    return torch.ones(lead + (rows, cols)).to_sparse_csr()


def test_every_new_refusal_comes_before_the_device(real):
    f = real.block_sparse_attention
    q = torch.rand(2, 4, 128, 64).bfloat16()
    k2, k1, lay = torch.rand(2, 2, 128, 64).bfloat16(), torch.rand(2, 1, 128, 64).bfloat16(), _layout(2, 2)
    grouped = r"block_sparse_attention: q of shape \(2, 4, 128, 64\) needs k \(2, 4, 'Sk', 64\) or, grouped, " \
              r"\(2, 'Hkv', 'Sk', 64\) with Hkv a divisor of 4, got "
    with pytest.raises(ValueError, match=grouped + r"\(2, 3, 128, 64\)"):      # Hq not divisible by Hkv
        f(q, *(torch.rand(2, 3, 128, 64).bfloat16(),) * 2, lay)
    with pytest.raises(ValueError, match=grouped + r"\(1, 2, 128, 64\)"):      # k's lead differs before the last dimension
        f(q, *(torch.rand(1, 2, 128, 64).bfloat16(),) * 2, lay)
    with pytest.raises(ValueError, match=grouped + r"\(2, 0, 128, 64\)"):
        f(q, *(torch.rand(2, 0, 128, 64).bfloat16(),) * 2, lay)
    with pytest.raises(ValueError, match=grouped + r"\(2, 8, 128, 64\)"):      # more k / v heads than query heads
        f(q, *(torch.rand(2, 8, 128, 64).bfloat16(),) * 2, lay)
    with pytest.raises(ValueError, match="block_sparse_attention: v must be a dense tensor with k's shape"):
        f(q, k2, k1, lay)
    # lengths: shape, dtype, layout
    lens = r"block_sparse_attention: {} must have a shape that is a leading part of {}.*got {}"
    for name in ("q_lens", "k_lens"):
        for bad, common, k in ((torch.tensor([128, 128, 128]), (2, 4), q), (torch.ones(4, dtype=torch.int64), (2, 4), q),
                               (torch.ones(2, 4, 1, dtype=torch.int32), (2, 4), q),
                               (torch.ones(2, 4, dtype=torch.int32), (2,), k2), (torch.ones(2, 2, dtype=torch.int32), (2,), k2)):
            with pytest.raises(ValueError, match=lens.format(name, re.escape(str(common)), re.escape(str(tuple(bad.shape))))):
                f(q, k, k, lay, **{name: bad})
        for bad in (torch.tensor([128.0, 64.0]), torch.tensor([True, False]), torch.tensor([1, 2], dtype=torch.int16)):
            with pytest.raises(ValueError, match=rf"block_sparse_attention: {name} must be an int32 or int64 tensor, got {bad.dtype}"):
                f(q, k2, k2, lay, **{name: bad})
        for bad in ([128, 64], 128, torch.ones(2, 2).to_sparse_csr()):
            with pytest.raises(ValueError, match=f"block_sparse_attention: {name} must be a dense tensor or None"):
                f(q, k2, k2, lay, **{name: bad})
    with pytest.raises(TypeError):  # keyword only
        f(q, k2, k2, lay, 64, None, False, torch.tensor([128, 64]))
    # host tensors: the last check, RuntimeError, and it names the lengths among the operands
    with pytest.raises(RuntimeError, match=r"block_sparse_attention: layout, q, k, v, q_lens, k_lens must be device \(HIP\) tensors"):
        f(q, k2, k2, lay, q_lens=torch.tensor([128, 64]), k_lens=torch.tensor([[1, 2, 3, 4]] * 2)[:, 0])
    with pytest.raises(RuntimeError, match=r"block_sparse_attention: layout, q, k, v must be device \(HIP\) tensors"):
        f(q, k1, k1, lay)


def test_old_refusals_stay_first_and_unchanged(real):
    """An old refusal wins over a new one made in the same call, with its old text."""
    f = real.block_sparse_attention
    x = torch.rand(2, 128, 64).bfloat16()
    lay, bad = _layout(2, 2), torch.tensor([1.5])
    with pytest.raises(ValueError, match="block_sparse_attention.*CSR"):
        f(x, x, x, lay.to_dense(), q_lens=bad)
    with pytest.raises(ValueError, match=r"block_sparse_attention: q must be bfloat16 or float16, got torch.float32"):
        f(x.float(), x.float(), x.float(), lay, q_lens=bad)
    with pytest.raises(ValueError, match="block_sparse_attention: block must be a positive multiple of 64"):
        f(x, x, x, lay, block=32, k_lens=bad)
    with pytest.raises(ValueError, match="block_sparse_attention: q of shape.*needs k"):
        f(x, torch.rand(3, 128, 64).bfloat16(), x, lay)
    r = torch.rand(2, 100, 64).bfloat16()
    with pytest.raises(ValueError, match="block_sparse_attention: Sq = 100 and Sk = 128.*ragged lengths are not supported"):
        f(r, x, x, lay, q_lens=torch.tensor([100, 100]))
    with pytest.raises(ValueError, match=r"block_sparse_attention: the layout must have shape.*\[\*l_lead, 2, 2\]"):
        f(x, x, x, _layout(2, 3), q_lens=bad)
    k = torch.rand(2, 192, 64).bfloat16()
    with pytest.raises(ValueError, match="block_sparse_attention: causal=True needs Sq == Sk, got 128 and 192"):
        f(x, k, k, _layout(2, 3), causal=True, q_lens=bad)
    with pytest.raises(RuntimeError, match=r"block_sparse_attention: layout, q, k, v must be device \(HIP\) tensors"):
        f(x, x, x, lay)
    g = torch.rand(4, 128, 64).bfloat16()  # 2-d lead (4,) against (2,): grouped, and the layout is indexed by the query item
    with pytest.raises(ValueError, match="block_sparse_attention: the layout must have shape"):
        f(g, x, x, _layout(2, 2, lead=(2,)))


def test_custom_mm_ex_bindings_refuse_host_tensors_and_keywords(built):
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import custom_mm
    offs, col = torch.tensor([[0, 1]], dtype=torch.int32), torch.tensor([0], dtype=torch.int32)
    x, kv, lse = torch.rand(2, 64, 32).bfloat16(), torch.rand(1, 64, 32).bfloat16(), torch.empty(2, 64)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.block_attention_forward_ex(offs, col, 1, x, kv, kv, 1.0, False, torch.empty_like(x), lse, None, None)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.block_attention_backward_ex(offs, col, offs, col, 1, x, kv, kv, x, x, lse, 1.0, False, torch.empty_like(x),
                                              torch.empty_like(kv), torch.empty_like(kv), None, None)
    both = r"(?s)(?=.*\bBFloat16\b)(?=.*\bHalf\b)"
    with pytest.raises(RuntimeError, match=both):
        custom_mm.block_attention_forward_ex(offs, col, 1, x, kv, kv.half(), 1.0, False, torch.empty_like(x), lse, None, None)
    with pytest.raises(TypeError):  # positional only
        custom_mm.block_attention_forward_ex(offs, col, 1, x, kv, kv, 1.0, False, torch.empty_like(x), lse, q_lens=None, k_lens=None)


# ---- routing and wiring on CPU tensors, float64 stand-in arithmetic on float16 storage -----------------------------

@pytest.fixture()
def mm(oracle_mod):
    """(matmuls bound to the float64 stand-in, the stand-in)."""
    import fake_custom_mm_block_attention_gqa as fake
    saved = {k: sys.modules.get(k) for k in ("custom_mm", "matmuls")}
    sys.modules["custom_mm"] = fake
    sys.modules.pop("matmuls", None)
    matmuls = importlib.import_module("matmuls")
    fake.calls.clear()
    yield matmuls, fake
    for k, v in saved.items():
        if v is None:
            sys.modules.pop(k, None)
        else:
            sys.modules[k] = v


def _block_layout(g, lead, rows, cols, keep):
    nb = 1
    for n in lead:
        nb *= n
    col = torch.stack([torch.randperm(cols, generator=g)[:keep] for _ in range(nb * rows)]).reshape(lead + (rows * keep,))
    crow = (torch.arange(rows + 1) * keep).expand(lead + (rows + 1,)).contiguous()
    return torch.sparse_csr_tensor(crow, col, torch.ones(col.shape), size=lead + (rows, cols))


def _dense_mask(layout, lead, causal, q_lens, k_lens):
    """Boolean [*lead, Sq, Sk]: 64-blocks of the layout, the lower triangle when causal, and the positions that exist
    (lens [B] or None against lead (B, H))."""
    m = torch.sparse_csr_tensor(layout.crow_indices(), layout.col_indices(), torch.ones_like(layout.values()),
                                size=layout.shape).to_dense() != 0
    m = m.repeat_interleave(64, -2).repeat_interleave(64, -1)
    m = m.expand(lead + tuple(m.shape[-2:])).clone()
    if causal:
        m &= torch.ones(m.shape[-2:], dtype=torch.bool).tril()
    Sq, Sk = m.shape[-2:]
    if q_lens is not None:
        m &= (torch.arange(Sq)[None, :] < q_lens[:, None])[:, None, :, None]
    if k_lens is not None:
        m &= (torch.arange(Sk)[None, :] < k_lens[:, None])[:, None, None, :]
    return m


def _reference(q, k, v, mask, scale, w, G):
    """torch autograd of dense masked attention in float64 on k, v repeated G times: the group's sum comes from autograd."""
    rq, rk, rv = (x.detach().double().requires_grad_(True) for x in (q, k, v))
    ek, ev = rk.repeat_interleave(G, -3), rv.repeat_interleave(G, -3)
    s = scale * (rq @ ek.transpose(-1, -2))
    empty = ~mask.any(-1, keepdim=True)
    p = torch.softmax(s.masked_fill(~mask & ~empty, -float("inf")), -1)
    p = torch.where(empty, torch.zeros_like(p), p)
    out = p @ ev
    return (out.detach(),) + torch.autograd.grad(out, (rq, rk, rv), grad_outputs=w.double())


def _poison(x, lens):
    """NaN in every row of x [B, H, S, D] at or beyond the item's length."""
    x = x.clone()
    for b, n in enumerate(lens.tolist()):
        x[b, :, max(n, 0):] = float("nan")
    return x


@pytest.mark.parametrize("G,l_lead,causal,q_lens,k_lens", [
    (2, (), False, None, None),
    (4, (4,), True, None, None),
    (1, (2, 4), False, [200, 65], [63, 256]),
    (2, (4,), True, [129, 256], [129, 300]),        # (300: clamped to Sk)
    (4, (), False, None, [1, 128]),
])
def test_grouped_and_lengths_match_dense_masked_autograd(mm, G, l_lead, causal, q_lens, k_lens):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(37 + G)
    B, H, S, D = 2, 4, 256, 32
    lead = (B, H)
    layout = _block_layout(g, l_lead, 4, 4, keep=3)
    ql = None if q_lens is None else torch.tensor(q_lens, dtype=torch.int64)
    kl = None if k_lens is None else torch.tensor(k_lens, dtype=torch.int32)
    full = torch.full((B,), S)
    mask = _dense_mask(layout, lead, causal, ql, None if kl is None else kl.clamp(max=S))
    q = torch.randn(B, H, S, D, generator=g).half()
    k, v = (torch.randn(B, H // G, S, D, generator=g).half() for _ in range(2))
    w = torch.randn(B, H, S, D, generator=g).half()
    ref = _reference(q, k, v, mask, 1.0 / D ** 0.5, w, G)
    # the padding is poisoned for the call: nothing of it may arrive
    qp, wp = (_poison(t, full if ql is None else ql) for t in (q, w))
    kp, vp = (_poison(t, full if kl is None else kl) for t in (k, v))
    qp, kp, vp = (t.requires_grad_(True) for t in (qp, kp, vp))
    out = matmuls.block_sparse_attention(qp, kp, vp, layout, causal=causal, q_lens=ql, k_lens=kl)
    out.backward(wp)
    for name, got, want in (("out", out.detach(), ref[0]), ("dq", qp.grad, ref[1]), ("dk", kp.grad, ref[2]), ("dv", vp.grad, ref[3])):
        assert got.dtype == torch.float16 and got.shape == want.shape, name
        assert torch.isfinite(got).all(), name
        assert torch.allclose(got.double(), want, rtol=4e-3, atol=4e-3), (name, float((got.double() - want).abs().max()))
    assert [c[0] for c in fake.calls if c[0].startswith("block_attention")] == ["block_attention_forward_ex", "block_attention_backward_ex"]
    for _, (qs, ks, L, nnz, c, group, hq, hk) in (c for c in fake.calls if c[0].startswith("block_attention")):
        assert qs == (B * H, S, D) and ks == (B * H // G, S, D) and group == G and c == causal
        for lens, handed in ((q_lens, hq), (k_lens, hk)):
            if q_lens is None and k_lens is None:
                assert handed is None
            elif lens is not None:  # [B] handed over as it is: contiguous int32, one entry per batch item, values untouched
                assert handed.dtype == torch.int32 and handed.is_contiguous() and handed.tolist() == lens


def test_equal_leads_without_lengths_reach_the_old_binding(mm):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(41)
    layout = _block_layout(g, (), 2, 2, keep=2)
    q, k, v = (torch.randn(2, 2, 128, 32, generator=g).half().requires_grad_(True) for _ in range(3))
    matmuls.block_sparse_attention(q, k, v, layout).sum().backward()
    assert [c[0] for c in fake.calls if c[0].startswith("block_attention")] == ["block_attention_forward", "block_attention_backward"]
    fake.calls.clear()
    matmuls.block_sparse_attention(q, k, v, layout, q_lens=None, k_lens=None)
    assert [c[0] for c in fake.calls if c[0].startswith("block_attention")] == ["block_attention_forward"]
    fake.calls.clear()
    matmuls.block_sparse_attention(q, k[:, :1], v[:, :1], layout)  # grouped
    matmuls.block_sparse_attention(q, k, v, layout, k_lens=torch.tensor([128, 128]))  # lengths, even if they change nothing
    assert [c[0] for c in fake.calls if c[0].startswith("block_attention")] == ["block_attention_forward_ex"] * 2


def test_lengths_are_handed_over_as_contiguous_int32_of_one_count(mm):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(43)
    layout = _block_layout(g, (), 2, 2, keep=2)
    q, k, v = (torch.randn(2, 3, 128, 32, generator=g).half() for _ in range(3))

    def handed(**kw):
        fake.calls.clear()
        matmuls.block_sparse_attention(q, k, v, layout, **kw)
        (name, args), = [c for c in fake.calls if c[0].startswith("block_attention")]
        assert name == "block_attention_forward_ex"
        for t in args[-2:]:
            assert t is None or (t.dtype == torch.int32 and t.is_contiguous() and t.dim() == 1)
        return [None if t is None else t.tolist() for t in args[-2:]]

    assert handed(q_lens=torch.tensor([100, 7], dtype=torch.int64)) == [[100, 7], None]            # int64, [B] against [B, H]
    assert handed(k_lens=torch.tensor([5, 128], dtype=torch.int32)) == [None, [5, 128]]
    per_head = torch.tensor([[1, 2, 3], [4, 5, 6]])
    assert handed(q_lens=per_head) == [[1, 2, 3, 4, 5, 6], None]                                    # the whole lead
    assert handed(q_lens=per_head.t().contiguous().t(), k_lens=torch.tensor([9, -3])) == \
        [[1, 2, 3, 4, 5, 6], [9, 9, 9, -3, -3, -3]]                  # a strided view; [B] beside [B, H]: one count, values as given
    assert handed(q_lens=torch.tensor(77)) == [[77], None]                                         # one length for all
    big = torch.tensor([2 ** 31 - 1, -2 ** 31])
    assert handed(k_lens=big) == [None, big.tolist()]
    # grouped: the lengths stop before the head dimension
    fake.calls.clear()
    matmuls.block_sparse_attention(q, k[:, :1], v[:, :1], layout, q_lens=torch.tensor([64, 128]))
    (name, args), = fake.calls[-1:]
    assert name == "block_attention_forward_ex" and args[5] == 3 and args[6].tolist() == [64, 128]


def test_saved_for_backward_adds_only_the_two_length_tensors(mm):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(47)
    layout = _block_layout(g, (), 2, 3, keep=2)
    q = torch.randn(2, 4, 128, 32, generator=g).half().requires_grad_(True)
    k, v = (torch.randn(2, 2, 192, 32, generator=g).half().requires_grad_(True) for _ in range(2))
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
        matmuls.block_sparse_attention(q, k, v, layout, q_lens=torch.tensor([100, 128]), k_lens=torch.tensor([192, 3]))
    dense = [t for t in saved if t.layout == torch.strided]
    own = {t.data_ptr() for t in (q, k, v)}
    extra = sorted((t for t in dense if t.data_ptr() not in own), key=lambda t: t.numel())
    assert [(tuple(t.shape), t.dtype) for t in extra] == [((2,), torch.int32), ((2,), torch.int32), ((8, 128), torch.float32),
                                                          ((8, 128, 32), torch.float16)]
