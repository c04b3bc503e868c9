"""Block-sparse attention without a GPU: block_attention_takes is a rule of (dtype, D, block) alone, every refusal of
matmuls.block_sparse_attention is raised with its message before any device call, the C-ABI declares and exports the new
entries and they validate their arguments before any HIP call, custom_mm refuses host tensors, the 128 → 64 layout
expansion has the expected indices, and the autograd wiring (expanded and transposed lists, layout broadcast, what is
saved) is checked on CPU tensors against torch autograd of the dense masked attention in float64, with a float64 stand-in
for the kernels (tests/fake_custom_mm_block_attention.py)."""
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
ENTRIES = tuple(f"mi_block_attention_fwd_{s}" for s in SUFFIXES) + tuple(f"mi_block_attention_bwd_{s}" for s in SUFFIXES) + \
    ("mi_block_attention_workspace_bytes",)
OK, EINVAL, ERANGE, ENOMEM = 0, -1, -2, -4
FAKE = 0x1000  # a non-null, 16-byte aligned address that is never dereferenced: every call below returns before the device


@pytest.fixture(scope="module")
def lib(built):
    import torch  # noqa: F401  (torch's HIP runtime first, as in the product)
    lib = ctypes.CDLL(str(built / "libmi_spmm.so"))
    vp, i64, i32, f32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_size_t
    dense = [vp, i64, i64]
    for s in SUFFIXES:
        getattr(lib, f"mi_block_attention_fwd_{s}").argtypes = [vp, vp, i64] + 6 * [i32] + 3 * dense + [f32] + dense + [vp, vp]
        getattr(lib, f"mi_block_attention_bwd_{s}").argtypes = [vp, vp, vp, vp, i64] + 6 * [i32] + 5 * dense + [vp, f32] + \
            3 * dense + [vp, sz, vp]
    lib.mi_block_attention_workspace_bytes.argtypes = [i32, i32]
    lib.mi_block_attention_workspace_bytes.restype = sz
    return lib


def test_header_declares_the_entries():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", text), name


def test_library_exports_the_entries(lib):
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert lib.mi_block_attention_workspace_bytes(8, 2048) == 8 * 2048 * 4
    assert lib.mi_block_attention_workspace_bytes(0, 2048) == 0 and lib.mi_block_attention_workspace_bytes(8, 0) == 0


DEFAULTS = dict(rowptr=FAKE, col=FAKE, t_rowptr=FAKE, t_col=FAKE, nnz=4, layouts=1, batch=2, Sq=128, Sk=192, D=64, causal=0, q=FAKE,
                k=FAKE, v=FAKE, out=FAKE, dout=FAKE, lse=FAKE, dq=FAKE, dk=FAKE, dv=FAKE, ws=FAKE, ws_bytes=1 << 20, ld=None)


def fwd(lib, s, **kw):
    a = {**DEFAULTS, **kw}
    ld = a["D"] if a["ld"] is None else a["ld"]
    return getattr(lib, f"mi_block_attention_fwd_{s}")(
        a["rowptr"], a["col"], a["nnz"], a["layouts"], a["batch"], a["Sq"], a["Sk"], a["D"], a["causal"], a["q"], ld, a["Sq"] * ld,
        a["k"], ld, a["Sk"] * ld, a["v"], ld, a["Sk"] * ld, 1.0, a["out"], ld, a["Sq"] * ld, a["lse"], None)


def bwd(lib, s, **kw):
    a = {**DEFAULTS, **kw}
    ld = a["D"] if a["ld"] is None else a["ld"]
    return getattr(lib, f"mi_block_attention_bwd_{s}")(
        a["rowptr"], a["col"], a["t_rowptr"], a["t_col"], a["nnz"], a["layouts"], a["batch"], a["Sq"], a["Sk"], a["D"], a["causal"],
        a["q"], ld, a["Sq"] * ld, a["k"], ld, a["Sk"] * ld, a["v"], ld, a["Sk"] * ld, a["out"], ld, a["Sq"] * ld, a["dout"], ld,
        a["Sq"] * ld, a["lse"], 1.0, a["dq"], ld, a["Sq"] * ld, a["dk"], ld, a["Sk"] * ld, a["dv"], ld, a["Sk"] * ld, a["ws"],
        a["ws_bytes"], None)


@pytest.mark.parametrize("s", SUFFIXES)
def test_entries_validate_before_any_hip_call(lib, s):
    for call, ptrs in ((fwd, ("rowptr", "col", "q", "k", "v", "out", "lse")),
                       (bwd, ("rowptr", "col", "t_rowptr", "t_col", "q", "k", "v", "out", "dout", "lse", "dq", "dk", "dv", "ws"))):
        for kw in ({"nnz": -1}, {"layouts": -1}, {"batch": -1}, {"Sq": -64}, {"Sk": -64}, {"D": -32}):
            assert call(lib, s, **kw) == EINVAL, (call.__name__, kw)
        assert call(lib, s, nnz=2 ** 31) == ERANGE
        # head sizes: 32, 64, 96 and 128 pass on to the pointer checks, nothing else does
        for D in (0, 8, 16, 48, 80, 100, 160, 256):
            assert call(lib, s, D=D) == EINVAL, (call.__name__, D)
        for D in (32, 64, 96, 128):
            assert call(lib, s, D=D, q=None) == EINVAL and call(lib, s, D=D, batch=0, q=None) == OK, (call.__name__, D)
        for kw in ({"Sq": 100}, {"Sk": 200}, {"Sq": 32}, {"causal": 1}, {"layouts": 0}, {"Sk": 0}):  # (Sk = 0 with entries)
            assert call(lib, s, **kw) == EINVAL, (call.__name__, kw)
        assert call(lib, s, causal=1, Sk=128, q=None) == EINVAL  # square: on to the pointers
        for p in ptrs:
            assert call(lib, s, **{p: None}) == EINVAL, (call.__name__, p)
        # an empty problem: nothing is touched, no pointer is looked at
        nulls = {p: None for p in ptrs}
        for kw in ({"batch": 0}, {"Sq": 0}):
            assert call(lib, s, **kw) == OK, (call.__name__, kw)
            assert call(lib, s, **kw, **nulls) == OK, (call.__name__, kw)
        assert call(lib, s, ld=32) == EINVAL  # rows shorter than D
        assert call(lib, s, ld=68) == EINVAL  # rows that do not start on 16 bytes
        for p in ptrs:
            if p not in ("rowptr", "col", "t_rowptr", "t_col", "lse"):
                assert call(lib, s, **{p: FAKE + 8}) == EINVAL, (call.__name__, p)
    assert bwd(lib, s, ws_bytes=2 * 128 * 4 - 1) == ENOMEM


def _host_args(dtype=torch.bfloat16):
    offs = torch.tensor([[0, 1]], dtype=torch.int32)
    col = torch.tensor([0], dtype=torch.int32)
    x = torch.rand(1, 64, 32).to(dtype)
    return offs, col, x, torch.empty(1, 64)


def test_custom_mm_refuses_host_tensors(built):
    import custom_mm
    for dtype in (torch.bfloat16, torch.float16):
        offs, col, x, lse = _host_args(dtype)
        with pytest.raises(RuntimeError, match="device"):
            custom_mm.block_attention_forward(offs, col, 1, x, x, x, 1.0, False, torch.empty_like(x), lse)
        with pytest.raises(RuntimeError, match="device"):
            custom_mm.block_attention_backward(offs, col, offs, col, 1, x, x, x, x, x, lse, 1.0, False, torch.empty_like(x),
                                               torch.empty_like(x), torch.empty_like(x))


def test_custom_mm_names_both_dtypes_of_mixed_operands(built):
    import custom_mm
    offs, col, x, lse = _host_args()
    both = r"(?s)(?=.*\bBFloat16\b)(?=.*\bHalf\b)"  # checked before the device, so host tensors show it
    with pytest.raises(RuntimeError, match=both):
        custom_mm.block_attention_forward(offs, col, 1, x, x, x.half(), 1.0, False, torch.empty_like(x), lse)
    with pytest.raises(RuntimeError, match=both):
        custom_mm.block_attention_backward(offs, col, offs, col, 1, x, x, x, x, x, lse, 1.0, False, torch.empty_like(x),
                                           torch.empty_like(x), torch.empty_like(x).half())
    with pytest.raises(TypeError):  # positional only
        custom_mm.block_attention_forward(offsets=offs, columns=col, nnz=1, q=x, k=x, v=x, scale=1.0, causal=False,
                                          out=torch.empty_like(x), lse=lse)


@pytest.fixture()
def real(built):
    """matmuls on the real extension, imported afresh."""
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import matmuls
    yield matmuls
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)


def test_block_attention_takes_is_a_rule_of_dtype_head_size_and_block(real):
    for D in range(0, 300):
        for block in (0, 1, 32, 63, 64, 65, 96, 128, 192, 200, 256, -64):
            want = D in (32, 64, 96, 128) and block > 0 and block % 64 == 0
            for dt in (torch.bfloat16, torch.float16):
                assert real.block_attention_takes(dt, D, block) == want, (dt, D, block)
            assert not real.block_attention_takes(torch.float32, D, block)
            assert not real.block_attention_takes(torch.float64, D, block)
    assert not real.block_attention_takes(torch.bfloat16, 64, 64.0)


def _layout(rows, cols, lead=()):
    return torch.ones(lead + (rows, cols)).to_sparse_csr()


def test_every_refusal_comes_before_the_device(real):
    f = real.block_sparse_attention
    x = torch.rand(2, 128, 64).bfloat16()
    lay = _layout(2, 2)
    sizes = r"32, 64, 96, 128.*multiple of 64"  # every size refusal names the accepted sizes
    with pytest.raises(ValueError, match="block_sparse_attention.*CSR"):
        f(x, x, x, lay.to_dense())
    with pytest.raises(ValueError, match="block_sparse_attention: k must be a dense tensor"):
        f(x, lay, x, lay)
    with pytest.raises(ValueError, match=r"block_sparse_attention: q must be bfloat16 or float16, got torch.float32.*" + sizes):
        f(x.float(), x.float(), x.float(), lay)
    with pytest.raises(ValueError, match="block_sparse_attention: v must be bfloat16 or float16, got torch.float64"):
        f(x, x, x.double(), lay)
    with pytest.raises(RuntimeError, match=r"block_sparse_attention: q is torch.bfloat16 but v is torch.float16.*one dtype"):
        f(x, x, x.half(), lay)
    for block in (32, 100, 0, -64, 64.0, True):
        with pytest.raises(ValueError, match="block_sparse_attention: block must be a positive multiple of 64.*" + sizes):
            f(x, x, x, lay, block=block)
    for D in (16, 48, 80, 256):
        y = torch.rand(2, 128, D).bfloat16()
        with pytest.raises(ValueError, match=rf"block_sparse_attention: head size D must be 32, 64, 96 or 128, got {D}.*" + sizes):
            f(y, y, y, lay)
    with pytest.raises(ValueError, match="block_sparse_attention.*one rank"):
        f(x, x[0], x[0], lay)
    with pytest.raises(ValueError, match="block_sparse_attention: q of shape.*needs k"):
        f(x, torch.rand(3, 128, 64).bfloat16(), x, lay)
    with pytest.raises(ValueError, match="block_sparse_attention: v must be a dense tensor with k's shape"):
        f(x, x, torch.rand(2, 192, 64).bfloat16(), lay)
    r = torch.rand(2, 100, 64).bfloat16()
    with pytest.raises(ValueError, match="block_sparse_attention: Sq = 100 and Sk = 128.*ragged.*" + sizes):
        f(r, x, x, lay)
    with pytest.raises(ValueError, match="block_sparse_attention: Sq = 128 and Sk = 128 must be multiples of block = 256"):
        f(x, x, x, lay, block=256)
    with pytest.raises(ValueError, match=r"block_sparse_attention: the layout must have shape.*\[\*l_lead, 2, 2\]"):
        f(x, x, x, _layout(2, 3))
    with pytest.raises(ValueError, match="block_sparse_attention: the layout must have shape"):
        f(x, x, x, _layout(2, 2, lead=(3,)))  # not a trailing part of lead = (2,)
    with pytest.raises(ValueError, match="block_sparse_attention: the layout must have shape"):
        f(x, x, x, lay, block=128)  # a 1 × 1 layout is wanted
    k = torch.rand(2, 192, 64).bfloat16()
    with pytest.raises(ValueError, match="block_sparse_attention: causal=True needs Sq == Sk, got 128 and 192"):
        f(x, k, k, _layout(2, 3), causal=True)
    # host tensors: the last check, and still before any device call
    for args in ((x, x, x, lay), (x.half(), k.half(), k.half(), _layout(2, 3)), (x, x, x, _layout(2, 2, lead=(2,))),
                 (x, x, x, _layout(1, 1), 128)):
        with pytest.raises(RuntimeError, match="block_sparse_attention.*device"):
            f(*args)


def test_expansion_of_a_2_by_3_layout_from_128_to_64():
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import fake_custom_mm_block_attention as fake
    sys.modules["custom_mm"] = fake
    try:
        matmuls = importlib.import_module("matmuls")
        # block row 0 keeps columns 2, 0 (in this order), block row 1 keeps column 1
        crow, col = torch.tensor([[0, 2, 3]]), torch.tensor([[2, 0, 1]])
        ncrow, ncol = matmuls._expand_block_layout(crow, col, 2)
        assert ncrow.tolist() == [[0, 4, 8, 10, 12]]
        assert ncol.tolist() == [[4, 5, 0, 1, 4, 5, 0, 1, 2, 3, 2, 3]]
        dense = torch.zeros(4, 6)
        for r in range(4):
            dense[r, ncol[0, ncrow[0, r]:ncrow[0, r + 1]]] = 1
        want = torch.tensor([[1., 0., 1.], [0., 1., 0.]]).repeat_interleave(2, 0).repeat_interleave(2, 1)
        assert torch.equal(dense, want)
        # two layouts at once, one with an empty row, int32 indices, a factor of 3; and f = 1 changes nothing
        crow2, col2 = torch.tensor([[0, 0, 2], [0, 1, 2]], dtype=torch.int32), torch.tensor([[1, 0], [0, 1]], dtype=torch.int32)
        c3, k3 = matmuls._expand_block_layout(crow2, col2, 3)
        assert c3.tolist() == [[0, 0, 0, 0, 6, 12, 18], [0, 3, 6, 9, 12, 15, 18]]
        assert k3.tolist() == [[3, 4, 5, 0, 1, 2] * 3, [0, 1, 2] * 3 + [3, 4, 5] * 3]
        c1, k1 = matmuls._expand_block_layout(crow2, col2, 1)
        assert c1.tolist() == crow2.tolist() and k1.tolist() == col2.tolist()
    finally:
        for k in ("custom_mm", "matmuls"):
            sys.modules.pop(k, None)


# ---- autograd wiring on CPU tensors, float64 stand-in arithmetic on float16 storage -------------------------------

@pytest.fixture()
def mm(oracle_mod):
    """(matmuls bound to the float64 stand-in, the stand-in)."""
    import fake_custom_mm_block_attention as fake
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
    """A CSR block layout [*lead, rows, cols] with exactly `keep` blocks per block row, columns in a shuffled order."""
    nb = 1
    for n in lead:
        nb *= n
    col = torch.stack([torch.randperm(cols, generator=g)[:keep] for _ in range(nb * rows)]).reshape(lead + (rows * keep,))
    crow = (torch.arange(rows + 1) * keep).expand(lead + (rows + 1,)).contiguous()
    return torch.sparse_csr_tensor(crow, col, torch.ones(col.shape), size=lead + (rows, cols))


def _dense_mask(layout, block, lead, causal):
    """Boolean [*lead, Sq, Sk]: the layout expanded by `block`, broadcast over lead, and-ed with the lower triangle."""
    m = torch.sparse_csr_tensor(layout.crow_indices(), layout.col_indices(), torch.ones_like(layout.values()),
                                size=layout.shape).to_dense() != 0
    m = m.repeat_interleave(block, -2).repeat_interleave(block, -1)
    m = m.expand(lead + tuple(m.shape[-2:])).clone()
    if causal:
        m &= torch.ones(m.shape[-2:], dtype=torch.bool).tril()
    return m


def _reference(q, k, v, mask, scale, w):
    rq, rk, rv = (x.detach().double().requires_grad_(True) for x in (q, k, v))
    s = scale * (rq @ rk.transpose(-1, -2))
    empty = ~mask.any(-1, keepdim=True)
    p = torch.softmax(s.masked_fill(~mask & ~empty, -float("inf")), -1)
    p = torch.where(empty, torch.zeros_like(p), p)
    out = p @ rv
    return (out.detach(),) + torch.autograd.grad(out, (rq, rk, rv), grad_outputs=w.double())


@pytest.mark.parametrize("lead,l_lead,Sq,Sk,block,causal,scale", [
    ((), (), 128, 192, 64, False, None),
    ((2, 3), (3,), 128, 128, 64, True, 0.3),
    ((2, 2), (2, 2), 256, 256, 128, False, None),
    ((3,), (), 256, 256, 128, True, None),
])
def test_block_sparse_attention_matches_dense_masked_autograd(mm, lead, l_lead, Sq, Sk, block, causal, scale):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(23)
    D = 32
    rows, cols = Sq // block, Sk // block
    layout = _block_layout(g, l_lead, rows, cols, keep=max(1, cols - 1))
    mask = _dense_mask(layout, block, lead, causal)
    q = torch.randn(lead + (Sq, D), generator=g).half().requires_grad_(True)
    k, v = (torch.randn(lead + (Sk, D), generator=g).half().requires_grad_(True) for _ in range(2))
    out = matmuls.block_sparse_attention(q, k, v, layout, block=block, scale=scale, causal=causal)
    w = torch.randn(out.shape, generator=g).half()
    ref = _reference(q, k, v, mask, 1.0 / D ** 0.5 if scale is None else scale, w)
    out.backward(w)
    for name, got, want in (("out", out.detach(), ref[0]), ("dq", q.grad, ref[1]), ("dk", k.grad, ref[2]), ("dv", v.grad, ref[3])):
        assert got.dtype == torch.float16 and got.shape == want.shape
        assert torch.allclose(got.double(), want, rtol=4e-3, atol=4e-3), (name, float((got.double() - want).abs().max()))
    names = [c[0] for c in fake.calls]
    assert names.count("block_attention_forward") == 1 and names.count("block_attention_backward") == 1
    f = block // 64
    n_layouts = 1
    for n in l_lead:
        n_layouts *= n
    fwd_call = [c for c in fake.calls if c[0] == "block_attention_forward"][0][1]
    assert fwd_call[2] == n_layouts and fwd_call[3] == layout.values().numel() * f * f
    # a second step on the same layout tensor expands and transposes nothing again
    before = len([c for c in fake.calls if c[0].startswith("csr_transpose")])
    assert before == 1
    out2 = matmuls.block_sparse_attention(q, k, v, layout, block=block, scale=scale, causal=causal)
    out2.backward(w)
    assert len([c for c in fake.calls if c[0].startswith("csr_transpose")]) == before
    assert torch.equal(out2.detach(), out.detach())


def test_saved_for_backward_is_the_operands_out_and_one_float_per_query_row(mm):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(29)
    layout = _block_layout(g, (), 2, 3, keep=2)
    q = torch.randn(2, 128, 32, generator=g).half().requires_grad_(True)
    k, v = (torch.randn(2, 192, 32, generator=g).half().requires_grad_(True) for _ in range(2))
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
        matmuls.block_sparse_attention(q, k, v, layout)
    dense = [t for t in saved if t.layout == torch.strided]
    own = {t.data_ptr() for t in (q, k, v)}
    extra = sorted((t for t in dense if t.data_ptr() not in own), key=lambda t: t.numel())
    assert [(tuple(t.shape), t.dtype) for t in extra] == [((2, 128), torch.float32), ((2, 128, 32), torch.float16)]
