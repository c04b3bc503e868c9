"""Fused sparse attention without a GPU: the C-ABI declares and exports the seven entries, they validate their arguments
before any HIP call, custom_mm refuses host tensors and mixed dtypes, fused_attention_takes is a rule of (dtype, D) alone,
and the autograd wiring of matmuls.fused_sparse_attention is checked on CPU tensors against torch autograd of the dense
masked attention in float64, with a float64 stand-in for the kernels (tests/fake_custom_mm_fused_attention.py)."""
import ctypes
import importlib
import re
import sys
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "mi_spmm.h"
SUFFIXES = ("f32", "bf16", "f16")
ENTRIES = tuple(f"mi_sparse_attention_{s}" for s in SUFFIXES) + tuple(f"mi_sparse_attention_backward_{s}" for s in SUFFIXES) + \
    ("mi_sparse_attention_workspace_bytes",)
OK, EINVAL, ERANGE = 0, -1, -2
FAKE = 0x1000  # a non-null, 16-byte aligned address that is never dereferenced: every call below returns before the device


@pytest.fixture(scope="module")
def lib(built):
    import torch  # noqa: F401  (torch's HIP runtime first, as in the product)
    lib = ctypes.CDLL(str(built / "libmi_spmm.so"))
    vp, i64, i32, f32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_size_t
    dense = [vp, i64, i64]
    for s in SUFFIXES:
        getattr(lib, f"mi_sparse_attention_{s}").argtypes = [vp, vp, i64, i32, i32, i32, i32] + 3 * dense + [f32] + dense + \
            [vp, vp, sz, vp]
        getattr(lib, f"mi_sparse_attention_backward_{s}").argtypes = [vp, vp, i64, i32, i32, i32, i32] + 4 * dense + \
            [vp, f32] + dense + [vp, vp, vp, sz, vp]
    lib.mi_sparse_attention_workspace_bytes.argtypes = [i64, i32, i32, i32]
    lib.mi_sparse_attention_workspace_bytes.restype = sz
    return lib


def test_header_declares_the_seven_entries():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", text), name
    assert "#define MI_SPMM_ABI_VERSION 1" in text


def test_library_exports_the_seven_entries(lib):
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert lib.mi_spmm_abi_version() == 1


DEFAULTS = dict(rowptr=FAKE, col=FAKE, nnz=10, batch=1, M=4, K=4, D=16, q=FAKE, k=FAKE, v=FAKE, out=FAKE, stats=FAKE,
                dout=FAKE, dq=FAKE, y=FAKE, ds=FAKE, ld=None)


def fwd(lib, s, **kw):
    a = {**DEFAULTS, **kw}
    ld = a["D"] if a["ld"] is None else a["ld"]
    return getattr(lib, f"mi_sparse_attention_{s}")(
        a["rowptr"], a["col"], a["nnz"], a["batch"], a["M"], a["K"], a["D"], a["q"], ld, a["M"] * ld, a["k"], ld, a["K"] * ld,
        a["v"], ld, a["K"] * ld, 1.0, a["out"], ld, a["M"] * ld, a["stats"], None, 0, None)


def bwd(lib, s, **kw):
    a = {**DEFAULTS, **kw}
    ld = a["D"] if a["ld"] is None else a["ld"]
    return getattr(lib, f"mi_sparse_attention_backward_{s}")(
        a["rowptr"], a["col"], a["nnz"], a["batch"], a["M"], a["K"], a["D"], a["q"], ld, a["M"] * ld, a["k"], ld, a["K"] * ld,
        a["v"], ld, a["K"] * ld, a["dout"], ld, a["M"] * ld, a["stats"], 1.0, a["dq"], ld, a["M"] * ld, a["y"], a["ds"],
        None, 0, None)


@pytest.mark.parametrize("s", SUFFIXES)
def test_entries_validate_before_any_hip_call(lib, s):
    step = 4 if s == "f32" else 8
    for call, ptrs in ((fwd, ("rowptr", "col", "q", "k", "v", "out")),
                       (bwd, ("rowptr", "col", "q", "k", "v", "dout", "stats", "dq", "y", "ds"))):
        for kw in ({"nnz": -1}, {"batch": -1}, {"M": -1}, {"K": -1}, {"D": -1}):
            assert call(lib, s, **kw) == EINVAL, (call.__name__, kw)
        assert call(lib, s, nnz=2 ** 31) == ERANGE
        assert call(lib, s, batch=2 ** 16, M=2 ** 15 - 1) == ERANGE  # batch · (M + 1) does not fit the int32 offsets
        assert call(lib, s, batch=2 ** 16, M=2 ** 15 - 2, rowptr=None) == EINVAL  # … and this one does: on to the pointers
        # head sizes: every multiple of 4 (T: of 8) from 8 to 128 passes on to the pointer checks, nothing else does
        for D in (0, 4, 6, 8 + step // 2, 132, 136, 260):
            assert call(lib, s, D=D) == EINVAL, (call.__name__, D)
        for p in ptrs:
            assert call(lib, s, **{p: None}) == EINVAL, (call.__name__, p)
        # no rows: nothing is touched, no pointer is looked at
        nulls = {p: None for p in ptrs}
        for kw in ({"batch": 0}, {"M": 0}):
            assert call(lib, s, **kw) == OK, (call.__name__, kw)
            assert call(lib, s, **kw, **nulls) == OK, (call.__name__, kw)
        assert call(lib, s, K=0) == EINVAL  # entries without columns to point at
        assert call(lib, s, ld=8) == EINVAL  # rows shorter than D
        for p in ptrs[2:]:
            if p in ("y", "ds"):  # T: their element's alignment
                assert s == "f32" or call(lib, s, **{p: FAKE + 1}) == EINVAL, (call.__name__, p)
            elif p != "stats":  # rows are read four columns at a time: 16-byte (T: 8-byte) alignment
                assert call(lib, s, **{p: FAKE + 4}) == EINVAL, (call.__name__, p)


def test_no_entry_needs_a_workspace(lib):
    for nnz, batch, M, D in ((0, 0, 0, 8), (10, 1, 4, 64), (10 ** 8, 384, 512, 64), (2 ** 31 - 1, 1, 10 ** 6, 128)):
        assert lib.mi_sparse_attention_workspace_bytes(nnz, batch, M, D) == 0


def _host_args(dtype=torch.float32):
    a = torch.tensor([[1., 0., 2.], [0., 3., 4.], [5., 0., 0.]]).to_sparse_csr()
    x = torch.rand(1, 3, 8).to(dtype)
    return a.crow_indices().int(), a.col_indices().int(), x


def test_custom_mm_refuses_host_tensors(built):
    import custom_mm
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        offs, col, x = _host_args(dtype)
        stats = torch.empty(3, 2)
        with pytest.raises(RuntimeError, match="device"):
            custom_mm.sparse_attention_fwd(offs, col, 5, 1, 3, 3, x, x, x, 1.0, torch.empty_like(x), stats)
        with pytest.raises(RuntimeError, match="device"):
            custom_mm.sparse_attention_bwd(offs, col, 5, 1, 3, 3, x, x, x, x, stats, 1.0, torch.empty_like(x),
                                           torch.empty(5, dtype=dtype), torch.empty(5, dtype=dtype))


def test_custom_mm_names_both_dtypes_of_mixed_operands(built):
    import custom_mm
    offs, col, x = _host_args(torch.bfloat16)
    stats = torch.empty(3, 2)
    both = r"(?s)(?=.*\bBFloat16\b)(?=.*\bHalf\b)"  # checked before the device, so host tensors show it
    with pytest.raises(RuntimeError, match=both):
        custom_mm.sparse_attention_fwd(offs, col, 5, 1, 3, 3, x, x, x.half(), 1.0, torch.empty_like(x), stats)
    with pytest.raises(RuntimeError, match=both):
        custom_mm.sparse_attention_bwd(offs, col, 5, 1, 3, 3, x, x, x, x, stats, 1.0, torch.empty_like(x),
                                       torch.empty(5, dtype=torch.bfloat16), torch.empty(5, dtype=torch.float16))
    with pytest.raises(RuntimeError, match=r"(?s)(?=.*\bFloat\b)(?=.*\bDouble\b)"):
        custom_mm.sparse_attention_fwd(offs, col, 5, 1, 3, 3, x.float(), x.float(), x.float(), 1.0, torch.empty(1, 3, 8, dtype=torch.float64), stats)
    with pytest.raises(TypeError):  # positional only
        custom_mm.sparse_attention_fwd(offsets=offs, columns=col, nnz=5, batch=1, rows=3, cols=3, q=x, k=x, v=x, scale=1.0,
                                       out=torch.empty_like(x), stats=stats)


def test_fused_attention_takes_is_a_rule_of_dtype_and_head_size(built):
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import matmuls
    for D in range(0, 300):
        assert matmuls.fused_attention_takes(torch.float32, D) == (8 <= D <= 128 and D % 4 == 0), D
        for dt in (torch.bfloat16, torch.float16):
            assert matmuls.fused_attention_takes(dt, D) == (8 <= D <= 128 and D % 8 == 0), (dt, D)
        assert not matmuls.fused_attention_takes(torch.float64, D)
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)


def test_fused_sparse_attention_refuses_what_sparse_attention_refuses(built):
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import matmuls
    p = torch.rand(4, 4).to_sparse_csr()
    x = torch.rand(4, 8)
    with pytest.raises(ValueError, match="fused_sparse_attention.*CSR"):
        matmuls.fused_sparse_attention(x, x, x, p.to_dense())
    with pytest.raises(ValueError, match="fused_sparse_attention.*shape"):
        matmuls.fused_sparse_attention(x, torch.rand(5, 8), x, p)
    with pytest.raises(ValueError, match="fused_sparse_attention: v"):
        matmuls.fused_sparse_attention(x, x, torch.rand(5, 8), p)
    with pytest.raises(ValueError, match="fused_sparse_attention.*float64"):
        matmuls.fused_sparse_attention(x.double(), x.double(), x.double(), p)
    with pytest.raises(RuntimeError, match="fused_sparse_attention.*dtype"):
        matmuls.fused_sparse_attention(x, x, x.half(), p)
    with pytest.raises(RuntimeError, match="fused_sparse_attention.*device"):
        matmuls.fused_sparse_attention(x, x, x, p)
    # a batched low-precision pattern is not refused for being one: it gets as far as the device check …
    bp = torch.rand(2, 4, 4).to_sparse_csr()
    with pytest.raises(RuntimeError, match="fused_sparse_attention.*device"):
        matmuls.fused_sparse_attention(*(torch.rand(2, 4, 8).half() for _ in range(3)), bp)
    # … and sparse_attention's own refusal stays
    with pytest.raises(RuntimeError, match=r"sparse_attention: a batched torch.float16 CSR pattern"):
        matmuls.sparse_attention(*(torch.rand(2, 4, 8).half() for _ in range(3)), bp)
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)


# ---- autograd wiring on CPU tensors, float64 stand-in arithmetic ------------------------------------------------

@pytest.fixture()
def mm(oracle_mod):
    """(matmuls bound to the float64 stand-in, the stand-in)."""
    import fake_custom_mm_fused_attention as fake
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


def _pattern(g, *shape, keep=0.4):
    """A CSR pattern (2-d or batched, equal entry counts per item) whose first row of every item is made empty where the
    counts allow it (2-d), and its dense 0/1 mask."""
    rows, cols = shape[-2], shape[-1]
    per_row = max(1, int(keep * cols))
    mask = torch.zeros(shape, dtype=torch.float64)
    flat = mask.view(-1, cols)
    for r in range(flat.shape[0]):
        flat[r, torch.randperm(cols, generator=g)[:per_row]] = 1.0
    if len(shape) == 2:
        mask[0] = 0.0  # an empty row, and …
        mask[3] = 0.0  # … another one
    else:
        # equal counts per item: item i's row i gives its entries to row i + 1
        for i, item in enumerate(mask.view(-1, rows, cols)):
            item[i % rows] = 0.0
            free = (item[(i + 1) % rows] == 0).nonzero().flatten()[:per_row]
            item[(i + 1) % rows, free] = 1.0
    return mask.to_sparse_csr(), mask


def _reference(q, k, v, mask, scale, w):
    rq, rk, rv = (x.detach().double().requires_grad_(True) for x in (q, k, v))
    s = scale * (rq @ rk.transpose(-1, -2))
    empty = mask.sum(-1, keepdim=True) == 0  # empty rows: zero rows (kept finite inside the softmax: no NaN gradients)
    p = torch.softmax(s.masked_fill((mask == 0) & ~empty, -float("inf")), -1)
    p = torch.where(empty, torch.zeros_like(p), p)
    out = p @ rv
    grads = torch.autograd.grad(out, (rq, rk, rv), grad_outputs=w.double())
    return (out.detach(),) + grads


@pytest.mark.parametrize("shape", [(9, 9), (6, 11), (2, 2, 8, 8), (3, 7, 5)])
@pytest.mark.parametrize("scale", [None, 0.5])
def test_fused_sparse_attention_matches_dense_masked_autograd(mm, shape, scale):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(17)
    csr, mask = _pattern(g, *shape)
    D = 5
    lead = shape[:-2]
    q = torch.randn(lead + (shape[-2], D), generator=g, dtype=torch.float64, requires_grad=True)
    k, v = (torch.randn(lead + (shape[-1], D), generator=g, dtype=torch.float64, requires_grad=True) for _ in range(2))
    out = matmuls.fused_sparse_attention(q, k, v, csr, scale)
    w = torch.randn(out.shape, generator=g, dtype=torch.float64)
    ref = _reference(q, k, v, mask, 1.0 / D ** 0.5 if scale is None else scale, w)
    assert out.shape == ref[0].shape and out.dtype == torch.float64
    assert torch.allclose(out.detach(), ref[0], rtol=1e-12, atol=1e-12)
    out.backward(w)
    for name, got, want in (("dq", q.grad, ref[1]), ("dk", k.grad, ref[2]), ("dv", v.grad, ref[3])):
        assert got.shape == want.shape
        assert torch.allclose(got, want, rtol=1e-11, atol=1e-12), (name, float((got - want).abs().max()))
    empty = mask.sum(-1) == 0
    assert empty.any() and (out.detach()[empty] == 0).all() and (q.grad[empty] == 0).all()
    names = [c[0] for c in fake.calls]
    assert names.count("sparse_attention_fwd") == 1 and names.count("sparse_attention_bwd") == 1
    assert not {"sddmm", "sddmm_batched", "csr_softmax", "csr_softmax_backward"} & set(names)


def test_a_low_precision_batch_runs_its_column_side_on_the_block_diagonal_matrix(mm):
    """float16 operands through the stand-in (float64 arithmetic, float16 storage): each column-side gradient is ONE 2-d
    product on the block-diagonal matrix [nb·S, nb·S]; held to float16 rounding of the stored stages."""
    matmuls, fake = mm
    g = torch.Generator().manual_seed(18)
    shape = (3, 8, 8)
    csr, mask = _pattern(g, *shape)
    q, k, v = (torch.randn(3, 8, 4, generator=g).half().requires_grad_(True) for _ in range(3))
    out = matmuls.fused_sparse_attention(q, k, v, csr)
    w = torch.randn(out.shape, generator=g).half()
    ref = _reference(q, k, v, mask, 0.5, w)
    out.backward(w)
    for name, got, want in (("out", out.detach(), ref[0]), ("dq", q.grad, ref[1]), ("dk", k.grad, ref[2]), ("dv", v.grad, ref[3])):
        assert got.dtype == torch.float16
        assert torch.allclose(got.double(), want, rtol=4e-3, atol=4e-3), (name, float((got.double() - want).abs().max()))
    assert [c for c in fake.calls if c[0] == "naive_spmm"] == [("naive_spmm", (24, 24))] * 2
    assert not any(c[0] == "naive_spmm_batched" for c in fake.calls)


def test_saved_for_backward_is_the_operands_the_pattern_and_two_floats_per_row(mm):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(19)
    csr, mask = _pattern(g, 2, 6, 6)
    q, k, v = (torch.randn(2, 6, 4, generator=g, dtype=torch.float64, requires_grad=True) for _ in range(3))
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
        matmuls.fused_sparse_attention(q, k, v, csr)
    dense = [t for t in saved if t.layout == torch.strided]
    own = {t.data_ptr() for t in (q, k, v)}
    extra = [t for t in dense if t.data_ptr() not in own]
    assert len(extra) == 1 and extra[0].shape == (12, 2) and extra[0].dtype == torch.float32
