"""CSR row softmax, sampled products and sparse attention without a GPU: the C-ABI declares and exports the seven softmax
entries, they validate their arguments before any HIP call, custom_mm refuses host tensors and mixed dtypes, the three
matmuls functions refuse what they document, and their autograd wiring (which saved tensor goes where, the formulas) is
checked on CPU tensors against torch autograd of the dense masked expression in float64, with a float64 stand-in for the
kernels (tests/fake_custom_mm_attention.py)."""
import ctypes
import importlib
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "mi_spmm.h"
SUFFIXES = ("f32", "bf16", "f16")
ENTRIES = tuple(f"mi_csr_softmax_{s}" for s in SUFFIXES) + tuple(f"mi_csr_softmax_backward_{s}" for s in SUFFIXES) + \
    ("mi_csr_softmax_workspace_bytes",)
OK, EINVAL, ERANGE, ENOMEM = 0, -1, -2, -4
FAKE = 0x1000  # a non-null address that is never dereferenced: every call below returns before touching the device


@pytest.fixture(scope="module")
def lib(built):
    import torch  # noqa: F401  (torch's HIP runtime first, as in the product)
    lib = ctypes.CDLL(str(built / "libmi_spmm.so"))
    vp, i64, i32, f32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_size_t
    for s in SUFFIXES:
        getattr(lib, f"mi_csr_softmax_{s}").argtypes = [vp, i64, i32, i32, vp, f32, vp, vp, sz, vp]
        getattr(lib, f"mi_csr_softmax_backward_{s}").argtypes = [vp, i64, i32, i32, vp, vp, f32, vp, vp, sz, vp]
    lib.mi_csr_softmax_workspace_bytes.argtypes = [i64, i32, i32]
    lib.mi_csr_softmax_workspace_bytes.restype = sz
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


def fwd(lib, s, *, rowptr=FAKE, nnz=10, batch=1, M=4, x=FAKE, y=FAKE, ws=None, ws_bytes=0):
    return getattr(lib, f"mi_csr_softmax_{s}")(rowptr, nnz, batch, M, x, 1.0, y, ws, ws_bytes, None)


def bwd(lib, s, *, rowptr=FAKE, nnz=10, batch=1, M=4, y=FAKE, dy=FAKE, dx=FAKE, ws=None, ws_bytes=0):
    return getattr(lib, f"mi_csr_softmax_backward_{s}")(rowptr, nnz, batch, M, y, dy, 1.0, dx, ws, ws_bytes, None)


@pytest.mark.parametrize("s", SUFFIXES)
def test_entries_validate_before_any_hip_call(lib, s):
    for call, ptrs in ((fwd, ("rowptr", "x", "y")), (bwd, ("rowptr", "y", "dy", "dx"))):
        for kw in ({"nnz": -1}, {"batch": -1}, {"M": -1}):
            assert call(lib, s, **kw) == EINVAL, (call.__name__, kw)
        assert call(lib, s, nnz=2 ** 31) == ERANGE
        assert call(lib, s, batch=2 ** 16, M=2 ** 15 - 1) == ERANGE  # batch · (M + 1) does not fit the int32 offsets
        assert call(lib, s, batch=2 ** 16, M=2 ** 15 - 2, rowptr=None) == EINVAL  # … and this one does: on to the pointers
        for p in ptrs:
            assert call(lib, s, **{p: None}) == EINVAL, (call.__name__, p)
        # the empty problems touch nothing: no pointer is looked at
        nulls = {p: None for p in ptrs}
        for kw in ({"nnz": 0}, {"batch": 0}, {"M": 0}):
            assert call(lib, s, **kw) == OK, (call.__name__, kw)
            assert call(lib, s, **kw, **nulls) == OK, (call.__name__, kw)
        if s != "f32":  # 2-byte alignment of 16-bit values
            for p in ptrs[1:]:
                assert call(lib, s, **{p: FAKE + 1}) == EINVAL, (call.__name__, p)


def test_no_entry_needs_a_workspace(lib):
    # every form works in registers and LDS: the size is 0 for every problem, so no workspace can be too small
    for nnz, batch, M in ((0, 0, 0), (10, 1, 4), (10 ** 8, 384, 512), (2 ** 31 - 1, 1, 10 ** 6)):
        assert lib.mi_csr_softmax_workspace_bytes(nnz, batch, M) == 0


def _host_csr(dtype=torch.float32):
    a = torch.tensor([[1., 0., 2.], [0., 3., 4.]]).to_sparse_csr()
    return a.values().to(dtype), a.crow_indices().int()


def test_custom_mm_refuses_host_tensors(built):
    import custom_mm
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        v, offs = _host_csr(dtype)
        with pytest.raises(RuntimeError, match="device"):
            custom_mm.csr_softmax(v, offs, 4, 1, 2, 1.0, torch.empty_like(v))
        with pytest.raises(RuntimeError, match="device"):
            custom_mm.csr_softmax_backward(v, v.clone(), offs, 4, 1, 2, 1.0, torch.empty_like(v))


def test_custom_mm_names_both_dtypes_of_mixed_operands(built):
    import custom_mm
    v, offs = _host_csr(torch.bfloat16)
    both = r"(?s)(?=.*\bBFloat16\b)(?=.*\bHalf\b)"  # checked before the device, so host tensors show it
    with pytest.raises(RuntimeError, match=both):
        custom_mm.csr_softmax(v, offs, 4, 1, 2, 1.0, torch.empty(4, dtype=torch.float16))
    with pytest.raises(RuntimeError, match=both):
        custom_mm.csr_softmax_backward(v, v.to(torch.float16), offs, 4, 1, 2, 1.0, torch.empty_like(v))
    with pytest.raises(RuntimeError, match=r"(?s)(?=.*\bFloat\b)(?=.*\bDouble\b)"):
        custom_mm.csr_softmax(v.float(), offs, 4, 1, 2, 1.0, torch.empty(4, dtype=torch.float64))
    with pytest.raises(TypeError):  # positional only
        custom_mm.csr_softmax(values=v, offsets=offs, nnz=4, batch=1, rows=2, scale=1.0, out=torch.empty_like(v))


def test_matmuls_functions_refuse_what_they_document(built):
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import matmuls
    a = torch.rand(4, 5).to_sparse_csr()
    q, k = torch.rand(4, 3), torch.rand(5, 3)
    # sparse_softmax
    with pytest.raises(ValueError, match="sparse_softmax.*CSR"):
        matmuls.sparse_softmax(a.to_dense())
    with pytest.raises(ValueError, match="sparse_softmax.*CSR"):
        matmuls.sparse_softmax(a.to_sparse_coo())
    with pytest.raises(ValueError, match="sparse_softmax.*float64"):
        matmuls.sparse_softmax(a.double())
    with pytest.raises(RuntimeError, match="sparse_softmax.*device"):
        matmuls.sparse_softmax(a)
    # sampled_matmul
    with pytest.raises(ValueError, match="sampled_matmul.*CSR"):
        matmuls.sampled_matmul(a.to_dense(), q, k)
    with pytest.raises(ValueError, match="sampled_matmul.*dense"):
        matmuls.sampled_matmul(a, a, k)
    with pytest.raises(ValueError, match="sampled_matmul.*float64"):
        matmuls.sampled_matmul(a, q.double(), k.double())
    with pytest.raises(RuntimeError, match=r"(?s)sampled_matmul(?=.*\bfloat32\b)(?=.*\bbfloat16\b)"):
        matmuls.sampled_matmul(a, q, k.bfloat16())
    with pytest.raises(ValueError, match="sampled_matmul.*2-d"):
        matmuls.sampled_matmul(a, q.unsqueeze(0), k)
    with pytest.raises(ValueError, match="sampled_matmul.*shape"):
        matmuls.sampled_matmul(a, q, torch.rand(4, 3))
    with pytest.raises(ValueError, match="sampled_matmul.*shape"):
        matmuls.sampled_matmul(a, q, torch.rand(5, 2))
    with pytest.raises(RuntimeError, match="sampled_matmul.*device"):
        matmuls.sampled_matmul(a, q, k)
    batched = torch.rand(2, 4, 5).to_sparse_csr()
    with pytest.raises(RuntimeError, match=r"sampled_matmul: a batched torch.bfloat16 CSR pattern \(3-d\) is not supported \(float32 only\)"):
        matmuls.sampled_matmul(batched, torch.rand(2, 4, 3).bfloat16(), torch.rand(2, 5, 3).bfloat16())
    # sparse_attention
    p = torch.rand(4, 4).to_sparse_csr()
    x = torch.rand(4, 3)
    with pytest.raises(ValueError, match="sparse_attention.*CSR"):
        matmuls.sparse_attention(x, x, x, p.to_dense())
    with pytest.raises(ValueError, match="sparse_attention.*shape"):
        matmuls.sparse_attention(x, torch.rand(5, 3), x, p)
    with pytest.raises(ValueError, match="sparse_attention: v"):
        matmuls.sparse_attention(x, x, torch.rand(5, 3), p)
    with pytest.raises(RuntimeError, match="sparse_attention.*dtype"):
        matmuls.sparse_attention(x, x, x.half(), p)
    with pytest.raises(RuntimeError, match="sparse_attention.*device"):
        matmuls.sparse_attention(x, x, x, p)
    with pytest.raises(RuntimeError, match=r"sparse_attention: a batched torch.float16 CSR pattern"):
        matmuls.sparse_attention(*(torch.rand(2, 4, 3).half() for _ in range(3)), torch.rand(2, 4, 4).to_sparse_csr())
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)


# ---- autograd wiring on CPU tensors, float64 stand-in arithmetic ------------------------------------------------

@pytest.fixture()
def mm(oracle_mod):
    """(matmuls bound to the float64 stand-in, the stand-in)."""
    import fake_custom_mm
    import fake_custom_mm_attention as fake
    saved = {k: sys.modules.get(k) for k in ("custom_mm", "matmuls")}
    sys.modules["custom_mm"] = fake
    sys.modules.pop("matmuls", None)
    matmuls = importlib.import_module("matmuls")
    fake.calls.clear()
    fake_custom_mm.batched_sddmm = True
    yield matmuls, fake
    fake_custom_mm.batched_sddmm = True
    for k, v in saved.items():
        if v is None:
            sys.modules.pop(k, None)
        else:
            sys.modules[k] = v


def _pattern(g, *shape, keep=0.4, index_dtype=torch.int64):
    """A CSR pattern (2-d or batched, equal entry counts per item, every row non-empty) and its dense 0/1 mask."""
    rows, cols = shape[-2], shape[-1]
    per_row = max(1, int(keep * cols))
    mask = torch.zeros(shape, dtype=torch.float64)
    flat = mask.view(-1, cols)
    for r in range(flat.shape[0]):
        flat[r, torch.randperm(cols, generator=g)[:per_row]] = 1.0
    csr = mask.to_sparse_csr()
    if index_dtype != torch.int64:
        csr = torch.sparse_csr_tensor(csr.crow_indices().to(index_dtype), csr.col_indices().to(index_dtype), csr.values(),
                                      size=shape)
    return csr, mask


def _values_like(csr, mask, dense):
    """The CSR tensor on csr's indices holding `dense` at the stored positions (row-major order = CSR order for sorted columns)."""
    vals = dense[mask.bool()].reshape(csr.values().shape)
    return torch.sparse_csr_tensor(csr.crow_indices(), csr.col_indices(), vals, size=csr.shape)


def _close(got, want, tol=1e-12):
    assert got.shape == want.shape and got.dtype == want.dtype
    assert torch.allclose(got, want, rtol=tol, atol=tol), float((got - want).abs().max())


@pytest.mark.parametrize("shape", [(7, 9), (2, 3, 6, 8)])
@pytest.mark.parametrize("scale", [1.0, 0.37])
def test_sparse_softmax_matches_dense_masked_autograd(mm, shape, scale):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(5)
    csr, mask = _pattern(g, *shape)
    dense = torch.randn(shape, generator=g, dtype=torch.float64)
    a = _values_like(csr, mask, dense).requires_grad_(True)
    out = matmuls.sparse_softmax(a, scale)
    assert out.layout == torch.sparse_csr and out.shape == a.shape
    assert out.crow_indices().data_ptr() == a.crow_indices().data_ptr()  # on a's own index tensors
    d = dense.clone().requires_grad_(True)
    ref = torch.softmax((scale * d).masked_fill(mask == 0, -float("inf")), -1)
    _close(out.to_dense().detach(), ref.detach())
    w = torch.randn(shape, generator=g, dtype=torch.float64)
    out.backward(_values_like(csr, mask, w))
    (ref * w * mask).sum().backward()
    assert a.grad.layout == torch.sparse_csr
    _close(a.grad.to_dense(), d.grad * mask)
    assert ("csr_softmax", (mask[..., 0, 0].numel(), shape[-2])) in fake.calls
    assert ("csr_softmax_backward", (mask[..., 0, 0].numel(), shape[-2])) in fake.calls


@pytest.mark.parametrize("shape,index_dtype,lds_form", [((7, 9), torch.int64, True), ((7, 9), torch.int32, True),
                                                       ((2, 3, 6, 8), torch.int64, True), ((2, 3, 6, 8), torch.int64, False),
                                                       ((3, 6, 8), torch.int32, True)])
def test_sampled_matmul_matches_dense_masked_autograd(mm, shape, index_dtype, lds_form):
    matmuls, fake = mm
    import fake_custom_mm
    fake_custom_mm.batched_sddmm = lds_form  # False: the block-diagonal form
    g = torch.Generator().manual_seed(6)
    csr, mask = _pattern(g, *shape, index_dtype=index_dtype)
    n = 5
    m1 = torch.randn(shape[:-1] + (n,), generator=g, dtype=torch.float64, requires_grad=True)
    m2t = torch.randn(shape[:-2] + (shape[-1], n), generator=g, dtype=torch.float64, requires_grad=True)
    out = matmuls.sampled_matmul(csr, m1, m2t)
    assert out.layout == torch.sparse_csr and out.dtype == torch.float64
    r1, r2 = m1.detach().clone().requires_grad_(True), m2t.detach().clone().requires_grad_(True)
    ref = (r1 @ r2.transpose(-1, -2)) * mask
    tol = 1e-12 if lds_form or len(shape) == 2 else 1e-6  # (the block-diagonal route keeps float32 index work only — same tolerance)
    _close(out.to_dense().detach(), ref.detach(), tol)
    w = torch.randn(shape, generator=g, dtype=torch.float64)
    out.backward(_values_like(csr, mask, w))
    (ref * w).sum().backward()
    _close(m1.grad, r1.grad, tol)
    _close(m2t.grad, r2.grad, tol)
    if len(shape) > 2:
        assert any(c[0] == ("sddmm_batched" if lds_form else "sddmm") for c in fake.calls)


@pytest.mark.parametrize("shape", [(9, 9), (2, 2, 8, 8)])
@pytest.mark.parametrize("scale", [None, 0.5])
def test_sparse_attention_matches_dense_masked_autograd(mm, shape, scale):
    """Through naiveSpMM the stand-in's outputs are float32 tensors (the product's own allocation), so this one is held to
    float32 rounding; the formulas and which saved tensor goes where are what it tests."""
    matmuls, fake = mm
    g = torch.Generator().manual_seed(7)
    csr, mask = _pattern(g, *shape)
    D = 4
    q, k, v = (torch.randn(shape[:-1] + (D,), generator=g, dtype=torch.float32, requires_grad=True) for _ in range(3))
    out = matmuls.sparse_attention(q, k, v, csr.float(), scale)
    rq, rk, rv = (x.detach().double().requires_grad_(True) for x in (q, k, v))
    s = (1.0 / D ** 0.5 if scale is None else scale) * (rq @ rk.transpose(-1, -2))
    ref = torch.softmax(s.masked_fill(mask == 0, -float("inf")), -1) @ rv
    assert out.shape == ref.shape
    assert torch.allclose(out.detach().double(), ref.detach(), rtol=1e-5, atol=1e-6)
    w = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    out.backward(w.float())
    (ref * w).sum().backward()
    for got, want in ((q.grad, rq.grad), (k.grad, rk.grad), (v.grad, rv.grad)):
        assert torch.allclose(got.double(), want, rtol=1e-4, atol=1e-5), float((got.double() - want).abs().max())
    names = [c[0] for c in fake.calls]
    assert "csr_softmax" in names and "csr_softmax_backward" in names


def test_a_static_pattern_is_narrowed_once_along_the_chain(mm):
    """sampled_matmul → sparse_softmax → naive_matmul on one pattern: the results sit on the pattern's index tensors and
    inherit what the pattern keeps, so the transposed pattern is built once for both backward products that need it."""
    matmuls, fake = mm
    g = torch.Generator().manual_seed(8)
    csr, mask = _pattern(g, 9, 9)
    csr = csr.float()
    q, k, v = (torch.randn(9, 4, generator=g, requires_grad=True) for _ in range(3))
    for _ in range(2):
        matmuls.sparse_attention(q, k, v, csr).sum().backward()
    assert [c[0] for c in fake.calls].count("csr_transpose") == 1
