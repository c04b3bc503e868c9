"""Block-sparse × dense products without a GPU: block_mm_takes is a rule of (dtype, block) alone, every refusal of
matmuls.block_sparse_mm is raised with its exception type before any device call, the C-ABI declares and exports the four
entries and they validate their arguments before any HIP call, custom_mm refuses host tensors, bsr_parts round-trips a
torch.sparse_bsr tensor, the sorted / transposed / entry-id lists of an unsorted rectangular layout are the hand-written
ones, and the autograd wiring is checked on CPU tensors against torch autograd of A_dense @ b in float64, with a float64
stand-in for the kernels (tests/fake_custom_mm_block_mm.py)."""
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
ENTRIES = tuple(f"mi_bsr_mm_{s}" for s in SUFFIXES) + tuple(f"mi_bsr_sddmm_{s}" for s in SUFFIXES)
OK, EINVAL, ERANGE = 0, -1, -2
FAKE = 0x1000  # a non-null, 16-byte aligned address that is never dereferenced: every call below returns before the device


@pytest.fixture(scope="module")
def lib(built):
    import torch  # noqa: F401  (torch's HIP runtime first, as in the product)
    lib = ctypes.CDLL(str(built / "libmi_spmm.so"))
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    for s in SUFFIXES:
        getattr(lib, f"mi_bsr_mm_{s}").argtypes = [vp, vp, vp, i64] + 5 * [i32] + [vp, i64, vp, i64, i64, vp, i64, i64, vp]
        getattr(lib, f"mi_bsr_sddmm_{s}").argtypes = [vp, vp, vp, i64] + 4 * [i32] + [vp, i64, i64, vp, i64, i64, vp, i64, vp]
    return lib


def test_header_declares_the_entries():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", text), name


def test_library_exports_the_entries(lib):
    for name in ENTRIES:
        assert hasattr(lib, name), name


MM = dict(rowptr=FAKE, col=FAKE, ids=FAKE, nnz=4, trans_a=0, rows=128, inner=192, N=40, batch=2, values=FAKE, nvalues=4, B=FAKE,
          ldb=None, sB=None, C=FAKE, ldc=None, sC=None)
SD = dict(row=FAKE, col=FAKE, ids=FAKE, nnz=4, M=128, K=192, N=40, batch=2, dC=FAKE, ldg=None, sG=None, B=FAKE, ldb=None, sB=None,
          out=FAKE, nvalues=4)


def mm_call(lib, s, **kw):
    a = {**MM, **kw}
    ldb, ldc = (a["N"] if a[k] is None else a[k] for k in ("ldb", "ldc"))
    sB = a["inner"] * ldb if a["sB"] is None else a["sB"]
    sC = a["rows"] * ldc if a["sC"] is None else a["sC"]
    return getattr(lib, f"mi_bsr_mm_{s}")(a["rowptr"], a["col"], a["ids"], a["nnz"], a["trans_a"], a["rows"], a["inner"], a["N"],
                                          a["batch"], a["values"], a["nvalues"], a["B"], ldb, sB, a["C"], ldc, sC, None)


def sd_call(lib, s, **kw):
    a = {**SD, **kw}
    ldg, ldb = (a["N"] if a[k] is None else a[k] for k in ("ldg", "ldb"))
    sG = a["M"] * ldg if a["sG"] is None else a["sG"]
    sB = a["K"] * ldb if a["sB"] is None else a["sB"]
    return getattr(lib, f"mi_bsr_sddmm_{s}")(a["row"], a["col"], a["ids"], a["nnz"], a["M"], a["K"], a["N"], a["batch"], a["dC"], ldg,
                                             sG, a["B"], ldb, sB, a["out"], a["nvalues"], None)


@pytest.mark.parametrize("s", SUFFIXES)
def test_product_entry_validates_before_any_hip_call(lib, s):
    for kw in ({"nnz": -1}, {"nvalues": -1}, {"rows": -64}, {"inner": -64}, {"N": -1}, {"batch": -1}, {"sB": -8}, {"sC": -8}):
        assert mm_call(lib, s, **kw) == EINVAL, kw
    for kw in ({"rows": 100}, {"inner": 200}, {"rows": 32}, {"ldb": 39}, {"ldc": 39}):
        assert mm_call(lib, s, **kw) == EINVAL, kw
    assert mm_call(lib, s, nnz=2 ** 31, nvalues=2 ** 31) == ERANGE
    assert mm_call(lib, s, nvalues=2 ** 31) == ERANGE
    assert mm_call(lib, s, ids=None, nvalues=3) == EINVAL  # fewer blocks than entries, and no ids to say which
    for trans_a in (0, 1):
        for p in ("rowptr", "col", "values", "B", "C"):
            assert mm_call(lib, s, trans_a=trans_a, **{p: None}) == EINVAL, p
        for p in ("B", "C"):
            assert mm_call(lib, s, trans_a=trans_a, **{p: FAKE + 1}) == EINVAL, p  # not even 2-byte aligned
        assert mm_call(lib, s, trans_a=trans_a, values=FAKE + 8) == EINVAL  # blocks start on 16 bytes
        assert mm_call(lib, s, trans_a=trans_a, inner=0) == EINVAL  # entries, and nothing they could meet
    # an empty problem: nothing is touched, no pointer is looked at
    nulls = {p: None for p in ("rowptr", "col", "ids", "values", "B", "C")}
    for kw in ({"rows": 0}, {"N": 0}, {"batch": 0}):
        assert mm_call(lib, s, **kw) == OK, kw
        assert mm_call(lib, s, **kw, **nulls) == OK, kw


@pytest.mark.parametrize("s", SUFFIXES)
def test_sampled_entry_validates_before_any_hip_call(lib, s):
    for kw in ({"nnz": -1}, {"nvalues": -1}, {"M": -64}, {"K": -64}, {"N": -1}, {"batch": -1}, {"sG": -8}, {"sB": -8}):
        assert sd_call(lib, s, **kw) == EINVAL, kw
    for kw in ({"M": 100}, {"K": 200}, {"K": 32}, {"ldg": 39}, {"ldb": 39}, {"M": 0}, {"K": 0}):
        assert sd_call(lib, s, **kw) == EINVAL, kw
    assert sd_call(lib, s, nnz=2 ** 31, nvalues=2 ** 31) == ERANGE
    assert sd_call(lib, s, batch=2 ** 16, N=2 ** 15) == ERANGE  # the flattened width does not fit an int32
    assert sd_call(lib, s, ids=None, nvalues=3) == EINVAL
    for p in ("row", "col", "dC", "B", "out"):
        assert sd_call(lib, s, **{p: None}) == EINVAL, p
    for p in ("dC", "B"):
        assert sd_call(lib, s, **{p: FAKE + 1}) == EINVAL, p
    assert sd_call(lib, s, out=FAKE + 8) == EINVAL
    nulls = {p: None for p in ("row", "col", "ids", "dC", "B", "out")}
    assert sd_call(lib, s, nnz=0, nvalues=0) == OK and sd_call(lib, s, nnz=0, nvalues=0, **nulls) == OK


def _host_args(dtype=torch.bfloat16):
    offs = torch.tensor([0, 1], dtype=torch.int32)
    col = torch.tensor([0], dtype=torch.int32)
    return offs, col, torch.rand(1, 64, 64).to(dtype), torch.rand(1, 64, 8).to(dtype)


def test_custom_mm_refuses_host_tensors(built):
    import custom_mm
    for dtype in (torch.bfloat16, torch.float16):
        offs, col, v, b = _host_args(dtype)
        for trans_a in (False, True):
            with pytest.raises(RuntimeError, match="device"):
                custom_mm.bsr_mm(offs, col, None, 1, v, b, torch.empty_like(b), trans_a)
        with pytest.raises(RuntimeError, match="device"):
            custom_mm.bsr_sddmm(col, col, col, 1, b, b, torch.empty_like(v))
    offs, col, v, b = _host_args()
    both = r"(?s)(?=.*\bBFloat16\b)(?=.*\bHalf\b)"  # checked before the device, so host tensors show it
    with pytest.raises(RuntimeError, match=both):
        custom_mm.bsr_mm(offs, col, None, 1, v, b.half(), torch.empty_like(b), False)
    with pytest.raises(RuntimeError, match=both):
        custom_mm.bsr_sddmm(col, col, None, 1, b, b, torch.empty_like(v).half())


@pytest.fixture()
def real(built):
    """matmuls on the real extension, imported afresh."""
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import matmuls
    yield matmuls
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)


def test_block_mm_takes_is_a_rule_of_dtype_and_block(real):
    for block in (0, 1, 16, 32, 63, 64, 65, 128, 256, -64):
        for dt in (torch.bfloat16, torch.float16):
            assert real.block_mm_takes(dt, block) == (block == 64), (dt, block)
        for dt in (torch.float32, torch.float64, torch.int32):
            assert not real.block_mm_takes(dt, block)
    assert not real.block_mm_takes(torch.bfloat16, 64.0) and not real.block_mm_takes(torch.bfloat16, True)


def _layout(rows, cols, lead=()):
    return torch.ones(lead + (rows, cols)).to_sparse_csr()


def test_every_refusal_comes_before_the_device(real):
    f = real.block_sparse_mm
    lay = _layout(2, 3)
    v = torch.rand(6, 64, 64).bfloat16()
    b = torch.rand(2, 192, 40).bfloat16()
    with pytest.raises(ValueError, match="block_sparse_mm.*CSR"):
        f(v, lay.to_dense(), b)
    with pytest.raises(ValueError, match="block_sparse_mm.*batched layout"):
        f(v, _layout(2, 3, lead=(2,)), b)
    with pytest.raises(ValueError, match="block_sparse_mm: b must be a dense tensor"):
        f(v, lay, lay)
    with pytest.raises(ValueError, match=r"block_sparse_mm: values must be bfloat16 or float16, got torch.float32.*block = 64"):
        f(v.float(), lay, b.float())
    with pytest.raises(ValueError, match="block_sparse_mm: b must be bfloat16 or float16, got torch.float64"):
        f(v, lay, b.double())
    with pytest.raises(RuntimeError, match=r"block_sparse_mm: values is torch.bfloat16 but b is torch.float16.*one dtype"):
        f(v, lay, b.half())
    for block in (32, 128, 0, -64, 64.0, True):
        with pytest.raises(ValueError, match="block_sparse_mm: block must be 64"):
            f(v, lay, b, block=block)
    with pytest.raises(ValueError, match=r"block_sparse_mm: values must be \[n, 64, 64\]"):
        f(torch.rand(6, 32, 32).bfloat16(), lay, b)
    with pytest.raises(ValueError, match=r"block_sparse_mm: values must be \[n, 64, 64\]"):
        f(torch.rand(2, 6, 64, 64).bfloat16(), lay, b)  # batched values
    with pytest.raises(ValueError, match="block_sparse_mm: values holds 5 blocks but the layout stores 6"):
        f(v[:5], lay, b)
    with pytest.raises(ValueError, match="block_sparse_mm: values must be contiguous"):
        f(v.transpose(1, 2), lay, b)
    with pytest.raises(ValueError, match="block_sparse_mm: b must be a"):
        f(v, lay, b[0, 0])
    for K in (128, 100, 200, 256):  # K not the layout's, a multiple of 64 or not
        with pytest.raises(ValueError, match=rf"block_sparse_mm: b of shape .* has K = {K} rows.*multiples of block"):
            f(v, lay, torch.rand(K, 8).bfloat16())
    # host tensors: the last check, and still before any device call
    for args in ((v, lay, b), (v.half(), lay, b.half()), (v, lay, b[0])):
        with pytest.raises(RuntimeError, match="block_sparse_mm.*device"):
            f(*args)
    with pytest.raises(ValueError, match="bsr_parts"):
        real.bsr_parts(lay)
    with pytest.raises(ValueError, match="bsr_parts.*64 × 64"):
        real.bsr_parts(torch.rand(64, 64).to_sparse_bsr((32, 32)))


def test_bsr_parts_round_trip(real):
    g = torch.Generator().manual_seed(5)
    keep = torch.tensor([[1, 0, 1], [0, 0, 0], [1, 1, 0]], dtype=torch.bool)
    dense = torch.randn(192, 192, generator=g).bfloat16() * keep.repeat_interleave(64, 0).repeat_interleave(64, 1)
    a = dense.to_sparse_bsr((64, 64))
    values, layout = real.bsr_parts(a)
    assert layout.layout == torch.sparse_csr and tuple(layout.shape) == (3, 3)
    assert values.data_ptr() == a.values().data_ptr() and tuple(values.shape) == (4, 64, 64)  # no copy
    assert layout.crow_indices().data_ptr() == a.crow_indices().data_ptr()
    assert layout.col_indices().data_ptr() == a.col_indices().data_ptr()
    assert layout.crow_indices().tolist() == [0, 2, 2, 4] and layout.col_indices().tolist() == [0, 2, 0, 1]
    back = torch.sparse_bsr_tensor(layout.crow_indices(), layout.col_indices(), values, size=(192, 192)).to_dense()
    assert torch.equal(back, a.to_dense()) and torch.equal(back, dense)


# ---- the lists and the autograd wiring on CPU tensors, float64 stand-in arithmetic ----------------------------------

@pytest.fixture()
def mm(oracle_mod):
    """(matmuls bound to the float64 stand-in, the stand-in)."""
    import fake_custom_mm_block_mm as fake
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


@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64])
def test_lists_of_an_unsorted_rectangular_layout(mm, index_dtype):
    matmuls, fake = mm
    # 2 × 5 blocks: block row 0 keeps columns 3, 0, 4 (entries 0, 1, 2, in this order), block row 1 columns 4, 0 (entries 3, 4)
    layout = torch.sparse_csr_tensor(torch.tensor([0, 3, 5], dtype=index_dtype), torch.tensor([3, 0, 4, 4, 0], dtype=index_dtype),
                                     torch.ones(5), size=(2, 5))
    st = matmuls._csr_state(layout)
    rec = matmuls._bsr_layout(layout, torch.device("cpu"), st)
    offsets, columns, ids, entry_row, n = rec["fwd"]
    assert all(t.dtype == torch.int32 for t in (offsets, columns, ids, entry_row)) and n == 5
    assert offsets.tolist() == [0, 3, 5]
    assert columns.tolist() == [0, 3, 4, 0, 4]
    assert ids.tolist() == [1, 0, 2, 4, 3]
    assert entry_row.tolist() == [0, 0, 0, 1, 1]
    t_off, t_col, t_ids = matmuls._bsr_layout_transposed(rec, 2, 5)
    assert all(t.dtype == torch.int32 for t in (t_off, t_col, t_ids))
    assert t_off.tolist() == [0, 2, 2, 2, 3, 5]
    assert t_col.tolist() == [0, 1, 0, 0, 1]
    assert t_ids.tolist() == [1, 4, 0, 2, 3]
    # kept: the same record, no second transpose
    assert matmuls._bsr_layout(layout, torch.device("cpu"), matmuls._csr_state(layout)) is rec
    matmuls._bsr_layout_transposed(rec, 2, 5)
    assert [c[0] for c in fake.calls].count("csr_transpose") == 1


def _random_layout(g, rows, cols, keep, index_dtype=torch.int64):
    """A CSR block layout with `keep[r]` blocks in block row r, columns in a shuffled order."""
    col = torch.cat([torch.randperm(cols, generator=g)[:k] for k in keep]).to(index_dtype)
    crow = torch.tensor([0] + list(torch.tensor(keep).cumsum(0))).to(index_dtype)
    return torch.sparse_csr_tensor(crow, col, torch.ones(col.numel()), size=(rows, cols))


@pytest.mark.parametrize("lead,rows,cols,keep,N,dtype", [
    ((), 2, 3, (2, 3), 40, torch.float16),
    ((2, 3), 3, 2, (1, 0, 2), 8, torch.bfloat16),
    ((2,), 4, 4, (4, 1, 0, 2), 1, torch.float16),
])
def test_block_sparse_mm_matches_dense_autograd(mm, lead, rows, cols, keep, N, dtype):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(31)
    layout = _random_layout(g, rows, cols, keep)
    n = sum(keep)
    values = (torch.randn(n, 64, 64, generator=g) / 8).to(dtype).requires_grad_(True)
    b = torch.randn(lead + (cols * 64, N), generator=g).to(dtype).requires_grad_(True)
    out = matmuls.block_sparse_mm(values, layout, b)
    w = torch.randn(out.shape, generator=g).to(dtype)
    out.backward(w)
    # the reference: A_dense built from a float64 leaf through torch's own BSR → dense, which differentiates on the CPU
    rv = values.detach().double().requires_grad_(True)
    rb = b.detach().double().requires_grad_(True)
    # (on the layout's sorted twin, the blocks permuted to match by a differentiable index: torch's backward of to_dense hands
    # the gradient back in sorted order)
    crow, col = layout.crow_indices(), layout.col_indices()
    row = torch.repeat_interleave(torch.arange(rows), crow[1:] - crow[:-1])
    order = torch.argsort(row * cols + col)
    a_dense = torch.sparse_bsr_tensor(crow, col[order], rv[order], size=(rows * 64, cols * 64)).to_dense()
    ref = a_dense @ rb
    gv, gb = torch.autograd.grad(ref, (rv, rb), grad_outputs=w.double())
    tol = 4e-3 if dtype == torch.float16 else 3e-2  # the stand-in computes in float64 and narrows once
    for name, got, want in (("out", out.detach(), ref.detach()), ("d values", values.grad, gv), ("d b", b.grad, gb)):
        assert got.dtype == dtype and got.shape == want.shape, name
        scale = float(want.abs().max()) + 1.0
        assert float((got.double() - want).abs().max()) <= tol * scale, (name, float((got.double() - want).abs().max()))
    names = [c[0] for c in fake.calls]
    assert names.count("bsr_mm") == 2 and names.count("bsr_sddmm") == 1 and names.count("csr_transpose") == 1
    trans = [c[1][3] for c in fake.calls if c[0] == "bsr_mm"]
    assert trans == [False, True]
    # a second step on the same layout tensor sorts and transposes nothing again; the layout gets no gradient
    out2 = matmuls.block_sparse_mm(values, layout, b)
    out2.backward(w)
    assert [c[0] for c in fake.calls].count("csr_transpose") == 1
    assert torch.equal(out2.detach(), out.detach())


def test_empty_cases_launch_nothing(mm):
    matmuls, fake = mm
    b = torch.randn(2, 128, 8).half().requires_grad_(True)
    none = torch.sparse_csr_tensor(torch.zeros(4, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), torch.zeros(0), size=(3, 2))
    values = torch.zeros(0, 64, 64).half().requires_grad_(True)
    out = matmuls.block_sparse_mm(values, none, b)
    assert tuple(out.shape) == (2, 192, 8) and out.dtype == torch.float16 and not out.any()
    out.backward(torch.ones_like(out))
    assert tuple(values.grad.shape) == (0, 64, 64) and tuple(b.grad.shape) == tuple(b.shape) and not b.grad.any()
    g = torch.Generator().manual_seed(3)
    layout = _random_layout(g, 3, 2, (1, 1, 2))
    v2 = torch.randn(4, 64, 64, generator=g).half().requires_grad_(True)
    e = torch.zeros(0, 128, 8).half().requires_grad_(True)
    out = matmuls.block_sparse_mm(v2, layout, e)
    assert tuple(out.shape) == (0, 192, 8)
    out.backward(torch.ones_like(out))
    assert tuple(v2.grad.shape) == (4, 64, 64) and not v2.grad.any() and tuple(e.grad.shape) == (0, 128, 8)
    assert not [c for c in fake.calls if c[0].startswith("bsr_")]


def test_saved_for_backward_is_the_operands_alone(mm):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(29)
    layout = _random_layout(g, 2, 3, (2, 1))
    values = torch.randn(3, 64, 64, generator=g).half().requires_grad_(True)
    b = torch.randn(2, 192, 16, generator=g).half().requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
        matmuls.block_sparse_mm(values, layout, b)
    dense = [t for t in saved if t.layout == torch.strided]
    assert {t.data_ptr() for t in dense} == {values.data_ptr(), b.data_ptr()}
