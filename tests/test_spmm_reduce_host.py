"""reduce = mean / amax / amin on the CSR product without a GPU: the C-ABI declares and exports the new entries, they
validate their arguments before any HIP call, custom_mm binds them, and matmuls.sparse_mm_reduce refuses what it cannot
run (no CPU path)."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "mi_spmm.h"
NEW_ENTRIES = ("mi_spmm_csr_reduce_f32", "mi_spmm_csr_reduce_workspace_bytes", "mi_spmm_rows_divide_f32",
               "mi_spmm_reduce_grad_val_f32", "mi_spmm_reduce_grad_b_f32")
SUM, MEAN, AMAX, AMIN = 0, 1, 2, 3
OK, EINVAL, ERANGE = 0, -1, -2


@pytest.fixture(scope="module")
def lib(built):
    import torch  # noqa: F401  (torch's HIP runtime first, as in the product)
    lib = ctypes.CDLL(str(built / "libmi_spmm.so"))
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    lib.mi_spmm_csr_reduce_f32.argtypes = [vp, vp, vp, i64, i32, i32, i32, vp, i64, vp, i64, vp, i64, ctypes.c_int, vp,
                                           ctypes.c_size_t, vp]
    lib.mi_spmm_csr_reduce_workspace_bytes.argtypes = [i64, i32]
    lib.mi_spmm_csr_reduce_workspace_bytes.restype = ctypes.c_size_t
    lib.mi_spmm_rows_divide_f32.argtypes = [vp, i32, i32, vp, i64, vp, i64, vp]
    lib.mi_spmm_reduce_grad_val_f32.argtypes = [vp, vp, i64, i32, i32, i32, vp, i64, vp, i64, vp, i64, vp, vp]
    lib.mi_spmm_reduce_grad_b_f32.argtypes = [vp, vp, vp, vp, i64, i32, i32, i32, vp, i64, vp, i64, vp, i64, vp]
    return lib


def test_header_declares_the_reduce_entries_and_codes():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(rf"\b{name}\s*\(", text), name
    for code, value in (("MI_REDUCE_SUM", SUM), ("MI_REDUCE_MEAN", MEAN), ("MI_REDUCE_AMAX", AMAX), ("MI_REDUCE_AMIN", AMIN)):
        assert re.search(rf"\b{code}\s*=\s*{value}\b", text), code
    assert "#define MI_SPMM_ABI_VERSION 1" in text


def test_library_exports_the_reduce_entries(lib):
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
    assert lib.mi_spmm_abi_version() == 1
    assert lib.mi_spmm_csr_reduce_workspace_bytes(0, 256) == 0
    # the hub-row list and partial rows for 10^8 entries at N = 256: room for every split row
    big = lib.mi_spmm_csr_reduce_workspace_bytes(100_000_000, 256)
    assert big >= (100_000_000 // 16384) * 256 * 8
    lib.mi_spmm_csr_workspace_bytes.argtypes = [ctypes.c_int64, ctypes.c_int32]
    lib.mi_spmm_csr_workspace_bytes.restype = ctypes.c_size_t
    assert big >= lib.mi_spmm_csr_workspace_bytes(100_000_000, 256)  # the sum path runs in the same workspace


# A non-null address that is never dereferenced: every call below must return before touching the device.
FAKE = 0x1000


def reduce_call(lib, reduce, *, nnz=10, M=4, K=4, N=8, arg=None, rowptr=FAKE, col=FAKE, val=FAKE, B=FAKE, C=FAKE,
                ldb=None, ldc=None):
    return lib.mi_spmm_csr_reduce_f32(rowptr, col, val, nnz, M, K, N, B, ldb if ldb is not None else N, C,
                                      ldc if ldc is not None else N, arg, N, reduce, None, 0, None)


def test_reduce_entry_validates_before_any_hip_call(lib):
    for bad in (-1, 4, 99):
        assert reduce_call(lib, bad) == EINVAL, bad
    for r in (SUM, MEAN):
        assert reduce_call(lib, r, arg=FAKE) == EINVAL, r
    for r in (SUM, MEAN, AMAX, AMIN):
        assert reduce_call(lib, r, M=0) == OK, r
        assert reduce_call(lib, r, M=0, rowptr=None, C=None) == OK, r
        assert reduce_call(lib, r, nnz=2 ** 31) == ERANGE, r
        assert reduce_call(lib, r, rowptr=None) == EINVAL, r
        assert reduce_call(lib, r, C=None) == EINVAL, r
        assert reduce_call(lib, r, col=None) == EINVAL, r
        assert reduce_call(lib, r, val=None) == EINVAL, r
        assert reduce_call(lib, r, B=None) == EINVAL, r
        assert reduce_call(lib, r, ldb=7) == EINVAL, r
        assert reduce_call(lib, r, ldc=7) == EINVAL, r
        assert reduce_call(lib, r, M=-1) == EINVAL, r
    # an arg buffer narrower than N
    assert lib.mi_spmm_csr_reduce_f32(FAKE, FAKE, FAKE, 10, 4, 4, 8, FAKE, 8, FAKE, 8, FAKE, 7, AMAX, None, 0, None) == EINVAL


def test_divide_and_gradient_entries_validate_before_any_hip_call(lib):
    assert lib.mi_spmm_rows_divide_f32(FAKE, 0, 8, None, 8, None, 8, None) == OK
    assert lib.mi_spmm_rows_divide_f32(None, 4, 8, FAKE, 8, FAKE, 8, None) == EINVAL
    assert lib.mi_spmm_rows_divide_f32(FAKE, 4, 8, FAKE, 7, FAKE, 8, None) == EINVAL
    assert lib.mi_spmm_rows_divide_f32(FAKE, -1, 8, FAKE, 8, FAKE, 8, None) == EINVAL
    gv = lib.mi_spmm_reduce_grad_val_f32
    assert gv(FAKE, FAKE, 10, 0, 4, 8, FAKE, 8, FAKE, 8, FAKE, 8, FAKE, None) == OK
    assert gv(FAKE, FAKE, 2 ** 31, 4, 4, 8, FAKE, 8, FAKE, 8, FAKE, 8, FAKE, None) == ERANGE
    assert gv(FAKE, FAKE, 10, 4, 4, 8, FAKE, 8, FAKE, 8, None, 8, FAKE, None) == EINVAL
    assert gv(FAKE, FAKE, 10, 4, 4, 8, FAKE, 8, FAKE, 8, FAKE, 8, None, None) == EINVAL
    gb = lib.mi_spmm_reduce_grad_b_f32
    assert gb(FAKE, FAKE, FAKE, FAKE, 10, 4, 0, 8, FAKE, 8, FAKE, 8, FAKE, 8, None) == OK
    assert gb(FAKE, FAKE, FAKE, FAKE, 2 ** 31, 4, 4, 8, FAKE, 8, FAKE, 8, FAKE, 8, None) == ERANGE
    assert gb(FAKE, FAKE, None, FAKE, 10, 4, 4, 8, FAKE, 8, FAKE, 8, FAKE, 8, None) == EINVAL
    assert gb(FAKE, FAKE, FAKE, FAKE, 10, 4, 4, 8, FAKE, 8, FAKE, 8, FAKE, 7, None) == EINVAL


def test_custom_mm_binds_the_reduce_entries(built):
    import custom_mm
    for name in ("naive_spmm_reduce", "spmm_rows_divide", "spmm_reduce_grad_val", "spmm_reduce_grad_b"):
        assert callable(getattr(custom_mm, name)), name
    a = torch.rand(2, 3).to_sparse_csr()
    args = (a.values(), a.col_indices().int(), a.crow_indices().int(), 6, 2, 3, torch.rand(3, 4), torch.zeros(2, 4))
    with pytest.raises(ValueError, match="reduce"):
        custom_mm.naive_spmm_reduce(*args, "max")
    for r in ("sum", "mean", "amax", "amin"):
        with pytest.raises(RuntimeError, match="device"):
            custom_mm.naive_spmm_reduce(*args, r)


def test_sparse_mm_reduce_refuses_what_it_cannot_run(built):
    import matmuls
    a = torch.rand(4, 5).to_sparse_csr()
    b = torch.rand(5, 3)
    for bad in ("max", "prod", "SUM", ""):
        with pytest.raises(ValueError, match="reduce"):
            matmuls.sparse_mm_reduce(a, b, bad)
    for r in matmuls.REDUCTIONS:
        with pytest.raises(RuntimeError, match="device"):  # host operands: no CPU fallback
            matmuls.sparse_mm_reduce(a, b, r)
        with pytest.raises(ValueError, match="CSR"):  # dense and COO mat1
            matmuls.sparse_mm_reduce(a.to_dense(), b, r)
        with pytest.raises(ValueError, match="CSR"):
            matmuls.sparse_mm_reduce(a.to_dense().to_sparse(), b, r)
        with pytest.raises(ValueError, match="CSR"):  # batched CSR
            matmuls.sparse_mm_reduce(torch.rand(2, 4, 5).to_sparse_csr(), b, r)
        with pytest.raises(ValueError, match="mat2"):
            matmuls.sparse_mm_reduce(a, b.double(), r)


def test_reduce_bindings_refuse_host_tensors_and_name_mixed_dtypes(built):
    import custom_mm
    a = torch.rand(2, 3).to_sparse_csr()
    vals, cols, offs = a.values(), a.col_indices().int(), a.crow_indices().int()
    B, G, arg, perm = torch.rand(3, 4), torch.rand(2, 4), torch.zeros(2, 4, dtype=torch.int32), torch.arange(6, dtype=torch.int32)
    t_offs = torch.tensor([0, 2, 4, 6], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.spmm_rows_divide(offs, 2, G, torch.empty(2, 4))
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.spmm_reduce_grad_val(cols, offs, 6, 2, 3, B, G, arg)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.spmm_reduce_grad_b(t_offs, cols, perm, vals, 6, 2, 3, G, arg)
    both = r"(?s)(?=.*\bFloat\b)(?=.*\bBFloat16\b)"  # checked before the device, so host tensors show it too
    for r in ("sum", "mean", "amax", "amin"):
        with pytest.raises(RuntimeError, match=both):
            custom_mm.naive_spmm_reduce(vals, cols, offs, 6, 2, 3, B.bfloat16(), torch.zeros(2, 4), r)
    with pytest.raises(RuntimeError, match=both):
        custom_mm.spmm_rows_divide(offs, 2, G, torch.empty(2, 4, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match=both):
        custom_mm.spmm_reduce_grad_val(cols, offs, 6, 2, 3, B, G.bfloat16(), arg)
    with pytest.raises(RuntimeError, match=both):
        custom_mm.spmm_reduce_grad_b(t_offs, cols, perm, vals, 6, 2, 3, G.bfloat16(), arg)
