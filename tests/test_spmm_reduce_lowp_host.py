"""bfloat16 / float16 reduce = sum / mean / amax / amin on the CSR product without a GPU: the C-ABI declares and exports the
low-precision twins of the reduce entries, they validate their arguments before any HIP call, custom_mm routes bf16 / fp16
operands to them (one dtype for every operand, no CPU path), and matmuls.sparse_mm_reduce takes the dtype rule over."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "mi_spmm.h"
SUFFIXES = ("bf16", "f16")
NEW_ENTRIES = tuple(f"{stem}_{sfx}" for stem in ("mi_spmm_csr_reduce", "mi_spmm_rows_divide", "mi_spmm_reduce_grad_val",
                                                 "mi_spmm_reduce_grad_b") for sfx in SUFFIXES)
SUM, MEAN, AMAX, AMIN = 0, 1, 2, 3
OK, EINVAL, ERANGE, ENOMEM = 0, -1, -2, -4
LOWP = (torch.bfloat16, torch.float16)
NAMES = {torch.float32: "float32", torch.bfloat16: "bfloat16", torch.float16: "float16"}
# A non-null address that is never dereferenced: every call below must return before touching the device.
FAKE = 0x1000


@pytest.fixture(scope="module")
def lib(built):
    import torch  # noqa: F401  (torch's HIP runtime first, as in the product)
    lib = ctypes.CDLL(str(built / "libmi_spmm.so"))
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    for sfx in SUFFIXES:
        getattr(lib, f"mi_spmm_csr_reduce_{sfx}").argtypes = [vp, vp, vp, i64, i32, i32, i32, vp, i64, vp, i64, vp, i64,
                                                              ctypes.c_int, vp, ctypes.c_size_t, vp]
        getattr(lib, f"mi_spmm_rows_divide_{sfx}").argtypes = [vp, i32, i32, vp, i64, vp, i64, vp]
        getattr(lib, f"mi_spmm_reduce_grad_val_{sfx}").argtypes = [vp, vp, i64, i32, i32, i32, vp, i64, vp, i64, vp, i64, vp, vp]
        getattr(lib, f"mi_spmm_reduce_grad_b_{sfx}").argtypes = [vp, vp, vp, vp, i64, i32, i32, i32, vp, i64, vp, i64, vp, i64,
                                                                 vp]
    lib.mi_spmm_csr_reduce_workspace_bytes.argtypes = [i64, i32]
    lib.mi_spmm_csr_reduce_workspace_bytes.restype = ctypes.c_size_t
    return lib


def test_header_declares_the_low_precision_reduce_entries():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(rf"\b{name}\s*\(", text), name
    assert "#define MI_SPMM_ABI_VERSION 1" in text


def test_library_exports_the_low_precision_reduce_entries(lib):
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
    assert lib.mi_spmm_abi_version() == 1


def reduce_call(lib, sfx, reduce, *, nnz=10, M=4, K=4, N=8, arg=None, rowptr=FAKE, col=FAKE, val=FAKE, B=FAKE, C=FAKE,
                ldb=None, ldc=None, ldarg=None, ws=None, ws_bytes=0):
    return getattr(lib, f"mi_spmm_csr_reduce_{sfx}")(rowptr, col, val, nnz, M, K, N, B, ldb if ldb is not None else N, C,
                                                     ldc if ldc is not None else N, arg, ldarg if ldarg is not None else N,
                                                     reduce, ws, ws_bytes, None)


@pytest.mark.parametrize("sfx", SUFFIXES)
def test_reduce_entry_validates_before_any_hip_call(lib, sfx):
    for bad in (-1, 4, 99):
        assert reduce_call(lib, sfx, bad) == EINVAL, bad
    for r in (SUM, MEAN):
        assert reduce_call(lib, sfx, r, arg=FAKE) == EINVAL, r
    for r in (SUM, MEAN, AMAX, AMIN):
        assert reduce_call(lib, sfx, r, M=0) == OK, r
        assert reduce_call(lib, sfx, r, M=0, rowptr=None, C=None) == OK, r
        assert reduce_call(lib, sfx, r, N=0, ldb=0, ldc=0) == OK, r
        assert reduce_call(lib, sfx, r, nnz=2 ** 31) == ERANGE, r
        for kw in ({"rowptr": None}, {"C": None}, {"col": None}, {"val": None}, {"B": None}, {"ldb": 7}, {"ldc": 7},
                   {"M": -1}, {"K": -1}, {"N": -1}, {"nnz": -1},
                   {"B": FAKE + 1}, {"C": FAKE + 1}, {"val": FAKE + 1}):  # 2-byte alignment
            assert reduce_call(lib, sfx, r, **kw) == EINVAL, (r, kw)
    for r in (AMAX, AMIN):
        assert reduce_call(lib, sfx, r, arg=FAKE, ldarg=7) == EINVAL, r  # an arg buffer narrower than N
        # a hub-row workspace that is too small, or not 16-byte aligned
        need = lib.mi_spmm_csr_reduce_workspace_bytes(100_000, 8)
        assert need > 16
        assert reduce_call(lib, sfx, r, nnz=100_000, ws=FAKE, ws_bytes=16) == ENOMEM, r
        assert reduce_call(lib, sfx, r, nnz=100_000, ws=FAKE + 8, ws_bytes=need) == EINVAL, r


@pytest.mark.parametrize("sfx", SUFFIXES)
def test_divide_and_gradient_entries_validate_before_any_hip_call(lib, sfx):
    div = getattr(lib, f"mi_spmm_rows_divide_{sfx}")
    assert div(FAKE, 0, 8, None, 8, None, 8, None) == OK
    assert div(FAKE, 4, 0, None, 8, None, 8, None) == OK
    assert div(None, 4, 8, FAKE, 8, FAKE, 8, None) == EINVAL
    assert div(FAKE, 4, 8, None, 8, FAKE, 8, None) == EINVAL
    assert div(FAKE, 4, 8, FAKE, 8, None, 8, None) == EINVAL
    assert div(FAKE, 4, 8, FAKE, 7, FAKE, 8, None) == EINVAL
    assert div(FAKE, 4, 8, FAKE, 8, FAKE, 7, None) == EINVAL
    assert div(FAKE, -1, 8, FAKE, 8, FAKE, 8, None) == EINVAL
    assert div(FAKE, 4, 8, FAKE + 1, 8, FAKE, 8, None) == EINVAL
    gv = getattr(lib, f"mi_spmm_reduce_grad_val_{sfx}")
    assert gv(FAKE, FAKE, 10, 0, 4, 8, FAKE, 8, FAKE, 8, FAKE, 8, FAKE, None) == OK
    assert gv(FAKE, FAKE, 0, 4, 4, 8, FAKE, 8, FAKE, 8, FAKE, 8, FAKE, None) == OK
    assert gv(FAKE, FAKE, 2 ** 31, 4, 4, 8, FAKE, 8, FAKE, 8, FAKE, 8, FAKE, None) == ERANGE
    assert gv(None, FAKE, 10, 4, 4, 8, FAKE, 8, FAKE, 8, FAKE, 8, FAKE, None) == EINVAL
    assert gv(FAKE, FAKE, 10, 4, 4, 8, None, 8, FAKE, 8, FAKE, 8, FAKE, None) == EINVAL
    assert gv(FAKE, FAKE, 10, 4, 4, 8, FAKE, 8, None, 8, FAKE, 8, FAKE, None) == EINVAL
    assert gv(FAKE, FAKE, 10, 4, 4, 8, FAKE, 8, FAKE, 8, None, 8, FAKE, None) == EINVAL
    assert gv(FAKE, FAKE, 10, 4, 4, 8, FAKE, 8, FAKE, 8, FAKE, 8, None, None) == EINVAL
    assert gv(FAKE, FAKE, 10, 4, 4, 8, FAKE, 7, FAKE, 8, FAKE, 8, FAKE, None) == EINVAL
    assert gv(FAKE, FAKE, 10, 4, 4, 8, FAKE, 8, FAKE, 7, FAKE, 8, FAKE, None) == EINVAL
    assert gv(FAKE, FAKE, 10, 4, 4, 8, FAKE, 8, FAKE, 8, FAKE, 7, FAKE, None) == EINVAL
    assert gv(FAKE, FAKE, 10, 4, 4, 8, FAKE + 1, 8, FAKE, 8, FAKE, 8, FAKE, None) == EINVAL
    gb = getattr(lib, f"mi_spmm_reduce_grad_b_{sfx}")
    assert gb(FAKE, FAKE, FAKE, FAKE, 10, 4, 0, 8, FAKE, 8, FAKE, 8, FAKE, 8, None) == OK
    assert gb(FAKE, FAKE, FAKE, FAKE, 2 ** 31, 4, 4, 8, FAKE, 8, FAKE, 8, FAKE, 8, None) == ERANGE
    assert gb(None, FAKE, FAKE, FAKE, 10, 4, 4, 8, FAKE, 8, FAKE, 8, FAKE, 8, None) == EINVAL
    assert gb(FAKE, FAKE, None, FAKE, 10, 4, 4, 8, FAKE, 8, FAKE, 8, FAKE, 8, None) == EINVAL
    assert gb(FAKE, FAKE, FAKE, None, 10, 4, 4, 8, FAKE, 8, FAKE, 8, FAKE, 8, None) == EINVAL
    assert gb(FAKE, FAKE, FAKE, FAKE, 10, 4, 4, 8, FAKE, 8, FAKE, 8, None, 8, None) == EINVAL
    assert gb(FAKE, FAKE, FAKE, FAKE, 10, 4, 4, 8, FAKE, 7, FAKE, 8, FAKE, 8, None) == EINVAL
    assert gb(FAKE, FAKE, FAKE, FAKE, 10, 4, 4, 8, FAKE, 8, FAKE, 7, FAKE, 8, None) == EINVAL
    assert gb(FAKE, FAKE, FAKE, FAKE, 10, 4, 4, 8, FAKE, 8, FAKE, 8, FAKE, 7, None) == EINVAL
    assert gb(FAKE, FAKE, FAKE, FAKE, 10, 4, 4, 8, FAKE, 8, FAKE, 8, FAKE + 1, 8, None) == EINVAL


@pytest.mark.parametrize("dtype", LOWP)
def test_custom_mm_refuses_host_low_precision_operands(built, dtype):
    import custom_mm
    a = torch.rand(2, 3).to_sparse_csr()
    vals, cols, offs = a.values().to(dtype), a.col_indices().int(), a.crow_indices().int()
    B, G = torch.rand(3, 4, dtype=dtype), torch.rand(2, 4, dtype=dtype)
    arg, perm = torch.zeros(2, 4, dtype=torch.int32), torch.arange(6, dtype=torch.int32)
    t_offs = torch.tensor([0, 2, 4, 6], dtype=torch.int32)
    for r in ("sum", "mean", "amax", "amin"):
        with pytest.raises(RuntimeError, match="device"):
            custom_mm.naive_spmm_reduce(vals, cols, offs, 6, 2, 3, B, torch.zeros(2, 4, dtype=dtype), r)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.spmm_rows_divide(offs, 2, G, torch.empty(2, 4, dtype=dtype))
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.spmm_reduce_grad_val(cols, offs, 6, 2, 3, B, G, arg)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.spmm_reduce_grad_b(t_offs, cols, perm, vals, 6, 2, 3, G, arg)


def test_custom_mm_names_both_dtypes_of_mixed_low_precision_operands(built):
    import custom_mm
    a = torch.rand(2, 3).to_sparse_csr()
    cols, offs = a.col_indices().int(), a.crow_indices().int()
    both = r"(?s)(?=.*\bBFloat16\b)(?=.*\bHalf\b)"  # checked before the device, so host tensors show it
    bf, hf = torch.bfloat16, torch.float16
    for r in ("sum", "mean", "amax", "amin"):
        with pytest.raises(RuntimeError, match=both):
            custom_mm.naive_spmm_reduce(a.values().to(bf), cols, offs, 6, 2, 3, torch.rand(3, 4, dtype=hf),
                                        torch.zeros(2, 4, dtype=hf), r)
    with pytest.raises(RuntimeError, match=both):
        custom_mm.spmm_rows_divide(offs, 2, torch.rand(2, 4, dtype=bf), torch.empty(2, 4, dtype=hf))
    with pytest.raises(RuntimeError, match=r"(?s)(?=.*\bDouble\b)(?=.*\bHalf\b)"):
        custom_mm.spmm_rows_divide(offs, 2, torch.rand(2, 4, dtype=torch.float64), torch.empty(2, 4, dtype=hf))


@pytest.mark.parametrize("dtype", LOWP)
def test_sparse_mm_reduce_refuses_host_low_precision_operands(built, dtype):
    import matmuls
    a = torch.rand(4, 5).to_sparse_csr().to(dtype)
    b = torch.rand(5, 3, dtype=dtype)
    for r in matmuls.REDUCTIONS:
        with pytest.raises(RuntimeError, match="device"):  # no CPU path in any dtype
            matmuls.sparse_mm_reduce(a, b, r)
        with pytest.raises(ValueError, match="mat2"):
            matmuls.sparse_mm_reduce(a, b.double(), r)
        with pytest.raises(ValueError, match="CSR"):
            matmuls.sparse_mm_reduce(a.to_dense(), b, r)


@pytest.mark.parametrize("d1,d2", [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32),
                                   (torch.float16, torch.bfloat16), (torch.float16, torch.float32)])
def test_sparse_mm_reduce_names_both_dtypes_when_they_differ(built, d1, d2):
    import matmuls
    a = torch.rand(4, 5).to_sparse_csr().to(d1)
    b = torch.rand(5, 3, dtype=d2)
    for r in matmuls.REDUCTIONS:
        with pytest.raises(RuntimeError, match=rf"(?s)(?=.*\b{NAMES[d1]}\b)(?=.*\b{NAMES[d2]}\b)"):
            matmuls.sparse_mm_reduce(a, b, r)
