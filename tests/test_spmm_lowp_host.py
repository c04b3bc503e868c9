"""bfloat16 / float16 CSR products without a GPU: the C-ABI declares and exports the low-precision entries, they validate
their arguments before any HIP call, custom_mm routes bf16 / fp16 operands to them (no CPU path, one dtype for every
operand), and matmuls refuses what it cannot run."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "mi_spmm.h"
NEW_ENTRIES = ("mi_spmm_csr_ex_bf16", "mi_spmm_csr_ex_f16", "mi_sddmm_csr_bf16", "mi_sddmm_csr_f16", "mi_gather_b16")
OK, EINVAL, ERANGE = 0, -1, -2
AUTO, NONE, SPLIT, PREPARED, AUTO_ZEROED = -1, 0, 1, 2, 3
LOWP = (torch.bfloat16, torch.float16)
# A non-null address that is never dereferenced: every call below must return before touching the device.
FAKE = 0x1000


@pytest.fixture(scope="module")
def lib(built):
    import torch  # noqa: F401  (torch's HIP runtime first, as in the product)
    lib = ctypes.CDLL(str(built / "libmi_spmm.so"))
    vp, i64, i32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_size_t
    for name in ("mi_spmm_csr_ex_bf16", "mi_spmm_csr_ex_f16"):
        getattr(lib, name).argtypes = [vp, vp, vp, i64, i32, i32, i32, vp, i64, vp, i64, ctypes.c_int, vp, sz, vp]
    for name in ("mi_sddmm_csr_bf16", "mi_sddmm_csr_f16"):
        getattr(lib, name).argtypes = [vp, vp, i64, i32, i32, i32, vp, i64, vp, i64, vp, vp]
    lib.mi_gather_b16.argtypes = [vp, vp, i64, vp, vp]
    return lib


def test_header_declares_the_low_precision_entries():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(rf"\b{name}\s*\(", text), name
    assert "#define MI_SPMM_ABI_VERSION 1" in text
    assert re.search(r"\bconst uint16_t\*\s*val\b", text)


def test_library_exports_the_low_precision_entries(lib):
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
    assert lib.mi_spmm_abi_version() == 1


def spmm_call(lib, name, *, nnz=10, M=4, K=4, N=8, rowptr=FAKE, col=FAKE, val=FAKE, B=FAKE, C=FAKE, ldb=None, ldc=None,
              mode=AUTO, ws=None, ws_bytes=0):
    return getattr(lib, name)(rowptr, col, val, nnz, M, K, N, B, ldb if ldb is not None else N, C,
                              ldc if ldc is not None else N, mode, ws, ws_bytes, None)


@pytest.mark.parametrize("name", ["mi_spmm_csr_ex_bf16", "mi_spmm_csr_ex_f16"])
def test_spmm_entries_validate_before_any_hip_call(lib, name):
    assert spmm_call(lib, name, mode=PREPARED) == EINVAL
    assert spmm_call(lib, name, mode=PREPARED, ws=FAKE, ws_bytes=1 << 20) == EINVAL
    for bad_mode in (-2, 4, 99):
        assert spmm_call(lib, name, mode=bad_mode) == EINVAL, bad_mode
    for kw in ({"M": -1}, {"K": -1}, {"N": -1}, {"nnz": -1}, {"ldb": 7}, {"ldc": 7}, {"rowptr": None}, {"C": None},
               {"col": None}, {"val": None}, {"B": None}, {"B": FAKE + 1}, {"C": FAKE + 1}):
        assert spmm_call(lib, name, **kw) == EINVAL, kw
    assert spmm_call(lib, name, nnz=2 ** 31) == ERANGE
    assert spmm_call(lib, name, M=0, rowptr=None, C=None) == OK
    assert spmm_call(lib, name, N=0, ldb=0, ldc=0) == OK
    # a product whose rows may be split needs a 16-byte-aligned workspace (AUTO and AUTO_ZEROED mean SPLIT here)
    for mode in (AUTO, SPLIT, AUTO_ZEROED):
        assert spmm_call(lib, name, nnz=100_000, mode=mode) == EINVAL, mode
        assert spmm_call(lib, name, nnz=100_000, mode=mode, ws=FAKE + 8, ws_bytes=1 << 30) == EINVAL, mode


@pytest.mark.parametrize("name", ["mi_sddmm_csr_bf16", "mi_sddmm_csr_f16"])
def test_sddmm_entries_validate_before_any_hip_call(lib, name):
    f = getattr(lib, name)
    assert f(FAKE, FAKE, 10, 0, 4, 8, FAKE, 8, FAKE, 8, FAKE, None) == OK
    assert f(FAKE, FAKE, 0, 4, 4, 8, FAKE, 8, FAKE, 8, FAKE, None) == OK
    assert f(FAKE, FAKE, 10, -1, 4, 8, FAKE, 8, FAKE, 8, FAKE, None) == EINVAL
    assert f(FAKE, FAKE, -1, 4, 4, 8, FAKE, 8, FAKE, 8, FAKE, None) == EINVAL
    assert f(FAKE, FAKE, 10, 4, 4, 8, FAKE, 7, FAKE, 8, FAKE, None) == EINVAL
    assert f(FAKE, FAKE, 10, 4, 4, 8, FAKE, 8, FAKE, 7, FAKE, None) == EINVAL
    assert f(None, FAKE, 10, 4, 4, 8, FAKE, 8, FAKE, 8, FAKE, None) == EINVAL
    assert f(FAKE, FAKE, 10, 4, 4, 8, FAKE, 8, None, 8, FAKE, None) == EINVAL
    assert f(FAKE, FAKE, 10, 4, 4, 8, FAKE, 8, FAKE, 8, None, None) == EINVAL


def test_gather_entry_validates_before_any_hip_call(lib):
    assert lib.mi_gather_b16(FAKE, FAKE, 0, FAKE, None) == OK
    assert lib.mi_gather_b16(FAKE, FAKE, -1, FAKE, None) == EINVAL
    assert lib.mi_gather_b16(None, FAKE, 4, FAKE, None) == EINVAL
    assert lib.mi_gather_b16(FAKE, None, 4, FAKE, None) == EINVAL
    assert lib.mi_gather_b16(FAKE, FAKE, 4, None, None) == EINVAL


def csr_args(dtype, b_dtype=None, c_dtype=None):
    a = torch.rand(4, 5).to_sparse_csr()
    vals = a.values().to(dtype)
    B = torch.rand(5, 3, dtype=b_dtype or dtype)
    C = torch.zeros(4, 3, dtype=c_dtype or dtype)
    return (vals, a.col_indices().int(), a.crow_indices().int(), vals.numel(), 4, 5, B, C)


def all_spmm_entries(custom_mm):
    return (custom_mm.naive_spmm, custom_mm.cusparse_mmul,
            lambda *a: custom_mm.naive_spmm_ex(*a, -1), lambda *a: custom_mm.naive_spmm_ex(*a, 0),
            lambda *a: custom_mm.naive_spmm_ex(*a, 1))


@pytest.mark.parametrize("dtype", LOWP)
def test_custom_mm_refuses_host_low_precision_tensors(built, dtype):
    import custom_mm
    for f in all_spmm_entries(custom_mm):
        with pytest.raises(RuntimeError, match="device"):
            f(*csr_args(dtype))
    vals, cols, offs, nnz, M, K, B, _ = csr_args(dtype)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.sddmm(cols, offs, nnz, M, K, torch.rand(M, 3, dtype=dtype), B)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.gather_perm(vals, torch.arange(nnz, dtype=torch.int32))


@pytest.mark.parametrize("a_dtype,b_dtype", [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32),
                                             (torch.bfloat16, torch.float16), (torch.float16, torch.bfloat16),
                                             (torch.float64, torch.half)])
def test_custom_mm_refuses_mixed_dtypes_naming_both(built, a_dtype, b_dtype):
    import custom_mm
    names = {torch.float32: "Float", torch.bfloat16: "BFloat16", torch.float16: "Half", torch.float64: "Double"}
    pattern = rf"(?s)(?=.*\b{names[a_dtype]}\b)(?=.*\b{names[b_dtype]}\b)"
    for f in all_spmm_entries(custom_mm):
        with pytest.raises(RuntimeError, match=pattern):
            f(*csr_args(a_dtype, b_dtype, b_dtype))
    _, cols, offs, nnz, M, K, _, _ = csr_args(a_dtype)
    with pytest.raises(RuntimeError, match=pattern):
        custom_mm.sddmm(cols, offs, nnz, M, K, torch.rand(M, 3, dtype=a_dtype), torch.rand(K, 3, dtype=b_dtype))


@pytest.mark.parametrize("dtype", LOWP)
def test_matmuls_refuses_a_host_low_precision_csr_operand(built, dtype):
    import matmuls
    a = torch.rand(4, 5).to_sparse_csr().to(dtype)
    b = torch.rand(5, 3, dtype=dtype)
    for f in (matmuls.naiveSpMM.apply, matmuls.cusparseMM.apply, matmuls.naive_matmul, matmuls.sparse_matmul):
        with pytest.raises(RuntimeError, match="device"):
            f(a, b)


@pytest.mark.parametrize("dtype", LOWP)
def test_matmuls_refuses_what_low_precision_does_not_cover(built, dtype):
    import matmuls
    a = torch.rand(4, 5).to_sparse_csr().to(dtype)
    b = torch.rand(5, 3, dtype=dtype)
    name = str(dtype).replace("torch.", "")
    for f in (matmuls.naive_matmul, matmuls.sparse_matmul):
        with pytest.raises(RuntimeError, match=name):  # mixed dtypes
            f(a, b.float())
        with pytest.raises(RuntimeError, match=name):
            f(torch.rand(4, 5).to_sparse_csr(), b)
        with pytest.raises(RuntimeError, match=rf"batched.*{name}"):
            f(torch.rand(2, 4, 5).to_sparse_csr().to(dtype), b)


def test_float32_only_entries_refuse_host_tensors_and_name_mixed_dtypes(built):
    """The entries without a bf16 / fp16 form apply the same dtype rule: one dtype for every value operand (named when mixed,
    before the device is looked at), then device tensors, then float32."""
    import custom_mm
    vals, cols, offs, nnz, M, K, B, C = csr_args(torch.float32)
    both = r"(?s)(?=.*\bFloat\b)(?=.*\bBFloat16\b)"
    bias = torch.rand(3)
    with pytest.raises(RuntimeError, match=both):
        custom_mm.naive_spmm_bias(vals, cols, offs, nnz, M, K, B.bfloat16(), bias, C)
    with pytest.raises(RuntimeError, match=both):
        custom_mm.naive_spmm_batched(vals, cols, offs, nnz, 1, M, K, B.bfloat16(), C[None])
    with pytest.raises(RuntimeError, match=both):
        custom_mm.naive_spmm_dense(torch.rand(M, K), B.bfloat16(), C)
    with pytest.raises(RuntimeError, match=both):
        custom_mm.spmm_plan(nnz, M, K, B.bfloat16(), C)
    for dtype in LOWP:
        with pytest.raises(RuntimeError, match="device"):
            custom_mm.naive_spmm_bias(vals.to(dtype), cols, offs, nnz, M, K, B.to(dtype), bias, C.to(dtype))
        with pytest.raises(RuntimeError, match="device"):
            custom_mm.csr_transpose(vals.to(dtype), cols, offs, nnz, M, K)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.validate_csr(vals, cols, offs, nnz, M, K)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.column_sums(C)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.gather_perm(vals, torch.arange(nnz, dtype=torch.int32))
