"""bfloat16 / float16 dense products without a GPU: the C-ABI declares and exports mi_gemm_bf16 / mi_gemm_f16, they
validate their arguments before any HIP call, and custom_mm's dense entries refuse host low-precision tensors ("device")
and mixed dtypes (naming both), whatever the device."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "mi_spmm.h"
ENTRIES = ("mi_gemm_bf16", "mi_gemm_f16")
OK, EINVAL = 0, -1
LOWP = (torch.bfloat16, torch.float16)
# A non-null address that is never dereferenced: every call below must return before touching the device.
FAKE = 0x1000


@pytest.fixture(scope="module")
def lib(built):
    import torch  # noqa: F401  (torch's HIP runtime first, as in the product)
    lib = ctypes.CDLL(str(built / "libmi_spmm.so"))
    vp, i64, i32, c_int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int
    for name in ENTRIES:
        f = getattr(lib, name)
        f.argtypes = [c_int, c_int, i32, i32, i32, vp, i64, i64, vp, i64, i64, vp, i64, i64, i32, vp]
        f.restype = c_int
    return lib


def test_header_declares_the_dense_low_precision_entries():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in ENTRIES:
        m = re.search(rf"\bint\s+{name}\s*\(([^;]*)\)\s*;", text)
        assert m, name
        args = m.group(1)
        assert re.search(r"const uint16_t\*\s*A\b", args) and re.search(r"const uint16_t\*\s*B\b", args), name
        assert re.search(r"\buint16_t\*\s*C\b", args), name
    assert "#define MI_SPMM_ABI_VERSION 1" in text


def test_library_exports_the_dense_low_precision_entries(built):
    lib = ctypes.CDLL(str(built / "libmi_spmm.so"))
    for name in ENTRIES:
        assert hasattr(lib, name), name


def call(lib, name, transa=0, transb=0, m=4, n=4, k=4, A=FAKE, lda=None, sA=0, B=FAKE, ldb=None, sB=0, C=FAKE, ldc=None,
         sC=0, batch=1):
    lda = (m if transa else k) if lda is None else lda
    ldb = (k if transb else n) if ldb is None else ldb
    ldc = n if ldc is None else ldc
    return getattr(lib, name)(transa, transb, m, n, k, A, lda, sA, B, ldb, sB, C, ldc, sC, batch, None)


@pytest.mark.parametrize("name", ENTRIES)
def test_entries_validate_before_any_hip_call(lib, name):
    for kw in (dict(m=-1), dict(n=-1), dict(k=-1), dict(batch=-1), dict(sA=-1), dict(sB=-1), dict(sC=-1)):
        assert call(lib, name, **kw) == EINVAL, kw
    # leading dimensions shorter than the stored rows
    assert call(lib, name, m=8, k=16, lda=15) == EINVAL                 # lda < k (A plain)
    assert call(lib, name, transa=1, m=8, k=16, lda=7) == EINVAL        # lda < m (A stored transposed)
    assert call(lib, name, n=8, k=16, ldb=7) == EINVAL                  # ldb < n (B plain)
    assert call(lib, name, transb=1, n=8, k=16, ldb=15) == EINVAL       # ldb < k (B stored transposed)
    assert call(lib, name, n=8, ldc=7) == EINVAL
    # null and odd pointers
    assert call(lib, name, A=None) == EINVAL
    assert call(lib, name, B=None) == EINVAL
    assert call(lib, name, C=None) == EINVAL
    assert call(lib, name, A=FAKE + 1) == EINVAL
    assert call(lib, name, C=FAKE + 1) == EINVAL
    # empty products: nothing to launch, even with null operands
    assert call(lib, name, m=0, A=None, B=None, C=None) == OK
    assert call(lib, name, n=0, A=None, B=None, C=None) == OK
    assert call(lib, name, batch=0, A=None, B=None, C=None) == OK


def test_abi_version_stays_1(lib):
    assert lib.mi_spmm_abi_version() == 1


@pytest.mark.parametrize("dtype", LOWP)
def test_custom_mm_refuses_host_low_precision_tensors(built, dtype):
    import custom_mm
    a, b, c = torch.rand(2, 3, dtype=dtype), torch.rand(3, 4, dtype=dtype), torch.zeros(2, 4, dtype=dtype)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.cublas_mmul(a, b, c, False, False)
    for dim, lead in ((3, (2,)), (4, (2, 3))):
        with pytest.raises(RuntimeError, match="device"):
            custom_mm.cublas_bmm(a.expand(*lead, 2, 3), b.expand(*lead, 3, 4), c.expand(*lead, 2, 4).contiguous(), dim,
                                 False, False)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.cublas_bmm(a, b, c, 2, False, False)


NAMES = {torch.float32: "Float", torch.bfloat16: "BFloat16", torch.float16: "Half", torch.float64: "Double"}
MIXED = [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32), (torch.bfloat16, torch.float16),
         (torch.float16, torch.bfloat16), (torch.float16, torch.float32)]


def _devices():
    return ["cpu"] + (["cuda"] if torch.cuda.is_available() else [])


@pytest.mark.parametrize("a_dtype,b_dtype", MIXED)
@pytest.mark.parametrize("device", _devices())
def test_custom_mm_refuses_mixed_dtypes_naming_both(built, a_dtype, b_dtype, device):
    import custom_mm
    pattern = rf"(?s)(?=.*\b{NAMES[a_dtype]}\b)(?=.*\b{NAMES[b_dtype]}\b)"
    a = torch.rand(2, 3, dtype=a_dtype, device=device)
    b = torch.rand(3, 4, dtype=b_dtype, device=device)
    for c_dtype in (a_dtype, b_dtype):
        c = torch.zeros(2, 4, dtype=c_dtype, device=device)
        with pytest.raises(RuntimeError, match=pattern):
            custom_mm.cublas_mmul(a, b, c, False, False)
        with pytest.raises(RuntimeError, match=pattern):
            custom_mm.cublas_bmm(a[None], b[None], c[None], 3, False, False)
        with pytest.raises(RuntimeError, match=pattern):
            custom_mm.cublas_bmm(a[None, None], b[None, None], c[None, None], 4, False, False)
    # a bf16 / fp16 A and B with a float32 C: refused, naming both
    if a_dtype == b_dtype:
        return
    lowp = a_dtype if a_dtype != torch.float32 else b_dtype
    pattern = rf"(?s)(?=.*\b{NAMES[lowp]}\b)(?=.*\bFloat\b)"
    with pytest.raises(RuntimeError, match=pattern):
        custom_mm.cublas_mmul(a.to(lowp), b.to(lowp), torch.zeros(2, 4, device=device), False, False)


@pytest.mark.parametrize("dtype", LOWP)
def test_float32_only_dense_entries_stay_float32(built, dtype):
    """The fused bias epilogue keeps its float32-only refusal, on the host too."""
    import custom_mm
    a, b = torch.rand(2, 3, dtype=dtype), torch.rand(3, 4, dtype=dtype)
    with pytest.raises(RuntimeError):
        custom_mm.cublas_mmul_bias(a, b, torch.rand(4, dtype=dtype), torch.zeros(2, 4, dtype=dtype), False, False)


@pytest.mark.parametrize("dtype", LOWP)
def test_custom_matmul_refuses_mixed_dtypes_naming_both(built, dtype):
    import matmuls
    name = str(dtype).replace("torch.", "")
    for other in (torch.float32, (set(LOWP) - {dtype}).pop()):
        a, b = torch.rand(4, 5, dtype=dtype), torch.rand(5, 3, dtype=other)
        oname = str(other).replace("torch.", "")
        for x, y in ((a, b), (b.t().contiguous(), a.t().contiguous())):
            with pytest.raises(RuntimeError, match=rf"(?s)(?=.*{name})(?=.*{oname})"):
                matmuls.custom_matmul(x.unsqueeze(0).expand(2, -1, -1), y.unsqueeze(0).expand(2, -1, -1))
