"""bfloat16 / float16 FC layers without a GPU: the C-ABI declares and exports the bias epilogue, the
split-k entries and the column sums; each validates its arguments before any HIP call; the split rule is a function of
the shape alone; custom_mm and fc_layers refuse host tensors ("device") and mixed dtypes (naming both)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "mi_spmm.h"
BIAS = ("mi_gemm_bias_bf16", "mi_gemm_bias_f16")
WS = ("mi_gemm_ws_bf16", "mi_gemm_ws_f16")
SPLIT = ("mi_gemm_split_bf16", "mi_gemm_split_f16")
COLSUM = ("mi_colsum_bf16", "mi_colsum_f16")
INT_ENTRIES = BIAS + WS + SPLIT + COLSUM + ("mi_gemm_lowp_split_count",)
OK, EINVAL, ENOMEM = 0, -1, -4
LOWP = (torch.bfloat16, torch.float16)
NAMES = {torch.float32: "Float", torch.bfloat16: "BFloat16", torch.float16: "Half"}
# A non-null, 16-byte-aligned address that is never dereferenced: every call below must return before touching the device.
FAKE = 0x1000


@pytest.fixture(scope="module")
def lib(built):
    import torch  # noqa: F401  (torch's HIP runtime first, as in the product)
    lib = ctypes.CDLL(str(built / "libmi_spmm.so"))
    vp, i64, i32, c_int, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int, ctypes.c_size_t
    head = [c_int, c_int, i32, i32, i32, vp, i64, i64, vp, i64, i64, vp, vp, i64, i64, i32]
    for name in BIAS:
        getattr(lib, name).argtypes = head + [vp]
    for name in WS:
        getattr(lib, name).argtypes = head + [vp, sz, vp]
    for name in SPLIT:
        getattr(lib, name).argtypes = [c_int, c_int, i32, i32, i32, vp, i64, vp, i64, vp, vp, i64, i32, vp, sz, vp]
    for name in COLSUM:
        getattr(lib, name).argtypes = [vp, i32, i32, i64, vp, vp, sz, vp]
    lib.mi_gemm_lowp_split_count.argtypes = [i32] * 4
    lib.mi_gemm_lowp_workspace_bytes.argtypes = [i32] * 4
    lib.mi_gemm_lowp_workspace_bytes.restype = sz
    lib.mi_colsum_workspace_bytes.argtypes = [i32, i32]
    lib.mi_colsum_workspace_bytes.restype = sz
    assert lib.mi_status_string is not None
    return lib


def test_status_codes_are_the_headers():
    text = HEADER.read_text()
    assert re.search(r"\bMI_EINVAL = -1,", text) and re.search(r"\bMI_ENOMEM = -4,", text)


def test_header_declares_the_entries():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in INT_ENTRIES:
        assert re.search(rf"\bint\s+{name}\s*\(([^;]*)\)\s*;", text), name
    assert re.search(r"\bsize_t\s+mi_gemm_lowp_workspace_bytes\s*\(", text)
    for name in BIAS + WS + SPLIT:
        args = re.search(rf"\bint\s+{name}\s*\(([^;]*)\)\s*;", text).group(1)
        assert re.search(r"const uint16_t\*\s*bias\b[^;]*\buint16_t\*\s*C\b", args, flags=re.S), name  # bias before C
    assert "#define MI_SPMM_ABI_VERSION 1" in text


def test_library_exports_the_entries(lib):
    for name in INT_ENTRIES + ("mi_gemm_lowp_workspace_bytes",):
        assert hasattr(lib, name), name
    assert lib.mi_spmm_abi_version() == 1


def call(lib, name, transa=0, transb=0, m=4, n=4, k=4, A=FAKE, lda=None, sA=0, B=FAKE, ldb=None, sB=0, bias=FAKE, C=FAKE,
         ldc=None, sC=0, batch=1, ws=None, ws_bytes=0):
    lda = (m if transa else k) if lda is None else lda
    ldb = (k if transb else n) if ldb is None else ldb
    ldc = n if ldc is None else ldc
    args = [transa, transb, m, n, k, A, lda, sA, B, ldb, sB, bias, C, ldc, sC, batch]
    if name in WS:
        args += [ws, ws_bytes]
    return getattr(lib, name)(*args, None)


@pytest.mark.parametrize("name", BIAS + WS)
def test_gemm_entries_validate_before_any_hip_call(lib, name):
    for kw in (dict(m=-1), dict(n=-1), dict(k=-1), dict(batch=-1), dict(sA=-1), dict(sB=-1), dict(sC=-1)):
        assert call(lib, name, **kw) == EINVAL, kw
    assert call(lib, name, m=8, k=16, lda=15) == EINVAL                 # lda < k (A plain)
    assert call(lib, name, transa=1, m=8, k=16, lda=7) == EINVAL        # lda < m (A stored transposed)
    assert call(lib, name, n=8, k=16, ldb=7) == EINVAL                  # ldb < n (B plain)
    assert call(lib, name, transb=1, n=8, k=16, ldb=15) == EINVAL       # ldb < k (B stored transposed)
    assert call(lib, name, n=8, ldc=7) == EINVAL
    for kw in (dict(A=None), dict(B=None), dict(C=None), dict(A=FAKE + 1), dict(B=FAKE + 1), dict(C=FAKE + 1),
               dict(bias=FAKE + 1), dict(bias=None, C=FAKE + 1)):
        assert call(lib, name, **kw) == EINVAL, kw
    for kw in (dict(m=0), dict(n=0), dict(batch=0)):
        assert call(lib, name, A=None, B=None, C=None, bias=None, **kw) == OK, kw


@pytest.mark.parametrize("name", WS)
def test_split_needs_its_workspace(lib, name):
    m, n, k = 768, 3072, 16384
    S = lib.mi_gemm_lowp_split_count(m, n, k, 1)
    need = lib.mi_gemm_lowp_workspace_bytes(m, n, k, 1)
    assert S > 1 and need == S * m * n * 4
    shape = dict(transa=1, m=m, n=n, k=k)
    assert call(lib, name, ws=None, ws_bytes=need, **shape) == EINVAL
    assert call(lib, name, ws=FAKE + 4, ws_bytes=need, **shape) == EINVAL      # not 16-byte aligned
    assert call(lib, name, ws=FAKE, ws_bytes=need - 1, **shape) == ENOMEM      # never a silent unsplit product
    assert call(lib, name, ws=FAKE, ws_bytes=0, **shape) == ENOMEM
    assert call(lib, name, ws=FAKE, ws_bytes=need, bias=FAKE + 1, **shape) == EINVAL
    assert call(lib, name, ws=FAKE, ws_bytes=need, C=None, **shape) == EINVAL


@pytest.mark.parametrize("name", SPLIT)
def test_explicit_split_validates(lib, name):
    f = getattr(lib, name)

    def go(m=128, n=128, k=4096, A=FAKE, lda=None, B=FAKE, ldb=None, bias=None, C=FAKE, ldc=None, S=4, ws=FAKE, wsb=None):
        wsb = S * m * n * 4 if wsb is None else wsb
        return f(0, 0, m, n, k, A, k if lda is None else lda, B, n if ldb is None else ldb, bias, C, n if ldc is None else ldc,
                 S, ws, wsb, None)

    assert go(S=0) == EINVAL and go(S=-2) == EINVAL
    assert go(k=4096 + 64, S=4) == EINVAL          # ranges must be whole 32-deep steps
    assert go(k=96, S=2) == EINVAL
    assert go(m=-1) == EINVAL and go(lda=4095) == EINVAL and go(ldc=127) == EINVAL
    assert go(A=None) == EINVAL and go(C=FAKE + 1) == EINVAL and go(bias=FAKE + 1) == EINVAL
    assert go(ws=None) == EINVAL and go(wsb=4 * 128 * 128 * 4 - 1) == ENOMEM
    assert go(m=0, A=None, B=None, C=None) == OK


@pytest.mark.parametrize("name", COLSUM)
def test_colsum_validates(lib, name):
    f = getattr(lib, name)
    need = lib.mi_colsum_workspace_bytes(64, 8)
    assert f(FAKE, -1, 8, 8, FAKE, FAKE, need, None) == EINVAL
    assert f(FAKE, 64, -1, 8, FAKE, FAKE, need, None) == EINVAL
    assert f(None, 64, 0, 8, None, None, 0, None) == OK
    assert f(FAKE, 64, 8, 8, None, FAKE, need, None) == EINVAL
    assert f(None, 64, 8, 8, FAKE, FAKE, need, None) == EINVAL
    assert f(FAKE, 64, 8, 7, FAKE, FAKE, need, None) == EINVAL          # ld < n
    assert f(FAKE + 1, 64, 8, 8, FAKE, FAKE, need, None) == EINVAL      # odd pointers
    assert f(FAKE, 64, 8, 8, FAKE + 1, FAKE, need, None) == EINVAL
    assert f(FAKE, 64, 8, 8, FAKE, None, need, None) == EINVAL
    assert f(FAKE, 64, 8, 8, FAKE, FAKE, need - 1, None) == ENOMEM


def test_split_count_is_a_function_of_the_shape(lib):
    g = np.random.Generator(np.random.PCG64(10))
    count, ws_bytes = lib.mi_gemm_lowp_split_count, lib.mi_gemm_lowp_workspace_bytes
    sizes = [1, 7, 64, 128, 255, 256, 768, 1000, 1536, 3072, 4096]
    ks = [0, 1, 31, 32, 1000, 2048, 4096, 4100, 8192, 16384, 16416, 65536, 100000]
    split = 0
    for _ in range(4000):
        m, n = (int(x) for x in g.choice(sizes, 2))
        k = int(g.choice(ks)) if g.random() < 0.7 else int(g.integers(0, 1 << 17))
        batch = int(g.choice([1, 1, 1, 2, 12]))
        S = count(m, n, k, batch)
        assert S >= 1 and count(m, n, k, batch) == S, (m, n, k, batch)
        if batch != 1:
            assert S == 1, (m, n, k, batch)
        if S > 1:
            split += 1
            assert k % (32 * S) == 0, (m, n, k, S)
        assert ws_bytes(m, n, k, batch) == (S * m * n * 4 if S > 1 else 0), (m, n, k, batch)
    assert split > 100  # the grid does reach the rule
    for shape in ((0, 5, 4096, 1), (5, 0, 4096, 1), (-1, 5, 4096, 1), (5, -1, 4096, 1), (5, 5, 0, 1), (5, 5, -4096, 1),
                  (5, 5, 4096, 0), (5, 5, 4096, -1)):
        assert count(*shape) == 1 and ws_bytes(*shape) == 0, shape
    assert count(768, 3072, 16384, 1) > 1      # the FC weight gradient, the shape the feature exists for
    assert count(3072, 768, 16384, 1) > 1
    assert count(768, 3072, 16384, 2) == 1


@pytest.mark.parametrize("dtype", LOWP)
def test_custom_mm_refuses_host_tensors(built, dtype):
    import custom_mm
    a, b, c = torch.rand(2, 3, dtype=dtype), torch.rand(3, 4, dtype=dtype), torch.zeros(2, 4, dtype=dtype)
    bias = torch.rand(4, dtype=dtype)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.cublas_mmul_bias(a, b, bias, c, False, False)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.column_sums(c)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.cublas_mmul_splitk(a, b, c, False, False)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.cublas_mmul_splitk(a, b, c, False, False, bias)
    assert bool((c == 0).all())


@pytest.mark.parametrize("dtype", LOWP)
def test_custom_mm_names_both_dtypes(built, dtype):
    import custom_mm
    other = torch.float16 if dtype == torch.bfloat16 else torch.bfloat16
    a, b, c = torch.rand(2, 3, dtype=dtype), torch.rand(3, 4, dtype=dtype), torch.zeros(2, 4, dtype=dtype)
    for bad in (torch.float32, other):
        pattern = rf"(?s)(?=.*\b{NAMES[dtype]}\b)(?=.*\b{NAMES[bad]}\b)"
        with pytest.raises(RuntimeError, match=pattern):
            custom_mm.cublas_mmul_bias(a, b, torch.rand(4).to(bad), c, False, False)
        with pytest.raises(RuntimeError, match=pattern):
            custom_mm.cublas_mmul_bias(a, b.to(bad), torch.rand(4).to(dtype), c, False, False)
        with pytest.raises(RuntimeError, match=pattern):
            custom_mm.cublas_mmul_splitk(a.to(bad), b, c, False, False)
        with pytest.raises(RuntimeError, match=pattern):
            custom_mm.cublas_mmul_splitk(a, b, c, False, False, torch.rand(4).to(bad))
    assert bool((c == 0).all())
    assert custom_mm.gemm_lowp_split_count(768, 3072, 16384) > 1 and custom_mm.gemm_lowp_split_count(8, 8, 64) == 1


@pytest.mark.parametrize("cls", ["cublasLinear", "cusparseLinear"])
@pytest.mark.parametrize("dtype", LOWP)
def test_layers_name_both_dtypes_before_anything_runs(built, cls, dtype):
    import fc_layers
    name = str(dtype).replace("torch.", "")
    pattern = rf"(?s)(?=.*{name})(?=.*float32)"
    layer = getattr(fc_layers, cls)(8, 4).to(dtype)
    with pytest.raises(RuntimeError, match=pattern):
        layer(torch.rand(3, 8))                                   # a float32 input into a T layer
    layer32 = getattr(fc_layers, cls)(8, 4)
    with pytest.raises(RuntimeError, match=pattern):
        layer32(torch.rand(3, 8).to(dtype))                       # and the reverse
    with pytest.raises(RuntimeError, match="device"):
        layer(torch.rand(3, 8).to(dtype))                         # a T host input reaches custom_mm, which has no CPU path
