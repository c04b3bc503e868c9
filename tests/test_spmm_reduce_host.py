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
OK, EINVAL, ERANGE, ENOMEM = 0, -1, -2, -4
DTYPES = ("f32", "bf16", "f16")


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
    for sfx in DTYPES[1:]:  # the 16-bit twins take the same argument lists
        for stem in ("mi_spmm_csr_reduce", "mi_spmm_rows_divide", "mi_spmm_reduce_grad_val", "mi_spmm_reduce_grad_b"):
            getattr(lib, f"{stem}_{sfx}").argtypes = getattr(lib, f"{stem}_f32").argtypes
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


# One argument list per entry, every pointer FAKE and every size consistent; a case overrides some of them.
def call_reduce(lib, sfx, *, reduce=AMAX, nnz=10, M=4, K=4, N=8, rowptr=FAKE, col=FAKE, val=FAKE, B=FAKE, ldb=8, C=FAKE,
                ldc=8, arg=None, ldarg=8, ws=None, ws_bytes=0):
    return getattr(lib, f"mi_spmm_csr_reduce_{sfx}")(rowptr, col, val, nnz, M, K, N, B, ldb, C, ldc, arg, ldarg, reduce, ws,
                                                     ws_bytes, None)


def call_divide(lib, sfx, *, M=4, N=8, rowptr=FAKE, src=FAKE, ldin=8, out=FAKE, ldout=8):
    return getattr(lib, f"mi_spmm_rows_divide_{sfx}")(rowptr, M, N, src, ldin, out, ldout, None)


def call_grad_val(lib, sfx, *, nnz=10, M=4, K=4, N=8, rowptr=FAKE, col=FAKE, B=FAKE, ldb=8, G=FAKE, ldg=8, arg=FAKE,
                  ldarg=8, grad_val=FAKE):
    return getattr(lib, f"mi_spmm_reduce_grad_val_{sfx}")(rowptr, col, nnz, M, K, N, B, ldb, G, ldg, arg, ldarg, grad_val, None)


def call_grad_b(lib, sfx, *, nnz=10, M=4, K=4, N=8, t_rowptr=FAKE, t_col=FAKE, perm=FAKE, val=FAKE, G=FAKE, ldg=8, arg=FAKE,
                ldarg=8, grad_b=FAKE, ldgb=8):
    return getattr(lib, f"mi_spmm_reduce_grad_b_{sfx}")(t_rowptr, t_col, perm, val, nnz, M, K, N, G, ldg, arg, ldarg, grad_b,
                                                        ldgb, None)


BIG = 2 ** 31            # the first nnz that does not fit the kernels' 32-bit entry index
HUB = dict(nnz=100_000)  # enough entries for the hub-row workspace to be looked at
ROOMY = 1 << 40          # a workspace size that is enough for HUB
# (what is wrong and what else is wrong after it, arguments, status): every case but the plain ones carries a second
# mistake that a LATER check would answer differently, so the order of the checks shows in the status.
SHARED_CASES = {
    "reduce": (call_reduce, [
        ("bad reduce code; nnz >= 2^31", dict(reduce=99, nnz=BIG), EINVAL),
        ("bad reduce code; empty call", dict(reduce=-1, M=0), EINVAL),
        ("arg with sum; nnz >= 2^31", dict(reduce=SUM, arg=FAKE, nnz=BIG), EINVAL),
        ("arg with mean; empty call", dict(reduce=MEAN, arg=FAKE, M=0), EINVAL),
        ("negative size; nnz >= 2^31", dict(K=-1, nnz=BIG), EINVAL),
        ("negative size; empty call", dict(N=-1, M=0), EINVAL),
        ("negative nnz; empty call", dict(nnz=-1, N=0), EINVAL),
        ("negative size; null pointer", dict(M=-1, rowptr=None), EINVAL),
        ("nnz >= 2^31; null pointer", dict(nnz=BIG, rowptr=None), ERANGE),
        ("nnz >= 2^31; empty call", dict(nnz=BIG, M=0), ERANGE),
        ("empty call (M = 0); null pointers, leading dimension below N", dict(M=0, rowptr=None, C=None, ldb=0), OK),
        ("empty call (N = 0); null pointer, short workspace", dict(N=0, B=None, ws=FAKE, ws_bytes=16, **HUB), OK),
        ("null pointer; short workspace", dict(col=None, ws=FAKE, ws_bytes=16, **HUB), EINVAL),
        ("null output; short workspace", dict(C=None, ws=FAKE, ws_bytes=16, **HUB), EINVAL),
        ("ldb below N; short workspace", dict(ldb=7, ws=FAKE, ws_bytes=16, **HUB), EINVAL),
        ("ldc below N; short workspace", dict(ldc=7, ws=FAKE, ws_bytes=16, **HUB), EINVAL),
        ("ldarg below N; short workspace", dict(arg=FAKE, ldarg=7, ws=FAKE, ws_bytes=16, **HUB), EINVAL),
        ("short workspace; misaligned workspace", dict(ws=FAKE + 8, ws_bytes=16, **HUB), ENOMEM),
        ("misaligned workspace", dict(ws=FAKE + 8, ws_bytes=ROOMY, **HUB), EINVAL),
    ]),
    "rows_divide": (call_divide, [
        ("negative size; empty call", dict(N=-1, M=0), EINVAL),
        ("negative size; null pointer", dict(M=-1, rowptr=None), EINVAL),
        ("empty call (M = 0); null pointers, leading dimension below N", dict(M=0, rowptr=None, src=None, out=None, ldin=0), OK),
        ("empty call (N = 0); null pointers", dict(N=0, src=None, out=None), OK),
        ("null rowptr", dict(rowptr=None), EINVAL),
        ("null input", dict(src=None), EINVAL),
        ("null output", dict(out=None), EINVAL),
        ("ldin below N", dict(ldin=7), EINVAL),
        ("ldout below N", dict(ldout=7), EINVAL),
    ]),
    "reduce_grad_val": (call_grad_val, [
        ("negative size; nnz >= 2^31", dict(N=-1, nnz=BIG), EINVAL),
        ("negative size; empty call", dict(K=-1, M=0), EINVAL),
        ("negative nnz; null pointer", dict(nnz=-1, rowptr=None), EINVAL),
        ("nnz >= 2^31; null pointer", dict(nnz=BIG, col=None), ERANGE),
        ("nnz >= 2^31; empty call", dict(nnz=BIG, M=0), ERANGE),
        ("empty call (M = 0); null pointers, leading dimension below N", dict(M=0, rowptr=None, grad_val=None, ldb=0), OK),
        ("empty call (nnz = 0); null pointers", dict(nnz=0, col=None, B=None), OK),
        ("null rowptr", dict(rowptr=None), EINVAL),
        ("null arg", dict(arg=None), EINVAL),
        ("null output", dict(grad_val=None), EINVAL),
        ("ldb below N", dict(ldb=7), EINVAL),
        ("ldg below N", dict(ldg=7), EINVAL),
        ("ldarg below N", dict(ldarg=7), EINVAL),
    ]),
    "reduce_grad_b": (call_grad_b, [
        ("negative size; nnz >= 2^31", dict(M=-1, nnz=BIG), EINVAL),
        ("negative size; empty call", dict(N=-1, K=0), EINVAL),
        ("negative nnz; null pointer", dict(nnz=-1, t_rowptr=None), EINVAL),
        ("nnz >= 2^31; null pointer", dict(nnz=BIG, perm=None), ERANGE),
        ("nnz >= 2^31; empty call", dict(nnz=BIG, K=0), ERANGE),
        ("empty call (K = 0); null pointers, leading dimension below N", dict(K=0, t_rowptr=None, grad_b=None, ldg=0), OK),
        ("empty call (N = 0); null pointers", dict(N=0, G=None, arg=None), OK),
        ("null t_rowptr", dict(t_rowptr=None), EINVAL),
        ("null perm", dict(perm=None), EINVAL),
        ("null output", dict(grad_b=None), EINVAL),
        ("ldg below N", dict(ldg=7), EINVAL),
        ("ldarg below N", dict(ldarg=7), EINVAL),
        ("ldgb below N", dict(ldgb=7), EINVAL),
    ]),
}


@pytest.mark.parametrize("entry", sorted(SHARED_CASES))
def test_every_dtype_answers_a_bad_argument_alike_and_in_the_same_order(lib, entry):
    """The float32, bfloat16 and float16 forms of an entry make the checks they share in one order: the same status for
    the same mistake, also when a second mistake follows that a later check would answer with another status."""
    call, cases = SHARED_CASES[entry]
    for what, kw, want in cases:
        # the reduce cases that name no code hold for both selections
        for extra in ({"reduce": AMAX}, {"reduce": AMIN}) if entry == "reduce" and "reduce" not in kw else ({},):
            got = {sfx: call(lib, sfx, **kw, **extra) for sfx in DTYPES}
            assert got == dict.fromkeys(DTYPES, want), (entry, what, extra, got)


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
