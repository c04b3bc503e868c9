"""matmuls.block_sparse_attention_prefill and its paged / fp8 forms without a GPU: every refusal with its
exception type, before the device — the decode calls' refusals through the one shared check, and what the prefill calls say
differently (no bound on the group, on B·Hkv or on T; q through its own strides; new_lens) —; the …_takes functions; the rule
including new_lens (slot t holds a token iff t ≥ T − new_lens[b] and pos ≥ 0; token at pos = k_len − T + t sees key j iff j ≤ pos
and the layout lists block (pos // block, j // block)) against a dense mask built here, through the float64 stand-in
tests/fake_custom_mm_block_attention_prefill.py; q, the cache and the table handed to the binding with their own data_ptr and
strides, no .contiguous() on q; the layout record shared with the training and decode calls; and the eight prefill entries of
the C ABI: declared, exported, MI_EINVAL before any HIP call, MI_OK for empty calls."""
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
FORMS = ("", "paged_", "fp8_", "paged_fp8_")
OK, EINVAL = 0, -1
FAKE = 0x1000  # a non-null, 16-byte aligned address that is never dereferenced: every call below returns before the device


# ---- the C ABI -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(built):
    import torch  # noqa: F401  (torch's HIP runtime first, as in the product)
    lib = ctypes.CDLL(str(built / "libmi_spmm.so"))
    vp, i64, i32, f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float
    for form in FORMS:
        for s in SUFFIXES:
            fn = getattr(lib, f"mi_block_attention_prefill_{form}{s}")
            fn.argtypes = [vp, vp, i64] + 5 * [i32] + ([vp, i64, i32, i32] if "paged" in form else []) + [i32] + \
                3 * [vp, i64, i64, i64] + [vp, i32, vp, i32, i32, f32] + ([vp, i32, vp, i32] if "fp8" in form else []) + \
                [vp, i64, i64, vp, vp]
            fn.restype = ctypes.c_int
    return lib


def test_header_declares_and_library_exports_the_prefill_entries(lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for form in FORMS:
        for s in SUFFIXES:
            name = f"mi_block_attention_prefill_{form}{s}"
            assert re.search(rf"\b{name}\s*\(", text), name
            assert hasattr(lib, name), name


DEFAULTS = dict(nnz=4, layouts=1, items=8, heads=2, T=100, Smax=512, D=64, q=FAKE, ldq=None, headQ=None, batchQ=None, k=FAKE, ldk=None,
                headK=None, outerK=None, k_lens=FAKE, lens_count=4, new_lens=None, new_lens_count=0, group=4, out=FAKE, ldo=None,
                lse=FAKE, table=FAKE, table_ld=32, pages=40, page=16, k_scale=None, k_scale_count=1, v_scale=FAKE, v_scale_count=2)


def prefill(lib, form, s, **kw):
    a = {**DEFAULTS, **kw}
    D, T = a["D"], a["T"]
    rows = a["page"] if "paged" in form else 512
    ldq, ldk, ldo = (D if a[n] is None else a[n] for n in ("ldq", "ldk", "ldo"))
    headQ = T * D if a["headQ"] is None else a["headQ"]
    batchQ = 8 * T * D if a["batchQ"] is None else a["batchQ"]
    headK = rows * D if a["headK"] is None else a["headK"]
    outerK = 2 * rows * D if a["outerK"] is None else a["outerK"]
    args = [FAKE, FAKE, a["nnz"], a["layouts"], a["items"], a["heads"], T, a["Smax"]]
    if "paged" in form:
        args += [a["table"], a["table_ld"], a["pages"], a["page"]]
    args += [D, a["q"], ldq, headQ, batchQ, a["k"], ldk, headK, outerK, FAKE, D, rows * D, 2 * rows * D, a["k_lens"], a["lens_count"],
             a["new_lens"], a["new_lens_count"], a["group"], 1.0]
    if "fp8" in form:
        args += [a["k_scale"], a["k_scale_count"], a["v_scale"], a["v_scale_count"]]
    args += [a["out"], ldo, T * ldo, a["lse"], None]
    return getattr(lib, f"mi_block_attention_prefill_{form}{s}")(*args)


@pytest.mark.parametrize("s", SUFFIXES)
@pytest.mark.parametrize("form", FORMS)
def test_prefill_entries_validate_before_any_hip_call(lib, form, s):
    unit = 16 if "fp8" in form else 8
    refused = [{"group": 0}, {"group": -1}, {"D": 48}, {"D": 256}, {"D": 0}, {"Smax": 500}, {"nnz": -1}, {"layouts": 0}, {"heads": 3},
               {"heads": 0}, {"T": -1}, {"items": -8},
               {"lens_count": 0}, {"lens_count": 3}, {"k_lens": None}, {"k_lens": FAKE + 2},
               {"new_lens": FAKE + 2, "new_lens_count": 4}, {"new_lens": FAKE, "new_lens_count": 3}, {"new_lens": FAKE, "new_lens_count": 0},
               {"q": None}, {"q": FAKE + 8}, {"ldq": 60}, {"headQ": 12}, {"batchQ": -8}, {"batchQ": 4},
               {"out": None}, {"out": FAKE + 2}, {"ldo": 60}, {"ldo": 68}, {"lse": None}, {"lse": FAKE + 1},
               {"k": None}, {"k": FAKE + 8}, {"ldk": 48}, {"ldk": 64 + unit // 2}, {"headK": unit // 2}, {"outerK": unit + unit // 2}]
    if "paged" in form:
        refused += [{"page": 0}, {"page": 8}, {"page": 24}, {"pages": -1}, {"table": None}, {"table": FAKE + 2}, {"table_ld": 31},
                    {"page": 1024}]  # (Smax % page != 0)
    if "fp8" in form:
        refused += [{"k_scale_count": 3}, {"v_scale_count": 0}, {"v_scale": FAKE + 2}, {"k_scale": FAKE + 1}]
    for kw in refused:
        assert prefill(lib, form, s, **kw) == EINVAL, kw
    # what the decode entries bound and these do not is NOT refused on its way to the operand checks: the refusal comes from
    # the operand named, and is the same with the large value
    for kw in ({"group": 17}, {"group": 1000}, {"items": 65536 * 2, "lens_count": 65536}, {"T": 1 << 20}):
        assert prefill(lib, form, s, q=None, **kw) == EINVAL and prefill(lib, form, s, lse=FAKE + 1, **kw) == EINVAL, kw
    # an empty problem is MI_OK after the checks that need no operand; a bad form is refused even then
    assert prefill(lib, form, s, items=0, q=None, out=None) == OK and prefill(lib, form, s, T=0, k_lens=None, lse=None) == OK
    assert prefill(lib, form, s, items=0, group=0) == EINVAL and prefill(lib, form, s, T=0, D=40) == EINVAL
    if "paged" in form:
        assert prefill(lib, form, s, items=0, page=8) == EINVAL
        assert prefill(lib, form, s, pages=0, k=None, q=None) == EINVAL  # (an empty pool is never read: k may be null, q not)
    if "fp8" in form:
        assert prefill(lib, form, s, T=0, k_scale_count=5) == EINVAL


# ---- matmuls on the real extension: refusals before the device ---------------------------------------------------

@pytest.fixture()
def real(built):
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import matmuls
    yield matmuls
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)


def _full(rows, lead=()):
    return torch.ones(lead + (rows, rows)).to_sparse_csr()


def test_every_refusal_comes_before_the_device_with_its_type(real):
    f = real.block_sparse_attention_prefill
    what = "block_sparse_attention_prefill: "
    q = torch.rand(2, 8, 100, 64).bfloat16()
    k = torch.rand(2, 2, 256, 64).bfloat16()
    lay, lens = _full(4), torch.tensor([100, 256])
    # the decode calls' refusals, through the one shared check
    with pytest.raises(ValueError, match=what + "layout must be a CSR tensor"):
        f(q, k, k, lay.to_dense(), lens)
    with pytest.raises(ValueError, match=what + "q must be bfloat16 or float16, got torch.float32"):
        f(q.float(), k, k, lay, lens)
    with pytest.raises(ValueError, match=what + "v must be a dense tensor"):
        f(q, k, lay, lay, lens)
    with pytest.raises(RuntimeError, match=what + "q is torch.bfloat16 but v is torch.float16"):
        f(q, k, k.half(), lay, lens)
    for bad in (32, 0, -64, 96, True, 64.0):
        with pytest.raises(ValueError, match=what + "block must be a positive multiple of 64.*Hq a multiple of Hkv"):
            f(q, k, k, lay, lens, block=bad)
    with pytest.raises(TypeError):  # there is no chunk
        f(q, k, k, lay, lens, chunk=2)
    with pytest.raises(ValueError, match=what + r"q must be \[B, Hq, T, D\]"):
        f(q[0], k[0], k[0], lay, lens)
    with pytest.raises(ValueError, match=what + "head size D must be 32, 64, 96 or 128, got 48"):
        f(q[..., :48], k[..., :48], k[..., :48], lay, lens)
    for kk in (torch.rand(2, 3, 256, 64), torch.rand(1, 2, 256, 64), torch.rand(2, 2, 256, 32), torch.rand(2, 0, 256, 64)):
        with pytest.raises(ValueError, match=what + r"q of shape \(2, 8, 100, 64\) needs k \(2, 'Hkv', 'Smax', 64\) with Hkv a divisor of 8"):
            f(q, kk.bfloat16(), kk.bfloat16(), lay, lens)
    with pytest.raises(ValueError, match=what + "v must be a dense tensor with k's shape"):
        f(q, k, k[:, :, :128], lay, lens)
    with pytest.raises(ValueError, match=what + "q must hold T >= 1 new tokens"):
        f(q[:, :, :0], k, k, lay, lens)
    with pytest.raises(ValueError, match=what + "Smax = 256 must be a multiple of block = 192"):
        f(q, k, k, lay, lens, block=192)
    for bad in (_full(2), _full(4, (8,)), _full(4, (2, 8)), _full(4, (1, 2)), torch.ones(4, 3).to_sparse_csr()):
        with pytest.raises(ValueError, match=what + r"the layout must have shape \[\*l_lead, Smax/block, Smax/block\] = \[\*l_lead, 4, 4\]"):
            f(q, k, k, bad, lens)
    with pytest.raises(ValueError, match=what + "k_lens is required and must be a dense tensor"):
        f(q, k, k, lay, None)
    with pytest.raises(TypeError):  # required
        f(q, k, k, lay)
    for bad in (torch.tensor([1.0, 2.0]), torch.tensor([True, False])):
        with pytest.raises(ValueError, match=what + f"k_lens must be an int32 or int64 tensor, got {bad.dtype}"):
            f(q, k, k, lay, bad)
    with pytest.raises(ValueError, match=what + r"k_lens must have shape \(2,\)"):
        f(q, k, k, lay, torch.tensor([1, 2, 3]))
    with pytest.raises(TypeError):  # keyword only
        f(q, k, k, lay, lens, 64, None, torch.tensor([1, 2]))
    # new_lens: rope_kv_cache_append's refusals
    with pytest.raises(ValueError, match=what + "new_lens must be None or a dense tensor"):
        f(q, k, k, lay, lens, new_lens=[3, 4])
    with pytest.raises(ValueError, match=what + "new_lens must be an int32 or int64 tensor, got torch.float32"):
        f(q, k, k, lay, lens, new_lens=torch.tensor([3.0, 4.0]))
    for bad in (torch.tensor(3), torch.tensor([3]), torch.tensor([1, 2, 3])):
        with pytest.raises(ValueError, match=what + r"new_lens must have shape \(2,\)"):
            f(q, k, k, lay, lens, new_lens=bad)
    # q through its own strides: ValueError naming the stride, never a silent copy
    wide = torch.rand(2, 8, 100, 128).bfloat16()
    with pytest.raises(ValueError, match=what + "q must have a last stride of 1, got 2"):
        f(wide[..., ::2], k, k, lay, lens)
    with pytest.raises(ValueError, match=what + "q's token stride must be a multiple of 8 elements, got 68"):
        f(torch.rand(2, 8, 100, 68).bfloat16()[..., :64], k, k, lay, lens)
    with pytest.raises(ValueError, match=what + "q's head stride must be a multiple of 8 elements, got 6404"):
        f(torch.rand(2, 8, 6404).bfloat16()[..., :6400].reshape(2, 8, 100, 64), k, k, lay, lens)
    # the cache's strides
    with pytest.raises(ValueError, match=what + "k must have a last stride of 1, got 2"):
        f(q, torch.rand(2, 2, 256, 128).bfloat16()[..., ::2], k, lay, lens)
    with pytest.raises(ValueError, match=what + "v's row stride must be a multiple of 8 elements and at least D = 64, got 68"):
        f(q, k, torch.rand(2, 2, 256, 68).bfloat16()[..., :64], lay, lens)
    # what the decode calls bound and these do not: a group of 17, T beyond 65535 reach the last check
    q34 = torch.rand(2, 34, 3, 64).bfloat16()
    with pytest.raises(RuntimeError, match=what + r"layout, q, k, v, k_lens must be device \(HIP\) tensors"):
        f(q34, k, k, lay, lens)
    k1 = torch.empty(1, 1, 64, 32).bfloat16()
    with pytest.raises(RuntimeError, match=what + r"layout, q, k, v, k_lens must be device \(HIP\) tensors"):
        f(torch.empty(1, 1, 65536, 32).bfloat16(), k1, k1, _full(1), torch.tensor(5))
    # host tensors: the last check, RuntimeError; a strided q is no refusal
    with pytest.raises(RuntimeError, match=what + r"layout, q, k, v, k_lens, new_lens must be device \(HIP\) tensors"):
        f(q.transpose(1, 2).contiguous().transpose(1, 2), k, k, lay, lens, new_lens=torch.tensor([5, 100]), return_lse=True)


def test_paged_and_fp8_calls_keep_the_decode_calls_refusals(real):
    q = torch.rand(2, 4, 70, 64).bfloat16()
    pool = torch.rand(9, 2, 32, 64).bfloat16()
    table = torch.arange(16).reshape(2, 8) % 9
    lay, lens = _full(4), torch.tensor([100, 256])
    f = real.block_sparse_attention_prefill_paged
    what = "block_sparse_attention_prefill_paged: "
    with pytest.raises(ValueError, match=what + r"the pool's pages must hold a power of two >= 16 keys, got page = 24"):
        f(q, pool[:, :, :24], pool[:, :, :24], table, lay, lens)
    with pytest.raises(ValueError, match=what + "block_table is required and must be a dense tensor"):
        f(q, pool, pool, None, lay, lens)
    with pytest.raises(ValueError, match=what + r"block_table must have shape \(2, W\)"):
        f(q, pool, pool, table[:1], lay, lens)
    with pytest.raises(ValueError, match=what + "k_pages's page stride must be a multiple of 8 elements"):
        f(q, torch.rand(9 * (2 * 32 * 64 + 4)).bfloat16().as_strided((9, 2, 32, 64), (2 * 32 * 64 + 4, 32 * 64, 64, 1)), pool, table, lay, lens)
    with pytest.raises(RuntimeError, match=what + r"layout, q, k_pages, v_pages, block_table, k_lens must be device \(HIP\) tensors"):
        f(q, pool, pool, table, lay, lens)
    k8 = torch.rand(2, 2, 256, 64).to(torch.float8_e4m3fn)
    f = real.block_sparse_attention_prefill_fp8
    what = "block_sparse_attention_prefill_fp8: "
    with pytest.raises(ValueError, match=what + "k must be float8_e4m3fn, got torch.uint8"):
        f(q, k8.view(torch.uint8), k8.view(torch.uint8), lay, lens)
    with pytest.raises(ValueError, match=what + "k must be float8_e4m3fn, got torch.float8_e5m2.*Hq a multiple of Hkv"):
        f(q, k8.view(torch.float8_e5m2), k8.view(torch.float8_e5m2), lay, lens)
    with pytest.raises(RuntimeError, match=what + "k is torch.float8_e4m3fn but v is torch.float8_e5m2"):
        f(q, k8, k8.view(torch.float8_e5m2), lay, lens)
    with pytest.raises(ValueError, match=what + r"k_scale must have shape \(\), \(1,\) or \(2,\)"):
        f(q, k8, k8, lay, lens, k_scale=torch.ones(3))
    with pytest.raises(ValueError, match=what + "v_scale must be a float32 tensor, got torch.float64"):
        f(q, k8, k8, lay, lens, v_scale=torch.ones(2, dtype=torch.float64))
    with pytest.raises(ValueError, match=what + "k's row stride must be a multiple of 16 elements and at least D = 64, got 72"):
        f(q, torch.rand(2, 2, 256, 72).to(torch.float8_e4m3fn)[..., :64], k8, lay, lens)
    with pytest.raises(RuntimeError, match=what + r"layout, q, k, v, k_lens, v_scale must be device \(HIP\) tensors"):
        f(q, k8, k8, lay, lens, k_scale=0.5, v_scale=torch.ones(2))
    pool8 = pool.to(torch.float8_e4m3fn)
    with pytest.raises(RuntimeError, match=r"block_sparse_attention_prefill_paged_fp8: layout, q, k_pages, v_pages, block_table, k_lens, "
                                           r"new_lens must be device \(HIP\) tensors"):
        real.block_sparse_attention_prefill_paged_fp8(q, pool8, pool8, table, lay, lens, new_lens=torch.tensor([1, 70]))


def test_custom_mm_prefill_binding_refuses_host_tensors_and_keywords(built):
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import custom_mm
    offs, col = torch.tensor([[0, 1]], dtype=torch.int32), torch.tensor([0], dtype=torch.int32)
    q, kv = torch.rand(1, 2, 3, 32).bfloat16(), torch.rand(1, 1, 64, 32).bfloat16()
    lens, lse = torch.tensor([5], dtype=torch.int32), torch.empty(1, 2, 3)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.block_attention_prefill(offs, col, 1, q, kv, kv, lens, None, 1.0, torch.empty_like(q), lse)
    with pytest.raises(RuntimeError, match=r"(?s)(?=.*\bBFloat16\b)(?=.*\bHalf\b)"):
        custom_mm.block_attention_prefill(offs, col, 1, q, kv, kv.half(), lens, None, 1.0, torch.empty_like(q), lse)
    with pytest.raises(TypeError):  # positional only
        custom_mm.block_attention_prefill(offs, col, 1, q, kv, kv, lens, None, 1.0, out=torch.empty_like(q), lse=lse)
    for name in ("block_attention_prefill_paged", "block_attention_prefill_fp8", "block_attention_prefill_paged_fp8"):
        assert callable(getattr(custom_mm, name))


def test_block_attention_prefill_takes(real):
    for dtype in (torch.bfloat16, torch.float16):
        for D in (32, 64, 96, 128):
            for block in (64, 128, 512):
                assert real.block_attention_prefill_takes(dtype, D, block) and real.block_attention_prefill_fp8_takes(dtype, D, block)
                for page in (16, 32, 64, 1024):
                    assert real.block_attention_prefill_paged_takes(dtype, D, block, page)
                    assert real.block_attention_prefill_paged_fp8_takes(dtype, D, block, page)
    for takes in (real.block_attention_prefill_takes, real.block_attention_prefill_fp8_takes):
        assert not takes(torch.float32, 64, 64) and not takes(torch.bfloat16, 48, 64) and not takes(torch.bfloat16, 256, 64)
        assert not takes(torch.float16, 64, 32) and not takes(torch.float16, 64, 96) and not takes(torch.float16, 64, True)
    for takes in (real.block_attention_prefill_paged_takes, real.block_attention_prefill_paged_fp8_takes):
        assert not takes(torch.float32, 64, 64, 16) and not takes(torch.float16, 64, 96, 16)
        assert not takes(torch.float16, 64, 64, 8) and not takes(torch.float16, 64, 64, 24) and not takes(torch.float16, 64, 64, True)


# ---- wiring on CPU tensors, float64 stand-in arithmetic on float16 storage -----------------------------------------

@pytest.fixture()
def mm(oracle_mod):
    """(matmuls bound to the float64 stand-in, the stand-in)."""
    import fake_custom_mm_block_attention_prefill as fake
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


def _random_layout(g, lead, rows, keep):
    """A CSR block layout [*lead, rows, rows] keeping the diagonal block and keep − 1 others per row, in shuffled order."""
    nb = 1
    for n in lead:
        nb *= n
    cols = []
    for _ in range(nb):
        for r in range(rows):
            others = [c for c in torch.randperm(rows, generator=g).tolist() if c != r][:keep - 1]
            row = others + [r]
            cols.append(torch.tensor(row)[torch.randperm(keep, generator=g)])
    col = torch.stack(cols).reshape(lead + (rows * keep,))
    crow = (torch.arange(rows + 1) * keep).expand(lead + (rows + 1,)).contiguous()
    return torch.sparse_csr_tensor(crow, col, torch.ones(col.shape), size=lead + (rows, rows))


def _visible(layout, B, Hkv, T, Smax, block, k_lens, new_lens=None, hidden=None):
    """Boolean [B, Hkv, T, Smax] built from the rule alone: slot t of item b holds a token iff t ≥ T − clamp(new_len, 0, T) and
    pos = clamp(k_len, 0, Smax) − T + t ≥ 0; it sees key j iff j ≤ pos and the dense form of the layout holds block
    (pos // block, j // block); layouts indexed by the k / v item.  hidden: Boolean [B, Smax], keys behind an invalid page."""
    dense = torch.sparse_csr_tensor(layout.crow_indices(), layout.col_indices(), torch.ones_like(layout.values()),
                                    size=layout.shape).to_dense() != 0
    dense = dense.reshape((-1,) + tuple(dense.shape[-2:]))
    vis = torch.zeros(B, Hkv, T, Smax, dtype=torch.bool)
    for b in range(B):
        n = T if new_lens is None else min(max(int(new_lens[b]), 0), T)
        for h in range(Hkv):
            lay = dense[(b * Hkv + h) % dense.shape[0]]
            for t in range(T - n, T):
                pos = min(max(int(k_lens[b]), 0), Smax) - T + t
                for j in range(0, max(pos + 1, 0)):
                    vis[b, h, t, j] = bool(lay[pos // block, j // block]) and not (hidden is not None and bool(hidden[b, j]))
    return vis


def _dense_reference(q, k, v, vis, scale, G):
    """(out, lse) of dense masked attention in float64 (k, v float64 [B, Hkv, Smax, D]); rows that see nothing: zero and −inf."""
    qd = q.double()
    kd = torch.where(vis.any(2)[..., None], k, torch.zeros((), dtype=torch.float64)).repeat_interleave(G, 1)
    vd = torch.where(vis.any(2)[..., None], v, torch.zeros((), dtype=torch.float64)).repeat_interleave(G, 1)
    m = vis.repeat_interleave(G, 1)
    s = (scale * (qd @ kd.transpose(-1, -2))).masked_fill(~m, -float("inf"))
    empty = ~m.any(-1, keepdim=True)
    lse = torch.logsumexp(s.masked_fill(empty, 0.0), -1).masked_fill(empty[..., 0], -float("inf"))
    p = torch.where(empty, torch.zeros_like(s), torch.softmax(s.masked_fill(empty, 0.0), -1))
    return p @ vd, lse


def _poison_unseen(x, vis):
    """NaN in every key row of x [B, Hkv, Smax, D] that no token of its item sees."""
    x = x.clone()
    x[~vis.any(2)] = float("nan")
    return x


def _check(out, lse, q, want, want_lse, vis, G):
    B, Hq, T, D = q.shape
    assert out.dtype == q.dtype and out.shape == q.shape and out.is_contiguous() and lse.dtype == torch.float32 and lse.shape == (B, Hq, T)
    assert torch.isfinite(out).all()
    assert torch.allclose(out.double(), want, rtol=2e-3, atol=2e-3), float((out.double() - want).abs().max())
    seen = vis.any(-1).repeat_interleave(G, 1)
    assert (out[~seen] == 0).all() and (lse[~seen] == -float("inf")).all()
    assert torch.allclose(lse[seen].double(), want_lse[seen], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("G,T,block,l_lead,k_lens,new_lens", [
    (4, 70, 64, (), [130, 256], None),               # positions 60 … 129: three position tiles, two of them partial
    (2, 5, 128, (), [130, 257], None),               # block = 128: the rows of the 128-grid; 257 is clamped to Smax
    (1, 64, 64, (2,), [64, 200], None),              # a layout per k / v head; an aligned first chunk
    (3, 9, 64, (2, 2), [200, 64], [4, 9]),           # a layout per k / v item; the last 4 of 9 slots hold tokens
    (2, 40, 64, (2,), [0, 12], None),                # k_len = 0 and k_len < T: slots with pos < 0
    (17, 3, 64, (), [1, 300], [0, 2]),               # a group of 17; an item without a new token
    (2, 6, 64, (), [100, 70], [-3, 60]),             # new_lens clamped to [0, T]
])
def test_the_rule_with_new_lens_against_a_dense_mask(mm, G, T, block, l_lead, k_lens, new_lens):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(83 + G + T)
    B, Hkv, Smax, D = 2, 2, 256, 32
    layout = _random_layout(g, l_lead, Smax // block, keep=max(1, Smax // block - 1))
    lens = torch.tensor(k_lens, dtype=torch.int64)
    news = None if new_lens is None else torch.tensor(new_lens, dtype=torch.int64)
    vis = _visible(layout, B, Hkv, T, Smax, block, k_lens, new_lens)
    q = torch.randn(B, Hkv * G, T, D, generator=g).half()
    k, v = (torch.randn(B, Hkv, Smax, D, generator=g).half() for _ in range(2))
    want, want_lse = _dense_reference(q, k.double(), v.double(), vis, 1.0 / D ** 0.5, G)
    out, lse = matmuls.block_sparse_attention_prefill(q, _poison_unseen(k, vis), _poison_unseen(v, vis), layout, lens, block=block,
                                                      new_lens=news, return_lse=True)
    _check(out, lse, q, want, want_lse, vis, G)
    for b, n in enumerate(k_lens):  # a slot with pos < 0, or ahead of the new tokens, holds no token
        for t in range(T):
            gone = min(n, Smax) - T + t < 0 or (new_lens is not None and t < T - min(max(new_lens[b], 0), T))
            if gone:
                assert (out[b, :, t] == 0).all() and (lse[b, :, t] == -float("inf")).all()
    (name, rec), = [c for c in fake.calls if c[0] == "block_attention_prefill"]
    assert rec["k_lens"].dtype == torch.int32 and rec["k_lens"].tolist() == k_lens      # as given: the kernel clamps
    assert (rec["new_lens"] is None) if new_lens is None else (rec["new_lens"].dtype == torch.int32 and rec["new_lens"].tolist() == new_lens)
    assert rec["layouts"] == max(1, int(torch.tensor(l_lead).prod()) if l_lead else 1)
    assert rec["scale"] == 1.0 / D ** 0.5


def test_the_paged_and_fp8_forms_follow_the_rule(mm):
    """The pool behind a shuffled table with a −1 and a P + 5 entry among the seen pages (their keys are hidden), NaN in the
    unreferenced pages; the fp8 cache with per-head scales."""
    matmuls, fake = mm
    g = torch.Generator().manual_seed(89)
    B, Hkv, G, T, Smax, D, page = 2, 2, 2, 50, 256, 32, 16
    k_lens, new_lens = [130, 256], [50, 20]
    layout = _random_layout(g, (), 4, keep=3)
    lens, news = torch.tensor(k_lens), torch.tensor(new_lens)
    q = torch.randn(B, Hkv * G, T, D, generator=g).half()
    k, v = (torch.randn(B, Hkv, Smax, D, generator=g).half() for _ in range(2))
    W, P = Smax // page, 2 * (Smax // page) + 3
    table = torch.randperm(P, generator=g)[:B * W].reshape(B, W).to(torch.int32)
    hidden = torch.zeros(B, Smax, dtype=torch.bool)
    pool_k, pool_v = (torch.full((P, Hkv, page, D), float("nan")).half() for _ in range(2))
    for b in range(B):
        for w in range(W):
            pool_k[table[b, w]] = k[b, :, w * page:(w + 1) * page]
            pool_v[table[b, w]] = v[b, :, w * page:(w + 1) * page]
    kept = (int(table[0, 2]), int(table[1, 9]))
    table[0, 2], table[1, 9] = -1, P + 5
    hidden[0, 2 * page:3 * page] = hidden[1, 9 * page:10 * page] = True
    vis = _visible(layout, B, Hkv, T, Smax, 64, k_lens, new_lens, hidden)
    assert vis[0].any() and vis[1].any()
    want, want_lse = _dense_reference(q, k.double(), v.double(), vis, 0.2, G)
    wide = torch.zeros(B, W + 3, dtype=torch.int32)
    wide[:, :W] = table
    out, lse = matmuls.block_sparse_attention_prefill_paged(q, pool_k, pool_v, wide[:, :W], layout, lens, scale=0.2, new_lens=news,
                                                            return_lse=True)
    _check(out, lse, q, want, want_lse, vis, G)
    (name, rec), = [c for c in fake.calls if c[0] == "block_attention_prefill_paged"]
    assert rec["table_ptr"] == wide.data_ptr() and rec["table_stride"] == (W + 3, 1) and rec["k_ptr"] == pool_k.data_ptr()
    # fp8, contiguous and paged, per-head scales
    vis = _visible(layout, B, Hkv, T, Smax, 64, k_lens, new_lens)
    k8, ks = matmuls.kv_to_fp8(k)
    v8, vs = matmuls.kv_to_fp8(v)
    kq = k8.float().double() * ks.double().reshape(1, Hkv, 1, 1)
    vq = v8.float().double() * vs.double().reshape(1, Hkv, 1, 1)
    want, want_lse = _dense_reference(q, kq, vq, vis, 1.0 / D ** 0.5, G)
    k8p, v8p = (x.view(torch.uint8).clone() for x in (k8, v8))
    k8p[~vis.any(2)] = 0x7F
    v8p[~vis.any(2)] = 0x7F
    out, lse = matmuls.block_sparse_attention_prefill_fp8(q, k8p.view(torch.float8_e4m3fn), v8p.view(torch.float8_e4m3fn), layout, lens,
                                                          k_scale=ks, v_scale=vs, new_lens=news, return_lse=True)
    _check(out, lse, q, want, want_lse, vis, G)
    (name, rec), = [c for c in fake.calls if c[0] == "block_attention_prefill_fp8"]
    assert rec["k_scale"]["ptr"] == ks.data_ptr() and rec["v_scale"]["ptr"] == vs.data_ptr() and rec["k_dtype"] == torch.float8_e4m3fn
    table[0, 2], table[1, 9] = kept
    pool8_k, pool8_v = (torch.full((P, Hkv, page, D), 0x7F, dtype=torch.uint8) for _ in range(2))
    for b in range(B):
        for w in range(W):
            pool8_k[table[b, w]] = k8.view(torch.uint8)[b, :, w * page:(w + 1) * page]
            pool8_v[table[b, w]] = v8.view(torch.uint8)[b, :, w * page:(w + 1) * page]
    paged = matmuls.block_sparse_attention_prefill_paged_fp8(q, pool8_k.view(torch.float8_e4m3fn), pool8_v.view(torch.float8_e4m3fn),
                                                             table.long(), layout, lens, k_scale=ks, v_scale=vs, new_lens=news,
                                                             return_lse=True)
    _check(paged[0], paged[1], q, want, want_lse, vis, G)
    (name, rec), = [c for c in fake.calls if c[0] == "block_attention_prefill_paged_fp8"]
    assert rec["table_dtype"] == torch.int32  # an int64 table is narrowed on its way


def test_q_and_the_cache_reach_the_binding_with_their_own_pointers_and_strides(mm):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(97)
    B, Hkv, Smax, D, G, T = 2, 2, 128, 32, 2, 10
    Hq = Hkv * G
    layout = _random_layout(g, (), 2, keep=2)
    lens = torch.tensor([100, 128])
    plain_k, plain_v = (torch.randn(B, Hkv, Smax, D, generator=g).half() for _ in range(2))
    bshd_k, bshd_v = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (plain_k, plain_v))
    # q as the slice of a fused projection [B, T, Hq + 2·Hkv, D] seen through .transpose(1, 2), and in a wider buffer
    fused = torch.randn(B, T, Hq + 2 * Hkv, D, generator=g).half()
    q_slice = fused[:, :, :Hq].transpose(1, 2)
    q_plain = q_slice.contiguous()
    q_wide = torch.zeros(B, Hq, T, D + 8).half()
    q_wide[..., :D] = q_plain
    assert not q_slice.is_contiguous() and q_slice.stride() == (T * (Hq + 2 * Hkv) * D, D, (Hq + 2 * Hkv) * D, 1)
    want = None
    for qq, kk, vv in ((q_plain, plain_k, plain_v), (q_slice, bshd_k, bshd_v), (q_wide[..., :D], plain_k, plain_v)):
        fake.calls.clear()
        out = matmuls.block_sparse_attention_prefill(qq, kk, vv, layout, lens)
        (name, rec), = [c for c in fake.calls if c[0] == "block_attention_prefill"]
        assert rec["q_ptr"] == qq.data_ptr() and rec["q_stride"] == tuple(qq.stride())  # no .contiguous() on q
        assert rec["k_ptr"] == kk.data_ptr() and rec["k_stride"] == tuple(kk.stride())
        assert rec["v_ptr"] == vv.data_ptr() and rec["v_stride"] == tuple(vv.stride())
        assert out.is_contiguous() and out.data_ptr() != qq.data_ptr()
        want = out if want is None else want
        assert torch.equal(out, want)


def test_the_layout_record_is_shared_with_the_training_and_decode_calls(mm):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(101)
    Smax, D = 256, 32
    layout = _random_layout(g, (), 2, keep=2)  # in blocks of 128
    q = torch.randn(1, 2, Smax, D, generator=g).half()
    k, v = (torch.randn(1, 2, Smax, D, generator=g).half() for _ in range(2))
    whole = matmuls.block_sparse_attention(q, k, v, layout, block=128, causal=True)
    st = matmuls._csr_state(layout)
    rec = st.block_layouts[(str(q.device), 2)]
    out = matmuls.block_sparse_attention_prefill(q, k, v, layout, torch.tensor([Smax]), block=128)
    matmuls.block_sparse_attention_decode(q[:, :, -1:], k, v, layout, torch.tensor([Smax]), block=128)
    assert list(st.block_layouts) == [(str(q.device), 2)] and st.block_layouts[(str(q.device), 2)] is rec
    assert rec["t"] is None  # only rec['fwd'] is used
    (name, call), = [c for c in fake.calls if c[0] == "block_attention_prefill"]
    assert call["offsets_ptr"] == rec["fwd"][0].data_ptr()
    # a whole prompt is the causal training call
    assert torch.allclose(out.double(), whole.double(), rtol=2e-3, atol=2e-3)
    # and the other way round: a layout first seen by the prefill call
    other = _random_layout(g, (), 4, keep=2)
    matmuls.block_sparse_attention_prefill(q[:, :, -7:], k, v, other, torch.tensor([Smax]))
    rec = matmuls._csr_state(other).block_layouts[(str(q.device), 1)]
    matmuls.block_sparse_attention(q, k, v, other)
    assert matmuls._csr_state(other).block_layouts[(str(q.device), 1)] is rec


def test_return_lse_no_autograd_and_the_decode_call_agrees(mm):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(103)
    layout = _random_layout(g, (), 2, keep=2)
    q = torch.randn(1, 2, 5, 32, generator=g).half().requires_grad_(True)
    k, v = (torch.randn(1, 1, 128, 32, generator=g).half().requires_grad_(True) for _ in range(2))
    lens = torch.tensor([66])
    out = matmuls.block_sparse_attention_prefill(q, k, v, layout, lens)
    assert isinstance(out, torch.Tensor) and not out.requires_grad and out.grad_fn is None
    both = matmuls.block_sparse_attention_prefill(q, k, v, layout, lens, return_lse=True)
    assert isinstance(both, tuple) and len(both) == 2 and torch.equal(both[0], out)
    assert both[1].shape == (1, 2, 5) and both[1].dtype == torch.float32 and not both[1].requires_grad
    dec = matmuls.block_sparse_attention_decode(q, k, v, layout, lens)
    assert torch.allclose(out.double(), dec.double(), rtol=2e-3, atol=2e-3)
    for name in ("block_sparse_attention_decode", "block_sparse_attention_decode_paged", "block_sparse_attention_decode_fp8",
                 "block_sparse_attention_decode_paged_fp8"):
        assert "prefill" in getattr(matmuls, name).__doc__  # the decode docstrings point here for T beyond a few tokens
