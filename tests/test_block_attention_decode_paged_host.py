"""matmuls.block_sparse_attention_decode_paged without a GPU: every refusal with its exception type,
before the device — the page size, W · page against block, the table's dtype, shape and strides, v_pages' shape, the pool's
strides, and the refusals shared with the contiguous call —; block_attention_decode_paged_takes; the visibility rule
against a dense mask built here, through the float64 stand-in tests/fake_custom_mm_block_attention_decode_paged.py, for
pages of 16 and 128 keys; an out-of-range entry under a seen key hiding exactly its page; the pool and an int32 strided
table slice handed to the binding uncopied, an int64 table narrowed; the layout record shared with the contiguous call and
block_sparse_attention; and the paged entries of the C ABI: declared, exported, MI_EINVAL / MI_ENOMEM before any HIP call."""
import ctypes
import importlib
import re
import sys
from pathlib import Path

import pytest
import torch

from test_block_attention_decode_host import _dense_reference, _random_layout, _visible

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "mi_spmm.h"
SUFFIXES = ("bf16", "f16")
OK, EINVAL, ENOMEM = 0, -1, -4
FAKE = 0x1000  # a non-null, 16-byte aligned address that is never dereferenced: every call below returns before the device
NAN = float("nan")


# ---- the C ABI -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(built):
    import torch  # noqa: F401  (torch's HIP runtime first, as in the product)
    lib = ctypes.CDLL(str(built / "libmi_spmm.so"))
    vp, i64, i32, f32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_size_t
    for s in SUFFIXES:
        fn = getattr(lib, f"mi_block_attention_decode_paged_{s}")
        fn.argtypes = [vp, vp, i64] + 5 * [i32] + [vp, i64, i32, i32] + [i32] + [vp, i64, i64] + 2 * [vp, i64, i64, i64] + \
            [vp, i32, i32, i32, f32] + [vp, i64, i64, vp, vp, sz, vp]
        fn.restype = ctypes.c_int
    lib.mi_block_attention_decode_workspace_bytes.argtypes = 6 * [i32]
    lib.mi_block_attention_decode_workspace_bytes.restype = sz
    return lib


def test_header_declares_and_library_exports_the_paged_entries(lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in tuple(f"mi_block_attention_decode_paged_{s}" for s in SUFFIXES):
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(lib, name), name
    args = re.search(r"mi_block_attention_decode_paged_bf16\s*\((.*?)\)", text, flags=re.S).group(1)
    names = [a.split()[-1].lstrip("*") for a in args.split(",")]
    assert names[7:12] == ["Smax", "block_table", "table_ld", "pages", "page"]
    assert names[16:20] == ["k_pages", "ldk", "headK", "pageK"] and names[20:24] == ["v_pages", "ldv", "headV", "pageV"]


DEFAULTS = dict(nnz=4, layouts=1, items=8, heads=2, T=1, Smax=512, table=FAKE, table_ld=32, pages=100, page=16, D=64, q=FAKE,
                ldq=None, k=FAKE, ldk=None, headK=16 * 64, pageK=2 * 16 * 64, k_lens=FAKE, lens_count=4, group=4, chunk=2, out=FAKE,
                lse=FAKE, ws=FAKE, ws_bytes=1 << 30)


def decode(lib, s, **kw):
    a = {**DEFAULTS, **kw}
    D = a["D"]
    ldq, ldk = (D if a[n] is None else a[n] for n in ("ldq", "ldk"))
    return getattr(lib, f"mi_block_attention_decode_paged_{s}")(
        FAKE, FAKE, a["nnz"], a["layouts"], a["items"], a["heads"], a["T"], a["Smax"], a["table"], a["table_ld"], a["pages"],
        a["page"], D, a["q"], ldq, a["T"] * ldq, a["k"], ldk, a["headK"], a["pageK"], FAKE, D, 16 * D, 2 * 16 * D, a["k_lens"],
        a["lens_count"], a["group"], a["chunk"], 1.0, a["out"], D, a["T"] * D, a["lse"], a["ws"], a["ws_bytes"], None)


@pytest.mark.parametrize("s", SUFFIXES)
def test_paged_entries_validate_before_any_hip_call(lib, s):
    for kw in ({"group": 0}, {"group": 17}, {"group": -1},                                     # what the contiguous entry refuses
               {"D": 48}, {"D": 256}, {"D": 0}, {"chunk": 0}, {"chunk": -3}, {"items": 65536}, {"T": 65536},
               {"Smax": 500}, {"nnz": -1}, {"layouts": 0}, {"heads": 3}, {"heads": 0},
               {"lens_count": 0}, {"lens_count": 3}, {"k_lens": None}, {"k_lens": FAKE + 2},
               {"q": None}, {"q": FAKE + 8}, {"out": FAKE + 2}, {"lse": None}, {"lse": FAKE + 1}, {"ldq": 60},
               {"ws": None}, {"ws": FAKE + 4},
               {"page": 8}, {"page": 24}, {"page": 48}, {"page": 0}, {"page": -16}, {"page": 1},   # no power of two ≥ 16
               {"page": 1024},                                                                 # Smax % page != 0
               {"pages": -1},
               {"table": None}, {"table": FAKE + 2}, {"table_ld": 31}, {"table_ld": 0},        # the table; 512 / 16 = 32 entries
               {"page": 256, "table_ld": 1},
               {"k": None}, {"k": FAKE + 8}, {"ldk": 60}, {"ldk": 68}, {"headK": 4}, {"pageK": 12}):  # the pool
        assert decode(lib, s, **kw) == EINVAL, kw
    need = lib.mi_block_attention_decode_workspace_bytes(8, 1, 4, 64, 512, 2)
    assert need > 0 and decode(lib, s, ws_bytes=need - 1) == ENOMEM and decode(lib, s, ws_bytes=0) == ENOMEM
    for page in (32, 64, 128, 256, 512):  # every page size is checked alike (table_ld 32 ≥ 512 / page)
        assert decode(lib, s, page=page, ws_bytes=need - 1) == ENOMEM, page
    # an empty problem is MI_OK after the argument checks that need no operand; a bad page is refused even then
    assert decode(lib, s, items=0, q=None) == OK and decode(lib, s, T=0, k_lens=None, table=None) == OK
    assert decode(lib, s, items=0, page=24) == EINVAL and decode(lib, s, T=0, pages=-1) == EINVAL
    # an empty pool is never read: its pointers may be null (the call is refused later, at the short workspace)
    assert decode(lib, s, pages=0, k=None, ws_bytes=0) == ENOMEM


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


def _pool(P, Hkv, page, D, dtype=torch.bfloat16):
    return torch.rand(P, Hkv, page, D).to(dtype)


def test_every_refusal_comes_before_the_device_with_its_type(real):
    f = real.block_sparse_attention_decode_paged
    what = "block_sparse_attention_decode_paged: "
    q = torch.rand(2, 8, 1, 64).bfloat16()
    kp = _pool(20, 2, 16, 64)
    table = torch.arange(32, dtype=torch.int32).reshape(2, 16) % 20   # Smax = 16 · 16 = 256
    lay, lens = _full(4), torch.tensor([100, 256])
    # the page size: a power of two ≥ 16
    for page in (8, 24, 48):
        with pytest.raises(ValueError, match=what + f"the pool's pages must hold a power of two >= 16 keys, got page = {page}"):
            pp = _pool(20, 2, page, 64)
            f(q, pp, pp, table, lay, lens)
    # W · page against block
    with pytest.raises(ValueError, match=what + "Smax = 256 must be a multiple of block = 192"):
        f(q, kp, kp, table, lay, lens, block=192)
    with pytest.raises(ValueError, match=what + "Smax = 240 must be a multiple of block = 64"):
        f(q, kp, kp, table[:, :15], lay, lens)
    # the table
    with pytest.raises(ValueError, match=what + "block_table is required and must be a dense tensor"):
        f(q, kp, kp, None, lay, lens)
    with pytest.raises(ValueError, match=what + "block_table is required and must be a dense tensor"):
        f(q, kp, kp, table.tolist(), lay, lens)
    for bad in (table.float(), table.to(torch.int16), table.bool()):
        with pytest.raises(ValueError, match=what + f"block_table must be an int32 or int64 tensor, got {bad.dtype}"):
            f(q, kp, kp, bad, lay, lens)
    for bad in (table[0], table[:1], table.reshape(2, 4, 4), torch.zeros(3, 16, dtype=torch.int32)):
        with pytest.raises(ValueError, match=what + r"block_table must have shape \(2, W\)"):
            f(q, kp, kp, bad, lay, lens)
    with pytest.raises(ValueError, match=what + "block_table must have a last stride of 1, got 2"):
        f(q, kp, kp, torch.zeros(2, 32, dtype=torch.int32)[:, ::2], lay, lens)
    with pytest.raises(ValueError, match=what + "block_table's row stride must be at least W = 16, got 0"):
        f(q, kp, kp, table[:1].expand(2, 16), lay, lens)
    # v_pages of another shape, the pool against q
    for vv in (_pool(21, 2, 16, 64), _pool(20, 2, 32, 64), _pool(20, 1, 16, 64)):
        with pytest.raises(ValueError, match=what + "v_pages must be a dense tensor with k_pages' shape"):
            f(q, kp, vv, table, lay, lens)
    for pp in (_pool(20, 3, 16, 64), _pool(20, 2, 16, 32), _pool(20, 0, 16, 64)):
        with pytest.raises(ValueError, match=what + r"q of shape \(2, 8, 1, 64\) needs k_pages \('P', 'Hkv', 'page', 64\) with Hkv a divisor of 8"):
            f(q, pp, pp, table, lay, lens)
    with pytest.raises(ValueError, match=what + r"q must be \[B, Hq, T, D\] and k_pages, v_pages \[P, Hkv, page, D\]"):
        f(q, kp[0], kp[0], table, lay, lens)
    # the pool's strides: ValueError naming the stride, never a silent copy
    wide = _pool(20, 2, 16, 128)
    with pytest.raises(ValueError, match=what + "k_pages must have a last stride of 1, got 2"):
        f(q, wide[..., ::2], kp, table, lay, lens)
    with pytest.raises(ValueError, match=what + "v_pages's row stride must be a multiple of 8 elements and at least D = 64, got 68"):
        f(q, kp, _pool(20, 2, 16, 68)[..., :64], table, lay, lens)
    with pytest.raises(ValueError, match=what + "k_pages's row stride must be a multiple of 8 elements and at least D = 64, got 0"):
        f(q, kp[:, :, :1].expand(20, 2, 16, 64), kp, table, lay, lens)
    odd_head = torch.rand(20, 2 * (16 * 64 + 4)).bfloat16().as_strided((20, 2, 16, 64), (2 * (16 * 64 + 4), 16 * 64 + 4, 64, 1))
    with pytest.raises(ValueError, match=what + "k_pages's head stride must be a multiple of 8 elements, got 1028"):
        f(q, odd_head, kp, table, lay, lens)
    odd_page = torch.rand(20 * (2 * 16 * 64 + 4)).bfloat16().as_strided((20, 2, 16, 64), (2 * 16 * 64 + 4, 16 * 64, 64, 1))
    with pytest.raises(ValueError, match=what + "v_pages's page stride must be a multiple of 8 elements, got 2052"):
        f(q, kp, odd_page, table, lay, lens)
    shifted = torch.rand(20 * 2 * 16 * 64 + 8).bfloat16()[4:4 + 20 * 2 * 16 * 64].reshape(20, 2, 16, 64)
    if shifted.data_ptr() % 16 != 0:
        with pytest.raises(ValueError, match=what + "k_pages's data pointer must be 16-byte aligned"):
            f(q, shifted, kp, table, lay, lens)
    # the shared refusals, with their types
    with pytest.raises(ValueError, match=what + "layout must be a CSR tensor"):
        f(q, kp, kp, table, lay.to_dense(), lens)
    with pytest.raises(ValueError, match=what + "q must be bfloat16 or float16, got torch.float32"):
        f(q.float(), kp, kp, table, lay, lens)
    with pytest.raises(ValueError, match=what + "v_pages must be a dense tensor"):
        f(q, kp, lay, table, lay, lens)
    with pytest.raises(RuntimeError, match=what + "q is torch.bfloat16 but v_pages is torch.float16"):
        f(q, kp, kp.half(), table, lay, lens)
    for bad in (32, 0, -64, 96, True, 64.0):
        with pytest.raises(ValueError, match=what + "block must be a positive multiple of 64"):
            f(q, kp, kp, table, lay, lens, block=bad)
    for bad in (0, -1, 2.0, True, "4", 2 ** 31):
        with pytest.raises(ValueError, match=what + "chunk must be None or a positive int"):
            f(q, kp, kp, table, lay, lens, chunk=bad)
    with pytest.raises(ValueError, match=what + "head size D must be 32, 64, 96 or 128, got 48"):
        f(q[..., :48], kp[..., :48], kp[..., :48], table, lay, lens)
    with pytest.raises(ValueError, match=what + "34 query heads over 2 k / v heads is a group of 17; 1 to 16 are taken"):
        f(torch.rand(2, 34, 1, 64).bfloat16(), kp, kp, table, lay, lens)
    with pytest.raises(ValueError, match=what + "q must hold T >= 1 new tokens"):
        f(q[:, :, :0], kp, kp, table, lay, lens)
    for bad in (_full(2), _full(4, (8,)), _full(4, (2, 8)), _full(4, (1, 2)), torch.ones(4, 3).to_sparse_csr()):
        with pytest.raises(ValueError, match=what + r"the layout must have shape \[\*l_lead, Smax/block, Smax/block\] = \[\*l_lead, 4, 4\]"):
            f(q, kp, kp, table, bad, lens)
    with pytest.raises(ValueError, match=what + "k_lens is required and must be a dense tensor"):
        f(q, kp, kp, table, lay, None)
    with pytest.raises(ValueError, match=what + "k_lens must be an int32 or int64 tensor, got torch.float32"):
        f(q, kp, kp, table, lay, torch.tensor([1.0, 2.0]))
    with pytest.raises(ValueError, match=what + r"k_lens must have shape \(2,\)"):
        f(q, kp, kp, table, lay, torch.tensor([1, 2, 3]))
    with pytest.raises(TypeError):  # keyword only
        f(q, kp, kp, table, lay, lens, 64, None, 4)
    k1, t1 = _pool(1, 1, 64, 32), torch.zeros(1, 1, dtype=torch.int32)
    with pytest.raises(ValueError, match=what + r"B·Hkv = 1 and T = 65536 must each be at most 65535"):
        f(torch.empty(1, 1, 65536, 32).bfloat16(), k1, k1, t1, _full(1), torch.tensor(5))
    # host tensors: the last check, RuntimeError — also for an empty pool and the transposed pool view, which are accepted
    with pytest.raises(RuntimeError, match=what + r"layout, q, k_pages, v_pages, block_table, k_lens must be device \(HIP\) tensors"):
        f(q, kp, kp, table, lay, lens)
    with pytest.raises(RuntimeError, match=what + r"layout, q, k_pages, v_pages, block_table, k_lens must be device \(HIP\) tensors"):
        f(q, kp[:0], kp[:0], table.long(), lay, torch.tensor(7), chunk=3, return_lse=True)
    with pytest.raises(RuntimeError, match=what + r"layout, q, k_pages, v_pages, block_table, k_lens must be device \(HIP\) tensors"):
        tr = kp.transpose(1, 2).contiguous().transpose(1, 2)
        f(q, tr, tr, torch.zeros(2, 40, dtype=torch.int32)[:, :16], lay, lens)


def test_custom_mm_paged_binding_refuses_host_tensors_and_keywords(built):
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import custom_mm
    offs, col = torch.tensor([[0, 1]], dtype=torch.int32), torch.tensor([0], dtype=torch.int32)
    q, pool = torch.rand(1, 2, 1, 32).bfloat16(), torch.rand(5, 1, 16, 32).bfloat16()
    table = torch.zeros(1, 4, dtype=torch.int32)
    lens, lse = torch.tensor([5], dtype=torch.int32), torch.empty(1, 2, 1)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.block_attention_decode_paged(offs, col, 1, q, pool, pool, table, lens, 1.0, 4, torch.empty_like(q), lse)
    with pytest.raises(RuntimeError, match=r"(?s)(?=.*\bBFloat16\b)(?=.*\bHalf\b)"):
        custom_mm.block_attention_decode_paged(offs, col, 1, q, pool, pool.half(), table, lens, 1.0, 4, torch.empty_like(q), lse)
    with pytest.raises(TypeError):  # positional only
        custom_mm.block_attention_decode_paged(offs, col, 1, q, pool, pool, table, lens, 1.0, chunk=4, out=torch.empty_like(q), lse=lse)


def test_block_attention_decode_paged_takes(real):
    takes = real.block_attention_decode_paged_takes
    for dtype in (torch.bfloat16, torch.float16):
        for D in (32, 64, 96, 128):
            for page in (16, 32, 64, 128, 256, 1024):
                assert takes(dtype, D, 64, 4, page) and takes(dtype, D, 128, 16, page) and takes(dtype, D, 512, 1, page)
    for page in (8, 24, 48, 0, -16, 1, 16.0, True, None):
        assert not takes(torch.bfloat16, 64, 64, 4, page), page
    # … and whatever block_attention_decode_takes refuses
    assert not takes(torch.float32, 64, 64, 4, 16) and not takes(torch.bfloat16, 48, 64, 4, 16)
    assert not takes(torch.float16, 64, 96, 4, 16) and not takes(torch.float16, 64, 64, 17, 16) and not takes(torch.float16, 64, 64, 0, 64)


# ---- wiring on CPU tensors, float64 stand-in arithmetic on float16 storage -----------------------------------------

@pytest.fixture()
def mm(oracle_mod):
    """(matmuls bound to the float64 stand-in, the stand-in)."""
    import fake_custom_mm_block_attention_decode_paged as fake
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


def _paged(g, k, v, page, extra=3, fill=NAN):
    """The cache k, v [B, Hkv, Smax, D] scattered into pools of B · W + extra pages under a seeded permutation (physical
    neighbours are not logical neighbours), unreferenced pages `fill`; returns (k_pages, v_pages, int32 table [B, W])."""
    B, Hkv, Smax, D = k.shape
    W = Smax // page
    P = B * W + extra
    table = torch.randperm(P, generator=g)[:B * W].reshape(B, W).to(torch.int32)
    pools = []
    for x in (k, v):
        pool = torch.full((P, Hkv, page, D), fill, dtype=x.dtype)
        pool[table.long().reshape(-1)] = x.reshape(B, Hkv, W, page, D).permute(0, 2, 1, 3, 4).reshape(B * W, Hkv, page, D)
        pools.append(pool)
    return pools[0], pools[1], table


def _gathered(pool, table):
    B, W = table.shape
    P, Hkv, page, D = pool.shape
    return pool[table.long().reshape(-1)].reshape(B, W, Hkv, page, D).permute(0, 2, 1, 3, 4).reshape(B, Hkv, W * page, D)


def _poison_pool(pool, table, vis):
    """NaN in every pool row that holds a key no token of its item sees (the pool's pages are not shared here)."""
    B, Hkv, T, Smax = vis.shape
    page = pool.shape[2]
    pool = pool.clone()
    unseen = ~vis.any(2)
    for b in range(B):
        for h in range(Hkv):
            for j in torch.nonzero(unseen[b, h]).flatten().tolist():
                pool[int(table[b, j // page]), h, j % page] = NAN
    return pool


@pytest.mark.parametrize("page", [16, 128])
@pytest.mark.parametrize("G,T,block,l_lead,k_lens", [
    (4, 3, 64, (), [130, 130]),                 # positions 127, 128, 129: two layout rows, a page boundary at 128
    (2, 3, 128, (), [130, 257]),                # block = 128
    (1, 2, 64, (2,), [65, 256]),                # a layout per k / v head
    (2, 3, 64, (2, 2), [0, 2]),                 # tokens that do not exist
    (16, 1, 64, (), [1, 300]),                  # (300: clamped to Smax)
])
def test_visibility_rule_against_a_dense_mask(mm, page, G, T, block, l_lead, k_lens):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(153 + G + T + page)
    B, Hkv, Smax, D = 2, 2, 256, 32
    layout = _random_layout(g, l_lead, Smax // block, keep=max(1, Smax // block - 1))
    lens = torch.tensor(k_lens, dtype=torch.int64)
    vis = _visible(layout, B, Hkv, T, Smax, block, k_lens)
    q = torch.randn(B, Hkv * G, T, D, generator=g).half()
    k, v = (torch.randn(B, Hkv, Smax, D, generator=g).half() for _ in range(2))
    want, want_lse = _dense_reference(q, k, v, vis, 1.0 / D ** 0.5, G)
    kp, vp, table = _paged(g, k, v, page)
    assert torch.equal(_gathered(kp, table), k)
    kp, vp = _poison_pool(kp, table, vis), _poison_pool(vp, table, vis)
    # the entries of logical pages no token sees are never consulted: out of range there
    unseen_pages = ~vis.any(2).any(1).reshape(B, Smax // page, page).any(-1)
    table[unseen_pages] = torch.tensor([-1, kp.shape[0] + 5], dtype=torch.int32).repeat(Smax)[:int(unseen_pages.sum())]
    out, lse = matmuls.block_sparse_attention_decode_paged(q, kp, vp, table, layout, lens, block=block, return_lse=True)
    assert out.dtype == torch.float16 and out.shape == q.shape and lse.dtype == torch.float32 and lse.shape == (B, Hkv * G, T)
    assert torch.isfinite(out).all()
    assert torch.allclose(out.double(), want, rtol=2e-3, atol=2e-3), float((out.double() - want).abs().max())
    seen = vis.any(-1).repeat_interleave(G, 1)
    assert (out[~seen] == 0).all() and (lse[~seen] == -float("inf")).all()
    assert torch.allclose(lse[seen].double(), want_lse[seen], rtol=1e-6, atol=1e-6)
    (name, rec), = [c for c in fake.calls if c[0] == "block_attention_decode_paged"]
    assert rec["k_lens"].dtype == torch.int32 and rec["k_lens"].tolist() == k_lens
    assert rec["chunk"] == matmuls._decode_chunk(Smax, D) and rec["scale"] == 1.0 / D ** 0.5
    # … and equals the contiguous call on the gathered cache (the stand-ins share their arithmetic)
    contiguous = matmuls.block_sparse_attention_decode(q, k, v, layout, lens, block=block)
    assert torch.equal(out, contiguous)


@pytest.mark.parametrize("page", [16, 128])
def test_an_out_of_range_entry_under_a_seen_key_hides_exactly_its_page(mm, page):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(171 + page)
    B, Hkv, G, T, Smax, D = 2, 2, 2, 2, 256, 32
    k_lens = [200, 256]
    layout = _random_layout(g, (), 4, keep=4)  # every block listed: the mask is causal
    vis = _visible(layout, B, Hkv, T, Smax, 64, k_lens)
    q = torch.randn(B, Hkv * G, T, D, generator=g).half()
    k, v = (torch.randn(B, Hkv, Smax, D, generator=g).half() for _ in range(2))
    kp, vp, table = _paged(g, k, v, page)
    P = kp.shape[0]
    hidden = {0: (0, -1), 1: (Smax // page - 1, P)}  # item → (logical page, the entry it gets): −1 and the first past the pool
    for b, (lp, entry) in hidden.items():
        assert vis[b, :, :, lp * page:(lp + 1) * page].any()  # seen keys
        kp[int(table[b, lp])] = NAN   # whoever loaded the page's old rows would show
        vp[int(table[b, lp])] = NAN
        table[b, lp] = entry
        vis[b, :, :, lp * page:(lp + 1) * page] = False
    want, want_lse = _dense_reference(q, k, v, vis, 1.0 / D ** 0.5, G)
    out, lse = matmuls.block_sparse_attention_decode_paged(q, kp, vp, table, layout, torch.tensor(k_lens), return_lse=True)
    assert torch.isfinite(out).all()
    assert torch.allclose(out.double(), want, rtol=2e-3, atol=2e-3)
    assert torch.allclose(lse.double(), want_lse, rtol=1e-6, atol=1e-6)
    # an item whose seen entries are all invalid: zero rows, lse −inf; an empty pool does the same for all
    table[0] = -1
    out, lse = matmuls.block_sparse_attention_decode_paged(q, kp, vp, table, layout, torch.tensor(k_lens), return_lse=True)
    assert (out[0] == 0).all() and (lse[0] == -float("inf")).all() and torch.isfinite(lse[1]).all()
    out, lse = matmuls.block_sparse_attention_decode_paged(q, kp[:0], vp[:0], table, layout, torch.tensor(k_lens), return_lse=True)
    assert (out == 0).all() and (lse == -float("inf")).all()


def test_the_pool_and_the_table_reach_the_binding_uncopied(mm):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(181)
    B, Hkv, Smax, D, G, page = 2, 2, 128, 32, 2, 16
    W = Smax // page
    layout = _random_layout(g, (), 2, keep=2)
    q = torch.randn(B, Hkv * G, 1, D, generator=g).half()
    lens = torch.tensor([100, 128])
    k, v = (torch.randn(B, Hkv, Smax, D, generator=g).half() for _ in range(2))
    plain_k, plain_v, table = _paged(g, k, v, page, fill=0.0)
    P = plain_k.shape[0]
    # [P, page, Hkv, D].transpose(1, 2), and a row stride > D inside a wider buffer
    phd_k, phd_v = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (plain_k, plain_v))
    wide_k, wide_v = (torch.zeros(P, Hkv, page, D + 8).half() for _ in range(2))
    wide_k[..., :D], wide_v[..., :D] = plain_k, plain_v
    # an int32 table as a slice of a wider one: handed over as it is
    wider = torch.full((B, W + 5), -1, dtype=torch.int32)
    wider[:, :W] = table
    sliced = wider[:, :W]
    assert not sliced.is_contiguous() and sliced.stride() == (W + 5, 1)
    want = matmuls.block_sparse_attention_decode(q, k, v, layout, lens)
    for kk, vv, tt in ((plain_k, plain_v, table), (phd_k, phd_v, sliced), (wide_k[..., :D], wide_v[..., :D], sliced)):
        fake.calls.clear()
        out = matmuls.block_sparse_attention_decode_paged(q, kk, vv, tt, layout, lens)
        (name, rec), = [c for c in fake.calls if c[0] == "block_attention_decode_paged"]
        assert rec["k_ptr"] == kk.data_ptr() and rec["k_stride"] == tuple(kk.stride())
        assert rec["v_ptr"] == vv.data_ptr() and rec["v_stride"] == tuple(vv.stride())
        assert rec["table_ptr"] == tt.data_ptr() and rec["table_stride"] == tuple(tt.stride()) and rec["table_dtype"] == torch.int32
        assert torch.equal(out, want)
    assert phd_k.stride() == (page * Hkv * D, D, Hkv * D, 1) and wide_k[..., :D].stride(2) == D + 8
    # an int64 table arrives as int32, with the same values
    fake.calls.clear()
    out = matmuls.block_sparse_attention_decode_paged(q, plain_k, plain_v, sliced.long(), layout, lens)
    (name, rec), = [c for c in fake.calls if c[0] == "block_attention_decode_paged"]
    assert rec["table_dtype"] == torch.int32 and rec["table_shape"] == (B, W) and torch.equal(out, want)
    # a strided q is made contiguous; one 0-d length serves all
    qt = torch.cat([q, q], -1)[..., :D]
    assert torch.equal(matmuls.block_sparse_attention_decode_paged(qt, plain_k, plain_v, table, layout, lens), want)
    one = matmuls.block_sparse_attention_decode_paged(q, plain_k, plain_v, table, layout, torch.tensor(100, dtype=torch.int32), chunk=5)
    assert torch.equal(one[0], want[0]) and fake.calls[-1][1]["chunk"] == 5 and fake.calls[-1][1]["k_lens"].tolist() == [100]


def test_the_layout_record_is_shared_with_the_other_attention_calls(mm):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(191)
    Smax, D, page = 256, 32, 32
    layout = _random_layout(g, (), 2, keep=2)  # in blocks of 128
    q = torch.randn(1, 2, Smax, D, generator=g).half()
    k, v = (torch.randn(1, 2, Smax, D, generator=g).half() for _ in range(2))
    kp, vp, table = _paged(g, k, v, page, fill=0.0)
    matmuls.block_sparse_attention(q, k, v, layout, block=128, causal=True)
    st = matmuls._csr_state(layout)
    rec = st.block_layouts[(str(q.device), 2)]
    matmuls.block_sparse_attention_decode(q[:, :, -1:], k, v, layout, torch.tensor([Smax]), block=128)
    matmuls.block_sparse_attention_decode_paged(q[:, :, -1:], kp, vp, table, layout, torch.tensor([Smax]), block=128)
    assert list(st.block_layouts) == [(str(q.device), 2)] and st.block_layouts[(str(q.device), 2)] is rec
    assert rec["t"] is None  # only rec['fwd'] is used
    (name, call), = [c for c in fake.calls if c[0] == "block_attention_decode_paged"]
    (_, other), = [c for c in fake.calls if c[0] == "block_attention_decode"]
    assert call["offsets_ptr"] == rec["fwd"][0].data_ptr() == other["offsets_ptr"]
    # and the other way round: a layout first seen by the paged call
    fresh = _random_layout(g, (), 4, keep=2)
    matmuls.block_sparse_attention_decode_paged(q[:, :, -1:], kp, vp, table, fresh, torch.tensor([Smax]))
    rec = matmuls._csr_state(fresh).block_layouts[(str(q.device), 1)]
    matmuls.block_sparse_attention_decode(q[:, :, -1:], k, v, fresh, torch.tensor([Smax]))
    matmuls.block_sparse_attention(q, k, v, fresh)
    assert matmuls._csr_state(fresh).block_layouts[(str(q.device), 1)] is rec


def test_return_lse_and_no_autograd(mm):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(197)
    layout = _random_layout(g, (), 2, keep=2)
    q = torch.randn(1, 2, 1, 32, generator=g).half().requires_grad_(True)
    kp, vp = (torch.randn(8, 1, 16, 32, generator=g).half().requires_grad_(True) for _ in range(2))
    table, lens = torch.arange(8).reshape(1, 8), torch.tensor([128])
    out = matmuls.block_sparse_attention_decode_paged(q, kp, vp, table, layout, lens)
    assert isinstance(out, torch.Tensor) and not out.requires_grad and out.grad_fn is None
    both = matmuls.block_sparse_attention_decode_paged(q, kp, vp, table, layout, lens, return_lse=True)
    assert isinstance(both, tuple) and len(both) == 2 and torch.equal(both[0], out)
    assert both[1].shape == (1, 2, 1) and both[1].dtype == torch.float32 and not both[1].requires_grad
