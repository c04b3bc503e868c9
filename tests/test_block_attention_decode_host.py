"""matmuls.block_sparse_attention_decode without a GPU: every refusal with its exception type, before the
device; block_attention_decode_takes; the visibility rule (token t at pos = k_len − T + t sees key j iff j ≤ pos and the
layout lists block (pos // block, j // block)) against a dense mask built here, through the float64 stand-in
tests/fake_custom_mm_block_attention_decode.py; the cache handed to the binding with its own data_ptr and strides; the
layout record shared with block_sparse_attention; return_lse; and the decode entries of the C ABI: declared, exported,
MI_EINVAL / MI_ENOMEM before any HIP call."""
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
OK, EINVAL, ENOMEM = 0, -1, -4
FAKE = 0x1000  # a non-null, 16-byte aligned address that is never dereferenced: every call below returns before the device


# ---- the C ABI -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(built):
    import torch  # noqa: F401  (torch's HIP runtime first, as in the product)
    lib = ctypes.CDLL(str(built / "libmi_spmm.so"))
    vp, i64, i32, f32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_size_t
    for s in SUFFIXES:
        fn = getattr(lib, f"mi_block_attention_decode_{s}")
        fn.argtypes = [vp, vp, i64] + 6 * [i32] + [vp, i64, i64] + 2 * [vp, i64, i64, i64] + [vp, i32, i32, i32, f32] + \
            [vp, i64, i64, vp, vp, sz, vp]
        fn.restype = ctypes.c_int
    lib.mi_block_attention_decode_workspace_bytes.argtypes = 6 * [i32]
    lib.mi_block_attention_decode_workspace_bytes.restype = sz
    return lib


def test_header_declares_and_library_exports_the_decode_entries(lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in ("mi_block_attention_decode_workspace_bytes",) + tuple(f"mi_block_attention_decode_{s}" for s in SUFFIXES):
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(lib, name), name


def test_workspace_holds_group_rows_per_item_token_and_chunk(lib):
    ws = lib.mi_block_attention_decode_workspace_bytes
    assert ws(6, 3, 5, 128, 512, 2) == 6 * 3 * 4 * 5 * (128 + 2) * 4      # 8 blocks in chunks of 2: G rows each, not 16
    assert ws(6, 3, 5, 128, 512, 3) == 6 * 3 * 3 * 5 * (128 + 2) * 4      # ceil(8 / 3)
    assert ws(6, 3, 5, 128, 512, 8) == 0 and ws(6, 3, 5, 128, 512, 64) == 0  # one chunk: no second launch, no workspace
    assert ws(0, 3, 5, 128, 512, 2) == 0 and ws(6, 3, 5, 128, 512, 0) == 0


DEFAULTS = dict(nnz=4, layouts=1, items=8, heads=2, T=1, Smax=512, D=64, q=FAKE, ldq=None, k=FAKE, ldk=None, headK=512 * 64,
                batchK=2 * 512 * 64, k_lens=FAKE, lens_count=4, group=4, chunk=2, out=FAKE, lse=FAKE, ws=FAKE, ws_bytes=1 << 30)


def decode(lib, s, **kw):
    a = {**DEFAULTS, **kw}
    D = a["D"]
    ldq, ldk = (D if a[n] is None else a[n] for n in ("ldq", "ldk"))
    return getattr(lib, f"mi_block_attention_decode_{s}")(
        FAKE, FAKE, a["nnz"], a["layouts"], a["items"], a["heads"], a["T"], a["Smax"], D, a["q"], ldq, a["T"] * ldq, a["k"], ldk,
        a["headK"], a["batchK"], FAKE, D, 512 * D, 2 * 512 * D, a["k_lens"], a["lens_count"], a["group"], a["chunk"], 1.0, a["out"],
        D, a["T"] * D, a["lse"], a["ws"], a["ws_bytes"], None)


@pytest.mark.parametrize("s", SUFFIXES)
def test_decode_entries_validate_before_any_hip_call(lib, s):
    for kw in ({"group": 0}, {"group": 17}, {"group": -1},                                     # group outside [1, 16]
               {"D": 48}, {"D": 256}, {"D": 0},                                                # a bad D
               {"chunk": 0}, {"chunk": -3},                                                    # chunk < 1
               {"items": 65536}, {"T": 65536},                                                 # beyond the grid
               {"Smax": 500}, {"nnz": -1}, {"layouts": 0}, {"heads": 3}, {"heads": 0},
               {"lens_count": 0}, {"lens_count": 3}, {"k_lens": None}, {"k_lens": FAKE + 2},
               {"q": None}, {"q": FAKE + 8}, {"out": FAKE + 2}, {"lse": None}, {"lse": FAKE + 1},   # misaligned / null pointers
               {"k": None}, {"k": FAKE + 8}, {"ldk": 60}, {"ldk": 68}, {"headK": 4}, {"batchK": 12}, {"ldq": 60},  # strides
               {"ws": None}, {"ws": FAKE + 4}):
        assert decode(lib, s, **kw) == EINVAL, kw
    need = lib.mi_block_attention_decode_workspace_bytes(8, 1, 4, 64, 512, 2)
    assert need > 0 and decode(lib, s, ws_bytes=need - 1) == ENOMEM and decode(lib, s, ws_bytes=0) == ENOMEM
    # an empty problem is MI_OK after the argument checks that need no operand; a bad group is refused even then
    assert decode(lib, s, items=0, q=None) == OK and decode(lib, s, T=0, k_lens=None) == OK
    assert decode(lib, s, items=0, group=0) == EINVAL and decode(lib, s, T=0, chunk=0) == EINVAL


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
    f = real.block_sparse_attention_decode
    what = "block_sparse_attention_decode: "
    q = torch.rand(2, 8, 1, 64).bfloat16()
    k = torch.rand(2, 2, 256, 64).bfloat16()
    lay, lens = _full(4), torch.tensor([100, 256])
    with pytest.raises(ValueError, match=what + "layout must be a CSR tensor"):
        f(q, k, k, lay.to_dense(), lens)
    with pytest.raises(ValueError, match=what + "q must be bfloat16 or float16, got torch.float32"):
        f(q.float(), k, k, lay, lens)
    with pytest.raises(ValueError, match=what + "v must be a dense tensor"):
        f(q, k, lay, lay, lens)
    with pytest.raises(RuntimeError, match=what + "q is torch.bfloat16 but v is torch.float16"):
        f(q, k, k.half(), lay, lens)
    for bad in (32, 0, -64, 96, True, 64.0):
        with pytest.raises(ValueError, match=what + "block must be a positive multiple of 64"):
            f(q, k, k, lay, lens, block=bad)
    for bad in (0, -1, 2.0, True, "4", 2 ** 31):
        with pytest.raises(ValueError, match=what + "chunk must be None or a positive int"):
            f(q, k, k, lay, lens, chunk=bad)
    with pytest.raises(ValueError, match=what + r"q must be \[B, Hq, T, D\]"):
        f(q[0], k[0], k[0], lay, lens)
    with pytest.raises(ValueError, match=what + "head size D must be 32, 64, 96 or 128, got 48"):
        f(q[..., :48], k[..., :48], k[..., :48], lay, lens)
    for kk in (torch.rand(2, 3, 256, 64), torch.rand(1, 2, 256, 64), torch.rand(2, 2, 256, 32), torch.rand(2, 0, 256, 64)):
        with pytest.raises(ValueError, match=what + r"q of shape \(2, 8, 1, 64\) needs k \(2, 'Hkv', 'Smax', 64\) with Hkv a divisor of 8"):
            f(q, kk.bfloat16(), kk.bfloat16(), lay, lens)
    q34 = torch.rand(2, 34, 1, 64).bfloat16()
    with pytest.raises(ValueError, match=what + "34 query heads over 2 k / v heads is a group of 17; 1 to 16 are taken"):
        f(q34, k, k, lay, lens)
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
    with pytest.raises(ValueError, match=what + "k_lens is required and must be a dense tensor"):
        f(q, k, k, lay, [100, 256])
    with pytest.raises(TypeError):  # required
        f(q, k, k, lay)
    for bad in (torch.tensor([1.0, 2.0]), torch.tensor([True, False]), torch.tensor([1, 2], dtype=torch.int16)):
        with pytest.raises(ValueError, match=what + f"k_lens must be an int32 or int64 tensor, got {bad.dtype}"):
            f(q, k, k, lay, bad)
    for bad in (torch.tensor([1, 2, 3]), torch.tensor([[1, 2]]), torch.ones(2, 2, dtype=torch.int64)):
        with pytest.raises(ValueError, match=what + r"k_lens must have shape \(2,\)"):
            f(q, k, k, lay, bad)
    with pytest.raises(TypeError):  # keyword only
        f(q, k, k, lay, lens, 64, None, 4)
    # the grid: B·Hkv and T
    big = torch.empty(65536, 1, 64, 32).bfloat16()
    with pytest.raises(ValueError, match=what + r"B·Hkv = 65536 and T = 1 must each be at most 65535"):
        f(torch.empty(65536, 1, 1, 32).bfloat16(), big, big, _full(1), torch.zeros(65536, dtype=torch.int32))
    k1 = torch.empty(1, 1, 64, 32).bfloat16()
    with pytest.raises(ValueError, match=what + r"B·Hkv = 1 and T = 65536 must each be at most 65535"):
        f(torch.empty(1, 1, 65536, 32).bfloat16(), k1, k1, _full(1), torch.tensor(5))
    # the cache's strides: ValueError naming the stride, never a silent copy
    wide = torch.rand(2, 2, 256, 128).bfloat16()
    with pytest.raises(ValueError, match=what + "k must have a last stride of 1, got 2"):
        f(q, wide[..., ::2], k, lay, lens)
    with pytest.raises(ValueError, match=what + "v's row stride must be a multiple of 8 elements and at least D = 64, got 68"):
        f(q, k, torch.rand(2, 2, 256, 68).bfloat16()[..., :64], lay, lens)
    with pytest.raises(ValueError, match=what + "k's row stride must be a multiple of 8 elements and at least D = 64, got 0"):
        f(q, k[:, :, :1].expand(2, 2, 256, 64), k, lay, lens)
    odd_head = torch.rand(2, 2 * (256 * 64 + 4)).bfloat16().as_strided((2, 2, 256, 64), (2 * (256 * 64 + 4), 256 * 64 + 4, 64, 1))
    with pytest.raises(ValueError, match=what + "k's head stride must be a multiple of 8 elements, got 16388"):
        f(q, odd_head, k, lay, lens)
    odd_batch = torch.rand(2 * (2 * 256 * 64 + 4)).bfloat16().as_strided((2, 2, 256, 64), (2 * 256 * 64 + 4, 256 * 64, 64, 1))
    with pytest.raises(ValueError, match=what + "v's batch stride must be a multiple of 8 elements, got 32772"):
        f(q, k, odd_batch, lay, lens)
    shifted = torch.rand(2 * 2 * 256 * 64 + 8).bfloat16()[4:4 + 2 * 2 * 256 * 64].reshape(2, 2, 256, 64)
    if shifted.data_ptr() % 16 != 0:
        with pytest.raises(ValueError, match=what + "k's data pointer must be 16-byte aligned"):
            f(q, shifted, k, lay, lens)
    # host tensors: the last check, RuntimeError
    with pytest.raises(RuntimeError, match=what + r"layout, q, k, v, k_lens must be device \(HIP\) tensors"):
        f(q, k, k, lay, lens)
    with pytest.raises(RuntimeError, match=what + r"layout, q, k, v, k_lens must be device \(HIP\) tensors"):
        f(q, k.transpose(1, 2).contiguous().transpose(1, 2), k, lay, torch.tensor(7), chunk=3, return_lse=True)


def test_custom_mm_decode_binding_refuses_host_tensors_and_keywords(built):
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import custom_mm
    offs, col = torch.tensor([[0, 1]], dtype=torch.int32), torch.tensor([0], dtype=torch.int32)
    q, kv = torch.rand(1, 2, 1, 32).bfloat16(), torch.rand(1, 1, 64, 32).bfloat16()
    lens, lse = torch.tensor([5], dtype=torch.int32), torch.empty(1, 2, 1)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.block_attention_decode(offs, col, 1, q, kv, kv, lens, 1.0, 4, torch.empty_like(q), lse)
    with pytest.raises(RuntimeError, match=r"(?s)(?=.*\bBFloat16\b)(?=.*\bHalf\b)"):
        custom_mm.block_attention_decode(offs, col, 1, q, kv, kv.half(), lens, 1.0, 4, torch.empty_like(q), lse)
    with pytest.raises(TypeError):  # positional only
        custom_mm.block_attention_decode(offs, col, 1, q, kv, kv, lens, 1.0, chunk=4, out=torch.empty_like(q), lse=lse)


def test_block_attention_decode_takes(real):
    takes = real.block_attention_decode_takes
    for dtype in (torch.bfloat16, torch.float16):
        for D in (32, 64, 96, 128):
            for block in (64, 128, 512):
                for group in (1, 5, 16):
                    assert takes(dtype, D, block, group)
    assert not takes(torch.float32, 64, 64, 4) and not takes(torch.bfloat16, 48, 64, 4) and not takes(torch.bfloat16, 256, 64, 4)
    assert not takes(torch.float16, 64, 32, 4) and not takes(torch.float16, 64, 96, 4) and not takes(torch.float16, 64, True, 4)
    assert not takes(torch.float16, 64, 64, 0) and not takes(torch.float16, 64, 64, 17) and not takes(torch.float16, 64, 64, True)
    assert not takes(torch.float16, 64, 64, 2.0)


# ---- wiring on CPU tensors, float64 stand-in arithmetic on float16 storage -----------------------------------------

@pytest.fixture()
def mm(oracle_mod):
    """(matmuls bound to the float64 stand-in, the stand-in)."""
    import fake_custom_mm_block_attention_decode as fake
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


def _visible(layout, B, Hkv, T, Smax, block, k_lens):
    """Boolean [B, Hkv, T, Smax] built from the rule alone: token t of item b at pos = k_len − T + t sees key j iff
    j ≤ pos and the dense form of the layout holds block (pos // block, j // block); layouts indexed by the k / v item."""
    dense = torch.sparse_csr_tensor(layout.crow_indices(), layout.col_indices(), torch.ones_like(layout.values()),
                                    size=layout.shape).to_dense() != 0
    dense = dense.reshape((-1,) + tuple(dense.shape[-2:]))
    vis = torch.zeros(B, Hkv, T, Smax, dtype=torch.bool)
    for b in range(B):
        for h in range(Hkv):
            lay = dense[(b * Hkv + h) % dense.shape[0]]
            for t in range(T):
                pos = min(max(int(k_lens[b]), 0), Smax) - T + t
                for j in range(0, max(pos + 1, 0)):
                    vis[b, h, t, j] = bool(lay[pos // block, j // block])
    return vis


def _dense_reference(q, k, v, vis, scale, G):
    """(out, lse) of dense masked attention in float64; rows that see nothing: zero and −inf.  Unseen keys are zeroed first."""
    qd = q.double()
    kd = torch.where(vis.any(2)[..., None], k.double(), torch.zeros((), dtype=torch.float64)).repeat_interleave(G, 1)
    vd = torch.where(vis.any(2)[..., None], v.double(), torch.zeros((), dtype=torch.float64)).repeat_interleave(G, 1)
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


@pytest.mark.parametrize("G,T,block,l_lead,k_lens", [
    (4, 3, 64, (), [130, 130]),                 # positions 127, 128, 129: two layout rows
    (2, 3, 128, (), [130, 257]),                # block = 128: the rows of the 128-grid
    (1, 2, 64, (2,), [65, 256]),                # a layout per k / v head
    (4, 1, 64, (2, 2), [200, 64]),              # a layout per k / v item
    (2, 3, 64, (2,), [0, 2]),                   # k_len = 0 and k_len < T: tokens that do not exist
    (16, 1, 64, (), [1, 300]),                  # (300: clamped to Smax)
])
def test_visibility_rule_against_a_dense_mask(mm, G, T, block, l_lead, k_lens):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(53 + G + T)
    B, Hkv, Smax, D = 2, 2, 256, 32
    layout = _random_layout(g, l_lead, Smax // block, keep=max(1, Smax // block - 1))
    lens = torch.tensor(k_lens, dtype=torch.int64)
    vis = _visible(layout, B, Hkv, T, Smax, block, k_lens)
    q = torch.randn(B, Hkv * G, T, D, generator=g).half()
    k, v = (torch.randn(B, Hkv, Smax, D, generator=g).half() for _ in range(2))
    want, want_lse = _dense_reference(q, k, v, vis, 1.0 / D ** 0.5, G)
    out, lse = matmuls.block_sparse_attention_decode(q, _poison_unseen(k, vis), _poison_unseen(v, vis), layout, lens, block=block,
                                                     return_lse=True)
    assert out.dtype == torch.float16 and out.shape == q.shape and lse.dtype == torch.float32 and lse.shape == (B, Hkv * G, T)
    assert torch.isfinite(out).all()
    assert torch.allclose(out.double(), want, rtol=2e-3, atol=2e-3), float((out.double() - want).abs().max())
    seen = vis.any(-1).repeat_interleave(G, 1)
    assert (out[~seen] == 0).all() and (lse[~seen] == -float("inf")).all()
    assert torch.allclose(lse[seen].double(), want_lse[seen], rtol=1e-6, atol=1e-6)
    for b, n in enumerate(k_lens):  # a token with pos < 0 does not exist
        for t in range(T):
            if min(n, Smax) - T + t < 0:
                assert not seen[b, :, t].any()
    (name, rec), = [c for c in fake.calls if c[0] == "block_attention_decode"]
    assert rec["k_lens"].dtype == torch.int32 and rec["k_lens"].tolist() == k_lens      # as given: the kernel clamps
    assert rec["layouts"] == max(1, int(torch.tensor(l_lead).prod()) if l_lead else 1)
    assert rec["chunk"] == matmuls._DECODE_CHUNK and rec["scale"] == 1.0 / D ** 0.5


def test_one_length_for_all_as_a_0d_tensor(mm):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(59)
    layout = _random_layout(g, (), 4, keep=3)
    q = torch.randn(2, 4, 2, 32, generator=g).half()
    k, v = (torch.randn(2, 2, 256, 32, generator=g).half() for _ in range(2))
    got = matmuls.block_sparse_attention_decode(q, k, v, layout, torch.tensor(131, dtype=torch.int32), chunk=5, scale=0.25)
    want = matmuls.block_sparse_attention_decode(q, k, v, layout, torch.tensor([131, 131]), chunk=5, scale=0.25)
    assert torch.equal(got, want)
    first, second = [c[1] for c in fake.calls if c[0] == "block_attention_decode"]
    assert first["k_lens"].tolist() == [131] and second["k_lens"].tolist() == [131, 131]
    assert first["chunk"] == 5 and first["scale"] == 0.25


def test_the_cache_reaches_the_binding_with_its_own_pointer_and_strides(mm):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(61)
    B, Hkv, Smax, D, G = 2, 2, 128, 32, 2
    layout = _random_layout(g, (), 2, keep=2)
    q = torch.randn(B, Hkv * G, 1, D, generator=g).half()
    lens = torch.tensor([100, 128])
    plain_k, plain_v = (torch.randn(B, Hkv, Smax, D, generator=g).half() for _ in range(2))
    # [B, Smax, Hkv, D].transpose(1, 2), and a row stride > D inside a wider buffer
    bshd_k, bshd_v = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (plain_k, plain_v))
    wide_k, wide_v = (torch.zeros(B, Hkv, Smax, D + 8).half() for _ in range(2))
    wide_k[..., :D], wide_v[..., :D] = plain_k, plain_v
    want = None
    for kk, vv in ((plain_k, plain_v), (bshd_k, bshd_v), (wide_k[..., :D], wide_v[..., :D])):
        fake.calls.clear()
        out = matmuls.block_sparse_attention_decode(q, kk, vv, layout, lens)
        (name, rec), = [c for c in fake.calls if c[0] == "block_attention_decode"]
        assert rec["k_ptr"] == kk.data_ptr() and rec["k_stride"] == tuple(kk.stride())
        assert rec["v_ptr"] == vv.data_ptr() and rec["v_stride"] == tuple(vv.stride())
        want = out if want is None else want
        assert torch.equal(out, want)
    assert bshd_k.stride() == (Smax * Hkv * D, D, Hkv * D, 1) and wide_k[..., :D].stride(2) == D + 8
    # q is small: a strided q is made contiguous
    qt = torch.cat([q, q], -1)[..., :D]
    assert not qt.is_contiguous() and torch.equal(matmuls.block_sparse_attention_decode(qt, plain_k, plain_v, layout, lens), want)


def test_the_layout_record_is_shared_with_block_sparse_attention(mm):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(67)
    Smax, D = 256, 32
    layout = _random_layout(g, (), 2, keep=2)  # in blocks of 128
    q = torch.randn(1, 2, Smax, D, generator=g).half()
    k, v = (torch.randn(1, 2, Smax, D, generator=g).half() for _ in range(2))
    matmuls.block_sparse_attention(q, k, v, layout, block=128, causal=True)
    st = matmuls._csr_state(layout)
    assert list(st.block_layouts) == [(str(q.device), 2)]
    rec = st.block_layouts[(str(q.device), 2)]
    matmuls.block_sparse_attention_decode(q[:, :, -1:], k, v, layout, torch.tensor([Smax]), block=128)
    assert list(st.block_layouts) == [(str(q.device), 2)] and st.block_layouts[(str(q.device), 2)] is rec
    assert rec["t"] is None  # only rec['fwd'] is used
    (name, call), = [c for c in fake.calls if c[0] == "block_attention_decode"]
    assert call["offsets_ptr"] == rec["fwd"][0].data_ptr()
    # and the other way round: a layout first seen by the decode call
    other = _random_layout(g, (), 4, keep=2)
    matmuls.block_sparse_attention_decode(q[:, :, -1:], k, v, other, torch.tensor([Smax]))
    rec = matmuls._csr_state(other).block_layouts[(str(q.device), 1)]
    matmuls.block_sparse_attention(q, k, v, other)
    assert matmuls._csr_state(other).block_layouts[(str(q.device), 1)] is rec


def test_return_lse_and_no_autograd(mm):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(71)
    layout = _random_layout(g, (), 2, keep=2)
    q = torch.randn(1, 2, 1, 32, generator=g).half().requires_grad_(True)
    k, v = (torch.randn(1, 1, 128, 32, generator=g).half().requires_grad_(True) for _ in range(2))
    lens = torch.tensor([128])
    out = matmuls.block_sparse_attention_decode(q, k, v, layout, lens)
    assert isinstance(out, torch.Tensor) and not out.requires_grad and out.grad_fn is None
    both = matmuls.block_sparse_attention_decode(q, k, v, layout, lens, return_lse=True)
    assert isinstance(both, tuple) and len(both) == 2 and torch.equal(both[0], out)
    assert both[1].shape == (1, 2, 1) and both[1].dtype == torch.float32 and not both[1].requires_grad
    # the last token of a causal prefill sees what the decode token sees
    full = torch.randn(1, 2, 128, 32, generator=g).half()
    full[:, :, -1] = q.detach()[:, :, 0]
    want = matmuls.block_sparse_attention(full, k.detach(), v.detach(), layout, causal=True)[:, :, -1:]
    assert torch.allclose(out.double(), want.double(), rtol=2e-3, atol=2e-3)
