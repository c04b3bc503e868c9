"""The speculative step without a GPU: tree_mask= of the eight decode calls, positions= of the two rope calls,
kv_cache_compact{,_paged} and tree_attention_mask.  Every refusal with its exception type, raised on host tensors by the real
extension's matmuls before a device call; the None paths reaching TODAY's bindings with today's argument lists and the new
operands reaching the new bindings as they are, through the stand-in tests/fake_custom_mm_spec_decode.py; tree_attention_mask
against a Python loop; and the new entries of the C ABI: declared, exported, MI_EINVAL / MI_OK before any HIP call."""
import ctypes
import importlib
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "mi_spmm.h"
OK, EINVAL = 0, -1
PTR = 0x1000  # a non-null, 16-byte aligned address that is never dereferenced: every call below returns before the device
F8 = torch.float8_e4m3fn
vp, i64, i32, f32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_size_t

TREE_ENTRIES = [(f"mi_block_attention_tree_decode{l}{p}{f}_{t}", bool(l), bool(p), bool(f))
                for l in ("", "_lists") for p in ("", "_paged") for f in ("", "_fp8") for t in ("bf16", "f16")]
ROPE_ENTRIES = [(f"mi_rope_pos_kv_append{p}{f}_{t}", bool(p), bool(f)) for p in ("", "_paged") for f in ("", "_fp8") for t in ("bf16", "f16")]


@pytest.fixture(scope="module")
def lib(built):
    import torch  # noqa: F401  (torch's HIP runtime first, as in the product)
    return ctypes.CDLL(str(built / "libmi_spmm.so"))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------

def test_the_new_entries_are_declared_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    names = [e[0] for e in TREE_ENTRIES] + [e[0] for e in ROPE_ENTRIES] + ["mi_kv_compact", "mi_kv_compact_paged"]
    assert len(TREE_ENTRIES) == 16 and len(ROPE_ENTRIES) == 8
    for name in names:
        assert re.search(rf"\bint {name}\(", text), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
    # the closed families of the header stay closed: no new name starts like an old one
    assert not any(n.startswith(("mi_block_attention_decode", "mi_rope_kv_append", "mi_kv_append")) for n in names)


def tree_call(lib, name, lists, paged, fp8, **change):
    a = dict(rowptr=PTR, col=PTR, nnz=1, layouts=1, block_ids=PTR, block_counts=PTR, K=1, items=2, heads=1, T=3, Smax=64,
             block_table=PTR, table_ld=4, pages=4, page=16, D=32, q=PTR, ldq=32, strideQ=96, k=PTR, ldk=32, headK=2048, outerK=2048,
             v=PTR, ldv=32, headV=2048, outerV=2048, k_lens=PTR, lens_count=1, group=1, chunk=1, scale=1.0, k_scale=PTR, k_scale_count=1,
             v_scale=PTR, v_scale_count=1, tree_mask=PTR, mask_rows=2, out=PTR, ldo=32, strideO=96, lse=PTR, workspace=None,
             workspace_bytes=0, stream=None)
    if paged:
        a.update(headK=512, outerK=512, headV=512, outerV=512)
    a.update(change)
    sig = ([("block_ids", vp), ("block_counts", vp), ("K", i32)] if lists else [("rowptr", vp), ("col", vp), ("nnz", i64), ("layouts", i32)])
    sig += [("items", i32), ("heads", i32), ("T", i32), ("Smax", i32)]
    sig += [("block_table", vp), ("table_ld", i64), ("pages", i32), ("page", i32)] if paged else []
    sig += [("D", i32), ("q", vp), ("ldq", i64), ("strideQ", i64), ("k", vp), ("ldk", i64), ("headK", i64), ("outerK", i64), ("v", vp),
            ("ldv", i64), ("headV", i64), ("outerV", i64), ("k_lens", vp), ("lens_count", i32), ("group", i32), ("chunk", i32), ("scale", f32)]
    sig += [("k_scale", vp), ("k_scale_count", i32), ("v_scale", vp), ("v_scale_count", i32)] if fp8 else []
    sig += [("tree_mask", vp), ("mask_rows", i32), ("out", vp), ("ldo", i64), ("strideO", i64), ("lse", vp), ("workspace", vp),
            ("workspace_bytes", sz), ("stream", vp)]
    fn = getattr(lib, name)
    fn.argtypes, fn.restype = [t for _, t in sig], ctypes.c_int
    return fn(*[a[n] for n, _ in sig])


@pytest.mark.parametrize("name,lists,paged,fp8", TREE_ENTRIES, ids=[e[0] for e in TREE_ENTRIES])
def test_tree_entries_validate_before_any_hip_call(lib, name, lists, paged, fp8):
    """Every row is refused (or, empty, answered) before a pointer is dereferenced: PTR is no memory.  The valid list itself is
    never sent: it would launch."""
    call = lambda **kw: tree_call(lib, name, lists, paged, fp8, **kw)  # noqa: E731
    assert call(tree_mask=None) == EINVAL
    assert call(tree_mask=PTR + 4) == EINVAL  # 8-byte alignment
    assert call(T=65, strideQ=65 * 32, strideO=65 * 32) == EINVAL
    for rows in (0, 3, -1):  # neither 1 nor the batch of 2
        assert call(mask_rows=rows) == EINVAL
    assert call(items=4, heads=2, mask_rows=4) == EINVAL  # the batch is items / heads = 2, not the items
    # the parent's refusals stand
    assert call(group=17) == EINVAL and call(chunk=0) == EINVAL and call(q=None) == EINVAL and call(k_lens=None) == EINVAL
    # the empty calls are answered as today, before the mask is looked at — but T > 64 is a size
    assert call(items=0, tree_mask=None, q=None) == OK and call(T=0, tree_mask=None, q=None) == OK
    assert call(items=0, T=65) == EINVAL


def rope_call(lib, name, paged, fp8, **change):
    a = dict(items=2, heads=1, T=3, Smax=64, block_table=PTR, table_ld=4, pages=4, page=16, D=32, q_heads=2, q=PTR, ldq=32, headQ=96,
             batchQ=192, q_out=PTR, ldqo=32, headQo=96, batchQo=192, k_new=PTR, ldkn=32, headKn=96, batchKn=96, v_new=PTR, ldvn=32,
             headVn=96, batchVn=96, k_out=None, ldko=32, headKo=0, batchKo=0, cos=PTR, sin=PTR, table_rows=64, ld=16, rotary_dim=32,
             interleaved=0, k=PTR, ldk=32, headK=2048, outerK=2048, v=PTR, ldv=32, headV=2048, outerV=2048, k_lens=PTR, lens_count=1,
             new_lens=None, positions=PTR, k_scale=PTR, k_scale_count=1, v_scale=PTR, v_scale_count=1, stream=None)
    if paged:
        a.update(headK=512, outerK=512, headV=512, outerV=512)
    a.update(change)
    sig = [("items", i32), ("heads", i32), ("T", i32), ("Smax", i32)]
    sig += [("block_table", vp), ("table_ld", i64), ("pages", i32), ("page", i32)] if paged else []
    sig += [("D", i32), ("q_heads", i32)]
    for n in ("q", "q_out", "k_new", "v_new", "k_out"):
        s = {"q": "Q", "q_out": "Qo", "k_new": "Kn", "v_new": "Vn", "k_out": "Ko"}[n]
        sig += [(n, vp), ("ld" + s.lower(), i64), ("head" + s, i64), ("batch" + s, i64)]
    sig += [("cos", vp), ("sin", vp), ("table_rows", i32), ("ld", i64), ("rotary_dim", i32), ("interleaved", i32)]
    sig += [("k", vp), ("ldk", i64), ("headK", i64), ("outerK", i64), ("v", vp), ("ldv", i64), ("headV", i64), ("outerV", i64)]
    sig += [("k_lens", vp), ("lens_count", i32), ("new_lens", vp), ("positions", vp)]
    sig += [("k_scale", vp), ("k_scale_count", i32), ("v_scale", vp), ("v_scale_count", i32)] if fp8 else []
    sig += [("stream", vp)]
    fn = getattr(lib, name)
    fn.argtypes, fn.restype = [t for _, t in sig], ctypes.c_int
    return fn(*[a[n] for n, _ in sig])


@pytest.mark.parametrize("name,paged,fp8", ROPE_ENTRIES, ids=[e[0] for e in ROPE_ENTRIES])
def test_rope_entries_with_positions_validate_before_any_hip_call(lib, name, paged, fp8):
    call = lambda **kw: rope_call(lib, name, paged, fp8, **kw)  # noqa: E731
    assert call(positions=None) == EINVAL and call(positions=PTR + 2) == EINVAL
    assert call(rotary_dim=8) == EINVAL and call(q=None) == EINVAL and call(k_lens=PTR + 2) == EINVAL  # the parent's refusals stand
    assert call(items=0, positions=None) == OK and call(T=0, positions=None) == OK


def compact_call(lib, paged, **change):
    a = dict(items=2, heads=1, T=3, Smax=64, block_table=PTR, table_ld=4, pages=4, page=16, D=32, elem_bytes=2, k=PTR, ldk=32,
             headK=512 if paged else 2048, outerK=512 if paged else 2048, v=PTR, ldv=32, headV=512 if paged else 2048,
             outerV=512 if paged else 2048, k_lens=PTR, lens_count=1, accept=PTR, accept_counts=PTR, stream=None)
    a.update(change)
    sig = [("items", i32), ("heads", i32), ("T", i32), ("Smax", i32)]
    sig += [("block_table", vp), ("table_ld", i64), ("pages", i32), ("page", i32)] if paged else []
    sig += [("D", i32), ("elem_bytes", i32), ("k", vp), ("ldk", i64), ("headK", i64), ("outerK", i64), ("v", vp), ("ldv", i64),
            ("headV", i64), ("outerV", i64), ("k_lens", vp), ("lens_count", i32), ("accept", vp), ("accept_counts", vp), ("stream", vp)]
    fn = lib.mi_kv_compact_paged if paged else lib.mi_kv_compact
    fn.argtypes, fn.restype = [t for _, t in sig], ctypes.c_int
    return fn(*[a[n] for n, _ in sig])


@pytest.mark.parametrize("paged", [False, True])
def test_compact_entries_validate_before_any_hip_call(lib, paged):
    call = lambda **kw: compact_call(lib, paged, **kw)  # noqa: E731
    for bad in (dict(elem_bytes=4), dict(elem_bytes=0), dict(T=65), dict(T=-1), dict(D=48), dict(items=65536), dict(heads=0),
                dict(items=3, heads=2), dict(lens_count=3), dict(k_lens=None), dict(k_lens=PTR + 2), dict(accept=None),
                dict(accept=PTR + 2), dict(accept_counts=None), dict(accept_counts=PTR + 2), dict(k=None), dict(v=PTR + 8),
                dict(ldk=16), dict(headV=4), dict(elem_bytes=1, ldk=40)):
        assert call(**bad) == EINVAL, bad
    if paged:
        for bad in (dict(page=8), dict(page=24), dict(block_table=None), dict(table_ld=3), dict(pages=-1)):
            assert call(**bad) == EINVAL, bad
        assert call(pages=0, k=None, v=None) == OK  # an empty pool: no row is touched
    assert call(items=0, k=None, accept=None) == OK and call(T=0, k=None, accept=None) == OK
    assert call(Smax=0, k=None, v=None, block_table=None) == OK


# ---- tree_attention_mask ---------------------------------------------------------------------------------------------------------

@pytest.fixture()
def real(built):
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import matmuls
    yield matmuls
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)


def loop_mask(parents):
    """(words as signed int64, depths) by the definition: bit i of word t iff i is t or an ancestor of t."""
    words, depths = [], []
    for t, p in enumerate(parents):
        bits, d, node = 1 << t, 0, p
        while node >= 0:
            bits |= 1 << node
            d += 1
            node = parents[node]
        words.append(bits - (1 << 64) if bits >= 1 << 63 else bits)
        depths.append(d)
    return words, depths


def test_tree_attention_mask_against_a_python_loop(real):
    g = np.random.Generator(np.random.PCG64(11))
    for T in (1, 2, 7, 63, 64):
        trees = [[t - 1 for t in range(T)], [-1] * T, [-1, -1][:T] + [t - 2 for t in range(2, T)]]
        trees += [[int(g.integers(-1, t)) for t in range(T)] for _ in range(5)]
        for dtype in (torch.int32, torch.int64):
            mask, depth = real.tree_attention_mask(torch.tensor(trees, dtype=dtype))
            assert mask.dtype == torch.int64 and depth.dtype == torch.int32 and mask.shape == depth.shape == (len(trees), T)
            assert mask.is_contiguous()
            for row, parents in enumerate(trees):
                words, depths = loop_mask(parents)
                assert mask[row].tolist() == words and depth[row].tolist() == depths, (T, parents)
        one = real.tree_attention_mask(torch.tensor(trees[-1]))  # [T]: the shared form
        assert one[0].shape == (T,) and one[0].tolist() == loop_mask(trees[-1])[0]
    chain = real.tree_attention_mask(torch.arange(-1, 63))[0]
    assert chain.tolist() == [x - (1 << 64) if x >= 1 << 63 else x for x in ((2 << t) - 1 for t in range(64))]  # the causal words


def test_tree_attention_mask_refusals(real):
    what = "tree_attention_mask: "
    for bad in (None, [0, 1], torch.zeros(3), torch.zeros(3, dtype=torch.bool), torch.zeros((), dtype=torch.int64),
                torch.zeros((2, 2, 2), dtype=torch.int64)):
        with pytest.raises(ValueError, match=what + "parents must be a dense integer tensor"):
            real.tree_attention_mask(bad)
    with pytest.raises(ValueError, match=what + "T = 65 must be at most 64"):
        real.tree_attention_mask(torch.full((65,), -1))
    for bad in ([0, 0, 1], [-1, 1, 0], [-2, 0, 1], [-1, 0, 3]):  # its own parent, a later parent, below −1, beyond T
        with pytest.raises(ValueError, match=what + r"parents\[t\] must lie in \[-1, t\)"):
            real.tree_attention_mask(torch.tensor(bad))


# ---- matmuls on the real extension: refusals before the device ----------------------------------------------------------------------

def _layout(blocks=4):
    crow = torch.arange(blocks + 1) * blocks
    col = torch.arange(blocks).repeat(blocks)
    return torch.sparse_csr_tensor(crow, col, torch.ones(blocks * blocks), size=(blocks, blocks))


def _decode_calls(m, T=3):
    """(name, f(tree_mask=…) → the call on host operands of valid shapes) of the eight calls; B = 2, Hkv = 2, Hq = 4."""
    B, Hkv, Hq, D, Smax, page = 2, 2, 4, 64, 256, 16
    q = torch.rand(B, Hq, T, D).bfloat16()
    k, pool = torch.rand(B, Hkv, Smax, D).bfloat16(), torch.rand(40, Hkv, page, D).bfloat16()
    k8, pool8 = k.to(F8), pool.to(F8)
    table = torch.arange(B * Smax // page, dtype=torch.int32).reshape(B, -1)
    lens, layout = torch.tensor([100, 256]), _layout()
    ids, counts = torch.zeros(B, Hkv, T, 3, dtype=torch.int32), torch.ones(B, Hkv, T, dtype=torch.int32)
    return [
        ("block_sparse_attention_decode", lambda **kw: m.block_sparse_attention_decode(q, k, k, layout, lens, **kw)),
        ("block_sparse_attention_decode_paged", lambda **kw: m.block_sparse_attention_decode_paged(q, pool, pool, table, layout, lens, **kw)),
        ("block_sparse_attention_decode_fp8", lambda **kw: m.block_sparse_attention_decode_fp8(q, k8, k8, layout, lens, **kw)),
        ("block_sparse_attention_decode_paged_fp8",
         lambda **kw: m.block_sparse_attention_decode_paged_fp8(q, pool8, pool8, table, layout, lens, **kw)),
        ("block_sparse_attention_decode_selected", lambda **kw: m.block_sparse_attention_decode_selected(q, k, k, ids, counts, lens, **kw)),
        ("block_sparse_attention_decode_selected_paged",
         lambda **kw: m.block_sparse_attention_decode_selected_paged(q, pool, pool, table, ids, counts, lens, **kw)),
        ("block_sparse_attention_decode_selected_fp8",
         lambda **kw: m.block_sparse_attention_decode_selected_fp8(q, k8, k8, ids, counts, lens, **kw)),
        ("block_sparse_attention_decode_selected_paged_fp8",
         lambda **kw: m.block_sparse_attention_decode_selected_paged_fp8(q, pool8, pool8, table, ids, counts, lens, **kw)),
    ]


def test_tree_mask_refusals_come_before_the_device_with_their_type(real):
    for name, f in _decode_calls(real):
        what = name + ": "
        for bad in ("x", [1, 3, 7], 7):
            with pytest.raises(ValueError, match=what + "tree_mask must be None or a dense int64 tensor"):
                f(tree_mask=bad)
        for bad in (torch.int32, torch.uint8, torch.float32, torch.bool):
            with pytest.raises(ValueError, match=what + r"tree_mask must be int64 .*got " + str(bad)):
                f(tree_mask=torch.ones(2, 3).to(bad))
        for bad in ((3, 2), (2, 4), (1, 3), (4,), (2, 3, 1), ()):
            with pytest.raises(ValueError, match=what + r"tree_mask must be \[B, T\] = \[2, 3\] or \[T\] = \[3\]"):
                f(tree_mask=torch.ones(bad, dtype=torch.int64))
        with pytest.raises(ValueError, match=what + "tree_mask must be contiguous"):
            f(tree_mask=torch.ones(2, 6, dtype=torch.int64)[:, ::2])
        with pytest.raises(RuntimeError, match=what + "tree_mask is on meta but q is on cpu"):
            f(tree_mask=torch.ones(2, 3, dtype=torch.int64, device="meta"))
        with pytest.raises(RuntimeError, match=what + r".*tree_mask must be device \(HIP\) tensors"):  # a host tensor: the last check
            f(tree_mask=torch.ones(2, 3, dtype=torch.int64))
        with pytest.raises(RuntimeError, match=what + r".*tree_mask must be device \(HIP\) tensors"):
            f(tree_mask=torch.ones(3, dtype=torch.int64))
        with pytest.raises(TypeError):  # keyword only
            f(None, None, None, None, None)
    for name, f in _decode_calls(real, T=65):
        with pytest.raises(ValueError, match=name + ": a tree mask needs T <= 64"):
            f(tree_mask=torch.ones(2, 65, dtype=torch.int64))


def _rope_operands(T=3):
    B, Hkv, Hq, D, Smax = 2, 2, 4, 64, 128
    q, kn = torch.rand(B, Hq, T, D).bfloat16(), torch.rand(B, Hkv, T, D).bfloat16()
    cos = torch.rand(Smax, D // 2)
    return q, kn, kn.clone(), cos, cos.clone(), torch.rand(B, Hkv, Smax, D).bfloat16(), torch.tensor([100, 128])


def test_positions_refusals_come_before_the_device_with_their_type(real):
    q, kn, vn, cos, sin, k, lens = _rope_operands()
    pool, table = torch.rand(20, 2, 16, 64).bfloat16(), torch.arange(16, dtype=torch.int32).reshape(2, 8)
    for what, f in (("rope_kv_cache_append: ", lambda **kw: real.rope_kv_cache_append(q, kn, vn, cos, sin, k, k.clone(), lens, **kw)),
                    ("rope_kv_cache_append_paged: ",
                     lambda **kw: real.rope_kv_cache_append_paged(q, kn, vn, cos, sin, pool, pool.clone(), table, lens, **kw))):
        for bad in ("x", [[1, 2, 3]] * 2, torch.ones(2, 3), torch.ones(2, 3, dtype=torch.int16), torch.ones(2, 3, dtype=torch.bool)):
            with pytest.raises(ValueError, match=what + "positions must be None or a dense int32 / int64 tensor"):
                f(positions=bad)
        for bad in ((3,), (2, 4), (3, 2), (2, 3, 1)):
            with pytest.raises(ValueError, match=what + r"positions must be \[B, T\] = \[2, 3\]"):
                f(positions=torch.ones(bad, dtype=torch.int64))
        with pytest.raises(RuntimeError, match=what + "positions is on meta but q is on cpu"):
            f(positions=torch.ones(2, 3, dtype=torch.int32, device="meta"))
        with pytest.raises(RuntimeError, match=what + r".*must be device \(HIP\) tensors"):  # host operands: the last check
            f(positions=torch.ones(2, 3, dtype=torch.int32))


def test_compact_refusals_come_before_the_device_with_their_type(real):
    B, Hkv, Smax, D, T = 2, 2, 128, 64, 4
    k, pool = torch.rand(B, Hkv, Smax, D).bfloat16(), torch.rand(20, Hkv, 16, D).bfloat16()
    table, lens = torch.arange(16, dtype=torch.int32).reshape(2, 8), torch.tensor([100, 128])
    accept, counts = torch.zeros(B, T, dtype=torch.int32), torch.ones(B, dtype=torch.int32)
    for what, kn, f, good in (("kv_cache_compact: ", "k", lambda k_, v_, *a: real.kv_cache_compact(k_, v_, lens, *a), k),
                              ("kv_cache_compact_paged: ", "k_pages", lambda k_, v_, *a: real.kv_cache_compact_paged(k_, v_, table, lens, *a),
                               pool)):
        vn = "v" if kn == "k" else "v_pages"
        with pytest.raises(ValueError, match=what + f"{kn} must be a dense tensor"):
            f(None, good, accept, counts, T)
        with pytest.raises(ValueError, match=what + f"{kn} must be bfloat16, float16 or float8_e4m3fn, got torch.float32"):
            f(good.float(), good.float(), accept, counts, T)
        with pytest.raises(RuntimeError, match=what + f"{kn} is torch.bfloat16 but {vn} is torch.float16"):
            f(good, good.half(), accept, counts, T)
        with pytest.raises(ValueError, match=what + f"{kn} must be float8_e4m3fn, got torch.uint8"):
            f(good.to(F8).view(torch.uint8), good.to(F8).view(torch.uint8), accept, counts, T)
        for bad in (0, 65, -1, 2.0, True, None):
            with pytest.raises(ValueError, match=what + r"T must be an int in \[1, 64\]"):
                f(good, good, accept, counts, bad)
        for bad in (accept.long(), accept.float(), "x"):
            with pytest.raises(ValueError, match=what + "accept must be a dense int32 tensor"):
                f(good, good, bad, counts, T)
        with pytest.raises(ValueError, match=what + "accept_counts must be a dense int32 tensor"):
            f(good, good, accept, counts.long(), T)
        for bad in (torch.zeros(B, T + 1, dtype=torch.int32), torch.zeros(T, dtype=torch.int32), torch.zeros(B, 2 * T, dtype=torch.int32)[:, ::2]):
            with pytest.raises(ValueError, match=what + r"accept must be a contiguous \[B, T\] = \[B, 4\] tensor"):
                f(good, good, bad, counts, T)
        with pytest.raises(ValueError, match=what + r"accept_counts must be a contiguous \[B\] = \[2\] tensor"):
            f(good, good, accept, torch.ones(3, dtype=torch.int32), T)
        with pytest.raises(ValueError, match=what + "head size D must be 32, 64, 96 or 128, got 48"):
            f(good[..., :48], good[..., :48], accept, counts, T)
        with pytest.raises(ValueError, match=what + f"{vn} must be a dense tensor with {kn}'s shape"):
            f(good, good[:, :1], accept, counts, T)
        with pytest.raises(ValueError, match=what + f"{kn}'s row stride must be a multiple of 8 elements"):
            f(torch.rand(*good.shape[:3], D + 4).bfloat16()[..., :D], good, accept, counts, T)
        with pytest.raises(RuntimeError, match=what + rf"{kn}, .*k_lens, accept, accept_counts must be device \(HIP\) tensors"):
            f(good, good.clone(), accept, counts, T)
    with pytest.raises(ValueError, match="kv_cache_compact: accept of shape .* needs k"):
        real.kv_cache_compact(k[:1], k[:1], lens, accept, counts, T)
    with pytest.raises(ValueError, match="kv_cache_compact_paged: the pool's pages must hold a power of two >= 16 rows, got page = 24"):
        real.kv_cache_compact_paged(torch.rand(20, Hkv, 24, D).bfloat16(), torch.rand(20, Hkv, 24, D).bfloat16(), table, lens, accept, counts, T)


def test_the_bindings_refuse_host_tensors(built):
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import custom_mm
    q, lens, lse = torch.rand(1, 2, 3, 32).bfloat16(), torch.tensor([5], dtype=torch.int32), torch.empty(1, 2, 3)
    k = torch.rand(1, 1, 64, 32).bfloat16()
    mask = torch.ones(1, 3, dtype=torch.int64)
    ids, counts = torch.zeros(1, 1, 3, 2, dtype=torch.int32), torch.ones(1, 1, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.block_attention_tree_decode_lists(ids, counts, q, k, k, lens, 1.0, mask, 4, torch.empty_like(q), lse)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.kv_compact(k, k.clone(), lens, torch.zeros(1, 3, dtype=torch.int32), torch.ones(1, dtype=torch.int32), 3)
    with pytest.raises(TypeError):  # positional only, the mask is no optional
        custom_mm.block_attention_tree_decode_lists(ids, counts, q, k, k, lens, 1.0, None, 4, torch.empty_like(q), lse)
    for name in ("block_attention_tree_decode", "block_attention_tree_decode_paged", "block_attention_tree_decode_fp8",
                 "block_attention_tree_decode_paged_fp8", "block_attention_tree_decode_lists_paged", "block_attention_tree_lists_decode_fp8",
                 "block_attention_tree_lists_decode_paged_fp8", "rope_kv_append_pos", "rope_kv_append_paged_pos", "kv_compact_paged"):
        assert hasattr(custom_mm, name), name


# ---- wiring on CPU tensors, through the stand-in -----------------------------------------------------------------------------------

@pytest.fixture()
def mm(oracle_mod):
    """(matmuls bound to the stand-in, the stand-in)."""
    import fake_custom_mm_spec_decode as fake
    saved = {k: sys.modules.get(k) for k in ("custom_mm", "matmuls")}
    sys.modules["custom_mm"] = fake
    sys.modules.pop("matmuls", None)
    matmuls = importlib.import_module("matmuls")
    fake.calls.clear()
    fake.spec_calls.clear()
    yield matmuls, fake
    for k, v in saved.items():
        if v is None:
            sys.modules.pop(k, None)
        else:
            sys.modules[k] = v


BINDINGS = ["block_attention_decode", "block_attention_decode_paged", "block_attention_decode_fp8", "block_attention_decode_paged_fp8",
            "block_attention_decode_lists", "block_attention_decode_lists_paged", "block_attention_lists_decode_fp8",
            "block_attention_lists_decode_paged_fp8"]


def test_without_a_mask_todays_bindings_are_called_with_todays_arguments_and_with_one_the_tree_bindings(mm):
    """The stand-ins of today's bindings are the existing ones, untouched: another argument list would be a TypeError.  With a
    mask the block_attention_tree_… binding receives it AS IT IS — the caller's tensor — right before chunk."""
    matmuls, fake = mm
    mask = torch.tensor([[1, 3, 5], [1, 1, 7]], dtype=torch.int64)
    for (name, f), binding in zip(_decode_calls(matmuls), BINDINGS):
        fake.calls.clear()
        fake.spec_calls.clear()
        plain = f(return_lse=True)
        assert [c[0] for c in fake.calls] == [binding] and not fake.spec_calls, name
        also = f(return_lse=True, tree_mask=None)
        assert [c[0] for c in fake.calls] == [binding, binding] and not fake.spec_calls, name
        assert torch.equal(plain[0], also[0])
        for m in (mask, mask[0].contiguous()):
            fake.spec_calls.clear()
            f(tree_mask=m, chunk=3)
            (got, rec), = fake.spec_calls
            assert got == fake.tree_name(binding) and rec["mask_ptr"] == m.data_ptr() and rec["mask_shape"] == tuple(m.shape), name
            assert rec["args"][-3] == 3 and rec["args"][-4] is not None  # the mask, then chunk, out, lse


def test_positions_and_compaction_reach_their_bindings(mm):
    matmuls, fake = mm
    q, kn, vn, cos, sin, k, lens = _rope_operands()
    v = k.clone()
    # None: today's binding, today's arguments
    matmuls.rope_kv_cache_append(q, kn, vn, cos, sin, k, v, lens, positions=None)
    assert [c[0] for c in fake.calls] == ["rope_kv_append"] and not fake.spec_calls
    # an int32 tensor is handed over as it is, an int64 one narrowed; the rotation itself is the stand-in parent's
    p32 = torch.tensor([[97, 98, 98], [125, 126, 126]], dtype=torch.int32)
    matmuls.rope_kv_cache_append(q, kn, vn, cos, sin, k, v, lens, positions=p32)
    (name, rec), = fake.spec_calls
    assert name == "rope_kv_append_pos" and rec["positions_ptr"] == p32.data_ptr() and len(rec["args"]) == 16
    fake.spec_calls.clear()
    pool, table = torch.rand(20, 2, 16, 64).bfloat16(), torch.arange(16, dtype=torch.int32).reshape(2, 8)
    matmuls.rope_kv_cache_append_paged(q, kn, vn, cos, sin, pool, pool.clone(), table, lens, positions=p32.long())
    (name, rec), = fake.spec_calls
    assert name == "rope_kv_append_paged_pos" and rec["args"][-1].dtype == torch.int32 and torch.equal(rec["args"][-1], p32)
    # the compaction: the caches and the lists uncopied, int64 lengths narrowed, the rule on the caller's tensors
    fake.spec_calls.clear()
    T = 4
    accept, counts = torch.tensor([[1, 2, 3, 0], [3, 9, -1, 0]], dtype=torch.int32), torch.tensor([3, 4], dtype=torch.int32)
    before = k.clone()
    assert matmuls.kv_cache_compact(k, v, lens, accept, counts, T) is None
    (name, rec), = fake.spec_calls
    assert name == "kv_compact" and rec["k_ptr"] == k.data_ptr() and rec["v_ptr"] == v.data_ptr() and rec["accept_ptr"] == accept.data_ptr()
    assert rec["counts_ptr"] == counts.data_ptr() and rec["k_lens"].dtype == torch.int32 and rec["T"] == T
    assert torch.equal(k[0, :, 96:99], before[0, :, 97:100]) and torch.equal(k[0, :, 99], before[0, :, 99])  # [1, 2, 3]: a gather
    assert torch.equal(k[1, :, 124], before[1, :, 127]) and torch.equal(k[1, :, 125:127], before[1, :, 125:127])  # offsets 9 and −1
    assert torch.equal(k[1, :, 127], before[1, :, 124]) and torch.equal(lens, torch.tensor([100, 128]))
    fake.spec_calls.clear()
    matmuls.kv_cache_compact_paged(pool, pool.clone(), table.long(), lens, accept, counts, T)
    (name, rec), = fake.spec_calls
    assert name == "kv_compact_paged" and rec["k_ptr"] == pool.data_ptr()
