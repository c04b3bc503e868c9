"""Sliding windows and sink keys without a GPU: window= and sink= of the sixteen reading calls and
sliding_window_layout.  Every refusal with its exception type, raised on host tensors by the real extension's matmuls before a
device call; the None path reaching TODAY's bindings with today's argument lists and the new operands reaching the new bindings,
through the stand-in tests/fake_custom_mm_window.py; sliding_window_layout against a double loop over the blocks; and the 32 new
entries of the C ABI: declared, exported, MI_EINVAL / MI_OK before any HIP call."""
import ctypes
import importlib
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from test_spec_decode_host import _decode_calls, _layout

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "mi_spmm.h"
OK, EINVAL = 0, -1
PTR = 0x1000  # a non-null, 16-byte aligned address that is never dereferenced: every call below returns before the device
F8 = torch.float8_e4m3fn
vp, i64, i32, f32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_size_t
TOP = 2 ** 31 - 1

FORMS = [(l, p, f, t) for l in ("", "_lists") for p in ("", "_paged") for f in ("", "_fp8") for t in ("bf16", "f16")]
DECODE_ENTRIES = [(f"mi_block_attention_window_decode{l}{p}{f}_{t}", bool(l), bool(p), bool(f)) for l, p, f, t in FORMS]
PREFILL_ENTRIES = [(f"mi_block_attention_window_prefill{l}{p}{f}_{t}", bool(l), bool(p), bool(f)) for l, p, f, t in FORMS]


@pytest.fixture(scope="module")
def lib(built):
    import torch  # noqa: F401  (torch's HIP runtime first, as in the product)
    return ctypes.CDLL(str(built / "libmi_spmm.so"))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------

def test_the_32_entries_are_declared_and_exported_and_no_name_starts_like_a_closed_family(lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    names = [e[0] for e in DECODE_ENTRIES + PREFILL_ENTRIES]
    assert len(set(names)) == 32
    for name in names:
        assert re.search(rf"\bint {name}\(", text), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
    closed = ("mi_block_attention_decode", "mi_block_attention_prefill", "mi_block_attention_tree_decode", "mi_block_attention_lists_decode",
              "mi_block_attention_lists_prefill")
    assert not any(n.startswith(closed) for n in names)
    # … nor does a binding
    cpp = (REPO / "matrix-multiplication_amd" / "csrc" / "custom_mm.cpp").read_text()
    bindings = re.findall(r'm\.def\("(block_attention_window_\w+)"', cpp)
    assert len(set(bindings)) == 16
    assert not any(b.startswith(("block_attention_decode", "block_attention_prefill", "block_attention_tree", "block_attention_lists"))
                   for b in bindings)


def _head(lists, paged):
    sig = ([("block_ids", vp), ("block_counts", vp), ("K", i32)] if lists else [("rowptr", vp), ("col", vp), ("nnz", i64), ("layouts", i32)])
    sig += [("items", i32), ("heads", i32), ("T", i32), ("Smax", i32)]
    return sig + ([("block_table", vp), ("table_ld", i64), ("pages", i32), ("page", i32)] if paged else [])


CACHE = [("k", vp), ("ldk", i64), ("headK", i64), ("outerK", i64), ("v", vp), ("ldv", i64), ("headV", i64), ("outerV", i64), ("k_lens", vp),
         ("lens_count", i32)]
SCALES = [("k_scale", vp), ("k_scale_count", i32), ("v_scale", vp), ("v_scale_count", i32)]


def _values(paged, change):
    a = dict(rowptr=PTR, col=PTR, nnz=1, layouts=1, block_ids=PTR, block_counts=PTR, K=1, items=2, heads=1, T=3, Smax=64,
             block_table=PTR, table_ld=4, pages=4, page=16, D=32, q=PTR, ldq=32, strideQ=96, headQ=96, batchQ=96, k=PTR, ldk=32,
             headK=2048, outerK=2048, v=PTR, ldv=32, headV=2048, outerV=2048, k_lens=PTR, lens_count=1, new_lens=None, new_lens_count=0,
             group=1, chunk=1, scale=1.0, k_scale=PTR, k_scale_count=1, v_scale=PTR, v_scale_count=1, window=5, sink=1, out=PTR, ldo=32,
             strideO=96, lse=PTR, workspace=None, workspace_bytes=0, stream=None)
    if paged:
        a.update(headK=512, outerK=512, headV=512, outerV=512)
    a.update(change)
    return a


def _send(lib, name, sig, a):
    fn = getattr(lib, name)
    fn.argtypes, fn.restype = [t for _, t in sig], ctypes.c_int
    return fn(*[a[n] for n, _ in sig])


def decode_call(lib, name, lists, paged, fp8, **change):
    sig = _head(lists, paged) + [("D", i32), ("q", vp), ("ldq", i64), ("strideQ", i64)] + CACHE + [("group", i32), ("chunk", i32), ("scale", f32)]
    sig += SCALES if fp8 else []
    sig += [("window", i32), ("sink", i32), ("out", vp), ("ldo", i64), ("strideO", i64), ("lse", vp), ("workspace", vp),
            ("workspace_bytes", sz), ("stream", vp)]
    return _send(lib, name, sig, _values(paged, change))


def prefill_call(lib, name, lists, paged, fp8, **change):
    sig = _head(lists, paged) + [("D", i32), ("q", vp), ("ldq", i64), ("headQ", i64), ("batchQ", i64)] + CACHE
    sig += [("new_lens", vp), ("new_lens_count", i32), ("group", i32), ("scale", f32)]
    sig += SCALES if fp8 else []
    sig += [("window", i32), ("sink", i32), ("out", vp), ("ldo", i64), ("strideO", i64), ("lse", vp), ("stream", vp)]
    return _send(lib, name, sig, _values(paged, change))


@pytest.mark.parametrize("name,lists,paged,fp8", DECODE_ENTRIES + PREFILL_ENTRIES, ids=[e[0] for e in DECODE_ENTRIES + PREFILL_ENTRIES])
def test_window_entries_validate_before_any_hip_call(lib, name, lists, paged, fp8):
    """Every row is refused (or, empty, answered) before a pointer is dereferenced: PTR is no memory.  The valid list itself is
    never sent: it would launch."""
    send = decode_call if "_decode" in name else prefill_call
    call = lambda **kw: send(lib, name, lists, paged, fp8, **kw)  # noqa: E731
    for bad in (dict(window=0), dict(window=-1), dict(window=-2 ** 31), dict(sink=-1), dict(sink=-2 ** 31)):
        assert call(**bad) == EINVAL, bad
        assert call(items=0, **bad) == EINVAL, bad  # the two values are looked at before anything else
    # the empty calls are answered as the plain twins answer them, at both ends of the two ranges
    for good in (dict(), dict(window=1, sink=0), dict(window=TOP, sink=TOP)):
        assert call(items=0, q=None, **good) == OK and call(T=0, q=None, **good) == OK, good
    # the twin's refusals stand
    assert call(q=None) == EINVAL and call(k_lens=None) == EINVAL and call(D=48) == EINVAL and call(lse=None) == EINVAL
    if "_decode" in name:
        assert call(group=17) == EINVAL and call(chunk=0) == EINVAL
        assert call(T=65, strideQ=65 * 32, strideO=65 * 32, q=None) == EINVAL  # (refused for q: T is not bound to 64 without a tree)
    else:
        assert call(new_lens=PTR + 2, new_lens_count=1) == EINVAL and call(new_lens=PTR, new_lens_count=3) == EINVAL
    if paged:
        assert call(page=8) == EINVAL and call(page=24) == EINVAL and call(block_table=None) == EINVAL
    if lists:
        assert call(K=0) == EINVAL and call(block_counts=None) == EINVAL


# ---- sliding_window_layout -----------------------------------------------------------------------------------------------------------

@pytest.fixture()
def real(built):
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import matmuls
    yield matmuls
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)


def loop_layout(Smax, W, S, block):
    """By the definition: block (r, c) is kept iff some position of row r sees some key of column c."""
    n = Smax // block
    pos, key = np.arange(Smax)[:, None], np.arange(Smax)[None, :]
    sees = (key <= pos) & ((key > pos - W) | (key < S))
    keep = np.zeros((n, n), dtype=bool)
    for r in range(n):
        for c in range(n):
            keep[r, c] = c <= r and sees[r * block:(r + 1) * block, c * block:(c + 1) * block].any()
    return keep


@pytest.mark.parametrize("S", [0, 1, 64, 70])
@pytest.mark.parametrize("W", [1, 5, 64, 65, 100, 512])
def test_sliding_window_layout_against_a_double_loop(real, W, S):
    got = real.sliding_window_layout(512, W, S)
    assert got.dtype == torch.bool and tuple(got.shape) == (8, 8) and got.device.type == "cpu"
    assert np.array_equal(got.numpy(), loop_layout(512, W, S, 64)), (W, S)
    wide = real.sliding_window_layout(512, W, sink=S, block=128)
    assert tuple(wide.shape) == (4, 4) and np.array_equal(wide.numpy(), loop_layout(512, W, S, 128)), (W, S)
    if W > 1 or S:
        assert got.to_sparse_csr().values().numel() == int(got.sum())  # what the calls take


def test_sliding_window_layout_edges_and_refusals(real):
    assert real.sliding_window_layout(512, TOP).numpy().tolist() == np.tril(np.ones((8, 8), dtype=bool)).tolist()
    assert real.sliding_window_layout(512, 1, TOP).numpy().tolist() == np.tril(np.ones((8, 8), dtype=bool)).tolist()
    assert real.sliding_window_layout(64, 1).tolist() == [[True]]
    what = "sliding_window_layout: "
    for bad in (0, -1, 2 ** 31, 1.0, True, None, torch.tensor(4)):
        with pytest.raises(ValueError, match=what + "window must be a Python int"):
            real.sliding_window_layout(512, bad)
    for bad in (-1, 2 ** 31, 0.0, False, None):
        with pytest.raises(ValueError, match=what + "sink must be a Python int"):
            real.sliding_window_layout(512, 4, bad)
    for smax, block in ((500, 64), (512, 96), (64, 128)):
        with pytest.raises(ValueError, match=what + "block = .* must be a multiple of 64 and Smax"):
            real.sliding_window_layout(smax, 4, 0, block)
    with pytest.raises(ValueError, match=what + "Smax must be a Python int"):
        real.sliding_window_layout(0, 4)


# ---- matmuls on the real extension: refusals before the device ----------------------------------------------------------------------

def _prefill_calls(m, T=70):
    """(name, f(**kw) → the call on host operands of valid shapes) of the eight prefill calls; B = 2, Hkv = 2, Hq = 4."""
    B, Hkv, Hq, D, Smax, page = 2, 2, 4, 64, 256, 16
    X = -(-T // 64) + 1
    q = torch.rand(B, Hq, T, D).bfloat16()
    k, pool = torch.rand(B, Hkv, Smax, D).bfloat16(), torch.rand(40, Hkv, page, D).bfloat16()
    k8, pool8 = k.to(F8), pool.to(F8)
    table = torch.arange(B * Smax // page, dtype=torch.int32).reshape(B, -1)
    lens, layout = torch.tensor([100, 256]), _layout()
    ids, counts = torch.zeros(B, Hkv, X, 3, dtype=torch.int32), torch.ones(B, Hkv, X, dtype=torch.int32)
    return [
        ("block_sparse_attention_prefill", lambda **kw: m.block_sparse_attention_prefill(q, k, k, layout, lens, **kw)),
        ("block_sparse_attention_prefill_paged", lambda **kw: m.block_sparse_attention_prefill_paged(q, pool, pool, table, layout, lens, **kw)),
        ("block_sparse_attention_prefill_fp8", lambda **kw: m.block_sparse_attention_prefill_fp8(q, k8, k8, layout, lens, **kw)),
        ("block_sparse_attention_prefill_paged_fp8",
         lambda **kw: m.block_sparse_attention_prefill_paged_fp8(q, pool8, pool8, table, layout, lens, **kw)),
        ("block_sparse_attention_prefill_selected", lambda **kw: m.block_sparse_attention_prefill_selected(q, k, k, ids, counts, lens, **kw)),
        ("block_sparse_attention_prefill_selected_paged",
         lambda **kw: m.block_sparse_attention_prefill_selected_paged(q, pool, pool, table, ids, counts, lens, **kw)),
        ("block_sparse_attention_prefill_selected_fp8",
         lambda **kw: m.block_sparse_attention_prefill_selected_fp8(q, k8, k8, ids, counts, lens, **kw)),
        ("block_sparse_attention_prefill_selected_paged_fp8",
         lambda **kw: m.block_sparse_attention_prefill_selected_paged_fp8(q, pool8, pool8, table, ids, counts, lens, **kw)),
    ]


def test_window_refusals_come_before_the_device_with_their_type(real):
    decode, prefill = _decode_calls(real), _prefill_calls(real)
    assert len(decode) == 8 and len(prefill) == 8
    for name, f in decode + prefill:
        what = name + ": "
        for bad in (True, False, 0, -1, 2 ** 31, 4.0, "4", torch.tensor(4), torch.tensor([4])):
            with pytest.raises(ValueError, match=what + "window must be None or a Python int"):
                f(window=bad)
        for bad in (True, -1, 2 ** 31, 1.0, None, torch.tensor(1)):
            with pytest.raises(ValueError, match=what + "sink must be a Python int"):
                f(window=4, sink=bad)
        for sink in (1, TOP):
            with pytest.raises(ValueError, match=what + f"sink = {sink} needs a window"):
                f(sink=sink)
        with pytest.raises(ValueError, match=what + "sink must be a Python int"):  # … also without a window
            f(sink=-1)
        with pytest.raises(TypeError):  # keyword only
            f(None, None, None, None, None, None)
        # the accepted values pass these checks: the call ends at the last one, the host operands
        for good in (dict(window=1), dict(window=TOP, sink=TOP), dict(window=100, sink=4), dict(window=None, sink=0)):
            with pytest.raises(RuntimeError, match=what + r".*must be device \(HIP\) tensors"):
                f(**good)
    for name, f in decode:
        mask = torch.ones(2, 3, dtype=torch.int64)
        with pytest.raises(ValueError, match=name + ": window and tree_mask do not go together"):
            f(window=4, tree_mask=mask)
    for name, f in prefill[:4]:
        with pytest.raises(ValueError, match=name + ": window and split do not go together"):
            f(window=4, split=2)
    for name, f in prefill[4:]:
        with pytest.raises(TypeError):  # the list calls have no split
            f(window=4, split=2)


def test_the_bindings_refuse_bad_windows_and_host_tensors(built):
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import custom_mm
    q, lens, lse = torch.rand(1, 2, 3, 32).bfloat16(), torch.tensor([5], dtype=torch.int32), torch.empty(1, 2, 3)
    k = torch.rand(1, 1, 64, 32).bfloat16()
    ids, counts = torch.zeros(1, 1, 3, 2, dtype=torch.int32), torch.ones(1, 1, 3, dtype=torch.int32)
    pids, pcounts = torch.zeros(1, 1, 2, 2, dtype=torch.int32), torch.ones(1, 1, 2, dtype=torch.int32)
    out = torch.empty_like(q)
    with pytest.raises(RuntimeError, match="block_attention_window_decode_lists: window must be a positive int32, got 0"):
        custom_mm.block_attention_window_decode_lists(ids, counts, q, k, k, lens, 1.0, 0, 0, 4, out, lse)
    with pytest.raises(RuntimeError, match="block_attention_window_decode_lists: sink must be an int32 >= 0, got -1"):
        custom_mm.block_attention_window_decode_lists(ids, counts, q, k, k, lens, 1.0, 4, -1, 4, out, lse)
    with pytest.raises(RuntimeError, match=r"block_attention_window_lists_prefill: window must be a positive int32, got 2147483648"):
        custom_mm.block_attention_window_lists_prefill(pids, pcounts, q, k, k, lens, None, 1.0, 2 ** 31, 0, out, lse)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.block_attention_window_decode_lists(ids, counts, q, k, k, lens, 1.0, 4, 1, 4, out, lse)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.block_attention_window_lists_prefill(pids, pcounts, q, k, k, lens, None, 1.0, 4, 1, out, lse)
    with pytest.raises(TypeError):  # positional only, the window is no optional
        custom_mm.block_attention_window_decode_lists(ids, counts, q, k, k, lens, 1.0, None, 0, 4, out, lse)
    import fake_custom_mm_window as fake
    for parent in fake.DECODE + fake.PREFILL:
        assert hasattr(custom_mm, parent) and hasattr(custom_mm, fake.window_name(parent)), parent


# ---- wiring on CPU tensors, through the stand-in -----------------------------------------------------------------------------------

@pytest.fixture()
def mm(oracle_mod):
    """(matmuls bound to the stand-in, the stand-in)."""
    import fake_custom_mm_window as fake
    saved = {k: sys.modules.get(k) for k in ("custom_mm", "matmuls")}
    sys.modules["custom_mm"] = fake
    sys.modules.pop("matmuls", None)
    matmuls = importlib.import_module("matmuls")
    fake.calls.clear()
    fake.spec_calls.clear()
    fake.window_calls.clear()
    yield matmuls, fake
    for k, v in saved.items():
        if v is None:
            sys.modules.pop(k, None)
        else:
            sys.modules[k] = v


def test_without_a_window_todays_bindings_are_called_with_todays_arguments_and_with_one_the_window_bindings(mm):
    """The stand-ins of today's bindings are strict: another argument list would be a TypeError.  With a window the
    block_attention_window_… binding receives the two ints right before chunk (decode) or out (prefill), and its parent's
    arguments around them."""
    matmuls, fake = mm
    calls = _decode_calls(matmuls) + _prefill_calls(matmuls)
    for (name, f), binding, tail in zip(calls, fake.DECODE + fake.PREFILL, [3] * 8 + [2] * 8):
        fake.calls.clear()
        fake.window_calls.clear()
        plain = f(return_lse=True)
        assert [c[0] for c in fake.calls] == [binding] and not fake.window_calls, name
        also = f(return_lse=True, window=None, sink=0)
        assert [c[0] for c in fake.calls] == [binding, binding] and not fake.window_calls and not fake.spec_calls, name
        assert torch.equal(plain[0], also[0]) and torch.equal(plain[1], also[1])
        for window, sink in ((100, 4), (1, 0), (TOP, TOP)):
            fake.calls.clear()
            fake.window_calls.clear()
            got = f(return_lse=True, window=window, sink=sink)
            (reached, rec), = fake.window_calls
            assert reached == fake.window_name(binding) and (rec["window"], rec["sink"]) == (window, sink), name
            assert rec["args"][-tail - 2:-tail] == (window, sink)  # … then chunk, out, lse — or out, lse
            assert [c[0] for c in fake.calls] == [binding], name  # the stand-in's parent got the rest, unchanged
            assert torch.equal(got[0], plain[0])
    # chunk still stands behind the window of a decode call
    name, f = _decode_calls(matmuls)[0]
    fake.window_calls.clear()
    f(window=7, sink=2, chunk=3)
    assert fake.window_calls[0][1]["args"][-5:-2] == (7, 2, 3)
