"""The query-aware key-block selection without a GPU: key_block_bounds[_paged], select_key_blocks and
block_sparse_attention_decode_selected[_paged] — every refusal with its exception type, before the device; the *_takes
functions; the visibility, candidate and forced rules against dense computations written here, through the float64 stand-in
tests/fake_custom_mm_block_select.py; the operands handed to the bindings uncopied; and the entries of the C ABI: declared,
exported, MI_EINVAL before any HIP call."""
import ctypes
import importlib
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from test_block_attention_decode_paged_host import _gathered, _paged

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "mi_spmm.h"
SUFFIXES = ("bf16", "f16")
OK, EINVAL, ERANGE, ENOMEM = 0, -1, -2, -4
FAKE = 0x1000  # a non-null, 16-byte aligned address that is never dereferenced: every call below returns before the device
NAN = float("nan")


# ---- the C ABI -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(built):
    import torch  # noqa: F401  (torch's HIP runtime first, as in the product)
    lib = ctypes.CDLL(str(built / "libmi_spmm.so"))
    vp, i64, i32, f32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_size_t
    operands = [i32] + [vp, i64, i64] + 2 * [vp, i64, i64, i64] + [vp, i32, i32, i32, f32] + [vp, i64, i64, vp, vp, sz, vp]
    for s in SUFFIXES:
        getattr(lib, f"mi_kv_block_bounds_{s}").argtypes = 3 * [i32] + [i32, vp, i64, i64, i64, vp, i32, i32, vp, vp]
        getattr(lib, f"mi_kv_block_bounds_paged_{s}").argtypes = 3 * [i32] + [vp, i64, i32, i32] + [i32, vp, i64, i64, i64, vp, i32, i32, vp, vp]
        getattr(lib, f"mi_block_select_{s}").argtypes = 6 * [i32] + [vp, i64, i64, i64, vp, vp] + 4 * [i32] + 4 * [vp]
        getattr(lib, f"mi_block_attention_decode_lists_{s}").argtypes = [vp, vp] + 5 * [i32] + operands
        getattr(lib, f"mi_block_attention_decode_lists_paged_{s}").argtypes = [vp, vp] + 5 * [i32] + [vp, i64, i32, i32] + operands
    lib.mi_block_attention_decode_workspace_bytes.argtypes = 6 * [i32]
    lib.mi_block_attention_decode_workspace_bytes.restype = sz
    return lib


ENTRIES = [f"mi_{stem}_{s}" for stem in ("kv_block_bounds", "kv_block_bounds_paged", "block_select", "block_attention_decode_lists",
                                         "block_attention_decode_lists_paged") for s in SUFFIXES]


def test_header_declares_and_library_exports_the_entries(lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in ENTRIES + ["mi_block_select_max_blocks"]:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(lib, name), name
    assert lib.mi_block_select_max_blocks() >= 16384


@pytest.mark.parametrize("s", SUFFIXES)
def test_bounds_entries_validate_before_any_hip_call(lib, s):
    base = dict(items=8, heads=2, Smax=512, D=64, k=FAKE, ldk=64, headK=512 * 64, outerK=2 * 512 * 64, lens=FAKE, lens_count=4, last=0,
                bounds=FAKE, table=FAKE, table_ld=32, pages=100, page=16)

    def flat(**kw):
        a = {**base, **kw}
        return getattr(lib, f"mi_kv_block_bounds_{s}")(a["items"], a["heads"], a["Smax"], a["D"], a["k"], a["ldk"], a["headK"], a["outerK"],
                                                       a["lens"], a["lens_count"], a["last"], a["bounds"], None)

    def paged(**kw):
        a = {**base, "headK": 16 * 64, "outerK": 2 * 16 * 64, **kw}
        return getattr(lib, f"mi_kv_block_bounds_paged_{s}")(a["items"], a["heads"], a["Smax"], a["table"], a["table_ld"], a["pages"],
                                                             a["page"], a["D"], a["k"], a["ldk"], a["headK"], a["outerK"], a["lens"],
                                                             a["lens_count"], a["last"], a["bounds"], None)

    shared = ({"D": 48}, {"D": 0}, {"Smax": 500}, {"Smax": -64}, {"last": -1}, {"items": 65536}, {"items": -1}, {"heads": 3}, {"heads": 0},
              {"lens_count": 0}, {"lens_count": 3}, {"lens": None}, {"lens": FAKE + 2}, {"bounds": None}, {"bounds": FAKE + 8},
              {"k": None}, {"k": FAKE + 8}, {"ldk": 60}, {"ldk": 68}, {"headK": 4}, {"outerK": 12})
    for kw in shared:
        assert flat(**kw) == EINVAL, kw
        assert paged(**kw) == EINVAL, kw
    for kw in ({"page": 8}, {"page": 24}, {"page": 0}, {"page": 1024}, {"pages": -1}, {"table": None}, {"table": FAKE + 2}, {"table_ld": 31}):
        assert paged(**kw) == EINVAL, kw
    assert flat(items=0, k=None) == OK and flat(Smax=0, k=None, bounds=None) == OK and paged(items=0, k=None) == OK
    assert paged(pages=0, k=None) == OK  # an empty pool: every key is invisible, nothing is read or written
    assert paged(items=0, page=24) == EINVAL


@pytest.mark.parametrize("s", SUFFIXES)
def test_select_entry_validates_before_any_hip_call(lib, s):
    base = dict(items=8, heads=2, T=1, Smax=512, D=64, group=4, q=FAKE, ldq=64, headQ=64, batchQ=8 * 64, bounds=FAKE, lens=FAKE,
                lens_count=4, K=4, sink=1, local=2, ids=FAKE, counts=FAKE, scores=None)

    def select(**kw):
        a = {**base, **kw}
        return getattr(lib, f"mi_block_select_{s}")(a["items"], a["heads"], a["T"], a["Smax"], a["D"], a["group"], a["q"], a["ldq"],
                                                    a["headQ"], a["batchQ"], a["bounds"], a["lens"], a["lens_count"], a["K"], a["sink"],
                                                    a["local"], a["ids"], a["counts"], a["scores"], None)

    cap = lib.mi_block_select_max_blocks()
    for kw in ({"K": 0}, {"K": -1}, {"sink": -1}, {"local": 0}, {"sink": 2, "local": 3}, {"K": 2}, {"group": 0}, {"group": 17},
               {"D": 48}, {"Smax": 500}, {"Smax": (cap + 1) * 64}, {"items": 65536}, {"heads": 3}, {"heads": 0}, {"lens_count": 3},
               {"lens": None}, {"lens": FAKE + 2}, {"ids": None}, {"ids": FAKE + 2}, {"counts": None}, {"counts": FAKE + 1},
               {"scores": FAKE + 2}, {"q": None}, {"q": FAKE + 8}, {"ldq": 60}, {"headQ": 4}, {"batchQ": 12}, {"bounds": None},
               {"bounds": FAKE + 8}):
        assert select(**kw) == EINVAL, kw
    assert select(items=0, q=None) == OK and select(T=0, lens=None) == OK
    assert select(items=0, K=0) == EINVAL and select(T=0, sink=3, local=2) == EINVAL


@pytest.mark.parametrize("s", SUFFIXES)
def test_lists_entries_validate_before_any_hip_call(lib, s):
    base = dict(ids=FAKE, counts=FAKE, K=4, items=8, heads=2, T=1, Smax=512, D=64, q=FAKE, ldq=64, k=FAKE, ldk=64, headK=512 * 64,
                outerK=2 * 512 * 64, lens=FAKE, lens_count=4, group=4, chunk=2, out=FAKE, lse=FAKE, ws=FAKE, ws_bytes=1 << 30,
                table=FAKE, table_ld=32, pages=100, page=16)

    def tail(a):
        D = a["D"]
        return (D, a["q"], a["ldq"], a["T"] * a["ldq"], a["k"], a["ldk"], a["headK"], a["outerK"], FAKE, D, a["headK"], a["outerK"],
                a["lens"], a["lens_count"], a["group"], a["chunk"], 1.0, a["out"], D, a["T"] * D, a["lse"], a["ws"], a["ws_bytes"], None)

    def flat(**kw):
        a = {**base, **kw}
        return getattr(lib, f"mi_block_attention_decode_lists_{s}")(a["ids"], a["counts"], a["K"], a["items"], a["heads"], a["T"],
                                                                    a["Smax"], *tail(a))

    def paged(**kw):
        a = {**base, "headK": 16 * 64, "outerK": 2 * 16 * 64, **kw}
        return getattr(lib, f"mi_block_attention_decode_lists_paged_{s}")(a["ids"], a["counts"], a["K"], a["items"], a["heads"], a["T"],
                                                                          a["Smax"], a["table"], a["table_ld"], a["pages"], a["page"],
                                                                          *tail(a))

    for kw in ({"K": 0}, {"K": -1}, {"K": 2 ** 31 // 64}, {"ids": None}, {"ids": FAKE + 2}, {"counts": None}, {"counts": FAKE + 2},
               {"group": 0}, {"group": 17}, {"D": 48}, {"chunk": 0}, {"items": 65536}, {"T": 65536}, {"Smax": 500}, {"heads": 3},
               {"lens_count": 3}, {"lens": None}, {"q": None}, {"q": FAKE + 8}, {"out": FAKE + 2}, {"lse": None}, {"ldq": 60},
               {"ws": None}, {"ws": FAKE + 4}, {"k": None}, {"k": FAKE + 8}, {"ldk": 60}, {"headK": 4}, {"outerK": 12}):
        assert flat(**kw) == EINVAL, kw
        assert paged(**kw) == EINVAL, kw
    for kw in ({"page": 8}, {"page": 24}, {"page": 0}, {"pages": -1}, {"table": None}, {"table_ld": 31}):
        assert paged(**kw) == EINVAL, kw
    # the workspace is that of K list positions, whatever Smax is
    need = lib.mi_block_attention_decode_workspace_bytes(8, 1, 4, 64, 4 * 64, 2)
    assert need > 0 and flat(ws_bytes=need - 1) == ENOMEM and paged(ws_bytes=need - 1) == ENOMEM
    assert flat(K=2, ws=None, ws_bytes=0, items=0) == OK  # one chunk: no workspace; an empty problem
    assert flat(items=65535, heads=1, lens_count=1, T=65535, K=2 ** 20) == ERANGE  # items · T · K beyond int32
    assert flat(items=0, q=None) == OK and paged(T=0, lens=None, table=None) == OK and flat(items=0, K=0) == EINVAL


# ---- matmuls on the real extension: refusals before the device ---------------------------------------------------

@pytest.fixture()
def real(built):
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import matmuls
    yield matmuls
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)


def test_takes(real):
    for dtype in (torch.bfloat16, torch.float16):
        for D in (32, 64, 96, 128):
            assert real.key_block_bounds_takes(dtype, D) and real.key_block_bounds_takes(dtype, D, 16) and real.key_block_bounds_takes(dtype, D, 256)
            assert real.select_key_blocks_takes(dtype, D, 1, 0) and real.select_key_blocks_takes(dtype, D, 16, 16384)
            assert real.block_attention_decode_selected_takes(dtype, D, 5) and real.block_attention_decode_selected_paged_takes(dtype, D, 16, 64)
    assert not real.key_block_bounds_takes(torch.float32, 64) and not real.key_block_bounds_takes(torch.bfloat16, 48)
    assert not real.key_block_bounds_takes(torch.bfloat16, 64, 24) and not real.key_block_bounds_takes(torch.bfloat16, 64, 8)
    assert not real.key_block_bounds_takes(torch.float8_e4m3fn, 64)
    assert not real.select_key_blocks_takes(torch.float16, 64, 17, 8) and not real.select_key_blocks_takes(torch.float16, 64, 0, 8)
    assert not real.select_key_blocks_takes(torch.float16, 64, 4, 16385) and not real.select_key_blocks_takes(torch.float16, 64, 4, -1)
    assert not real.select_key_blocks_takes(torch.float32, 64, 4, 8) and not real.select_key_blocks_takes(torch.float16, 64, True, 8)
    assert not real.block_attention_decode_selected_takes(torch.float16, 64, 17) and not real.block_attention_decode_selected_takes(torch.float32, 64, 1)
    assert not real.block_attention_decode_selected_paged_takes(torch.float16, 64, 4, 8)


def test_bounds_refusals_come_before_the_device_with_their_type(real):
    f, fp = real.key_block_bounds, real.key_block_bounds_paged
    what = "key_block_bounds: "
    k = torch.rand(2, 2, 256, 64).bfloat16()
    lens = torch.tensor([100, 256])
    with pytest.raises(ValueError, match=what + "k must be bfloat16 or float16, got torch.float32"):
        f(k.float(), lens)
    with pytest.raises(ValueError, match=what + "k must be a dense tensor"):
        f(None, lens)
    with pytest.raises(ValueError, match=what + r"k must be \[B, Hkv, Smax, D\], got 3-d"):
        f(k[0], lens)
    with pytest.raises(ValueError, match=what + "head size D must be 32, 64, 96 or 128, got 48"):
        f(k[..., :48], lens)
    with pytest.raises(ValueError, match=what + "Smax = 200 must be a multiple of 64"):
        f(k[:, :, :200], lens)
    with pytest.raises(ValueError, match=what + "k must have a last stride of 1, got 2"):
        f(torch.rand(2, 2, 256, 128).bfloat16()[..., ::2], lens)
    with pytest.raises(ValueError, match=what + "k's row stride must be a multiple of 8 elements and at least D = 64, got 68"):
        f(torch.rand(2, 2, 256, 68).bfloat16()[..., :64], lens)
    with pytest.raises(ValueError, match=what + "k_lens must be an int32 or int64 tensor"):
        f(k, lens.float())
    with pytest.raises(ValueError, match=what + r"k_lens must have shape \(2,\)"):
        f(k, torch.tensor([1, 2, 3]))
    for bad in (0, -1, 1.0, True, "1", 2 ** 31):
        with pytest.raises(ValueError, match=what + "last must be None"):
            f(k, lens, last=bad)
    for bad in (torch.empty(2, 2, 4, 2, 32).bfloat16(), torch.empty(2, 2, 3, 2, 64).bfloat16(), torch.empty(2, 2, 4, 4, 64).bfloat16()[:, :, :, ::2],
                "x"):
        with pytest.raises(ValueError, match=what + "bounds must be None or a contiguous dense tensor"):
            f(k, lens, bad)
    with pytest.raises(RuntimeError, match=what + "k is torch.bfloat16 but bounds is torch.float16"):
        f(k, lens, torch.empty(2, 2, 4, 2, 64).half())
    with pytest.raises(TypeError):  # keyword only
        f(k, lens, None, 1)
    with pytest.raises(RuntimeError, match=what + r"k, k_lens must be device \(HIP\) tensors"):
        f(k, lens)
    with pytest.raises(RuntimeError, match=what + r"k, k_lens, bounds must be device \(HIP\) tensors"):
        f(k.transpose(1, 2).contiguous().transpose(1, 2), torch.tensor(7), torch.empty(2, 2, 4, 2, 64).bfloat16(), last=3)
    # … the paged form
    what = "key_block_bounds_paged: "
    pool, table = torch.rand(20, 2, 16, 64).bfloat16(), torch.arange(32, dtype=torch.int32).reshape(2, 16) % 20
    for page in (8, 24):
        with pytest.raises(ValueError, match=what + f"the pool's pages must hold a power of two >= 16 keys, got page = {page}"):
            fp(torch.rand(20, 2, page, 64).bfloat16(), table, lens)
    with pytest.raises(ValueError, match=what + "block_table is required"):
        fp(pool, None, lens)
    with pytest.raises(ValueError, match=what + "block_table must be an int32 or int64 tensor"):
        fp(pool, table.float(), lens)
    with pytest.raises(ValueError, match=what + "Smax = 240 must be a multiple of 64"):
        fp(pool, table[:, :15], lens)
    with pytest.raises(ValueError, match=what + "k_pages's page stride must be a multiple of 8 elements"):
        fp(torch.rand(20 * (2 * 16 * 64 + 4)).bfloat16().as_strided((20, 2, 16, 64), (2 * 16 * 64 + 4, 16 * 64, 64, 1)), table, lens)
    with pytest.raises(RuntimeError, match=what + r"k_pages, block_table, k_lens must be device \(HIP\) tensors"):
        fp(pool, table.long(), lens)


def test_select_refusals_come_before_the_device_with_their_type(real):
    f = real.select_key_blocks
    what = "select_key_blocks: "
    q, bounds, lens = torch.rand(2, 8, 1, 64).bfloat16(), torch.rand(2, 2, 4, 2, 64).bfloat16(), torch.tensor([100, 256])
    for K, kw, msg in ((0, {}, "K must be a positive int32"), (-3, {}, "K must be a positive int32"), (2 ** 31, {}, "K must be a positive int32"),
                       (4, {"sink": -1}, "sink must be >= 0"), (4, {"local": 0}, "local must be >= 1"),
                       (2, {}, "sink \\+ local = 3 forced blocks do not fit K = 2"), (4, {"sink": 3}, "sink \\+ local = 5 forced blocks do not fit K = 4"),
                       (4.0, {}, "K must be an int"), (True, {}, "K must be an int"), (4, {"sink": 1.0}, "sink must be an int"),
                       (4, {"local": None}, "local must be an int")):
        with pytest.raises(ValueError, match=what + msg):
            f(q, bounds, lens, K, **kw)
    with pytest.raises(ValueError, match=what + "q must be bfloat16 or float16"):
        f(q.float(), bounds, lens, 4)
    with pytest.raises(RuntimeError, match=what + "q is torch.bfloat16 but bounds is torch.float16"):
        f(q, bounds.half(), lens, 4)
    with pytest.raises(ValueError, match=what + r"q must be \[B, Hq, T, D\] and bounds \[B, Hkv, Smax/64, 2, D\]"):
        f(q, bounds[0], lens, 4)
    with pytest.raises(ValueError, match=what + "head size D must be 32, 64, 96 or 128, got 48"):
        f(q[..., :48], bounds[..., :48], lens, 4)
    for bad in (torch.rand(3, 2, 4, 2, 64), torch.rand(2, 3, 4, 2, 64), torch.rand(2, 2, 4, 3, 64), torch.rand(2, 2, 4, 2, 32),
                torch.rand(2, 0, 4, 2, 64), bounds.repeat(1, 1, 2, 1, 1)[:, :, ::2]):
        with pytest.raises(ValueError, match=what + r"q of shape \(2, 8, 1, 64\) needs contiguous bounds"):
            f(q, bad.bfloat16() if bad.is_contiguous() else bad, lens, 4)
    with pytest.raises(ValueError, match=what + "34 query heads over 2 k / v heads is a group of 17"):
        f(torch.rand(2, 34, 1, 64).bfloat16(), bounds, lens, 4)
    with pytest.raises(ValueError, match=what + "q must hold T >= 1 new tokens"):
        f(q[:, :, :0], bounds, lens, 4)
    with pytest.raises(ValueError, match=what + "16385 blocks per item exceed the 16384"):
        f(torch.rand(1, 1, 1, 32).bfloat16(), torch.empty(1, 1, 16385, 2, 32).bfloat16(), torch.tensor(5), 4)
    with pytest.raises(ValueError, match=what + "k_lens is required"):
        f(q, bounds, None, 4)
    with pytest.raises(ValueError, match=what + "q's head stride must be a multiple of 8 elements"):
        f(torch.rand(2, 8 * 68).bfloat16().as_strided((2, 8, 1, 64), (8 * 68, 68, 64, 1)), bounds, lens, 4)
    with pytest.raises(TypeError):  # keyword only
        f(q, bounds, lens, 4, 1, 2)
    with pytest.raises(RuntimeError, match=what + r"q, bounds, k_lens must be device \(HIP\) tensors"):
        f(q, bounds, lens, 4)
    with pytest.raises(RuntimeError, match=what + r"q, bounds, k_lens must be device \(HIP\) tensors"):  # a strided q is taken
        f(torch.rand(2, 1, 8, 64).bfloat16().transpose(1, 2), bounds, torch.tensor(3), 9, sink=0, local=1, return_scores=True)


def test_decode_selected_refusals_come_before_the_device_with_their_type(real):
    f, fp = real.block_sparse_attention_decode_selected, real.block_sparse_attention_decode_selected_paged
    what = "block_sparse_attention_decode_selected: "
    q, k, lens = torch.rand(2, 8, 1, 64).bfloat16(), torch.rand(2, 2, 256, 64).bfloat16(), torch.tensor([100, 256])
    ids, counts = torch.zeros(2, 2, 1, 3, dtype=torch.int32), torch.ones(2, 2, 1, dtype=torch.int32)
    for bad in (ids.long(), ids.float(), None, ids.tolist()):
        with pytest.raises(ValueError, match=what + "block_ids must be a dense int32 tensor"):
            f(q, k, k, bad, counts, lens)
    with pytest.raises(ValueError, match=what + "block_counts must be a dense int32 tensor"):
        f(q, k, k, ids, counts.long(), lens)
    for bad in (ids[0], ids[:, :1], torch.zeros(2, 2, 2, 3, dtype=torch.int32), ids[..., :0], torch.zeros(2, 2, 1, 6, dtype=torch.int32)[..., ::2]):
        with pytest.raises(ValueError, match=what + r"block_ids must be a contiguous \[B, Hkv, T, K\] = \[2, 2, 1, K >= 1\]"):
            f(q, k, k, bad, counts, lens)
    for bad in (counts[0], torch.ones(2, 2, 2, dtype=torch.int32), torch.ones(2, 2, 2, dtype=torch.int32)[..., ::2]):
        with pytest.raises(ValueError, match=what + r"block_counts must be a contiguous \[B, Hkv, T\] = \[2, 2, 1\]"):
            f(q, k, k, ids, bad, lens)
    with pytest.raises(ValueError, match=what + "q must be bfloat16 or float16"):
        f(q.float(), k, k, ids, counts, lens)
    with pytest.raises(RuntimeError, match=what + "q is torch.bfloat16 but v is torch.float16"):
        f(q, k, k.half(), ids, counts, lens)
    for bad in (0, -1, 2.0, True, "4", 2 ** 31):
        with pytest.raises(ValueError, match=what + "chunk must be None or a positive int"):
            f(q, k, k, ids, counts, lens, chunk=bad)
    with pytest.raises(ValueError, match=what + "head size D must be 32, 64, 96 or 128, got 48"):
        f(q[..., :48], k[..., :48], k[..., :48], ids, counts, lens)
    with pytest.raises(ValueError, match=what + r"q of shape \(2, 8, 1, 64\) needs k \(2, 'Hkv', 'Smax', 64\) with Hkv a divisor of 8"):
        f(q, torch.rand(2, 3, 256, 64).bfloat16(), k, ids, counts, lens)
    with pytest.raises(ValueError, match=what + "v must be a dense tensor with k's shape"):
        f(q, k, k[:, :, :128], ids, counts, lens)
    with pytest.raises(ValueError, match=what + "Smax = 200 must be a multiple of 64"):
        f(q, k[:, :, :200], k[:, :, :200], ids, counts, lens)
    with pytest.raises(ValueError, match=what + "k's row stride must be a multiple of 8 elements and at least D = 64, got 68"):
        f(q, torch.rand(2, 2, 256, 68).bfloat16()[..., :64], k, ids, counts, lens)
    with pytest.raises(ValueError, match=what + r"k_lens must have shape \(2,\)"):
        f(q, k, k, ids, counts, torch.tensor([1, 2, 3]))
    with pytest.raises(TypeError):  # keyword only
        f(q, k, k, ids, counts, lens, None, 4)
    with pytest.raises(RuntimeError, match=what + r"q, k, v, block_ids, block_counts, k_lens must be device \(HIP\) tensors"):
        f(q, k, k, ids, counts, lens)
    what = "block_sparse_attention_decode_selected_paged: "
    pool, table = torch.rand(20, 2, 16, 64).bfloat16(), torch.arange(32, dtype=torch.int32).reshape(2, 16) % 20
    with pytest.raises(ValueError, match=what + "the pool's pages must hold a power of two >= 16 keys, got page = 24"):
        pp = torch.rand(20, 2, 24, 64).bfloat16()
        fp(q, pp, pp, table, ids, counts, lens)
    with pytest.raises(ValueError, match=what + "block_table is required and must be a dense tensor"):
        fp(q, pool, pool, None, ids, counts, lens)
    with pytest.raises(ValueError, match=what + "Smax = 240 must be a multiple of 64"):
        fp(q, pool, pool, table[:, :15], ids, counts, lens)
    with pytest.raises(RuntimeError, match=what + r"q, k_pages, v_pages, block_table, block_ids, block_counts, k_lens must be device"):
        fp(q, pool, pool, table, ids, counts, lens)


def test_bindings_refuse_host_tensors_and_keywords(built):
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import custom_mm
    q, k = torch.rand(1, 2, 1, 32).bfloat16(), torch.rand(1, 1, 64, 32).bfloat16()
    lens, lse = torch.tensor([5], dtype=torch.int32), torch.empty(1, 2, 1)
    bounds = torch.empty(1, 1, 1, 2, 32).bfloat16()
    ids, counts = torch.zeros(1, 1, 1, 2, dtype=torch.int32), torch.ones(1, 1, 1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.kv_block_bounds(k, lens, 0, bounds)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.kv_block_bounds_paged(k, torch.zeros(1, 1, dtype=torch.int32), lens, 0, bounds)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.block_select(q, bounds, lens, 2, 0, 1, ids, counts, None)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.block_attention_decode_lists(ids, counts, q, k, k, lens, 1.0, 4, torch.empty_like(q), lse)
    with pytest.raises(RuntimeError, match=r"(?s)(?=.*\bBFloat16\b)(?=.*\bHalf\b)"):
        custom_mm.block_attention_decode_lists(ids, counts, q, k, k.half(), lens, 1.0, 4, torch.empty_like(q), lse)
    with pytest.raises(TypeError):  # positional only
        custom_mm.block_select(q, bounds, lens, K=2, sink=0, local=1, block_ids=ids, block_counts=counts, scores=None)


# ---- wiring on CPU tensors, float64 stand-in arithmetic ----------------------------------------------------------------

@pytest.fixture()
def mm(oracle_mod):
    """(matmuls bound to the float64 stand-in, the stand-in)."""
    import fake_custom_mm_block_select as fake
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


def _dense_bounds(k, lens, sentinel):
    """min / max over the seen rows of every block, written here; blocks without a key hold `sentinel`."""
    B, Hkv, Smax, D = k.shape
    ref = torch.full((B, Hkv, Smax // 64, 2, D), sentinel, dtype=k.dtype)
    for b in range(B):
        for J in range(Smax // 64):
            hi = min(64 * J + 64, int(lens[b]))
            if hi > 64 * J:
                ref[b, :, J, 0] = k[b, :, 64 * J:hi].float().amin(1).to(k.dtype)
                ref[b, :, J, 1] = k[b, :, 64 * J:hi].float().amax(1).to(k.dtype)
    return ref


def test_bounds_rules_and_operands_uncopied(mm):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(3)
    base = torch.randn(2, 256, 2, 72, generator=g).half()
    k = base.transpose(1, 2)[..., :64]            # a strided view: head stride 72, row stride 144
    lens = torch.tensor([130, 64])
    for b in range(2):
        k[b, :, int(lens[b]):] = NAN              # unseen rows are never read
    out = matmuls.key_block_bounds(k, lens)
    name, call = fake.calls[-1]
    assert name == "kv_block_bounds" and call["k_ptr"] == k.data_ptr() and call["k_stride"] == tuple(k.stride()) and call["last"] == 0
    assert out.shape == (2, 2, 4, 2, 64) and out.dtype == torch.float16 and not out.requires_grad
    ref = _dense_bounds(k, lens, 0.0)
    for b, blocks in ((0, 3), (1, 1)):
        assert torch.equal(out[b, :, :blocks], ref[b, :, :blocks])
    # in place, last=T: only the blocks of the T newest positions change
    pre = torch.full((2, 2, 4, 2, 64), 7.0).half()
    same = matmuls.key_block_bounds(k, lens, pre, last=3)
    assert same is pre and fake.calls[-1][1]["bounds_ptr"] == pre.data_ptr() and fake.calls[-1][1]["last"] == 3
    assert torch.equal(pre[0, :, 1:3], ref[0, :, 1:3]) and torch.all(pre[0, :, 0] == 7) and torch.all(pre[0, :, 3] == 7)   # 127 … 129
    assert torch.equal(pre[1, :, 0], ref[1, :, 0]) and torch.all(pre[1, :, 1:] == 7)
    # paged: an int32 table handed over as it is, an int64 one narrowed; an out-of-range entry hides its 16 keys
    kc = k.contiguous()
    kp, _, table = _paged(g, kc, kc, 16)
    got = matmuls.key_block_bounds_paged(kp, table, lens)
    call = fake.calls[-1][1]
    assert fake.calls[-1][0] == "kv_block_bounds_paged" and call["k_ptr"] == kp.data_ptr() and call["table_ptr"] == table.data_ptr()
    for b, blocks in ((0, 3), (1, 1)):
        assert torch.equal(got[b, :, :blocks], out[b, :, :blocks])
    matmuls.key_block_bounds_paged(kp, table.long(), lens)
    assert fake.calls[-1][1]["table_dtype"] == torch.int32 and fake.calls[-1][1]["table_ptr"] != table.data_ptr()
    hidden = table.clone()
    hidden[0, 1] = -1                              # keys 16 … 31 of item 0
    got = matmuls.key_block_bounds_paged(kp, hidden, lens)
    kk = kc.clone()
    kk[0, :, 16:32] = kk[0, :, 0:1]                # the same minimum / maximum as leaving them out
    assert torch.equal(got[0, :, 0], _dense_bounds(kk, lens, 0.0)[0, :, 0]) and torch.equal(got[0, :, 1:3], out[0, :, 1:3])


def _select_reference(q, bounds, lens, K, sink, local):
    """The contract, written out densely in float64: candidates, forced blocks, (score descending, index ascending), −1s."""
    B, Hq, T, D = q.shape
    Hkv, blocks = bounds.shape[1], bounds.shape[2]
    G = Hq // Hkv
    ids, counts = np.full((B, Hkv, T, K), -1, np.int64), np.zeros((B, Hkv, T), np.int64)
    scores = np.full((B, Hkv, T, blocks), -np.inf)
    for b in range(B):
        for h in range(Hkv):
            for t in range(T):
                pos = min(max(int(lens[b]), 0), blocks * 64) - T + t
                if pos < 0:
                    continue
                cand = list(range(pos // 64 + 1))
                for J in cand:
                    lo, hi = bounds[b, h, J, 0].double(), bounds[b, h, J, 1].double()
                    scores[b, h, t, J] = max(float(torch.maximum(q[b, h * G + g, t].double() * lo, q[b, h * G + g, t].double() * hi).sum())
                                             for g in range(G))
                forced = {J for J in cand if J < sink} | {J for J in cand if J > pos // 64 - local}
                rest = sorted((J for J in cand if J not in forced), key=lambda J: (-scores[b, h, t, J], J))
                n = min(K, len(cand))
                chosen = sorted(forced | set(rest[:n - len(forced)]))
                assert len(chosen) == n
                ids[b, h, t, :n], counts[b, h, t] = chosen, n
    return ids, counts, scores


def test_select_rules_and_operands_uncopied(mm):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(5)
    q = torch.randint(-4, 5, (2, 3, 6, 32), generator=g).half().transpose(1, 2)   # [2, 6, 3, 32] through its own strides
    lo = torch.randint(-8, 9, (2, 2, 8, 32), generator=g)
    hi = lo + torch.randint(0, 4, (2, 2, 8, 32), generator=g)
    bounds = torch.stack([lo, hi], 3).half()
    lens = torch.tensor([2, 450])                 # item 0: pos −1, 0, 1; item 1: 447, 448, 449 — two candidate sets
    for K, sink, local in ((3, 1, 2), (4, 0, 1), (5, 2, 1), (12, 1, 2)):
        ids, counts, scores = matmuls.select_key_blocks(q, bounds, lens, K, sink=sink, local=local, return_scores=True)
        name, call = fake.calls[-1]
        assert name == "block_select" and call["q_ptr"] == q.data_ptr() and call["q_stride"] == tuple(q.stride())
        assert call["bounds_ptr"] == bounds.data_ptr() and (call["K"], call["sink"], call["local"]) == (K, sink, local)
        r_ids, r_counts, r_scores = _select_reference(q, bounds, lens, K, sink, local)
        assert ids.dtype == torch.int32 and np.array_equal(ids.numpy(), r_ids) and np.array_equal(counts.numpy(), r_counts)
        assert np.array_equal(scores.numpy().astype(np.float64), r_scores)
        assert counts[0, :, 0].eq(0).all() and ids[0, :, 0].eq(-1).all()       # pos < 0
    two = matmuls.select_key_blocks(q, bounds, lens, 3)
    assert len(two) == 2 and not fake.calls[-1][1]["scores"]


def test_decode_selected_visibility_and_operands_uncopied(mm):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(7)
    B, Hkv, G, T, D, Smax = 2, 2, 3, 2, 32, 256
    q = torch.randn(B, Hkv * G, T, D, generator=g).half()
    k, v = (torch.randn(B, Smax, Hkv, D + 8, generator=g).half().transpose(1, 2)[..., :D] for _ in range(2))
    lens = torch.tensor([200, 70])
    for b in range(B):
        k[b, :, int(lens[b]):], v[b, :, int(lens[b]):] = NAN, NAN
    ids = torch.tensor([[3, 0, -1, 2], [1, 0, 0, 0]], dtype=torch.int32).repeat(B, Hkv, 1, 1).contiguous()   # [B, Hkv, T, 4]
    counts = torch.tensor([4, 1], dtype=torch.int32).repeat(B, Hkv, 1).contiguous()
    out, lse = matmuls.block_sparse_attention_decode_selected(q, k, v, ids, counts, lens, chunk=2, return_lse=True)
    name, call = fake.calls[-1]
    assert name == "block_attention_decode_lists" and call["ids_ptr"] == ids.data_ptr() and call["counts_ptr"] == counts.data_ptr()
    assert call["k_ptr"] == k.data_ptr() and call["k_stride"] == tuple(k.stride()) and call["v_ptr"] == v.data_ptr() and call["chunk"] == 2
    assert not out.requires_grad and not torch.isnan(out).any()
    for b in range(B):
        for h in range(Hkv):
            for t in range(T):
                pos = int(lens[b]) - T + t
                listed = ids[b, h, t, :int(counts[b, h, t])].tolist()
                keys = [j for J in listed if 0 <= J < Smax // 64 for j in range(64 * J, 64 * J + 64) if j <= pos]
                for gq in range(G):
                    s = (k[b, h][keys].double() @ q[b, h * G + gq, t].double()) / D ** 0.5
                    ref = torch.softmax(s, 0) @ v[b, h][keys].double()
                    assert torch.allclose(out[b, h * G + gq, t].double(), ref, atol=2e-3), (b, h, t, gq)
                    assert abs(float(lse[b, h * G + gq, t]) - float(torch.logsumexp(s, 0))) < 1e-3
    # the paged form: the pool and the table uncopied, the contiguous result on the gathered cache
    kp, vp, table = _paged(g, k.contiguous(), v.contiguous(), 16)
    got = matmuls.block_sparse_attention_decode_selected_paged(q, kp, vp, table, ids, counts, lens, chunk=2)
    name, call = fake.calls[-1]
    assert name == "block_attention_decode_lists_paged" and call["k_ptr"] == kp.data_ptr() and call["table_ptr"] == table.data_ptr()
    assert torch.equal(got, out) and torch.equal(_gathered(kp, table)[0, :, :200], k.contiguous()[0, :, :200])
    # count 0 and pos < 0: zero rows, lse −inf
    out0, lse0 = matmuls.block_sparse_attention_decode_selected(q, k, v, ids, torch.zeros_like(counts), lens, return_lse=True)
    assert out0.eq(0).all() and torch.isinf(lse0).all()
