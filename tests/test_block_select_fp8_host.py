"""The key-block selection over an FP8 cache without a GPU: key_block_bounds[_paged]_fp8 and
block_sparse_attention_decode_selected[_paged]_fp8 — the ordering claim the bit contract rests on, the *_takes functions,
every refusal with its exception type before the device, the operands handed to the bindings uncopied (through
tests/fake_custom_mm_block_select_fp8.py), and the eight entries of the C ABI: declared, exported, MI_EINVAL before any HIP
call."""
import ctypes
import importlib
import re
import sys
from pathlib import Path

import pytest
import torch

from test_block_attention_decode_fp8_host import F8, finite_codes, random_fp8
from test_block_attention_decode_paged_host import _gathered, _paged

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "mi_spmm.h"
SUFFIXES = ("bf16", "f16")
LOWP = (torch.bfloat16, torch.float16)
OK, EINVAL, ERANGE, ENOMEM = 0, -1, -2, -4
FAKE = 0x1000  # a non-null, 16-byte aligned address that is never dereferenced: every call below returns before the device


def _bytes(*shape):
    return torch.zeros(shape, dtype=torch.uint8)


# ---- the claim under the bit contract -------------------------------------------------------------------------------------

def ordered8(b):
    """The kernel's order of e4m3fn bytes: sign and magnitude turned into one unsigned order."""
    return (~b & 0xFF) if b & 0x80 else (b | 0x80)


def ordered16(h):
    """… and the 2-byte kernel's, of bfloat16 / float16 patterns."""
    return (~h & 0xFFFF) if h & 0x8000 else (h | 0x8000)


@pytest.mark.parametrize("dtype", LOWP)
def test_the_ordered_bytes_are_strictly_monotone_into_the_ordered_patterns_of_the_widened_codes(dtype):
    codes = finite_codes()
    assert codes.numel() == 254
    wide = codes.view(F8).to(dtype).view(torch.int16).to(torch.int32) & 0xFFFF
    pairs = sorted((ordered8(int(c)), ordered16(int(w))) for c, w in zip(codes, wide))
    assert len({p[0] for p in pairs}) == 254
    for (b0, h0), (b1, h1) in zip(pairs, pairs[1:]):
        assert b0 < b1 and h0 < h1, (b0, b1, h0, h1)          # strictly: minimum and maximum commute with the widening
    # −0 < +0 in both orders, and −0 widens to 0x8000
    assert ordered8(0x80) + 1 == ordered8(0x00) and ordered16(0x8000) + 1 == ordered16(0x0000)
    assert int(wide[codes == 0x80]) == 0x8000 and int(wide[codes == 0x00]) == 0
    # the two NaN codes lie beyond the finite ones on their sign's side
    assert ordered8(0x7F) > pairs[-1][0] and ordered8(0xFF) < pairs[0][0]
    # the way back is the code
    for c in range(256):
        o = ordered8(c)
        assert ((o & 0x7F) if o & 0x80 else (~o & 0xFF)) == c


# ---- the C ABI ------------------------------------------------------------------------------------------------------------

BOUNDS = [f"mi_kv_block_bounds_{form}fp8_{s}" for form in ("", "paged_") for s in SUFFIXES]
LISTS = [f"mi_block_attention_lists_decode_{form}fp8_{s}" for form in ("", "paged_") for s in SUFFIXES]


@pytest.fixture(scope="module")
def lib(built):
    import torch  # noqa: F401  (torch's HIP runtime first, as in the product)
    lib = ctypes.CDLL(str(built / "libmi_spmm.so"))
    vp, i64, i32, f32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_size_t
    bounds = [i32, vp, i64, i64, i64, vp, i32, i32, vp, vp]
    operands = [i32] + [vp, i64, i64] + 2 * [vp, i64, i64, i64] + [vp, i32, i32, i32, f32, vp, i32, vp, i32] + [vp, i64, i64, vp, vp, sz, vp]
    for s in SUFFIXES:
        getattr(lib, f"mi_kv_block_bounds_fp8_{s}").argtypes = 3 * [i32] + bounds
        getattr(lib, f"mi_kv_block_bounds_paged_fp8_{s}").argtypes = 3 * [i32] + [vp, i64, i32, i32] + bounds
        getattr(lib, f"mi_block_attention_lists_decode_fp8_{s}").argtypes = [vp, vp] + 5 * [i32] + operands
        getattr(lib, f"mi_block_attention_lists_decode_paged_fp8_{s}").argtypes = [vp, vp] + 5 * [i32] + [vp, i64, i32, i32] + operands
    lib.mi_block_attention_decode_workspace_bytes.argtypes = 6 * [i32]
    lib.mi_block_attention_decode_workspace_bytes.restype = sz
    return lib


def _params(text, name):
    args = re.search(rf"\b{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    for macro in re.findall(r"\bMI_\w+", args):  # a parameter list kept in a macro of the header
        body = re.search(rf"#define {macro}\b(.*?[^\\])\n", text, flags=re.S).group(1).replace("\\\n", " ")
        args = args.replace(macro, body)
    return args, [a.split()[-1].lstrip("*") for a in args.split(",")]


def test_header_declares_and_library_exports_the_eight_entries(lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in BOUNDS + LISTS:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(lib, name), name
        assert not name.startswith("mi_block_attention_decode")  # that family of the header is closed
    for form in ("", "paged_"):
        for s in SUFFIXES:
            # the bounds: the 2-byte entry's list with a byte cache
            args, names = _params(text, f"mi_kv_block_bounds_{form}fp8_{s}")
            parent_args, parents = _params(text, f"mi_kv_block_bounds_{form}{s}")
            assert names == parents and len(re.findall(r"const uint8_t\s*\*\s*k\b", args)) == 1 and "uint8_t" not in parent_args
            assert re.search(r"uint16_t\s*\*\s*bounds", args)
            # the lists: the 2-byte lists entry's list with byte caches and the four scale parameters after `scale`
            args, names = _params(text, f"mi_block_attention_lists_decode_{form}fp8_{s}")
            parent_args, parents = _params(text, f"mi_block_attention_decode_lists_{form}{s}")
            at = names.index("k_scale")
            assert names[at:at + 4] == ["k_scale", "k_scale_count", "v_scale", "v_scale_count"] and names[at - 1] == "scale"
            assert names[:at] + names[at + 4:] == parents
            assert len(re.findall(r"const uint8_t\s*\*", args)) == 2 and "uint8_t" not in parent_args
            # … as the fp8 layout entries place them
            _, layout = _params(text, f"mi_block_attention_decode_{form}fp8_{s}")
            assert layout[layout.index("scale"):] == names[names.index("scale"):]


@pytest.mark.parametrize("s", SUFFIXES)
def test_bounds_entries_validate_before_any_hip_call(lib, s):
    base = dict(items=8, heads=2, Smax=512, D=64, k=FAKE, ldk=64, headK=512 * 64, outerK=2 * 512 * 64, lens=FAKE, lens_count=4, last=0,
                bounds=FAKE, table=FAKE, table_ld=32, pages=100, page=16)

    def flat(**kw):
        a = {**base, **kw}
        return getattr(lib, f"mi_kv_block_bounds_fp8_{s}")(a["items"], a["heads"], a["Smax"], a["D"], a["k"], a["ldk"], a["headK"],
                                                           a["outerK"], a["lens"], a["lens_count"], a["last"], a["bounds"], None)

    def paged(**kw):
        a = {**base, "headK": 16 * 64, "outerK": 2 * 16 * 64, **kw}
        return getattr(lib, f"mi_kv_block_bounds_paged_fp8_{s}")(a["items"], a["heads"], a["Smax"], a["table"], a["table_ld"], a["pages"],
                                                                 a["page"], a["D"], a["k"], a["ldk"], a["headK"], a["outerK"], a["lens"],
                                                                 a["lens_count"], a["last"], a["bounds"], None)

    shared = ({"D": 48}, {"D": 0}, {"Smax": 500}, {"Smax": -64}, {"last": -1}, {"items": 65536}, {"items": -1}, {"heads": 3}, {"heads": 0},
              {"lens_count": 0}, {"lens_count": 3}, {"lens": None}, {"lens": FAKE + 2}, {"bounds": None}, {"bounds": FAKE + 8},
              {"k": None}, {"k": FAKE + 8}, {"ldk": 60}, {"ldk": 48}, {"headK": 4},
              {"ldk": 72}, {"headK": 8}, {"headK": 1032}, {"outerK": 2056}, {"outerK": 8})   # bytes: multiples of 16, not of 8
    for kw in shared:
        assert flat(**kw) == EINVAL, kw
        assert paged(**kw) == EINVAL, kw
    for kw in ({"page": 8}, {"page": 24}, {"page": 0}, {"page": 1024}, {"pages": -1}, {"table": None}, {"table": FAKE + 2}, {"table_ld": 31}):
        assert paged(**kw) == EINVAL, kw
    # empty calls are answered before a pointer is looked at, but after the cache's form
    assert flat(items=0, k=None) == OK and flat(Smax=0, k=None, bounds=None) == OK and paged(items=0, k=None) == OK
    assert paged(pages=0, k=None) == OK  # an empty pool: every key is invisible, nothing is read or written
    assert paged(items=0, page=24) == EINVAL and flat(items=0, D=48) == EINVAL


@pytest.mark.parametrize("s", SUFFIXES)
def test_lists_entries_validate_before_any_hip_call(lib, s):
    base = dict(ids=FAKE, counts=FAKE, K=4, items=8, heads=2, T=1, Smax=512, D=64, q=FAKE, ldq=64, k=FAKE, ldk=64, headK=512 * 64,
                outerK=2 * 512 * 64, lens=FAKE, lens_count=4, group=4, chunk=2, k_scale=FAKE, k_count=2, v_scale=None, v_count=1,
                out=FAKE, lse=FAKE, ws=FAKE, ws_bytes=1 << 30, table=FAKE, table_ld=32, pages=100, page=16)

    def tail(a):
        D = a["D"]
        return (D, a["q"], a["ldq"], a["T"] * a["ldq"], a["k"], a["ldk"], a["headK"], a["outerK"], FAKE, D, a["headK"], a["outerK"],
                a["lens"], a["lens_count"], a["group"], a["chunk"], 1.0, a["k_scale"], a["k_count"], a["v_scale"], a["v_count"],
                a["out"], D, a["T"] * D, a["lse"], a["ws"], a["ws_bytes"], None)

    def flat(**kw):
        a = {**base, **kw}
        return getattr(lib, f"mi_block_attention_lists_decode_fp8_{s}")(a["ids"], a["counts"], a["K"], a["items"], a["heads"], a["T"],
                                                                        a["Smax"], *tail(a))

    def paged(**kw):
        a = {**base, "headK": 16 * 64, "outerK": 2 * 16 * 64, **kw}
        return getattr(lib, f"mi_block_attention_lists_decode_paged_fp8_{s}")(a["ids"], a["counts"], a["K"], a["items"], a["heads"],
                                                                              a["T"], a["Smax"], a["table"], a["table_ld"], a["pages"],
                                                                              a["page"], *tail(a))

    for kw in ({"K": 0}, {"K": -1}, {"K": 2 ** 31 // 64}, {"ids": None}, {"ids": FAKE + 2}, {"counts": None}, {"counts": FAKE + 2},
               {"group": 0}, {"group": 17}, {"D": 48}, {"chunk": 0}, {"items": 65536}, {"T": 65536}, {"Smax": 500}, {"heads": 3},
               {"lens_count": 3}, {"lens": None}, {"q": None}, {"q": FAKE + 8}, {"out": FAKE + 2}, {"lse": None}, {"ldq": 60},
               {"ws": None}, {"ws": FAKE + 4}, {"k": None}, {"k": FAKE + 8}, {"ldk": 60},            # what the lists entries refuse
               {"ldk": 72}, {"headK": 8}, {"headK": 1032}, {"outerK": 2056},                          # bytes: 16, not 8
               {"k_count": 0}, {"k_count": 3}, {"k_count": 8}, {"v_count": 0}, {"v_count": 4}, {"k_count": -1},  # 1 or heads = 2
               {"k_scale": FAKE + 2}, {"v_scale": FAKE + 1}):
        assert flat(**kw) == EINVAL, kw
        assert paged(**kw) == EINVAL, kw
    for kw in ({"page": 8}, {"page": 24}, {"page": 0}, {"pages": -1}, {"table": None}, {"table_ld": 31}):
        assert paged(**kw) == EINVAL, kw
    # the workspace is that of K list positions, whatever Smax is
    need = lib.mi_block_attention_decode_workspace_bytes(8, 1, 4, 64, 4 * 64, 2)
    assert need > 0 and flat(ws_bytes=need - 1) == ENOMEM and paged(ws_bytes=need - 1) == ENOMEM
    for kw in ({"k_scale": None, "k_count": 1}, {"k_count": 1}, {"v_scale": FAKE, "v_count": 2}, {"ldk": 80}):  # accepted so far
        assert flat(ws_bytes=need - 1, **kw) == ENOMEM, kw
    assert flat(K=2, ws=None, ws_bytes=0, items=0) == OK  # one chunk: no workspace; an empty problem
    assert flat(items=65535, heads=1, lens_count=1, k_count=1, T=65535, K=2 ** 20) == ERANGE  # items · T · K beyond int32
    # empty calls: before a pointer is looked at, after the cache's form
    assert flat(items=0, q=None) == OK and paged(T=0, lens=None, table=None) == OK
    assert flat(items=0, K=0) == EINVAL and flat(items=0, k_count=3) == EINVAL and paged(items=0, page=24) == EINVAL


# ---- matmuls on the real extension: refusals before the device ---------------------------------------------------------------

@pytest.fixture()
def real(built):
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import matmuls
    yield matmuls
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)


def test_takes(real):
    for dtype in LOWP:
        for D in (32, 64, 96, 128):
            assert real.key_block_bounds_fp8_takes(dtype, D) and real.key_block_bounds_fp8_takes(dtype, D, 16)
            assert real.key_block_bounds_fp8_takes(dtype, D, 256)
            assert real.block_attention_decode_selected_fp8_takes(dtype, D, 5)
            assert real.block_attention_decode_selected_paged_fp8_takes(dtype, D, 16, 64)
    # dtype is the BOUNDS' dtype: the cache's is fixed
    assert not real.key_block_bounds_fp8_takes(F8, 64) and not real.key_block_bounds_fp8_takes(torch.float32, 64)
    assert not real.key_block_bounds_fp8_takes(torch.bfloat16, 48) and not real.key_block_bounds_fp8_takes(torch.bfloat16, 64, 24)
    assert not real.key_block_bounds_fp8_takes(torch.bfloat16, 64, 8)
    assert not real.block_attention_decode_selected_fp8_takes(torch.float16, 64, 17)
    assert not real.block_attention_decode_selected_fp8_takes(F8, 64, 1)
    assert not real.block_attention_decode_selected_paged_fp8_takes(torch.float16, 64, 4, 8)
    # the 2-byte call keeps refusing an fp8 cache
    assert not real.key_block_bounds_takes(F8, 64) and not real.key_block_bounds_takes(F8, 64, 16)


def _bounds_calls(m):
    lens = torch.tensor([100, 256])
    table = torch.arange(32, dtype=torch.int32).reshape(2, 16) % 20
    flat = lambda k, *a, **kw: m.key_block_bounds_fp8(k, lens, *a, **kw)  # noqa: E731
    paged = lambda k, *a, **kw: m.key_block_bounds_paged_fp8(k, table, lens, *a, **kw)  # noqa: E731
    return (("key_block_bounds_fp8: ", flat, (2, 2, 256, 64), "k", "batch"),
            ("key_block_bounds_paged_fp8: ", paged, (20, 2, 16, 64), "k_pages", "page"))


def test_bounds_refusals_come_before_the_device_with_their_type(real):
    for what, f, shape, kn, outer in _bounds_calls(real):
        n0, H, S, D = shape
        good = _bytes(*shape).view(F8)
        for bad in (torch.float8_e4m3fnuz, torch.float8_e5m2, torch.uint8):
            other = _bytes(*shape) if bad == torch.uint8 else _bytes(*shape).view(bad)
            with pytest.raises(ValueError, match=what + f"{kn} must be float8_e4m3fn, got {bad}: the OCP e4m3fn encoding is what is read"):
                f(other, dtype=torch.bfloat16)
        with pytest.raises(ValueError, match=what + f"{kn} must be float8_e4m3fn, got torch.bfloat16"):  # a 2-byte cache
            f(good.to(torch.bfloat16), dtype=torch.bfloat16)
        with pytest.raises(ValueError, match=what + f"{kn} must be a dense tensor"):
            f(None, dtype=torch.bfloat16)
        # dtype: missing, wrong, or disagreeing with bounds
        for bad in (None, torch.float32, F8, "bfloat16"):
            with pytest.raises(ValueError, match=what + r"dtype must be torch.bfloat16 or torch.float16 when bounds is None"):
                f(good, dtype=bad)
        with pytest.raises(RuntimeError, match=what + "dtype is torch.bfloat16 but bounds is torch.float16"):
            f(good, torch.empty(2, 2, 4, 2, 64).half(), dtype=torch.bfloat16)
        with pytest.raises(ValueError, match=what + "bounds must be bfloat16 or float16, got torch.float32"):
            f(good, torch.empty(2, 2, 4, 2, 64))
        with pytest.raises(ValueError, match=what + "bounds must be bfloat16 or float16, got torch.float8_e4m3fn"):  # no fp8 bounds
            f(good, _bytes(2, 2, 4, 2, 64).view(F8))
        # bounds of wrong shape or non-contiguous
        for bad in (torch.empty(2, 2, 4, 2, 32).bfloat16(), torch.empty(2, 2, 3, 2, 64).bfloat16(),
                    torch.empty(2, 2, 4, 4, 64).bfloat16()[:, :, :, ::2], "x"):
            with pytest.raises(ValueError, match=what + "bounds must be None or a contiguous dense tensor"):
                f(good, bad)
        # byte strides that are no multiple of 16
        with pytest.raises(ValueError, match=what + f"{kn} must have a last stride of 1, got 2"):
            f(_bytes(n0, H, S, 2 * D).view(F8)[..., ::2], dtype=torch.float16)
        with pytest.raises(ValueError, match=what + f"{kn}'s row stride must be a multiple of 16 elements and at least D = 64, got 72"):
            f(_bytes(n0, H, S, D + 8).view(F8)[..., :D], dtype=torch.float16)
        odd_head = _bytes(n0 * H * (S * D + 8)).view(F8).as_strided(shape, (H * (S * D + 8), S * D + 8, D, 1))
        with pytest.raises(ValueError, match=what + f"{kn}'s head stride must be a multiple of 16 elements, got {S * D + 8}"):
            f(odd_head, dtype=torch.float16)
        odd_outer = _bytes(n0 * (H * S * D + 8)).view(F8).as_strided(shape, (H * S * D + 8, S * D, D, 1))
        with pytest.raises(ValueError, match=what + f"{kn}'s {outer} stride must be a multiple of 16 elements, got {H * S * D + 8}"):
            f(odd_outer, dtype=torch.float16)
        with pytest.raises(ValueError, match=what + "head size D must be 32, 64, 96 or 128, got 48"):
            f(_bytes(n0, H, S, 48).view(F8), dtype=torch.float16)
        for bad in (0, -1, 1.0, True, "1", 2 ** 31):
            with pytest.raises(ValueError, match=what + "last must be None"):
                f(good, dtype=torch.bfloat16, last=bad)
        with pytest.raises(TypeError):  # dtype and last are keyword only
            f(good, None, torch.bfloat16)
        with pytest.raises(RuntimeError, match=what + rf"{kn}, .*k_lens must be device \(HIP\) tensors"):
            f(good, dtype=torch.bfloat16)
        with pytest.raises(RuntimeError, match=what + rf"{kn}, .*k_lens, bounds must be device \(HIP\) tensors"):
            f(good, torch.empty(2, 2, 4, 2, 64).half(), dtype=torch.float16, last=3)
    what = "key_block_bounds_paged_fp8: "
    pool, lens = _bytes(20, 2, 16, 64).view(F8), torch.tensor([100, 256])
    table = torch.arange(32, dtype=torch.int32).reshape(2, 16) % 20
    for page in (8, 24):
        with pytest.raises(ValueError, match=what + f"the pool's pages must hold a power of two >= 16 keys, got page = {page}"):
            real.key_block_bounds_paged_fp8(_bytes(20, 2, page, 64).view(F8), table, lens, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match=what + "block_table is required"):
        real.key_block_bounds_paged_fp8(pool, None, lens, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match=what + "Smax = 240 must be a multiple of 64"):
        real.key_block_bounds_paged_fp8(pool, table[:, :15], lens, dtype=torch.bfloat16)


def _selected_calls(m):
    q, lens = torch.rand(2, 8, 1, 64).bfloat16(), torch.tensor([100, 256])
    ids, counts = torch.zeros(2, 2, 1, 3, dtype=torch.int32), torch.ones(2, 2, 1, dtype=torch.int32)
    table = torch.arange(32, dtype=torch.int32).reshape(2, 16) % 20

    def flat(k, v, ids=ids, counts=counts, q=q, **kw):
        return m.block_sparse_attention_decode_selected_fp8(q, k, v, ids, counts, lens, **kw)

    def paged(k, v, ids=ids, counts=counts, q=q, **kw):
        return m.block_sparse_attention_decode_selected_paged_fp8(q, k, v, table, ids, counts, lens, **kw)

    return (("block_sparse_attention_decode_selected_fp8: ", flat, (2, 2, 256, 64), "k", "v", "batch"),
            ("block_sparse_attention_decode_selected_paged_fp8: ", paged, (20, 2, 16, 64), "k_pages", "v_pages", "page"))


def test_decode_selected_refusals_come_before_the_device_with_their_type(real):
    for what, f, shape, kn, vn, outer in _selected_calls(real):
        n0, H, S, D = shape
        good = _bytes(*shape).view(F8)
        ids, counts = torch.zeros(2, 2, 1, 3, dtype=torch.int32), torch.ones(2, 2, 1, dtype=torch.int32)
        for bad in (torch.float8_e4m3fnuz, torch.float8_e5m2, torch.uint8):
            other = _bytes(*shape) if bad == torch.uint8 else _bytes(*shape).view(bad)
            with pytest.raises(ValueError, match=what + f"{kn} must be float8_e4m3fn, got {bad}: the OCP e4m3fn encoding is what is read"):
                f(other, other)
            with pytest.raises(RuntimeError, match=what + f"{kn} is torch.float8_e4m3fn but {vn} is {bad}"):  # a mixed cache
                f(good, other)
        with pytest.raises(RuntimeError, match=what + f"{kn} is torch.bfloat16 but {vn} is torch.float8_e4m3fn"):
            f(good.to(torch.bfloat16), good)
        with pytest.raises(ValueError, match=what + f"{kn} must be float8_e4m3fn, got torch.bfloat16"):  # a 2-byte cache
            f(good.to(torch.bfloat16), good.to(torch.bfloat16))
        with pytest.raises(ValueError, match=what + "q must be bfloat16 or float16"):
            f(good, good, q=torch.rand(2, 8, 1, 64))
        # the lists
        for bad in (ids.long(), ids.float(), None, ids.tolist()):
            with pytest.raises(ValueError, match=what + "block_ids must be a dense int32 tensor"):
                f(good, good, ids=bad)
        with pytest.raises(ValueError, match=what + "block_counts must be a dense int32 tensor"):
            f(good, good, counts=counts.long())
        for bad in (ids[0], ids[:, :1], torch.zeros(2, 2, 2, 3, dtype=torch.int32), ids[..., :0],
                    torch.zeros(2, 2, 1, 6, dtype=torch.int32)[..., ::2]):
            with pytest.raises(ValueError, match=what + r"block_ids must be a contiguous \[B, Hkv, T, K\] = \[2, 2, 1, K >= 1\]"):
                f(good, good, ids=bad)
        for bad in (counts[0], torch.ones(2, 2, 2, dtype=torch.int32), torch.ones(2, 2, 2, dtype=torch.int32)[..., ::2]):
            with pytest.raises(ValueError, match=what + r"block_counts must be a contiguous \[B, Hkv, T\] = \[2, 2, 1\]"):
                f(good, good, counts=bad)
        # byte strides
        with pytest.raises(ValueError, match=what + f"{vn}'s row stride must be a multiple of 16 elements and at least D = 64, got 72"):
            f(good, _bytes(n0, H, S, D + 8).view(F8)[..., :D])
        odd_outer = _bytes(n0 * (H * S * D + 8)).view(F8).as_strided(shape, (H * S * D + 8, S * D, D, 1))
        with pytest.raises(ValueError, match=what + f"{kn}'s {outer} stride must be a multiple of 16 elements, got {H * S * D + 8}"):
            f(odd_outer, good)
        # the scales: shape, dtype, device
        for name in ("k_scale", "v_scale"):
            for bad in (torch.ones(2, dtype=torch.float64), torch.ones(2, dtype=torch.bfloat16), torch.ones(2, dtype=torch.int32)):
                with pytest.raises(ValueError, match=what + f"{name} must be a float32 tensor, got {bad.dtype}"):
                    f(good, good, **{name: bad})
            for bad in (torch.ones(3), torch.ones(8), torch.ones(2, 1), torch.ones(0)):
                with pytest.raises(ValueError, match=what + rf"{name} must have shape \(\), \(1,\) or \(2,\)"):
                    f(good, good, **{name: bad})
            for bad in ("0.5", [0.5, 0.5], True):
                with pytest.raises(ValueError, match=what + f"{name} must be None, a float or a dense float32 tensor"):
                    f(good, good, **{name: bad})
            with pytest.raises(RuntimeError, match=what + f"{name} is on meta but q is on cpu"):
                f(good, good, **{name: torch.ones(2, device="meta")})
        for bad in (0, -1, 2.0, True, "4", 2 ** 31):
            with pytest.raises(ValueError, match=what + "chunk must be None or a positive int"):
                f(good, good, chunk=bad)
        with pytest.raises(ValueError, match=what + f"{vn} must be a dense tensor with {kn}'? ?s? shape"):
            f(good, _bytes(n0, H, S * 2, D).view(F8))
        # host tensors: the last check — the scales are named with the operands
        with pytest.raises(RuntimeError, match=what + r"q, .*block_ids, block_counts, k_lens, k_scale, v_scale must be device \(HIP\) tensors"):
            f(good, good, k_scale=torch.ones(2), v_scale=torch.ones(()))
        with pytest.raises(RuntimeError, match=what + r"q, .*block_ids, block_counts, k_lens must be device \(HIP\) tensors"):
            f(good, good, k_scale=0.5)
    with pytest.raises(ValueError, match="block_sparse_attention_decode_selected_fp8: Smax = 200 must be a multiple of 64"):
        k = _bytes(2, 2, 200, 64).view(F8)
        real.block_sparse_attention_decode_selected_fp8(torch.rand(2, 8, 1, 64).bfloat16(), k, k, torch.zeros(2, 2, 1, 3, dtype=torch.int32),
                                                        torch.ones(2, 2, 1, dtype=torch.int32), torch.tensor([100, 200]))


def test_the_four_existing_calls_still_refuse_an_fp8_cache(real):
    q, lens = torch.rand(2, 8, 1, 64).bfloat16(), torch.tensor([100, 256])
    k8, pool = _bytes(2, 2, 256, 64).view(F8), _bytes(20, 2, 16, 64).view(F8)
    table = torch.arange(32, dtype=torch.int32).reshape(2, 16) % 20
    ids, counts = torch.zeros(2, 2, 1, 3, dtype=torch.int32), torch.ones(2, 2, 1, dtype=torch.int32)
    with pytest.raises(ValueError, match="key_block_bounds: k must be bfloat16 or float16, got torch.float8_e4m3fn"):
        real.key_block_bounds(k8, lens)
    with pytest.raises(ValueError, match="key_block_bounds_paged: k_pages must be bfloat16 or float16, got torch.float8_e4m3fn"):
        real.key_block_bounds_paged(pool, table, lens)
    with pytest.raises(ValueError, match="block_sparse_attention_decode_selected: k must be bfloat16 or float16, got torch.float8_e4m3fn"):
        real.block_sparse_attention_decode_selected(q, k8, k8, ids, counts, lens)
    with pytest.raises(ValueError, match="block_sparse_attention_decode_selected_paged: k_pages must be bfloat16 or float16, got "
                                         "torch.float8_e4m3fn"):
        real.block_sparse_attention_decode_selected_paged(q, pool, pool, table, ids, counts, lens)


def test_bindings_refuse_host_tensors_other_dtypes_and_keywords(built):
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import custom_mm
    q, lens, lse = torch.rand(1, 2, 1, 32).bfloat16(), torch.tensor([5], dtype=torch.int32), torch.empty(1, 2, 1)
    k8, pool, table = _bytes(1, 1, 64, 32).view(F8), _bytes(5, 1, 16, 32).view(F8), torch.zeros(1, 4, dtype=torch.int32)
    bounds = torch.empty(1, 1, 1, 2, 32).bfloat16()
    ids, counts = torch.zeros(1, 1, 1, 2, dtype=torch.int32), torch.ones(1, 1, 1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.kv_block_bounds_fp8(k8, lens, 0, bounds)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.kv_block_bounds_paged_fp8(pool, table, lens, 0, bounds)
    with pytest.raises(RuntimeError, match="OCP e4m3fn encoding is what is read"):
        custom_mm.kv_block_bounds_fp8(k8.view(torch.uint8), lens, 0, bounds)
    with pytest.raises(RuntimeError, match="OCP e4m3fn encoding is what is read"):
        custom_mm.kv_block_bounds_fp8(k8.to(torch.bfloat16), lens, 0, bounds)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.block_attention_lists_decode_fp8(ids, counts, q, k8, k8, lens, 1.0, None, None, 4, torch.empty_like(q), lse)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.block_attention_lists_decode_paged_fp8(ids, counts, q, pool, pool, table, lens, 1.0, None, None, 4, torch.empty_like(q), lse)
    with pytest.raises(RuntimeError, match="OCP e4m3fn encoding is what is read"):
        custom_mm.block_attention_lists_decode_fp8(ids, counts, q, k8.view(torch.float8_e4m3fnuz), k8, lens, 1.0, None, None, 4,
                                                   torch.empty_like(q), lse)
    with pytest.raises(TypeError):  # positional only
        custom_mm.block_attention_lists_decode_fp8(ids, counts, q, k8, k8, lens, 1.0, None, None, chunk=4, out=torch.empty_like(q), lse=lse)


# ---- wiring on CPU tensors, through the stand-in -----------------------------------------------------------------------------

@pytest.fixture()
def mm(oracle_mod):
    """(matmuls bound to the stand-in, the stand-in)."""
    import fake_custom_mm_block_select_fp8 as fake
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


@pytest.mark.parametrize("dtype", LOWP)
def test_bounds_operands_uncopied_and_the_result_of_the_widened_cache(mm, dtype):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(3)
    base = random_fp8(g, (2, 256, 2, 80))
    k = base.transpose(1, 2)[..., :64]            # a strided view: head stride 80, row stride 160 bytes
    lens = torch.tensor([130, 64])
    for b in range(2):
        k.view(torch.uint8)[b, :, int(lens[b]):] = 0x7F   # unseen rows are never read
    out = matmuls.key_block_bounds_fp8(k, lens, dtype=dtype)
    name, call = fake.calls[-1]
    assert name == "kv_block_bounds_fp8" and call["k_ptr"] == k.data_ptr() and call["k_stride"] == tuple(k.stride())
    assert call["k_dtype"] == F8 and call["last"] == 0 and call["bounds_dtype"] == dtype
    assert out.shape == (2, 2, 4, 2, 64) and out.dtype == dtype and not out.requires_grad
    wide = k.to(dtype)
    ref = matmuls.key_block_bounds(wide, lens, torch.zeros(2, 2, 4, 2, 64, dtype=dtype))
    for b, blocks in ((0, 3), (1, 1)):
        assert torch.equal(out[b, :, :blocks].view(torch.int16), ref[b, :, :blocks].view(torch.int16))
        assert not torch.isnan(out[b, :, :blocks].float()).any()
    # in place: the same object comes back, its dtype decides, last reaches the binding
    pre = torch.full((2, 2, 4, 2, 64), 7.0, dtype=dtype)
    same = matmuls.key_block_bounds_fp8(k, lens, pre, last=3)
    assert same is pre and fake.calls[-1][1]["bounds_ptr"] == pre.data_ptr() and fake.calls[-1][1]["last"] == 3
    assert torch.equal(pre[0, :, 1:3], ref[0, :, 1:3]) and torch.all(pre[0, :, 0] == 7) and torch.all(pre[0, :, 3] == 7)
    assert matmuls.key_block_bounds_fp8(k, lens, pre, dtype=dtype) is pre   # an agreeing dtype is accepted
    # paged: the pool uncopied, an int32 table handed over as it is, an int64 one narrowed
    kc = k.contiguous()
    kp, _, table = _paged(g, kc.view(torch.uint8), kc.view(torch.uint8), 16, fill=0x7F)
    kp = kp.view(F8)
    got = matmuls.key_block_bounds_paged_fp8(kp, table, lens, dtype=dtype)
    name, call = fake.calls[-1]
    assert name == "kv_block_bounds_paged_fp8" and call["k_ptr"] == kp.data_ptr() and call["table_ptr"] == table.data_ptr()
    for b, blocks in ((0, 3), (1, 1)):
        assert torch.equal(got[b, :, :blocks], out[b, :, :blocks])
    matmuls.key_block_bounds_paged_fp8(kp, table.long(), lens, dtype=dtype)
    assert fake.calls[-1][1]["table_dtype"] == torch.int32 and fake.calls[-1][1]["table_ptr"] != table.data_ptr()
    assert torch.equal(_gathered(kp.view(torch.uint8), table)[0, :, :130], kc.view(torch.uint8)[0, :, :130])


def test_decode_selected_operands_and_scales_uncopied(mm):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(7)
    B, Hkv, G, T, D, Smax = 2, 2, 3, 2, 32, 256
    q = torch.randn(B, Hkv * G, T, D, generator=g).half()
    k, v = (random_fp8(g, (B, Smax, Hkv, D + 16)).transpose(1, 2)[..., :D] for _ in range(2))
    lens = torch.tensor([200, 70])
    for b in range(B):
        k.view(torch.uint8)[b, :, int(lens[b]):] = 0x7F
        v.view(torch.uint8)[b, :, int(lens[b]):] = 0x7F
    ids = torch.tensor([[3, 0, -1, 2], [1, 0, 0, 0]], dtype=torch.int32).repeat(B, Hkv, 1, 1).contiguous()   # [B, Hkv, T, 4]
    counts = torch.tensor([4, 1], dtype=torch.int32).repeat(B, Hkv, 1).contiguous()
    ks, vs = torch.tensor([0.5, 2.0]), torch.tensor(0.25)
    out, lse = matmuls.block_sparse_attention_decode_selected_fp8(q, k, v, ids, counts, lens, k_scale=ks, v_scale=vs, chunk=2,
                                                                  return_lse=True)
    name, call = fake.calls[-1]
    assert name == "block_attention_lists_decode_fp8" and call["ids_ptr"] == ids.data_ptr() and call["counts_ptr"] == counts.data_ptr()
    assert call["k_ptr"] == k.data_ptr() and call["k_stride"] == tuple(k.stride()) and call["v_ptr"] == v.data_ptr()
    assert call["k_dtype"] == F8 and call["v_dtype"] == F8 and call["chunk"] == 2
    assert call["k_scale"]["ptr"] == ks.data_ptr() and call["v_scale"]["ptr"] == vs.data_ptr() and call["v_scale"]["shape"] == ()
    assert not out.requires_grad and not torch.isnan(out).any()
    # the 2-byte selected call on the dequantised cache (exact in float16: powers of two)
    kd = (k.to(torch.float16) * ks.half().reshape(1, 2, 1, 1)).contiguous()
    vd = (v.to(torch.float16) * vs.half()).contiguous()
    for x, n in ((kd, lens), (vd, lens)):
        for b in range(B):
            x[b, :, int(n[b]):] = 0
    ref, ref_lse = matmuls.block_sparse_attention_decode_selected(q, kd, vd, ids, counts, lens, chunk=2, return_lse=True)
    assert torch.equal(out, ref) and torch.equal(lse, ref_lse)
    # floats become 0-d tensors; None stays None
    matmuls.block_sparse_attention_decode_selected_fp8(q, k, v, ids, counts, lens, k_scale=0.5)
    call = fake.calls[-1][1]
    assert call["k_scale"]["shape"] == () and float(call["k_scale"]["value"]) == 0.5 and call["v_scale"] is None
    # the paged form: the pool and the table uncopied, the contiguous result on the gathered bytes
    kp, vp, table = _paged(g, k.contiguous().view(torch.uint8), v.contiguous().view(torch.uint8), 16, fill=0x7F)
    kp, vp = kp.view(F8), vp.view(F8)
    got = matmuls.block_sparse_attention_decode_selected_paged_fp8(q, kp, vp, table, ids, counts, lens, k_scale=ks, v_scale=vs, chunk=2)
    name, call = fake.calls[-1]
    assert name == "block_attention_lists_decode_paged_fp8" and call["k_ptr"] == kp.data_ptr() and call["table_ptr"] == table.data_ptr()
    assert torch.equal(got, out)
    # count 0: zero rows, lse −inf
    out0, lse0 = matmuls.block_sparse_attention_decode_selected_fp8(q, k, v, ids, torch.zeros_like(counts), lens, return_lse=True)
    assert out0.eq(0).all() and torch.isinf(lse0).all()
