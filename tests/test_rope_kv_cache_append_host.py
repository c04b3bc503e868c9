"""matmuls.rope_kv_cache_append and rope_kv_cache_append_paged without a GPU: every refusal with its exception
type, before the device — the append's own and those of q, cos / sin, rotary_dim, new_lens, q_out and k_out —; what reaches the
bindings through the stand-in tests/fake_custom_mm_rope_kv_append.py — q, k_new, v_new, the cache, an int32 table, cos, sin
and tensor scales uncopied, int64 lengths narrowed —; the rule on CPU tensors; the two `takes`; and the eight entries of the
C ABI: declared, exported, MI_EINVAL / MI_ERANGE before any HIP call."""
import ctypes
import importlib
import re
import sys
from pathlib import Path

import pytest
import torch

import rope_reference as ref

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "mi_spmm.h"
OK, EINVAL, ERANGE = 0, -1, -2
FAKE = 0x1000  # a non-null, 16-byte aligned address that is never dereferenced: every call below returns before the device
F8 = torch.float8_e4m3fn
ENTRIES = ("mi_rope_kv_append_bf16", "mi_rope_kv_append_f16", "mi_rope_kv_append_paged_bf16", "mi_rope_kv_append_paged_f16",
           "mi_rope_kv_append_fp8_bf16", "mi_rope_kv_append_fp8_f16", "mi_rope_kv_append_paged_fp8_bf16",
           "mi_rope_kv_append_paged_fp8_f16")


# ---- the C ABI -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(built):
    import torch  # noqa: F401  (torch's HIP runtime first, as in the product)
    lib = ctypes.CDLL(str(built / "libmi_spmm.so"))
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    for name in ENTRIES:
        fn = getattr(lib, name)
        table = [vp, i64, i32, i32] if "paged" in name else []
        scales = [vp, i32, vp, i32] if "fp8" in name else []
        fn.argtypes = (4 * [i32] + table + [i32] + [i32] + 5 * [vp, i64, i64, i64] + [vp, vp, i32, i64, i32, i32] + 2 * [vp, i64, i64, i64]
                       + [vp, i32, vp] + scales + [vp])
        fn.restype = ctypes.c_int
    return lib


def test_header_declares_and_library_exports_the_eight_entries(lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    operands = re.search(r"#define MI_ROPE_KV_APPEND_OPERANDS\(CT\)(.*?)\n(?!\s)", text.replace("\\\n", " "), flags=re.S).group(1)
    names = [a.split()[-1].lstrip("*") for a in operands.split(",")]
    assert names[:5] == ["q_heads", "q", "ldq", "headQ", "batchQ"] and names[-1] == "new_lens"
    for must in ("q_out", "k_new", "v_new", "k_out", "cos", "sin", "table_rows", "ld", "rotary_dim", "interleaved", "k", "v", "k_lens",
                 "lens_count"):
        assert must in names, must
    assert len(re.findall(r"const uint16_t\s*\*", operands)) == 3 and len(re.findall(r"const float\s*\*", operands)) == 2
    assert len(re.findall(r"\bCT\s*\*", operands)) == 2
    for name in ENTRIES:
        assert hasattr(lib, name), name
        args = re.search(rf"\b{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        head = [a.split()[-1].lstrip("*") for a in args.split("MI_ROPE_KV_APPEND_OPERANDS")[0].split(",") if a.strip()]
        assert head[:4] == ["items", "heads", "T", "Smax"] and head[-1] == "D" and args.rstrip().endswith("stream")
        assert ("block_table" in head) == ("paged" in name) and ("k_scale" in args) == ("fp8" in name)
        assert f"MI_ROPE_KV_APPEND_OPERANDS({'uint8_t' if 'fp8' in name else 'uint16_t'})" in args


DEFAULTS = dict(items=8, heads=2, T=3, Smax=512, table=FAKE, table_ld=32, pages=100, page=16, D=64, q_heads=4, q=FAKE, ldq=None,
                headQ=None, batchQ=None, q_out=FAKE, ldqo=None, k_new=FAKE, ldkn=None, headKn=None, batchKn=None, k_out=None, ldko=None,
                headKo=None, cos=FAKE, sin=FAKE, table_rows=1024, ld=32, R=64, inter=0, k=FAKE, ldk=None, headK=None, outerK=None,
                k_lens=FAKE, lens_count=4, new_lens=None, k_scale=FAKE, k_count=2, v_scale=None, v_count=1)


def rope(lib, name, **kw):
    a = {**DEFAULTS, **kw}
    D, T, heads, Hq = a["D"], a["T"], a["heads"], a["q_heads"]
    rows = a["page"] if "paged" in name else a["Smax"]
    d = lambda n, v: v if a[n] is None else a[n]  # noqa: E731
    table = (a["table"], a["table_ld"], a["pages"], a["page"]) if "paged" in name else ()
    scales = (a["k_scale"], a["k_count"], a["v_scale"], a["v_count"]) if "fp8" in name else ()
    return getattr(lib, name)(
        a["items"], heads, T, a["Smax"], *table, D, Hq,
        a["q"], d("ldq", D), d("headQ", T * D), d("batchQ", Hq * T * D), a["q_out"], d("ldqo", D), T * D, Hq * T * D,
        a["k_new"], d("ldkn", D), d("headKn", T * D), d("batchKn", heads * T * D), FAKE, D, T * D, heads * T * D,
        a["k_out"], d("ldko", D), d("headKo", T * D), heads * T * D,
        a["cos"], a["sin"], a["table_rows"], a["ld"], a["R"], a["inter"],
        a["k"], d("ldk", D), d("headK", rows * D), d("outerK", heads * rows * D), FAKE, D, rows * D, heads * rows * D,
        a["k_lens"], a["lens_count"], a["new_lens"], *scales, None)


@pytest.mark.parametrize("name", ENTRIES)
def test_rope_entries_validate_before_any_hip_call(lib, name):
    unit = 16 if "fp8" in name else 8
    for kw in ({"D": 48}, {"D": 0}, {"D": 256}, {"items": -1}, {"items": 65536}, {"T": -1}, {"Smax": -16}, {"heads": 3}, {"heads": -2},
               {"lens_count": 3}, {"lens_count": 0}, {"lens_count": 8}, {"lens_count": 2},      # 1 or B = 4: q has no k / v head
               {"k_lens": None}, {"k_lens": FAKE + 2}, {"new_lens": FAKE + 2},
               {"k_new": None}, {"k_new": FAKE + 8}, {"ldkn": 60}, {"ldkn": -8}, {"headKn": 100}, {"batchKn": 4},   # the source: 8 elements
               {"q": None}, {"q": FAKE + 8}, {"ldq": 60}, {"headQ": -8}, {"batchQ": 4}, {"q_heads": -1}, {"q_heads": 0},
               {"q_out": None}, {"q_out": FAKE + 2}, {"ldqo": 68},
               {"k_out": FAKE + 4}, {"k_out": FAKE, "ldko": 12}, {"k_out": FAKE, "headKo": -8},
               {"R": 0}, {"R": 8}, {"R": 24}, {"R": 80}, {"R": 128}, {"R": -16},                                      # 16 ≤ R ≤ D = 64, R % 16 == 0
               {"cos": None}, {"sin": None}, {"cos": FAKE + 8}, {"sin": FAKE + 4}, {"ld": 31}, {"ld": 16}, {"ld": 34}, {"table_rows": -1},
               {"k": None}, {"k": FAKE + 8}, {"ldk": 48}, {"ldk": 64 + unit // 2}, {"headK": unit // 2}, {"outerK": 512 * 64 * 2 + 4},
               {"outerK": -unit}):
        assert rope(lib, name, **kw) == EINVAL, kw
    if "paged" in name:
        for kw in ({"page": 8}, {"page": 24}, {"page": 0}, {"page": 1024}, {"pages": -1}, {"table": None}, {"table": FAKE + 2},
                   {"table_ld": 31}):
            assert rope(lib, name, **kw) == EINVAL, kw
    if "fp8" in name:
        for kw in ({"k_count": 0}, {"k_count": 3}, {"k_count": 8}, {"v_count": 4}, {"k_count": -1}, {"k_scale": FAKE + 2},
                   {"v_scale": FAKE + 1}):
            assert rope(lib, name, **kw) == EINVAL, kw
    assert rope(lib, name, items=0, k_new=None, q=None) == OK and rope(lib, name, T=0, k=None, q_out=None) == OK     # nothing to do
    assert rope(lib, name, items=0, D=48) == EINVAL and rope(lib, name, T=0, R=24) == EINVAL                          # … but checked first
    assert rope(lib, name, items=65534, T=2 ** 31 - 1, lens_count=1) == ERANGE              # B · (Hq + 2·heads) · T · D/8 ≥ 2³¹
    assert rope(lib, name, items=2, T=2 ** 24, q_heads=2 ** 20, lens_count=1) == ERANGE     # … through q's heads alone


# ---- matmuls on the real extension: refusals before the device -------------------------------------------------------

@pytest.fixture()
def real(built):
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import matmuls
    yield matmuls
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)


B, HQ, HKV, T, D, SMAX, PAGE, P, W, PMAX = 2, 4, 2, 3, 64, 96, 16, 20, 6, 128


def _tables(R=D, pmax=PMAX):
    ang = torch.arange(pmax, dtype=torch.float64)[:, None] * 10000.0 ** (-2.0 * torch.arange(R // 2, dtype=torch.float64) / R)
    return ang.cos().float(), ang.sin().float()


def _forms(m):
    """(prefix, call(q, k_new, v_new, cos, sin, k, v, **kw), cache shape, names, outer) of the two calls."""
    lens = torch.tensor([50, 96])
    table = torch.arange(B * W, dtype=torch.int32).reshape(B, W) % P
    flat = lambda q, kn, vn, c, s, k, v, lens=lens, **kw: m.rope_kv_cache_append(q, kn, vn, c, s, k, v, lens, **kw)  # noqa: E731
    paged = lambda q, kn, vn, c, s, k, v, lens=lens, table=table, **kw: m.rope_kv_cache_append_paged(  # noqa: E731
        q, kn, vn, c, s, k, v, table, lens, **kw)
    return (("rope_kv_cache_append: ", flat, (B, HKV, SMAX, D), "k", "v", "batch"),
            ("rope_kv_cache_append_paged: ", paged, (P, HKV, PAGE, D), "k_pages", "v_pages", "page"))


def test_every_refusal_comes_before_the_device_with_its_type(real):
    cos, sin = _tables()
    for what, f, shape, kn, vn, outer in _forms(real):
        n0, H, S, _ = shape
        q = torch.zeros(B, HQ, T, D, dtype=torch.bfloat16)
        new = torch.zeros(B, HKV, T, D, dtype=torch.bfloat16)
        c16, c8 = torch.zeros(shape, dtype=torch.bfloat16), torch.zeros(shape, dtype=torch.uint8).view(F8)
        # ---- the append's own, through the same functions: what the source and the cache are …
        with pytest.raises(ValueError, match=what + "k_new must be bfloat16 or float16, got torch.float32"):
            f(q, new.float(), new, cos, sin, c16, c16)
        with pytest.raises(ValueError, match=what + "v_new must be a dense tensor"):
            f(q, new, None, cos, sin, c16, c16)
        with pytest.raises(RuntimeError, match=what + "q is torch.bfloat16 but v_new is torch.float16"):
            f(q, new, new.half(), cos, sin, c16, c16)
        with pytest.raises(ValueError, match=what + f"{kn} must be a dense tensor"):
            f(q, new, new, cos, sin, torch.ones(4, 4).to_sparse_csr(), c16)
        with pytest.raises(ValueError, match=what + f"{kn} must have k_new's dtype or be float8_e4m3fn, got torch.float32"):
            f(q, new, new, cos, sin, c16.float(), c16.float())
        with pytest.raises(RuntimeError, match=what + f"k_new is torch.bfloat16 but {vn} is torch.float16"):
            f(q, new, new, cos, sin, c16, c16.half())
        for bad in (torch.float8_e4m3fnuz, torch.float8_e5m2, torch.uint8):
            with pytest.raises(ValueError, match=what + f"{kn} must be float8_e4m3fn, got {bad}: the OCP e4m3fn encoding is what is read"):
                f(q, new, new, cos, sin, c8.view(bad), c8.view(bad))
        with pytest.raises(ValueError, match=what + "k_scale goes with a float8_e4m3fn cache only"):
            f(q, new, new, cos, sin, c16, c16, k_scale=0.5)
        # … shapes, lengths, strides, scales
        with pytest.raises(ValueError, match=what + "k_new and v_new must be .B, Hkv, T, D."):
            f(q, new[0], new[0], cos, sin, c16, c16)
        with pytest.raises(ValueError, match=what + "v_new must have k_new's shape"):
            f(q, new, new[:, :, :2], cos, sin, c16, c16)
        with pytest.raises(ValueError, match=what + "head size D must be 32, 64, 96 or 128, got 48"):
            f(q[..., :48], new[..., :48], new[..., :48], cos, sin, c16[..., :48], c16[..., :48])
        with pytest.raises(ValueError, match=what + "k_new must hold T >= 1 new tokens"):
            f(q[:, :, :0], new[:, :, :0], new[:, :, :0], cos, sin, c16, c16)
        with pytest.raises(ValueError, match=what + f"k_new of shape .* needs {kn}"):
            f(q, new, new, cos, sin, c16[:, :1], c16[:, :1])
        with pytest.raises(ValueError, match=what + "k_lens is required and must be a dense tensor"):
            f(q, new, new, cos, sin, c16, c16, lens=None)
        with pytest.raises(ValueError, match=what + "k_lens must be an int32 or int64 tensor, got torch.float32"):
            f(q, new, new, cos, sin, c16, c16, lens=torch.tensor([1.0, 2.0]))
        with pytest.raises(ValueError, match=what + r"k_lens must have shape \(2,\)"):
            f(q, new, new, cos, sin, c16, c16, lens=torch.tensor([1, 2, 3]))
        with pytest.raises(ValueError, match=what + f"v_new's token stride must be a multiple of 8 elements, got {D + 4}"):
            f(q, new, torch.zeros(B, HKV, T, D + 4, dtype=torch.bfloat16)[..., :D], cos, sin, c16, c16)
        with pytest.raises(ValueError, match=what + f"{kn}'s row stride must be a multiple of 8 elements and at least D = 64, got 68"):
            f(q, new, new, cos, sin, torch.zeros(n0, H, S, D + 4, dtype=torch.bfloat16)[..., :D], c16)
        with pytest.raises(ValueError, match=what + f"{vn}'s row stride must be a multiple of 16 elements and at least D = 64, got 72"):
            f(q, new, new, cos, sin, c8, torch.zeros(n0, H, S, D + 8, dtype=torch.uint8).view(F8)[..., :D])
        with pytest.raises(ValueError, match=what + r"k_scale must have shape \(\), \(1,\) or \(2,\)"):
            f(q, new, new, cos, sin, c8, c8, k_scale=torch.ones(3))
        with pytest.raises(RuntimeError, match=what + "v_scale is on meta but k_new is on cpu"):
            f(q, new, new, cos, sin, c8, c8, v_scale=torch.ones(2, device="meta"))
        # ---- q
        with pytest.raises(ValueError, match=what + "q must be a dense tensor"):
            f(None, new, new, cos, sin, c16, c16)
        with pytest.raises(ValueError, match=what + "q must be bfloat16 or float16, got torch.float32"):
            f(q.float(), new, new, cos, sin, c16, c16)
        with pytest.raises(RuntimeError, match=what + "q is torch.bfloat16 but k_new is torch.float16"):
            f(q, new.half(), new.half(), cos, sin, c16, c16)
        for bad in (q[0], q[:1], q[:, :, :2], q[..., :32], q[:, :0]):
            with pytest.raises(ValueError, match=what + "k_new of shape .* needs q .2, 'Hq', 3, 64. with Hq >= 1"):
                f(bad, new, new, cos, sin, c16, c16)
        wide = torch.zeros(B, HQ, T, 2 * D, dtype=torch.bfloat16)
        with pytest.raises(ValueError, match=what + "q must have a last stride of 1, got 2"):
            f(wide[..., ::2], new, new, cos, sin, c16, c16)
        with pytest.raises(ValueError, match=what + f"q's token stride must be a multiple of 8 elements, got {D + 4}"):
            f(torch.zeros(B, HQ, T, D + 4, dtype=torch.bfloat16)[..., :D], new, new, cos, sin, c16, c16)
        odd_head = torch.zeros(B * HQ * (T * D + 4), dtype=torch.bfloat16).as_strided((B, HQ, T, D), (HQ * (T * D + 4), T * D + 4, D, 1))
        with pytest.raises(ValueError, match=what + f"q's head stride must be a multiple of 8 elements, got {T * D + 4}"):
            f(odd_head, new, new, cos, sin, c16, c16)
        buf = torch.zeros(q.numel() + 16, dtype=torch.bfloat16)
        shifted = buf[(16 - buf.data_ptr() % 16) // 2 + 4:][:q.numel()].reshape(q.shape)
        assert shifted.data_ptr() % 16 == 8
        with pytest.raises(ValueError, match=what + "q's data pointer must be 16-byte aligned"):
            f(shifted, new, new, cos, sin, c16, c16)
        # ---- rotary_dim
        for bad in (24, 8, 0, 80, 128, -16, 32.0, True):
            with pytest.raises(ValueError, match=what + "rotary_dim must be None or a multiple of 16 with 16 <= rotary_dim <= D = 64"):
                f(q, new, new, cos, sin, c16, c16, rotary_dim=bad)
        with pytest.raises(ValueError, match=what + "interleaved must be a bool"):
            f(q, new, new, cos, sin, c16, c16, interleaved=1)
        # ---- cos / sin
        with pytest.raises(ValueError, match=what + "cos must be a dense tensor"):
            f(q, new, new, None, sin, c16, c16)
        with pytest.raises(ValueError, match=what + "sin must be a float32 tensor, got torch.float64"):
            f(q, new, new, cos, sin.double(), c16, c16)
        with pytest.raises(ValueError, match=what + "cos must be a float32 tensor, got torch.bfloat16"):
            f(q, new, new, cos.bfloat16(), sin, c16, c16)
        with pytest.raises(ValueError, match=what + r"cos must have shape \(Pmax, rotary_dim / 2 = 32\)"):
            f(q, new, new, cos[:, :16], sin[:, :16], c16, c16)
        with pytest.raises(ValueError, match=what + r"cos must have shape \(Pmax, rotary_dim / 2 = 16\)"):
            f(q, new, new, cos, sin, c16, c16, rotary_dim=32)
        with pytest.raises(ValueError, match=what + r"cos must have shape \(Pmax, rotary_dim / 2 = 32\)"):
            f(q, new, new, cos[0], sin[0], c16, c16)
        with pytest.raises(ValueError, match=what + "sin must have cos's shape"):
            f(q, new, new, cos, sin[:64], c16, c16)
        both = torch.zeros(PMAX, D)
        with pytest.raises(ValueError, match=what + "cos must have a last stride of 1, got 2"):
            f(q, new, new, both[:, ::2], sin, c16, c16)
        with pytest.raises(ValueError, match=what + "sin's row stride must be a multiple of 4 elements and at least rotary_dim / 2 = 32, got 34"):
            f(q, new, new, cos, torch.zeros(PMAX, 34)[:, :32], c16, c16)
        with pytest.raises(ValueError, match=what + "cos's row stride must be a multiple of 4 elements and at least rotary_dim / 2 = 32, got 0"):
            f(q, new, new, cos[:1].expand(PMAX, 32), sin, c16, c16)
        with pytest.raises(ValueError, match=what + "cos and sin must have one row stride, got 32 and 64"):
            f(q, new, new, cos, both[:, :32], c16, c16)
        with pytest.raises(ValueError, match=what + "sin's data pointer must be 16-byte aligned"):
            f(q, new, new, cos, torch.zeros(PMAX, 36)[:, 2:34].as_strided((PMAX, 32), (36, 1), 2), c16, c16)
        # ---- new_lens
        with pytest.raises(ValueError, match=what + "new_lens must be None or a dense tensor"):
            f(q, new, new, cos, sin, c16, c16, new_lens=[1, 2])
        with pytest.raises(ValueError, match=what + "new_lens must be an int32 or int64 tensor, got torch.int16"):
            f(q, new, new, cos, sin, c16, c16, new_lens=torch.tensor([1, 2], dtype=torch.int16))
        for bad in (torch.tensor(2), torch.tensor([1, 2, 3]), torch.tensor([[1, 2]])):
            with pytest.raises(ValueError, match=what + r"new_lens must have shape \(2,\)"):
                f(q, new, new, cos, sin, c16, c16, new_lens=bad)
        # ---- q_out / k_out
        for name, like, like_name, heads in (("q_out", q, "q", HQ), ("k_out", new, "k_new", HKV)):
            with pytest.raises(ValueError, match=what + f"{name} must be None or a dense tensor"):
                f(q, new, new, cos, sin, c16, c16, **{name: 1.0})
            with pytest.raises(ValueError, match=what + f"{name} must be bfloat16 or float16, got torch.float32"):
                f(q, new, new, cos, sin, c16, c16, **{name: like.float()})
            with pytest.raises(RuntimeError, match=what + f"{like_name} is torch.bfloat16 but {name} is torch.float16"):
                f(q, new, new, cos, sin, c16, c16, **{name: like.half()})
            with pytest.raises(ValueError, match=what + f"{name} must have {like_name}'s shape"):
                f(q, new, new, cos, sin, c16, c16, **{name: like[:, :1]})
            with pytest.raises(ValueError, match=what + f"{name}'s token stride must be a multiple of 8 elements, got {D + 4}"):
                f(q, new, new, cos, sin, c16, c16, **{name: torch.zeros(B, heads, T, D + 4, dtype=torch.bfloat16)[..., :D]})
            with pytest.raises(ValueError, match=what + f"{name} must have a last stride of 1, got 2"):
                f(q, new, new, cos, sin, c16, c16, **{name: torch.zeros(B, heads, T, 2 * D, dtype=torch.bfloat16)[..., ::2]})
        with pytest.raises(TypeError):  # everything behind k_lens is keyword only
            real.rope_kv_cache_append(q, new, new, cos, sin, c16, c16, torch.tensor([50, 96]), True) if outer == "batch" else \
                real.rope_kv_cache_append_paged(q, new, new, cos, sin, c16, c16, torch.zeros(B, W, dtype=torch.int32),
                                                torch.tensor([50, 96]), True)
        # ---- the index count: B · (Hq + 2·Hkv) · T · D/8 < 2³¹, through q's heads
        many = torch.zeros(1, 1, 1, D, dtype=torch.bfloat16).expand(B, 2 ** 27, T, D)
        with pytest.raises(ValueError, match=what + r"B·\(Hq \+ 2·Hkv\)·T·D/8 = \d+ must fit an int32 index"):
            f(many, new, new, cos, sin, c16, c16)
        # ---- host tensors: the last checks
        with pytest.raises(RuntimeError, match=what + rf"k_new, v_new, {kn}, {vn}, .*k_lens must be device \(HIP\) tensors"):
            f(q, new, new, cos, sin, c16, c16)


def test_custom_mm_bindings_refuse_host_tensors_and_mismatched_operands(built):
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import custom_mm
    q, new = torch.zeros(1, 2, 1, 32, dtype=torch.bfloat16), torch.zeros(1, 1, 1, 32, dtype=torch.bfloat16)
    lens, cos = torch.tensor([5], dtype=torch.int32), torch.zeros(8, 16)
    k16, pool, table = torch.zeros(1, 1, 64, 32, dtype=torch.bfloat16), torch.zeros(5, 1, 16, 32, dtype=torch.bfloat16), torch.zeros(1, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.rope_kv_append(q, new, new, cos, cos, k16, k16, lens, None, q, None, 32, False, None, None)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.rope_kv_append_paged(q, new, new, cos, cos, pool, pool, table, lens, None, q, None, 32, False, None, None)
    with pytest.raises(RuntimeError, match="q is BFloat16 but v_new is Half"):
        custom_mm.rope_kv_append(q, new, new.half(), cos, cos, k16, k16, lens, None, q, None, 32, False, None, None)
    with pytest.raises(TypeError):  # positional only
        custom_mm.rope_kv_append(q, new, new, cos, cos, k16, k16, lens, None, q, None, 32, False, k_scale=None, v_scale=None)


def test_takes_are_functions_of_their_arguments_alone(real):
    takes, paged = real.rope_kv_cache_append_takes, real.rope_kv_cache_append_paged_takes
    for dtype in (torch.bfloat16, torch.float16):
        for D_ in (32, 64, 96, 128):
            for R in [None] + list(range(16, D_ + 1, 16)):
                assert takes(dtype, dtype, D_, R) and takes(dtype, F8, D_, R)
                assert all(paged(dtype, c, D_, R, page) for c in (dtype, F8) for page in (16, 256))
            for R in (0, 8, 24, D_ + 16, -16, 16.0, True):
                assert not takes(dtype, dtype, D_, R) and not paged(dtype, F8, D_, R, 16)
    assert not takes(torch.bfloat16, torch.float16, 64, None) and not takes(torch.float32, torch.float32, 64, 32)
    assert not takes(torch.bfloat16, torch.float8_e5m2, 64, None) and not takes(torch.bfloat16, F8, 48, 16)
    assert not paged(torch.bfloat16, F8, 64, None, 8) and not paged(torch.bfloat16, F8, 64, 32, 24) and not paged(torch.float16, F8, 64, 64, True)


# ---- wiring on CPU tensors through the stand-in ----------------------------------------------------------------------------

@pytest.fixture()
def mm(oracle_mod):
    """(matmuls bound to the stand-in, the stand-in)."""
    import fake_custom_mm_rope_kv_append as fake
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


def _record(fake, name):
    (_, rec), = [c for c in fake.calls if c[0] == name]
    return rec


def _projection(g, dtype):
    """q, k_new, v_new as slices of one fused projection [B, T, Hq + 2·Hkv, D] through .transpose(1, 2)."""
    qkv = torch.randn(B, T, HQ + 2 * HKV, D, generator=g).to(dtype)
    return qkv, qkv[:, :, :HQ].transpose(1, 2), qkv[:, :, HQ:HQ + HKV].transpose(1, 2), qkv[:, :, HQ + HKV:].transpose(1, 2)


def _i16(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_the_rule_on_a_flat_cache_and_nothing_is_copied(mm, dtype):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(2501)
    _, q, kn, vn = _projection(g, dtype)
    assert not q.is_contiguous() and q.stride() == (T * 8 * D, D, 8 * D, 1)
    wide = torch.zeros(2, PMAX, D // 2 + 4)
    wide[0, :, :D // 2], wide[1, :, :D // 2] = _tables()
    cos, sin = wide[0, :, :D // 2], wide[1, :, :D // 2]                       # a padded row stride
    base = torch.randn(2, B, SMAX, HKV, D, generator=g).to(dtype)            # a [B, Smax, Hkv, D].transpose(1, 2) cache
    for k_lens, lens_dtype, inter in (([50, 96], torch.int32, False), ([2, 98], torch.int64, True), ([0, 1], torch.int32, False)):
        k, v = base[0].clone().transpose(1, 2), base[1].clone().transpose(1, 2)
        lens = torch.tensor(k_lens, dtype=lens_dtype)
        fake.calls.clear()
        out = matmuls.rope_kv_cache_append(q, kn, vn, cos, sin, k, v, lens, interleaved=inter)
        rec = _record(fake, "rope_kv_append")
        for name, t in (("q", q), ("k_new", kn), ("v_new", vn), ("k", k), ("v", v)):          # the caller's memory, through its strides
            assert rec[f"{name}_ptr"] == t.data_ptr() and rec[f"{name}_stride"] == tuple(t.stride()) and rec[f"{name}_dtype"] == dtype
        for name, t in (("cos", cos), ("sin", sin)):
            assert rec[f"{name}_ptr"] == t.data_ptr() and rec[f"{name}_stride"] == (D // 2 + 4, 1)
        assert rec["k_lens_dtype"] == torch.int32 and rec["k_lens_shape"] == (B,)     # narrowed on the way
        assert (rec["k_lens_ptr"] == lens.data_ptr()) == (lens_dtype == torch.int32)
        assert rec["k_scale"] is None and rec["new_lens"] is None and rec["k_out"] is None
        assert rec["rotary_dim"] == D and rec["interleaved"] is inter
        assert out.is_contiguous() and out.shape == q.shape and rec["q_out_ptr"] == out.data_ptr()     # a fresh contiguous q_out
        pos, token = ref.token_slots(B, T, k_lens, PMAX)
        want_q = ref.rotated(_i16(q), dtype, cos, sin, pos, token, D, inter)
        k_rot = ref.rotated(_i16(kn), dtype, cos, sin, pos, token, D, inter)
        assert torch.equal(_i16(out), want_q)
        want_k, want_v = base[0].clone().transpose(1, 2), base[1].clone().transpose(1, 2)
        rows = [(b, t, int(pos[b, t])) for b in range(B) for t in range(T) if token[b, t] and pos[b, t] < SMAX]
        for b, t, p in rows:
            want_k[b, :, p], want_v[b, :, p] = k_rot[b, :, t].view(dtype), vn[b, :, t]
        assert torch.equal(_i16(k), _i16(want_k)) and torch.equal(_i16(v), _i16(want_v))
        assert len(rows) == {50: 6, 2: 3, 0: 1}[k_lens[0]]      # [2, 98]: one dropped in front (zeros in q), two behind (q rotated)
        for b in range(B):
            for t in range(T):
                assert bool(token[b, t]) == bool((out[b, :, t] != 0).any())           # a slot without a token: zero rows
        assert not torch.equal(_i16(out), _i16(q))
    # a 0-d length serves every item; rotation at position 0 is the identity (cos 1, sin 0)
    k, v = base[0].clone().transpose(1, 2), base[1].clone().transpose(1, 2)
    fake.calls.clear()
    out = matmuls.rope_kv_cache_append(q[:, :, 2:], kn[:, :, 2:], vn[:, :, 2:], cos, sin, k, v, torch.tensor(1))
    assert _record(fake, "rope_kv_append")["k_lens_shape"] == (1,)
    assert torch.equal(_i16(out), _i16(q[:, :, 2:])) and torch.equal(_i16(k[:, :, :1]), _i16(kn[:, :, 2:]))
    # no autograd: operands that require grad are detached
    qr = q.clone().float().requires_grad_(True)
    out = matmuls.rope_kv_cache_append(qr.to(dtype), kn, vn, cos, sin, k, v, torch.tensor(7))
    assert not out.requires_grad and not k.requires_grad


def test_outputs_ragged_batches_partial_rotation_and_an_int64_new_lens(mm):
    matmuls, fake = mm
    dtype, R = torch.float16, 32
    g = torch.Generator().manual_seed(2502)
    qkv, q, kn, vn = _projection(g, dtype)
    before = qkv.clone()
    cos, sin = _tables(R)
    k_lens, new_lens = [34, 96], [2, 9]       # item 0: slots 1, 2 at 32, 33; item 1: clamped to 3, at 93, 94, 95
    k, v = (torch.zeros(B, HKV, SMAX, D, dtype=dtype) for _ in range(2))
    q_out = torch.zeros(B, T, HQ, D, dtype=dtype).transpose(1, 2)
    k_out = torch.zeros(B, HKV, T, D, dtype=dtype)
    nl = torch.tensor(new_lens, dtype=torch.int64)
    got = matmuls.rope_kv_cache_append(q, kn, vn, cos, sin, k, v, torch.tensor(k_lens), rotary_dim=R, new_lens=nl, q_out=q_out, k_out=k_out)
    rec = _record(fake, "rope_kv_append")
    assert got is q_out and rec["q_out_ptr"] == q_out.data_ptr() and rec["q_out_stride"] == tuple(q_out.stride())
    assert rec["k_out"]["k_out_ptr"] == k_out.data_ptr() and rec["rotary_dim"] == R
    assert rec["new_lens"]["new_lens_dtype"] == torch.int32 and rec["new_lens"]["new_lens_ptr"] != nl.data_ptr()     # narrowed
    pos, token = ref.token_slots(B, T, k_lens, PMAX, new_lens)
    assert token.tolist() == [[False, True, True], [True, True, True]]
    want_q, want_k = (ref.rotated(_i16(x), dtype, cos, sin, pos, token, R, False) for x in (q, kn))
    assert torch.equal(_i16(q_out), want_q) and torch.equal(_i16(k_out), want_k)
    assert torch.equal(q_out[1, :, :, R:], q[1, :, :, R:]) and not torch.equal(q_out[1, :, :, :R], q[1, :, :, :R])     # the tail: a copy
    assert (q_out[0, :, 0] == 0).all() and (k_out[0, :, 0] == 0).all() and (k[0, :, 31] == 0).all() and (k[0, :, 32] != 0).any()
    assert torch.equal(_i16(k[0, :, 32:34]), want_k[0, :, 1:]) and torch.equal(v[1, :, 93:96], vn[1])
    assert torch.equal(qkv, before)                                              # the source is only read …
    # … unless the outputs are the sources: in place
    fake.calls.clear()
    nl32 = torch.tensor(new_lens, dtype=torch.int32)
    got = matmuls.rope_kv_cache_append(q, kn, vn, cos, sin, k, v, torch.tensor(k_lens), rotary_dim=R, new_lens=nl32, q_out=q, k_out=kn)
    rec = _record(fake, "rope_kv_append")
    assert got is q and rec["q_out_ptr"] == q.data_ptr() and rec["k_out"]["k_out_ptr"] == kn.data_ptr()
    assert rec["new_lens"]["new_lens_ptr"] == nl32.data_ptr()                     # int32: as it is
    assert torch.equal(_i16(q), want_q) and torch.equal(_i16(kn), want_k) and torch.equal(vn, before[:, :, HQ + HKV:].transpose(1, 2))


def test_the_rule_on_a_paged_fp8_cache_the_table_and_the_scales(mm):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(2503)
    dtype = torch.float16
    _, q, kn, vn = _projection(g, dtype)
    cos, sin = _tables(pmax=95)                # position 95 has no table row: that slot holds no token
    table = torch.tensor([[7, 3, -1, 19, 0, 20], [5, 9, 11, 2, 4, 8]], dtype=torch.int32)      # −1 and P = 20: out of the pool
    ks, vs = torch.tensor([0.3, 3.0]), torch.tensor(2.0 ** -7)
    k_lens = [34, 96]      # item 0: pos 31 (page 1 = pool 3), 32, 33 (logical page 2 = −1: dropped); item 1: 93, 94 in pool 8, 95 no token
    pos, token = ref.token_slots(B, T, k_lens, 95)
    assert token.tolist() == [[True, True, True], [True, True, False]]
    want_q, k_rot = (ref.rotated(_i16(x), dtype, cos, sin, pos, token, D, True) for x in (q, kn))
    for tt, scales in ((table, dict(k_scale=ks, v_scale=vs)), (table.long(), dict(v_scale=0.37))):
        kp, vp = (torch.full((P, HKV, PAGE, D), 0x7F, dtype=torch.uint8).view(F8) for _ in range(2))
        fake.calls.clear()
        out = matmuls.rope_kv_cache_append_paged(q, kn, vn, cos, sin, kp, vp, tt, torch.tensor(k_lens), interleaved=True, **scales)
        rec = _record(fake, "rope_kv_append_paged")
        assert rec["k_ptr"] == kp.data_ptr() and rec["v_ptr"] == vp.data_ptr() and rec["k_dtype"] == F8
        assert rec["q_ptr"] == q.data_ptr() and rec["k_new_stride"] == tuple(kn.stride()) and rec["interleaved"] is True
        assert rec["table_dtype"] == torch.int32 and (rec["table_ptr"] == tt.data_ptr()) == (tt.dtype == torch.int32)
        if "k_scale" in scales:
            assert rec["k_scale"]["ptr"] == ks.data_ptr() and rec["v_scale"]["ptr"] == vs.data_ptr()   # the caller's tensors themselves
        else:
            assert rec["k_scale"] is None and rec["v_scale"]["shape"] == ()
        assert torch.equal(_i16(out), want_q) and (out[1, :, 2] == 0).all() and (out[0, :, 2] != 0).any()   # dropped k / v: q still rotated
        want_k, want_v = (torch.full((P, HKV, PAGE, D), 0x7F, dtype=torch.uint8) for _ in range(2))
        k8 = matmuls.kv_to_fp8(k_rot.view(dtype), scales.get("k_scale", 1.0))[0].view(torch.uint8)
        v8 = matmuls.kv_to_fp8(vn, scales.get("v_scale", 1.0))[0].view(torch.uint8)
        written = 0
        for b in range(B):
            for t in range(T):
                p = int(pos[b, t])
                e = int(table[b, p // PAGE])
                if token[b, t] and 0 <= e < P:
                    want_k[e, :, p % PAGE], want_v[e, :, p % PAGE] = k8[b, :, t], v8[b, :, t]
                    written += 1
        assert written == 3                                          # 31 and 93, 94
        assert torch.equal(kp.view(torch.uint8), want_k) and torch.equal(vp.view(torch.uint8), want_v)


def test_an_empty_cache_still_rotates_q_and_an_empty_batch_does_not_reach_the_bindings(mm):
    matmuls, fake = mm
    dtype = torch.bfloat16
    _, q, kn, vn = _projection(torch.Generator().manual_seed(2504), dtype)
    cos, sin = _tables()
    empty = torch.zeros(B, HKV, 0, D, dtype=dtype)
    out = matmuls.rope_kv_cache_append(q, kn, vn, cos, sin, empty, empty, torch.tensor([10, 20]))       # Smax = 0: k, v dropped
    pos, token = ref.token_slots(B, T, [10, 20], PMAX)
    assert torch.equal(_i16(out), ref.rotated(_i16(q), dtype, cos, sin, pos, token, D, False)) and len(fake.calls) == 1
    pool = torch.zeros(P, HKV, PAGE, D, dtype=dtype)
    out = matmuls.rope_kv_cache_append_paged(q, kn, vn, cos, sin, pool, pool, torch.zeros(B, 0, dtype=torch.int64), torch.tensor([10, 20]))
    assert torch.equal(_i16(out), ref.rotated(_i16(q), dtype, cos, sin, pos, token, D, False)) and not pool.any()
    out = matmuls.rope_kv_cache_append(q, kn, vn, cos[:0], sin[:0], pool[:B], pool[:B], torch.tensor([10, 20]))     # no table rows: no tokens
    assert not out.any() and not pool.any()
    fake.calls.clear()
    none = torch.zeros(0, HKV, T, D, dtype=dtype)
    out = matmuls.rope_kv_cache_append(torch.zeros(0, HQ, T, D, dtype=dtype), none, none, cos, sin, torch.zeros(0, HKV, SMAX, D, dtype=dtype),
                                       torch.zeros(0, HKV, SMAX, D, dtype=dtype), torch.zeros(0, dtype=torch.int32))
    assert out.shape == (0, HQ, T, D) and fake.calls == []
