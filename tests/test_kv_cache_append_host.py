"""matmuls.kv_cache_append and kv_cache_append_paged without a GPU: every refusal with its exception type,
before the device; what reaches the bindings through the stand-in tests/fake_custom_mm_kv_append.py — source, cache, an int32
table and tensor scales uncopied, int64 lengths and tables narrowed, a float scale as a 0-d tensor, empty calls not at all —;
the rule `pos = k_lens − T + t, written iff it fits` on CPU tensors; the two `takes`; and the six entries of the C ABI:
declared, exported, MI_EINVAL before any HIP call."""
import ctypes
import importlib
import re
import sys
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "mi_spmm.h"
OK, EINVAL, ERANGE = 0, -1, -2
FAKE = 0x1000  # a non-null, 16-byte aligned address that is never dereferenced: every call below returns before the device
F8 = torch.float8_e4m3fn
ENTRIES = ("mi_kv_append_b16", "mi_kv_append_paged_b16", "mi_kv_append_fp8_bf16", "mi_kv_append_fp8_f16",
           "mi_kv_append_paged_fp8_bf16", "mi_kv_append_paged_fp8_f16")


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
        fn.argtypes = 4 * [i32] + table + [i32] + 4 * [vp, i64, i64, i64] + [vp, i32] + scales + [vp]
        fn.restype = ctypes.c_int
    return lib


def test_header_declares_and_library_exports_the_append_entries(lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert int(re.search(r"MI_ERANGE\s*=\s*(-?\d+)", HEADER.read_text()).group(1)) == ERANGE
    for name in ENTRIES:
        assert hasattr(lib, name), name
        args = re.search(rf"\b{name}\s*\((.*?)\)", text, flags=re.S).group(1)
        names = [a.split()[-1].lstrip("*") for a in args.split(",")]
        assert names[:4] == ["items", "heads", "T", "Smax"] and names[-1] == "stream"
        assert ("block_table" in names) == ("paged" in name) and ("k_scale" in names) == ("fp8" in name)
        assert len(re.findall(r"const uint16_t\s*\*", args)) == 2                   # the source: 2-byte patterns, read only
        assert len(re.findall(r"(?<!const )uint8_t\s*\*", args)) == (2 if "fp8" in name else 0)


DEFAULTS = dict(items=8, heads=2, T=3, Smax=512, table=FAKE, table_ld=32, pages=100, page=16, D=64, k_new=FAKE, ldkn=None, headKn=None,
                batchKn=None, k=FAKE, ldk=None, headK=None, outerK=None, k_lens=FAKE, lens_count=4, k_scale=FAKE, k_count=2,
                v_scale=None, v_count=1)


def append(lib, name, **kw):
    a = {**DEFAULTS, **kw}
    D, T, heads = a["D"], a["T"], a["heads"]
    rows = a["page"] if "paged" in name else a["Smax"]
    ldkn, ldk = (D if a[n] is None else a[n] for n in ("ldkn", "ldk"))
    headKn, batchKn = (T * D if a["headKn"] is None else a["headKn"]), (heads * T * D if a["batchKn"] is None else a["batchKn"])
    headK, outerK = (rows * D if a["headK"] is None else a["headK"]), (heads * rows * D if a["outerK"] is None else a["outerK"])
    table = (a["table"], a["table_ld"], a["pages"], a["page"]) if "paged" in name else ()
    scales = (a["k_scale"], a["k_count"], a["v_scale"], a["v_count"]) if "fp8" in name else ()
    return getattr(lib, name)(a["items"], heads, T, a["Smax"], *table, D, a["k_new"], ldkn, headKn, batchKn, FAKE, D, T * D,
                              heads * T * D, a["k"], ldk, headK, outerK, FAKE, D, rows * D, heads * rows * D, a["k_lens"],
                              a["lens_count"], *scales, None)


@pytest.mark.parametrize("name", ENTRIES)
def test_append_entries_validate_before_any_hip_call(lib, name):
    unit = 16 if "fp8" in name else 8
    for kw in ({"D": 48}, {"D": 0}, {"D": 256}, {"items": -1}, {"items": 65536}, {"T": -1}, {"Smax": -16}, {"heads": 3}, {"heads": -2},
               {"lens_count": 3}, {"lens_count": 0}, {"k_lens": None}, {"k_lens": FAKE + 2},
               {"k_new": None}, {"k_new": FAKE + 8}, {"ldkn": 60}, {"ldkn": -8}, {"headKn": 100}, {"batchKn": 4},   # the source: 8 elements
               {"k": None}, {"k": FAKE + 8}, {"ldk": 48}, {"ldk": 64 + unit // 2}, {"headK": unit // 2}, {"outerK": 512 * 64 * 2 + 4},
               {"outerK": -unit}):
        assert append(lib, name, **kw) == EINVAL, kw
    if "paged" in name:
        for kw in ({"page": 8}, {"page": 24}, {"page": 0}, {"page": 1024}, {"pages": -1}, {"table": None}, {"table": FAKE + 2},
                   {"table_ld": 31}):
            assert append(lib, name, **kw) == EINVAL, kw
        assert append(lib, name, pages=0, k=None) == OK          # an empty pool: every token dropped, nothing launched
    if "fp8" in name:
        for kw in ({"k_count": 0}, {"k_count": 3}, {"k_count": 8}, {"v_count": 4}, {"k_count": -1}, {"k_scale": FAKE + 2},
                   {"v_scale": FAKE + 1}):
            assert append(lib, name, **kw) == EINVAL, kw
    assert append(lib, name, items=0, k_new=None) == OK and append(lib, name, T=0, k=None) == OK     # nothing to write
    assert append(lib, name, items=0, D=48) == EINVAL                                                  # … but checked first
    assert append(lib, name, Smax=0, k=None, table_ld=0) == OK                                         # nothing fits
    assert append(lib, name, items=65534, T=2 ** 31 - 1, lens_count=1) == ERANGE                       # items · T · D/8 ≥ 2³¹


# ---- matmuls on the real extension: refusals before the device -------------------------------------------------------

@pytest.fixture()
def real(built):
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import matmuls
    yield matmuls
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)


B, HKV, T, D, SMAX, PAGE, P, W = 2, 2, 3, 64, 96, 16, 20, 6


def _forms(m, dtype=torch.bfloat16):
    """(prefix, call(k_new, v_new, k, v, **kw), cache shape, names, outer) of the two calls on B = 2, Hkv = 2, T = 3, D = 64."""
    lens = torch.tensor([50, 96])
    table = torch.arange(B * W, dtype=torch.int32).reshape(B, W) % P
    flat = lambda kn, vn, k, v, lens=lens, **kw: m.kv_cache_append(kn, vn, k, v, lens, **kw)  # noqa: E731
    paged = lambda kn, vn, k, v, lens=lens, table=table, **kw: m.kv_cache_append_paged(kn, vn, k, v, table, lens, **kw)  # noqa: E731
    return (("kv_cache_append: ", flat, (B, HKV, SMAX, D), "k", "v", "batch"),
            ("kv_cache_append_paged: ", paged, (P, HKV, PAGE, D), "k_pages", "v_pages", "page"))


def test_every_refusal_comes_before_the_device_with_its_type(real):
    for what, f, shape, kn, vn, outer in _forms(real):
        n0, H, S, _ = shape
        new = torch.zeros(B, HKV, T, D, dtype=torch.bfloat16)
        c16, c8 = torch.zeros(shape, dtype=torch.bfloat16), torch.zeros(shape, dtype=torch.uint8).view(F8)
        # what the source is
        with pytest.raises(ValueError, match=what + "k_new must be bfloat16 or float16, got torch.float32"):
            f(new.float(), new, c16, c16)
        with pytest.raises(ValueError, match=what + "v_new must be a dense tensor"):
            f(new, None, c16, c16)
        with pytest.raises(RuntimeError, match=what + "k_new is torch.bfloat16 but v_new is torch.float16"):
            f(new, new.half(), c16, c16)
        # what the cache is: the source's dtype, or e4m3fn and no other 8-bit type
        with pytest.raises(ValueError, match=what + f"{kn} must be a dense tensor"):
            f(new, new, torch.ones(4, 4).to_sparse_csr(), c16)
        with pytest.raises(ValueError, match=what + f"{kn} must have k_new's dtype or be float8_e4m3fn, got torch.float32"):
            f(new, new, c16.float(), c16.float())
        with pytest.raises(RuntimeError, match=what + f"k_new is torch.bfloat16 but {kn} is torch.float16"):
            f(new, new, c16.half(), c16.half())
        with pytest.raises(RuntimeError, match=what + f"k_new is torch.bfloat16 but {vn} is torch.float16"):
            f(new, new, c16, c16.half())
        for bad in (torch.float8_e4m3fnuz, torch.float8_e5m2, torch.uint8):
            other = c8.view(bad)
            with pytest.raises(ValueError, match=what + f"{kn} must be float8_e4m3fn, got {bad}: the OCP e4m3fn encoding is what is read"):
                f(new, new, other, other)
            with pytest.raises(RuntimeError, match=what + f"{kn} is torch.float8_e4m3fn but {vn} is {bad}"):
                f(new, new, c8, other)
        with pytest.raises(RuntimeError, match=what + f"{kn} is torch.bfloat16 but {vn} is torch.float8_e4m3fn"):
            f(new, new, c16, c8)
        # a scale with a 2-byte cache
        for name in ("k_scale", "v_scale"):
            with pytest.raises(ValueError, match=what + f"{name} goes with a float8_e4m3fn cache only"):
                f(new, new, c16, c16, **{name: 0.5})
            with pytest.raises(ValueError, match=what + f"{name} goes with a float8_e4m3fn cache only"):
                f(new, new, c16, c16, **{name: torch.ones(2)})
        # shapes
        with pytest.raises(ValueError, match=what + "k_new and v_new must be .B, Hkv, T, D."):
            f(new[0], new[0], c16, c16)
        with pytest.raises(ValueError, match=what + "v_new must have k_new's shape"):
            f(new, new[:, :, :2], c16, c16)
        with pytest.raises(ValueError, match=what + "head size D must be 32, 64, 96 or 128, got 48"):
            f(new[..., :48], new[..., :48], c16[..., :48], c16[..., :48])
        with pytest.raises(ValueError, match=what + "k_new must hold T >= 1 new tokens"):
            f(new[:, :, :0], new[:, :, :0], c16, c16)
        with pytest.raises(ValueError, match=what + f"k_new of shape .* needs {kn}"):
            f(new, new, c16[:, :1], c16[:, :1])
        with pytest.raises(ValueError, match=what + f"{vn} must be a dense tensor with {kn}'s shape"):
            f(new, new, c16, torch.zeros(n0, H, 2 * S, D, dtype=torch.bfloat16))
        big = torch.zeros(1, 1, 1, D, dtype=torch.bfloat16).expand(32768, 2, 1, D)
        with pytest.raises(ValueError, match=what + "B·Hkv = 65536 must be at most 65535"):
            if outer == "batch":
                huge = torch.zeros(1, 1, 16, D, dtype=torch.bfloat16).expand(32768, 2, 16, D)
                f(big, big, huge, huge, lens=torch.tensor(1))
            else:
                f(big, big, c16, c16, lens=torch.tensor(1), table=torch.zeros(32768, 1, dtype=torch.int32))
        # k_lens
        with pytest.raises(ValueError, match=what + "k_lens is required and must be a dense tensor"):
            f(new, new, c16, c16, lens=None)
        with pytest.raises(ValueError, match=what + "k_lens must be an int32 or int64 tensor, got torch.float32"):
            f(new, new, c16, c16, lens=torch.tensor([1.0, 2.0]))
        with pytest.raises(ValueError, match=what + r"k_lens must have shape \(2,\)"):
            f(new, new, c16, c16, lens=torch.tensor([1, 2, 3]))
        # the source's strides, named: a fused projection with an odd head size does not fit, nor a shifted pointer
        wide = torch.zeros(B, HKV, T, 2 * D, dtype=torch.bfloat16)
        with pytest.raises(ValueError, match=what + "k_new must have a last stride of 1, got 2"):
            f(wide[..., ::2], new, c16, c16)
        with pytest.raises(ValueError, match=what + f"v_new's token stride must be a multiple of 8 elements, got {D + 4}"):
            f(new, torch.zeros(B, HKV, T, D + 4, dtype=torch.bfloat16)[..., :D], c16, c16)
        odd_head = torch.zeros(B * HKV * (T * D + 4), dtype=torch.bfloat16).as_strided((B, HKV, T, D), (HKV * (T * D + 4), T * D + 4, D, 1))
        with pytest.raises(ValueError, match=what + f"k_new's head stride must be a multiple of 8 elements, got {T * D + 4}"):
            f(odd_head, new, c16, c16)
        odd_batch = torch.zeros(B * (HKV * T * D + 4), dtype=torch.bfloat16).as_strided((B, HKV, T, D), (HKV * T * D + 4, T * D, D, 1))
        with pytest.raises(ValueError, match=what + f"v_new's batch stride must be a multiple of 8 elements, got {HKV * T * D + 4}"):
            f(new, odd_batch, c16, c16)
        buf = torch.zeros(new.numel() + 16, dtype=torch.bfloat16)
        shifted = buf[(16 - buf.data_ptr() % 16) // 2 + 4:][:new.numel()].reshape(new.shape)
        assert shifted.data_ptr() % 16 == 8
        with pytest.raises(ValueError, match=what + "k_new's data pointer must be 16-byte aligned"):
            f(shifted, new, c16, c16)
        # the cache's strides: _check_cache_strides, with 8 for a 2-byte cache and 16 for fp8
        with pytest.raises(ValueError, match=what + f"{kn}'s row stride must be a multiple of 8 elements and at least D = 64, got 68"):
            f(new, new, torch.zeros(n0, H, S, D + 4, dtype=torch.bfloat16)[..., :D], c16)
        with pytest.raises(ValueError, match=what + f"{vn}'s row stride must be a multiple of 16 elements and at least D = 64, got 72"):
            f(new, new, c8, torch.zeros(n0, H, S, D + 8, dtype=torch.uint8).view(F8)[..., :D])
        odd_outer = torch.zeros(n0 * (H * S * D + 8), dtype=torch.uint8).view(F8).as_strided(shape, (H * S * D + 8, S * D, D, 1))
        with pytest.raises(ValueError, match=what + f"{kn}'s {outer} stride must be a multiple of 16 elements, got {H * S * D + 8}"):
            f(new, new, odd_outer, c8)
        # the scales of an fp8 cache
        for name in ("k_scale", "v_scale"):
            with pytest.raises(ValueError, match=what + f"{name} must be a float32 tensor, got torch.float64"):
                f(new, new, c8, c8, **{name: torch.ones(2, dtype=torch.float64)})
            with pytest.raises(ValueError, match=what + rf"{name} must have shape \(\), \(1,\) or \(2,\)"):
                f(new, new, c8, c8, **{name: torch.ones(3)})
            with pytest.raises(ValueError, match=what + f"{name} must be None, a float or a dense float32 tensor"):
                f(new, new, c8, c8, **{name: "1"})
            with pytest.raises(RuntimeError, match=what + f"{name} is on meta but k_new is on cpu"):
                f(new, new, c8, c8, **{name: torch.ones(2, device="meta")})
        with pytest.raises(TypeError):  # the scales are keyword only
            f(new, new, c8, c8, torch.tensor([50, 96]), 0.5) if outer == "batch" else real.kv_cache_append_paged(
                new, new, c8, c8, torch.zeros(B, W, dtype=torch.int32), torch.tensor([50, 96]), 0.5)
        # host tensors: the last check
        with pytest.raises(RuntimeError, match=what + rf"k_new, v_new, {kn}, {vn}, .*k_lens must be device \(HIP\) tensors"):
            f(new, new, c16, c16)
        with pytest.raises(RuntimeError, match=what + r"k_new, .*k_lens, k_scale must be device \(HIP\) tensors"):
            f(new.half(), new.half(), c8, c8, k_scale=torch.ones(2), v_scale=2.0)


def test_the_paged_call_refuses_bad_pages_and_tables(real):
    what = "kv_cache_append_paged: "
    new = torch.zeros(B, HKV, T, D, dtype=torch.float16)
    pool, lens = torch.zeros(P, HKV, PAGE, D, dtype=torch.float16), torch.tensor([5, 6])
    table = torch.zeros(B, W, dtype=torch.int32)
    for page in (8, 24):
        bad = torch.zeros(P, HKV, page, D, dtype=torch.float16)
        with pytest.raises(ValueError, match=what + f"the pool's pages must hold a power of two >= 16 rows, got page = {page}"):
            real.kv_cache_append_paged(new, new, bad, bad, table, lens)
    with pytest.raises(ValueError, match=what + "block_table is required and must be a dense tensor"):
        real.kv_cache_append_paged(new, new, pool, pool, None, lens)
    with pytest.raises(ValueError, match=what + "block_table must be an int32 or int64 tensor, got torch.int16"):
        real.kv_cache_append_paged(new, new, pool, pool, table.to(torch.int16), lens)
    with pytest.raises(ValueError, match=what + r"block_table must have shape \(2, W\)"):
        real.kv_cache_append_paged(new, new, pool, pool, table[:1], lens)
    with pytest.raises(ValueError, match=what + "block_table must have a last stride of 1, got 2"):
        real.kv_cache_append_paged(new, new, pool, pool, torch.zeros(B, 2 * W, dtype=torch.int32)[:, ::2], lens)
    with pytest.raises(ValueError, match=what + "block_table's row stride must be at least W = 6, got 0"):
        real.kv_cache_append_paged(new, new, pool, pool, table[:1].expand(B, W), lens)
    with pytest.raises(RuntimeError, match=what + r"k_new, v_new, k_pages, v_pages, block_table, k_lens must be device \(HIP\) tensors"):
        real.kv_cache_append_paged(new, new, pool, pool, table, lens)


def test_custom_mm_bindings_refuse_host_tensors_and_mismatched_operands(built):
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import custom_mm
    new, lens = torch.zeros(1, 1, 1, 32, dtype=torch.bfloat16), torch.tensor([5], dtype=torch.int32)
    k16, pool, table = torch.zeros(1, 1, 64, 32, dtype=torch.bfloat16), torch.zeros(5, 1, 16, 32, dtype=torch.bfloat16), torch.zeros(1, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.kv_append(new, new, k16, k16, lens, None, None)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.kv_append_paged(new, new, pool, pool, table, lens, None, None)
    with pytest.raises(RuntimeError, match="k_new is BFloat16 but v_new is Half"):
        custom_mm.kv_append(new, new.half(), k16, k16, lens, None, None)
    with pytest.raises(TypeError):  # positional only
        custom_mm.kv_append(new, new, k16, k16, lens, k_scale=None, v_scale=None)


def test_takes_are_functions_of_their_arguments_alone(real):
    takes, paged = real.kv_cache_append_takes, real.kv_cache_append_paged_takes
    for dtype in (torch.bfloat16, torch.float16):
        for D_ in (32, 64, 96, 128):
            assert takes(dtype, dtype, D_) and takes(dtype, F8, D_)
            assert all(paged(dtype, c, D_, page) for c in (dtype, F8) for page in (16, 32, 256, 1024))
    assert not takes(torch.bfloat16, torch.float16, 64) and not takes(torch.float16, torch.bfloat16, 64)
    assert not takes(torch.float32, torch.float32, 64) and not takes(F8, F8, 64) and not takes(torch.float32, F8, 64)
    for bad in (torch.float8_e4m3fnuz, torch.float8_e5m2, torch.uint8, torch.float32):
        assert not takes(torch.bfloat16, bad, 64)
    assert not takes(torch.bfloat16, torch.bfloat16, 48) and not takes(torch.bfloat16, F8, 256) and not takes(torch.bfloat16, F8, True)
    assert not paged(torch.bfloat16, F8, 64, 8) and not paged(torch.bfloat16, F8, 64, 24) and not paged(torch.bfloat16, F8, 48, 16)
    assert not paged(torch.float16, torch.bfloat16, 64, 16) and not paged(torch.float16, F8, 64, True)


# ---- wiring on CPU tensors through the stand-in ----------------------------------------------------------------------------

@pytest.fixture()
def mm(oracle_mod):
    """(matmuls bound to the stand-in, the stand-in)."""
    import fake_custom_mm_kv_append as fake
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
    """k_new, v_new [B, Hkv, T, D] as slices of one fused projection [B, T, Hq + 2·Hkv, D] through .transpose(1, 2)."""
    Hq = 4
    qkv = torch.randn(B, T, Hq + 2 * HKV, D, generator=g).to(dtype)
    return qkv[:, :, Hq:Hq + HKV].transpose(1, 2), qkv[:, :, Hq + HKV:].transpose(1, 2)


def _expected_rows(k_lens, smax):
    """[(b, t, pos)] of the tokens that are written."""
    return [(b, t, n - T + t) for b, n in enumerate(k_lens) for t in range(T) if 0 <= n - T + t < smax]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_the_rule_on_a_flat_cache_and_nothing_is_copied(mm, dtype):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(2301)
    kn, vn = _projection(g, dtype)
    assert not kn.is_contiguous() and kn.stride() == (T * 8 * D, D, 8 * D, 1)
    base = torch.randn(2, B, SMAX, HKV, D, generator=g).to(dtype)            # a [B, Smax, Hkv, D].transpose(1, 2) cache
    for k_lens, lens_dtype in (([50, 96], torch.int32), ([2, 98], torch.int64), ([0, 1], torch.int32)):
        k, v = base[0].clone().transpose(1, 2), base[1].clone().transpose(1, 2)
        lens = torch.tensor(k_lens, dtype=lens_dtype)
        fake.calls.clear()
        assert matmuls.kv_cache_append(kn, vn, k, v, lens) is None
        rec = _record(fake, "kv_append")
        for name, t in (("k_new", kn), ("v_new", vn), ("k", k), ("v", v)):          # the caller's memory, through its strides
            assert rec[f"{name}_ptr"] == t.data_ptr() and rec[f"{name}_stride"] == tuple(t.stride()) and rec[f"{name}_dtype"] == dtype
        assert rec["k_lens_dtype"] == torch.int32 and rec["k_lens_shape"] == (B,)     # narrowed on the way
        assert (rec["k_lens_ptr"] == lens.data_ptr()) == (lens_dtype == torch.int32)
        assert rec["k_scale"] is None and rec["v_scale"] is None
        want_k, want_v = base[0].clone().transpose(1, 2), base[1].clone().transpose(1, 2)
        rows = _expected_rows(k_lens, SMAX)
        for b, t, pos in rows:
            want_k[b, :, pos], want_v[b, :, pos] = kn[b, :, t], vn[b, :, t]
        assert torch.equal(k.view(torch.int16), want_k.view(torch.int16)) and torch.equal(v.view(torch.int16), want_v.view(torch.int16))
        assert len(rows) == {50: 6, 2: 3, 0: 1}[k_lens[0]]      # [2, 98]: two dropped in front, two behind; [0, 1]: one written
    # a 0-d length serves every item
    k, v = base[0].clone().transpose(1, 2), base[1].clone().transpose(1, 2)
    fake.calls.clear()
    matmuls.kv_cache_append(kn, vn, k, v, torch.tensor(7))
    assert _record(fake, "kv_append")["k_lens_shape"] == (1,)
    assert torch.equal(k[:, :, 4:7], kn) and torch.equal(k[:, :, :4], base[0].transpose(1, 2)[:, :, :4])
    # no autograd: operands that require grad are detached, nothing is returned
    kr = kn.clone().float().requires_grad_(True)
    assert matmuls.kv_cache_append(kr.to(dtype), vn, k, v, torch.tensor(7)) is None and not k.requires_grad


def test_the_rule_on_a_paged_fp8_cache_the_table_and_the_scales(mm):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(2302)
    dtype = torch.float16
    kn, vn = _projection(g, dtype)
    table = torch.tensor([[7, 3, -1, 19, 0, 20], [5, 9, 11, 2, 4, 8]], dtype=torch.int32)      # −1 and P = 20: out of the pool
    wider = torch.full((B, W + 4), -1, dtype=torch.int32)
    wider[:, :W] = table
    ks, vs = torch.tensor([0.3, 3.0]), torch.tensor(2.0 ** -7)
    k_lens = [34, 96]      # item 0: pos 31 (page 1 = pool 3), 32, 33 (logical page 2 = −1: dropped); item 1: 93, 94, 95 in page 5 = pool 8
    for tt, scales in ((table, dict(k_scale=ks, v_scale=vs)), (wider[:, :W], dict(k_scale=ks)), (table.long(), dict(v_scale=0.37))):
        kp, vp = (torch.full((P, HKV, PAGE, D), 0x7F, dtype=torch.uint8).view(F8) for _ in range(2))
        fake.calls.clear()
        assert matmuls.kv_cache_append_paged(kn, vn, kp, vp, tt, torch.tensor(k_lens), **scales) is None
        rec = _record(fake, "kv_append_paged")
        assert rec["k_ptr"] == kp.data_ptr() and rec["v_ptr"] == vp.data_ptr() and rec["k_dtype"] == F8
        assert rec["k_new_ptr"] == kn.data_ptr() and rec["k_new_stride"] == tuple(kn.stride())
        assert rec["table_dtype"] == torch.int32 and rec["table_shape"] == (B, W)
        assert (rec["table_ptr"] == tt.data_ptr()) == (tt.dtype == torch.int32)             # int32: as it is; int64: narrowed
        assert rec["table_stride"] == (tuple(tt.stride()) if tt.dtype == torch.int32 else (W, 1))
        assert rec["k_lens_dtype"] == torch.int32 and rec["k_lens_ptr"] != 0
        if "k_scale" in scales:
            assert rec["k_scale"]["ptr"] == ks.data_ptr() and rec["k_scale"]["shape"] == (2,)   # the caller's tensor itself
        else:
            assert rec["k_scale"] is None
        if scales.get("v_scale") is vs:
            assert rec["v_scale"]["ptr"] == vs.data_ptr() and rec["v_scale"]["shape"] == ()
        elif "v_scale" in scales:   # a float: a 0-d float32 tensor of that value
            assert rec["v_scale"]["shape"] == () and rec["v_scale"]["value"].dtype == torch.float32
            assert rec["v_scale"]["value"].item() == torch.tensor(0.37, dtype=torch.float32).item()
        else:
            assert rec["v_scale"] is None
        want_k, want_v = (torch.full((P, HKV, PAGE, D), 0x7F, dtype=torch.uint8) for _ in range(2))
        k8 = matmuls.kv_to_fp8(kn, scales.get("k_scale", 1.0))[0].view(torch.uint8)   # (None there: a scale from amax; here: 1)
        v8 = matmuls.kv_to_fp8(vn, scales.get("v_scale", 1.0))[0].view(torch.uint8)
        for b, t, pos in _expected_rows(k_lens, W * PAGE):
            e = int(table[b, pos // PAGE])
            if 0 <= e < P:
                want_k[e, :, pos % PAGE], want_v[e, :, pos % PAGE] = k8[b, :, t], v8[b, :, t]
        assert torch.equal(kp.view(torch.uint8), want_k) and torch.equal(vp.view(torch.uint8), want_v)
        assert (want_k != 0x7F).any(-1).sum() == 4 * HKV            # 31 and 93, 94, 95: 32 and 33 have no page
    # a flat fp8 cache with a row stride of D + 16: the gaps keep their bytes
    k, v = (torch.full((B, HKV, SMAX, D + 16), 0x7F, dtype=torch.uint8).view(F8)[..., :D] for _ in range(2))
    fake.calls.clear()
    matmuls.kv_cache_append(kn, vn, k, v, torch.tensor([3, 96]), k_scale=ks, v_scale=vs)
    rec = _record(fake, "kv_append")
    assert rec["k_stride"] == tuple(k.stride()) and rec["k_stride"][2] == D + 16 and rec["k_ptr"] == k.data_ptr()
    assert torch.equal(k.view(torch.uint8)[0, :, :3], matmuls.kv_to_fp8(kn, ks)[0].view(torch.uint8)[0])
    assert torch.equal(v.view(torch.uint8)[1, :, 93:], matmuls.kv_to_fp8(vn, vs)[0].view(torch.uint8)[1])


def test_empty_calls_do_not_reach_the_bindings(mm):
    matmuls, fake = mm
    new = torch.zeros(0, HKV, T, D, dtype=torch.bfloat16)
    assert matmuls.kv_cache_append(new, new, torch.zeros(0, HKV, SMAX, D, dtype=torch.bfloat16), torch.zeros(0, HKV, SMAX, D, dtype=torch.bfloat16),
                                   torch.zeros(0, dtype=torch.int32)) is None
    new = torch.zeros(B, HKV, T, D, dtype=torch.bfloat16)
    empty = torch.zeros(B, HKV, 0, D, dtype=torch.bfloat16)
    assert matmuls.kv_cache_append(new, new, empty, empty, torch.tensor([1, 2])) is None                    # Smax = 0: nothing fits
    pool = torch.zeros(0, HKV, PAGE, D, dtype=torch.uint8).view(F8)
    assert matmuls.kv_cache_append_paged(new, new, pool, pool, torch.zeros(B, W, dtype=torch.int32), torch.tensor([1, 2]), k_scale=2.0) is None
    pool = torch.zeros(P, HKV, PAGE, D, dtype=torch.bfloat16)
    assert matmuls.kv_cache_append_paged(new, new, pool, pool, torch.zeros(B, 0, dtype=torch.int64), torch.tensor([1, 2])) is None
    assert fake.calls == []
