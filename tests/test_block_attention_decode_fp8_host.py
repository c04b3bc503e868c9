"""matmuls.block_sparse_attention_decode_fp8 and its paged form without a GPU: every refusal of their
own with its exception type — the other 8-bit dtypes, a mixed cache, strides that are no multiples of 16, a misaligned
pointer, a scale of the wrong dtype, shape or device — and the shared ones; that the 2-byte calls still refuse an fp8
cache; what reaches the binding through the float64 stand-in tests/fake_custom_mm_block_attention_decode_fp8.py (the cache
and an int32 table uncopied, the scales as pointers or None); kv_to_fp8; the claim under the contract on bits, that every
finite e4m3fn code widens exactly to bfloat16 and to float16; and the four fp8 entries of the C ABI: declared, exported,
MI_EINVAL / MI_ENOMEM before any HIP call."""
import ctypes
import importlib
import re
import sys
from pathlib import Path

import pytest
import torch

from test_block_attention_decode_host import _dense_reference, _random_layout, _visible
from test_block_attention_decode_paged_host import _gathered, _paged

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "mi_spmm.h"
SUFFIXES = ("bf16", "f16")
OK, EINVAL, ENOMEM = 0, -1, -4
FAKE = 0x1000  # a non-null, 16-byte aligned address that is never dereferenced: every call below returns before the device
F8 = torch.float8_e4m3fn
NAN_CODE = 0x7F


def finite_codes():
    """The 254 finite e4m3fn codes as a uint8 tensor (0x7F and 0xFF are the NaNs)."""
    return torch.tensor([c for c in range(256) if c & 0x7F != NAN_CODE], dtype=torch.uint8)


def random_fp8(g, shape):
    """Random finite e4m3fn values of moderate size, built from bytes: no fp8 operator of torch is needed but the cast up."""
    codes = finite_codes()
    codes = codes[(codes & 0x7F) < 0x48]  # |x| < 4
    return codes[torch.randint(len(codes), shape, generator=g)].view(F8)


# ---- the claim under the contract ------------------------------------------------------------------------------------

def test_every_finite_code_widens_exactly_to_bfloat16_and_float16():
    codes = finite_codes()
    assert codes.numel() == 254
    # the value of a code from its fields alone: OCP e4m3fn, bias 7, subnormals at exponent field 0, no infinities
    c = codes.to(torch.int64)
    sign, e, m = 1 - 2 * (c >> 7), (c >> 3) & 0xF, c & 0x7
    want = torch.where(e == 0, m.double() / 8 * 2.0 ** -6, (1 + m.double() / 8) * 2.0 ** (e.double() - 7)) * sign
    x = codes.view(F8)
    assert torch.equal(x.to(torch.float32).double(), want)
    assert want.abs().max() == 448 and want.abs()[want != 0].min() == 2.0 ** -9
    for dtype in (torch.bfloat16, torch.float16):
        wide = x.to(dtype)
        assert torch.equal(wide.double(), want), dtype       # nothing is lost …
        assert torch.equal(wide.to(torch.float32).to(F8).view(torch.uint8), codes), dtype  # … and the way back is the code
    assert torch.signbit(x.to(torch.bfloat16)[codes == 0x80]).all()  # −0 keeps its sign
    nan = torch.tensor([0x7F, 0xFF], dtype=torch.uint8).view(F8)
    assert torch.isnan(nan.to(torch.float32)).all()


# ---- the C ABI -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(built):
    import torch  # noqa: F401  (torch's HIP runtime first, as in the product)
    lib = ctypes.CDLL(str(built / "libmi_spmm.so"))
    vp, i64, i32, f32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_size_t
    tail = [vp, i32, i32, i32, f32, vp, i32, vp, i32] + [vp, i64, i64, vp, vp, sz, vp]
    for s in SUFFIXES:
        fn = getattr(lib, f"mi_block_attention_decode_fp8_{s}")
        fn.argtypes = [vp, vp, i64] + 6 * [i32] + [vp, i64, i64] + 2 * [vp, i64, i64, i64] + tail
        fn.restype = ctypes.c_int
        fn = getattr(lib, f"mi_block_attention_decode_paged_fp8_{s}")
        fn.argtypes = [vp, vp, i64] + 5 * [i32] + [vp, i64, i32, i32] + [i32] + [vp, i64, i64] + 2 * [vp, i64, i64, i64] + tail
        fn.restype = ctypes.c_int
    lib.mi_block_attention_decode_workspace_bytes.argtypes = 6 * [i32]
    lib.mi_block_attention_decode_workspace_bytes.restype = sz
    return lib


def test_header_declares_and_library_exports_the_fp8_entries(lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for form in ("", "paged_"):
        for s in SUFFIXES:
            name = f"mi_block_attention_decode_{form}fp8_{s}"
            assert re.search(rf"\b{name}\s*\(", text), name
            assert hasattr(lib, name), name
            args = re.search(rf"{name}\s*\((.*?)\)", text, flags=re.S).group(1)
            parent = re.search(rf"mi_block_attention_decode_{form}{s}\s*\((.*?)\)", text, flags=re.S).group(1)
            names = [a.split()[-1].lstrip("*") for a in args.split(",")]
            parents = [a.split()[-1].lstrip("*") for a in parent.split(",")]
            at = names.index("k_scale")
            assert names[at:at + 4] == ["k_scale", "k_scale_count", "v_scale", "v_scale_count"] and names[at - 1] == "scale"
            assert names[:at] + names[at + 4:] == parents  # the parent's list with the scales after `scale`
            assert len(re.findall(r"const uint8_t\s*\*", args)) == 2 and "uint8_t" not in parent


DEFAULTS = dict(nnz=4, layouts=1, items=8, heads=2, T=1, Smax=512, table=FAKE, table_ld=32, pages=100, page=16, D=64, q=FAKE,
                ldq=None, k=FAKE, ldk=None, headK=16 * 64, outerK=2 * 16 * 64, k_lens=FAKE, lens_count=4, group=4, chunk=2,
                k_scale=FAKE, k_count=2, v_scale=None, v_count=1, out=FAKE, lse=FAKE, ws=FAKE, ws_bytes=1 << 30)


def decode(lib, form, s, **kw):
    a = {**DEFAULTS, **kw}
    D = a["D"]
    ldq, ldk = (D if a[n] is None else a[n] for n in ("ldq", "ldk"))
    table = (a["table"], a["table_ld"], a["pages"], a["page"]) if form == "paged_" else ()
    return getattr(lib, f"mi_block_attention_decode_{form}fp8_{s}")(
        FAKE, FAKE, a["nnz"], a["layouts"], a["items"], a["heads"], a["T"], a["Smax"], *table, D, a["q"], ldq, a["T"] * ldq,
        a["k"], ldk, a["headK"], a["outerK"], FAKE, D, 16 * D, 2 * 16 * D, a["k_lens"], a["lens_count"], a["group"], a["chunk"],
        1.0, a["k_scale"], a["k_count"], a["v_scale"], a["v_count"], a["out"], D, a["T"] * D, a["lse"], a["ws"], a["ws_bytes"], None)


@pytest.mark.parametrize("s", SUFFIXES)
@pytest.mark.parametrize("form", ["", "paged_"])
def test_fp8_entries_validate_before_any_hip_call(lib, form, s):
    for kw in ({"group": 0}, {"group": 17}, {"D": 48}, {"chunk": 0}, {"items": 65536}, {"T": 65536}, {"Smax": 500}, {"nnz": -1},
               {"heads": 3}, {"lens_count": 3}, {"k_lens": None}, {"q": None}, {"q": FAKE + 8}, {"out": FAKE + 2}, {"lse": None},
               {"ldq": 60}, {"ws": None},                                                 # what the parents refuse
               {"k": None}, {"k": FAKE + 8}, {"ldk": 60}, {"ldk": 72}, {"headK": 8}, {"headK": 1032}, {"outerK": 2056},  # 16, not 8
               {"k_count": 0}, {"k_count": 3}, {"k_count": 8}, {"v_count": 0}, {"v_count": 4}, {"k_count": -1},  # 1 or heads = 2
               {"k_scale": FAKE + 2}, {"v_scale": FAKE + 1}):
        assert decode(lib, form, s, **kw) == EINVAL, kw
    if form:
        for kw in ({"page": 8}, {"page": 24}, {"page": 0}, {"page": 1024}, {"pages": -1}, {"table": None}, {"table_ld": 31}):
            assert decode(lib, form, s, **kw) == EINVAL, kw
    need = lib.mi_block_attention_decode_workspace_bytes(8, 1, 4, 64, 512, 2)
    assert need > 0 and decode(lib, form, s, ws_bytes=need - 1) == ENOMEM
    for kw in ({"k_scale": None, "k_count": 1}, {"k_count": 1}, {"v_scale": FAKE, "v_count": 2}, {"ldk": 80}):  # accepted so far
        assert decode(lib, form, s, ws_bytes=need - 1, **kw) == ENOMEM, kw
    assert decode(lib, form, s, items=0, q=None) == OK and decode(lib, form, s, items=0, k_count=3) == EINVAL


# ---- matmuls on the real extension: refusals before the device -------------------------------------------------------

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


def _bytes(*shape):
    return torch.zeros(shape, dtype=torch.uint8)


def _calls(m):
    """(call, cache maker, name of k, name of v, name of the outer stride) of the two forms, on B = 2, Hkv = 2, Smax = 256, D = 64."""
    q, lay, lens = torch.rand(2, 8, 1, 64).bfloat16(), _full(4), torch.tensor([100, 256])
    table = torch.arange(32, dtype=torch.int32).reshape(2, 16) % 20
    flat = lambda k, v, **kw: m.block_sparse_attention_decode_fp8(q, k, v, lay, lens, **kw)  # noqa: E731
    paged = lambda k, v, **kw: m.block_sparse_attention_decode_paged_fp8(q, k, v, table, lay, lens, **kw)  # noqa: E731
    return (("block_sparse_attention_decode_fp8: ", flat, (2, 2, 256, 64), "k", "v", "batch"),
            ("block_sparse_attention_decode_paged_fp8: ", paged, (20, 2, 16, 64), "k_pages", "v_pages", "page"))


def test_every_refusal_of_the_fp8_calls_comes_before_the_device_with_its_type(real):
    for what, f, shape, kn, vn, outer in _calls(real):
        n0, H, S, D = shape
        good = _bytes(*shape).view(F8)
        # the other 8-bit types: ValueError that says which encoding is read
        for bad in (torch.float8_e4m3fnuz, torch.float8_e5m2, torch.uint8):
            other = _bytes(*shape) if bad == torch.uint8 else _bytes(*shape).view(bad)
            with pytest.raises(ValueError, match=what + f"{kn} must be float8_e4m3fn, got {bad}: the OCP e4m3fn encoding is what is read"):
                f(other, other)
            with pytest.raises(RuntimeError, match=what + f"{kn} is torch.float8_e4m3fn but {vn} is {bad}"):  # a mixed cache
                f(good, other)
        with pytest.raises(RuntimeError, match=what + f"{kn} is torch.bfloat16 but {vn} is torch.float8_e4m3fn"):
            f(good.to(torch.bfloat16), good)
        with pytest.raises(ValueError, match=what + f"{kn} must be float8_e4m3fn, got torch.bfloat16"):
            f(good.to(torch.bfloat16), good.to(torch.bfloat16))
        with pytest.raises(ValueError, match=what + f"{vn} must be a dense tensor"):
            f(good, _full(4))
        # strides: multiples of 16 elements, named
        with pytest.raises(ValueError, match=what + f"{kn} must have a last stride of 1, got 2"):
            f(_bytes(n0, H, S, 2 * D).view(F8)[..., ::2], good)
        with pytest.raises(ValueError, match=what + f"{vn}'s row stride must be a multiple of 16 elements and at least D = 64, got 72"):
            f(good, _bytes(n0, H, S, D + 8).view(F8)[..., :D])   # 72: a multiple of 8, which the 2-byte calls take
        with pytest.raises(ValueError, match=what + f"{kn}'s row stride must be a multiple of 16 elements and at least D = 64, got 0"):
            f(good[:, :, :1].expand(shape), good)
        odd_head = _bytes(n0 * H * (S * D + 8)).view(F8).as_strided(shape, (H * (S * D + 8), S * D + 8, D, 1))
        with pytest.raises(ValueError, match=what + f"{kn}'s head stride must be a multiple of 16 elements, got {S * D + 8}"):
            f(odd_head, good)
        odd_outer = _bytes(n0 * (H * S * D + 8)).view(F8).as_strided(shape, (H * S * D + 8, S * D, D, 1))
        with pytest.raises(ValueError, match=what + f"{vn}'s {outer} stride must be a multiple of 16 elements, got {H * S * D + 8}"):
            f(good, odd_outer)
        n = n0 * H * S * D
        buf = _bytes(n + 32)
        shifted = buf[8 - buf.data_ptr() % 8:][:n].view(F8).reshape(shape)  # 8 past a 16-byte boundary or on one
        if shifted.data_ptr() % 16 == 0:
            shifted = buf[16 - buf.data_ptr() % 16 + 8:][:n].view(F8).reshape(shape)
        assert shifted.data_ptr() % 16 != 0
        with pytest.raises(ValueError, match=what + f"{kn}'s data pointer must be 16-byte aligned"):
            f(shifted, good)
        # the scales
        for name in ("k_scale", "v_scale"):
            for bad in (torch.ones(2, dtype=torch.float64), torch.ones(2, dtype=torch.bfloat16), torch.ones(2, dtype=torch.int32)):
                with pytest.raises(ValueError, match=what + f"{name} must be a float32 tensor, got {bad.dtype}"):
                    f(good, good, **{name: bad})
            for bad in (torch.ones(3), torch.ones(8), torch.ones(2, 1), torch.ones(1, 1), torch.ones(0)):
                with pytest.raises(ValueError, match=what + rf"{name} must have shape \(\), \(1,\) or \(2,\)"):
                    f(good, good, **{name: bad})
            for bad in ("0.5", [0.5, 0.5], True):
                with pytest.raises(ValueError, match=what + f"{name} must be None, a float or a dense float32 tensor"):
                    f(good, good, **{name: bad})
            with pytest.raises(RuntimeError, match=what + f"{name} is on meta but q is on cpu"):
                f(good, good, **{name: torch.ones(2, device="meta")})
        # shared refusals keep their texts and types
        with pytest.raises(ValueError, match=what + "chunk must be None or a positive int"):
            f(good, good, chunk=0)
        with pytest.raises(ValueError, match=what + f"{vn} must be a dense tensor with {kn}'? ?s? shape"):
            f(good, _bytes(n0, H, S * 2, D).view(F8))
        with pytest.raises(TypeError):  # the scales are keyword only
            f(good, good, 64, None, 0.5)
        # host tensors: the last check — the scales are named with the operands
        with pytest.raises(RuntimeError, match=what + r"layout, q, .*k_lens, k_scale, v_scale must be device \(HIP\) tensors"):
            f(good, good, k_scale=torch.ones(2), v_scale=torch.ones(()))
        with pytest.raises(RuntimeError, match=what + r"layout, q, .*k_lens must be device \(HIP\) tensors"):
            f(good.transpose(1, 2).contiguous().transpose(1, 2), good, k_scale=0.5)


def test_the_two_byte_calls_still_refuse_an_fp8_cache(real):
    q, lay, lens = torch.rand(2, 8, 1, 64).bfloat16(), _full(4), torch.tensor([100, 256])
    k8 = _bytes(2, 2, 256, 64).view(F8)
    with pytest.raises(ValueError, match="block_sparse_attention_decode: k must be bfloat16 or float16, got torch.float8_e4m3fn"):
        real.block_sparse_attention_decode(q, k8, k8, lay, lens)
    with pytest.raises(ValueError, match="block_sparse_attention_decode: v must be bfloat16 or float16, got torch.float8_e4m3fn"):
        real.block_sparse_attention_decode(q, q.new_zeros(2, 2, 256, 64), k8, lay, lens)
    pool, table = _bytes(20, 2, 16, 64).view(F8), torch.arange(32, dtype=torch.int32).reshape(2, 16) % 20
    with pytest.raises(ValueError, match="block_sparse_attention_decode_paged: k_pages must be bfloat16 or float16, got torch.float8_e4m3fn"):
        real.block_sparse_attention_decode_paged(q, pool, pool, table, lay, lens)
    with pytest.raises(ValueError, match="block_sparse_attention: k must be bfloat16 or float16"):
        real.block_sparse_attention(torch.rand(2, 256, 64).bfloat16(), k8[0], k8[0], lay)


def test_custom_mm_fp8_bindings_refuse_host_tensors_other_dtypes_and_keywords(built):
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import custom_mm
    offs, col = torch.tensor([[0, 1]], dtype=torch.int32), torch.tensor([0], dtype=torch.int32)
    q, lens, lse = torch.rand(1, 2, 1, 32).bfloat16(), torch.tensor([5], dtype=torch.int32), torch.empty(1, 2, 1)
    k8, pool, table = _bytes(1, 1, 64, 32).view(F8), _bytes(5, 1, 16, 32).view(F8), torch.zeros(1, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.block_attention_decode_fp8(offs, col, 1, q, k8, k8, lens, 1.0, None, None, 4, torch.empty_like(q), lse)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.block_attention_decode_paged_fp8(offs, col, 1, q, pool, pool, table, lens, 1.0, None, None, 4, torch.empty_like(q), lse)
    with pytest.raises(RuntimeError, match="OCP e4m3fn encoding is what is read"):
        custom_mm.block_attention_decode_fp8(offs, col, 1, q, k8.view(torch.float8_e4m3fnuz), k8, lens, 1.0, None, None, 4,
                                             torch.empty_like(q), lse)
    with pytest.raises(RuntimeError, match="OCP e4m3fn encoding is what is read"):
        custom_mm.block_attention_decode_paged_fp8(offs, col, 1, q, pool, pool.view(torch.uint8), table, lens, 1.0, None, None, 4,
                                                   torch.empty_like(q), lse)
    with pytest.raises(TypeError):  # positional only
        custom_mm.block_attention_decode_fp8(offs, col, 1, q, k8, k8, lens, 1.0, None, None, chunk=4, out=torch.empty_like(q), lse=lse)


def test_fp8_takes_are_the_parents(real):
    for dtype in (torch.bfloat16, torch.float16):
        for D in (32, 64, 96, 128):
            assert real.block_attention_decode_fp8_takes(dtype, D, 64, 4) and real.block_attention_decode_fp8_takes(dtype, D, 128, 16)
            assert real.block_attention_decode_paged_fp8_takes(dtype, D, 64, 1, 16)
    takes, paged = real.block_attention_decode_fp8_takes, real.block_attention_decode_paged_fp8_takes
    assert not takes(F8, 64, 64, 4) and not takes(torch.float32, 64, 64, 4) and not takes(torch.bfloat16, 48, 64, 4)
    assert not takes(torch.float16, 64, 96, 4) and not takes(torch.float16, 64, 64, 17)
    assert not paged(torch.bfloat16, 64, 64, 4, 8) and not paged(torch.bfloat16, 64, 64, 4, 24) and not paged(F8, 64, 64, 4, 16)


# ---- kv_to_fp8 ----------------------------------------------------------------------------------------------------------

def test_kv_to_fp8_scales_per_head_saturates_and_round_trips(real):
    g = torch.Generator().manual_seed(2201)
    x = torch.randn(3, 4, 50, 32, generator=g) * torch.tensor([0.01, 1.0, 30.0, 1000.0]).reshape(1, 4, 1, 1)
    x8, scale = real.kv_to_fp8(x)
    assert x8.dtype == F8 and x8.shape == x.shape and scale.dtype == torch.float32 and scale.shape == (4,)
    assert torch.equal(scale, (x.abs().amax(dim=(0, 2, 3)) / 448).float())      # per head: amax over all but dim 1
    back = x8.to(torch.float32) * scale.reshape(1, 4, 1, 1)
    assert torch.isfinite(back).all()
    big = x.abs() >= 2.0 ** -6 * scale.reshape(1, 4, 1, 1)   # the normal range of e4m3fn: 3 mantissa bits, half an ulp ≤ 2⁻⁴ |x|
    assert big.any() and ((back - x).abs()[big] <= 2.0 ** -4 * x.abs()[big]).all()
    assert (x8.to(torch.float32).abs().amax(dim=(0, 2, 3)) == 448).all()        # each head's amax lands on 448
    # a given scale: entries beyond ±448 · scale saturate — torch's cast alone would give NaN
    assert torch.isnan((x / 0.001).to(F8).to(torch.float32)).any()
    for given in (0.001, torch.tensor(0.001), torch.full((4,), 0.001)):
        y8, s = real.kv_to_fp8(x, given)
        y = y8.to(torch.float32)
        assert s.shape == (4,) and s.dtype == torch.float32 and torch.equal(s, torch.full((4,), 0.001))
        assert torch.isfinite(y).all() and y.abs().max() == 448
        beyond = x.abs() > 448 * 0.001
        assert beyond.any() and torch.equal(y[beyond], torch.sign(x[beyond]) * 448)
    # a pool has the heads in dim 1 too; zeros get the floor, not a zero scale; bf16 input
    z8, s = real.kv_to_fp8(torch.zeros(5, 2, 16, 32).bfloat16())
    assert s.tolist() == [torch.finfo(torch.float32).tiny] * 2 and (z8.view(torch.uint8) == 0).all()
    with pytest.raises(ValueError, match="kv_to_fp8: scale must hold 1 or Hkv = 4 entries"):
        real.kv_to_fp8(x, torch.ones(3))
    with pytest.raises(ValueError, match="kv_to_fp8: x must be a floating-point tensor"):
        real.kv_to_fp8(torch.zeros(2, 2, 4, 4, dtype=torch.int32))


# ---- wiring on CPU tensors through the float64 stand-in --------------------------------------------------------------

@pytest.fixture()
def mm(oracle_mod):
    """(matmuls bound to the float64 stand-in, the stand-in)."""
    import fake_custom_mm_block_attention_decode_fp8 as fake
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


def _poison(x8, vis):
    """0x7F in every key row of the fp8 cache [B, Hkv, Smax, D] that no token of its item sees — through the uint8 view."""
    x8 = x8.clone()
    x8.view(torch.uint8)[~vis.any(2)] = NAN_CODE
    return x8


@pytest.mark.parametrize("page", [None, 16, 128])
@pytest.mark.parametrize("G,T,block,l_lead,k_lens", [(4, 3, 64, (), [130, 130]), (2, 3, 128, (2,), [130, 257]), (16, 1, 64, (2, 2), [0, 65])])
def test_the_rule_and_the_scales_against_dense_attention_on_the_dequantised_cache(mm, page, G, T, block, l_lead, k_lens):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(2203 + G + (page or 0))
    B, Hkv, Smax, D = 2, 2, 256, 32
    layout = _random_layout(g, l_lead, Smax // block, keep=max(1, Smax // block - 1))
    vis = _visible(layout, B, Hkv, T, Smax, block, k_lens)
    q = torch.randn(B, Hkv * G, T, D, generator=g).half()
    k8, v8 = random_fp8(g, (B, Hkv, Smax, D)), random_fp8(g, (B, Hkv, Smax, D))
    ks, vs = torch.tensor([0.37, 1.9]), torch.tensor([0.11, 3.0])
    kd, vd = (x.to(torch.float32).double() * s.double().reshape(1, Hkv, 1, 1) for x, s in ((k8, ks), (v8, vs)))
    want, want_lse = _dense_reference(q, kd, vd, vis, 1.0 / D ** 0.5, G)
    lens = torch.tensor(k_lens)
    if page is None:
        out, lse = matmuls.block_sparse_attention_decode_fp8(q, _poison(k8, vis), _poison(v8, vis), layout, lens, block=block,
                                                             k_scale=ks, v_scale=vs, return_lse=True)
    else:
        kp, vp, table = _paged(g, _poison(k8, vis).view(torch.uint8), _poison(v8, vis).view(torch.uint8), page, fill=NAN_CODE)
        assert torch.equal(_gathered(kp, table), _poison(k8, vis).view(torch.uint8))
        out, lse = matmuls.block_sparse_attention_decode_paged_fp8(q, kp.view(F8), vp.view(F8), table, layout, lens, block=block,
                                                                   k_scale=ks, v_scale=vs, return_lse=True)
    assert out.dtype == torch.float16 and out.shape == q.shape and lse.dtype == torch.float32 and not out.requires_grad
    assert torch.isfinite(out).all()
    assert torch.allclose(out.double(), want, rtol=2e-3, atol=2e-3), float((out.double() - want).abs().max())
    seen = vis.any(-1).repeat_interleave(G, 1)
    assert (out[~seen] == 0).all() and (lse[~seen] == -float("inf")).all()
    assert torch.allclose(lse[seen].double(), want_lse[seen], rtol=1e-6, atol=1e-6)


def test_the_cache_the_table_and_the_scales_reach_the_bindings_as_they_are(mm):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(2207)
    B, Hkv, Smax, D, G, page = 2, 2, 128, 32, 2, 16
    W = Smax // page
    layout = _random_layout(g, (), 2, keep=2)
    q = torch.randn(B, Hkv * G, 1, D, generator=g).half()
    lens = torch.tensor([100, 128])
    k8, v8 = random_fp8(g, (B, Hkv, Smax, D)), random_fp8(g, (B, Hkv, Smax, D))
    ks, vs = torch.tensor([0.5, 0.25]), torch.tensor(2.0)
    want = matmuls.block_sparse_attention_decode(q, (k8.float() * ks.reshape(1, 2, 1, 1)).half(), (v8.float() * 2).half(), layout, lens)

    def record(name):
        (_, rec), = [c for c in fake.calls if c[0] == name]
        return rec

    # the contiguous form: [B, Hkv, S, D], the transposed view of [B, S, Hkv, D], a row stride of D + 16
    bshd_k, bshd_v = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (k8, v8))
    wide_k, wide_v = (torch.zeros(B, Hkv, Smax, D + 16, dtype=torch.uint8).view(F8) for _ in range(2))
    wide_k.view(torch.uint8)[..., :D], wide_v.view(torch.uint8)[..., :D] = k8.view(torch.uint8), v8.view(torch.uint8)
    for kk, vv in ((k8, v8), (bshd_k, bshd_v), (wide_k[..., :D], wide_v[..., :D])):
        fake.calls.clear()
        out = matmuls.block_sparse_attention_decode_fp8(q, kk, vv, layout, lens, k_scale=ks, v_scale=vs)
        rec = record("block_attention_decode_fp8")
        assert rec["k_ptr"] == kk.data_ptr() and rec["k_stride"] == tuple(kk.stride()) and rec["k_dtype"] == F8
        assert rec["v_ptr"] == vv.data_ptr() and rec["v_stride"] == tuple(vv.stride()) and rec["v_dtype"] == F8
        assert rec["k_scale"]["ptr"] == ks.data_ptr() and rec["k_scale"]["shape"] == (2,)      # the caller's tensors themselves
        assert rec["v_scale"]["ptr"] == vs.data_ptr() and rec["v_scale"]["shape"] == ()
        assert rec["scale"] == 1.0 / D ** 0.5 and rec["chunk"] == matmuls._decode_chunk(Smax, D)
        assert torch.equal(out, want)
    assert bshd_k.stride() == (Smax * Hkv * D, D, Hkv * D, 1) and wide_k[..., :D].stride(2) == D + 16
    # None stays None; a float arrives as a 0-d float32 tensor of that value; a (1,) tensor as it is
    fake.calls.clear()
    matmuls.block_sparse_attention_decode_fp8(q, k8, v8, layout, lens)
    rec = record("block_attention_decode_fp8")
    assert rec["k_scale"] is None and rec["v_scale"] is None
    fake.calls.clear()
    one = torch.tensor([0.75])
    matmuls.block_sparse_attention_decode_fp8(q, k8, v8, layout, lens, k_scale=0.37, v_scale=one, chunk=5)
    rec = record("block_attention_decode_fp8")
    assert rec["k_scale"]["shape"] == () and rec["k_scale"]["value"].dtype == torch.float32
    assert rec["k_scale"]["value"].item() == torch.tensor(0.37, dtype=torch.float32).item()
    assert rec["v_scale"]["ptr"] == one.data_ptr() and rec["v_scale"]["shape"] == (1,) and rec["chunk"] == 5
    # the paged form: both pool forms, an int32 table slice handed over untouched, an int64 table narrowed
    kp, vp, table = _paged(g, k8.view(torch.uint8), v8.view(torch.uint8), page, fill=0)
    kp, vp = kp.view(F8), vp.view(F8)
    phd_k, phd_v = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (kp, vp))
    wider = torch.full((B, W + 5), -1, dtype=torch.int32)
    wider[:, :W] = table
    sliced = wider[:, :W]
    for kk, vv, tt in ((kp, vp, table), (phd_k, phd_v, sliced)):
        fake.calls.clear()
        out = matmuls.block_sparse_attention_decode_paged_fp8(q, kk, vv, tt, layout, lens, k_scale=ks, v_scale=vs)
        rec = record("block_attention_decode_paged_fp8")
        assert rec["k_ptr"] == kk.data_ptr() and rec["k_stride"] == tuple(kk.stride()) and rec["k_dtype"] == F8
        assert rec["v_ptr"] == vv.data_ptr() and rec["v_stride"] == tuple(vv.stride())
        assert rec["table_ptr"] == tt.data_ptr() and rec["table_stride"] == tuple(tt.stride()) and rec["table_dtype"] == torch.int32
        assert rec["k_scale"]["ptr"] == ks.data_ptr() and rec["v_scale"]["ptr"] == vs.data_ptr()
        assert torch.equal(out, want)
    fake.calls.clear()
    out = matmuls.block_sparse_attention_decode_paged_fp8(q, kp, vp, sliced.long(), layout, lens, k_scale=ks, v_scale=vs)
    rec = record("block_attention_decode_paged_fp8")
    assert rec["table_dtype"] == torch.int32 and rec["table_shape"] == (B, W) and torch.equal(out, want)
    # the layout's record is the one the 2-byte calls keep
    st = matmuls._csr_state(layout)
    assert list(st.block_layouts) == [(str(q.device), 1)] and rec["offsets_ptr"] == st.block_layouts[(str(q.device), 1)]["fwd"][0].data_ptr()
