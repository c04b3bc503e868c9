"""matmuls.rope_kv_cache_append and rope_kv_cache_append_paged on the MI355X: the rotary embedding fused into
the KV-cache append.  The contract is on bits.  The yardstick is torch's CPU result of (a.float() * c − b.float() * s).to(dtype)
(tests/rope_reference.py); the cache is built on the CPU by `place` of tests/test_gpu_kv_cache_append.py, which knows the
append's rule and nothing of the kernel.  Every test compares q_out and the WHOLE cache, pool or underlying buffer.  Elements
that are no NaN are compared bit for bit; where the yardstick's ROTATED element is a NaN the kernel must give a NaN (its payload
is not specified); a NaN that is only copied (d ≥ rotary_dim, v into a 2-byte cache) keeps its bits.

B · Hkv ≤ 8, Hq ≤ 8, T ≤ 5, Smax ≤ 512."""
import pytest
import torch

import rope_reference as ref
from gpu_helpers import assert_same_bits
from test_gpu_block_attention_decode import ROWS, layout_from_rows, lens_tensor
from test_gpu_block_attention_decode_paged import gathered, scatter
from test_gpu_kv_cache_append import F8, NANB, _decode, codes, i16, patterns, place, quantised, values

pytestmark = pytest.mark.gpu

WIDTHS = [32, 64, 96, 128]
DTYPES = [torch.bfloat16, torch.float16]


def tables(pmax, R, base=10000.0):
    """cos, sin float32 [pmax, R/2] on the CPU: the angles p · base^(−2i/R), taken in float64."""
    ang = torch.arange(pmax, dtype=torch.float64)[:, None] * base ** (-2.0 * torch.arange(R // 2, dtype=torch.float64) / R)
    return ang.cos().float(), ang.sin().float()


def yardstick(dtype, q16, k16, cos, sin, k_lens, R, inter, new_lens=None):
    """(rotated q, rotated k, token [B, T]) as int16 bits on the CPU; the rows of a slot without a token are zeros."""
    B, _, T, _ = q16.shape
    pos, token = ref.token_slots(B, T, k_lens, cos.shape[0], new_lens)
    return (ref.rotated(q16, dtype, cos, sin, pos, token, R, inter), ref.rotated(k16, dtype, cos, sin, pos, token, R, inter), token)


def rotated_nan(x16, dtype, R):
    """Where a rotated element of the yardstick is a NaN: the kernel's payload there is free."""
    m = torch.isnan(x16.view(dtype).float())
    m[..., R:] = False
    return m


def same(got, want, what, loose=None, dtype=None):
    """Raw integers (int16 bits or e4m3fn bytes) equal everywhere; where `loose`, a NaN of `dtype` (None: a NaN code) instead."""
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    loose = torch.zeros(got.shape, dtype=torch.bool) if loose is None else loose
    bad = torch.nonzero((got != want) & ~loose)
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} of {got.numel()} elements differ, first at {bad[:4].tolist()}: got " \
                             f"{[int(got[tuple(i)]) for i in bad[:4]]} want {[int(want[tuple(i)]) for i in bad[:4]]}"
    if loose.any():
        nan = torch.isnan(got.view(dtype).float())[loose] if got.dtype == torch.int16 else (got[loose] & 0x7F) == NANB
        assert nan.all(), f"{what}: {int((~nan).sum())} elements are no NaN where the yardstick is one"


def expected_cache(mm, dtype, cache_k, cache_v, k_rot, v16, k_lens, token, R, table=None, scales=None):
    """Places the tokens' rows into the CPU caches (raw integers, in place) as kv_cache_append would leave them for the
    yardstick's rotated k; scales None: a 2-byte cache, else (k_scale, v_scale) of an fp8 one.  Returns (pairs written, where
    the k cache's NaN is free, where the v cache's is: an fp8 byte of a NaN source)."""
    fp8 = scales is not None
    rows_k = quantised(mm, k_rot, dtype, scales[0]) if fp8 else k_rot
    rows_v = quantised(mm, v16.contiguous(), dtype, scales[1]) if fp8 else v16
    n = ref.place_tokens(place, cache_k, rows_k, k_lens, token, table)
    assert ref.place_tokens(place, cache_v, rows_v, k_lens, token, table) == n
    loose_k, loose_v = torch.zeros_like(cache_k), torch.zeros_like(cache_v)
    nan_k = torch.isnan(k_rot.view(dtype).float()) if fp8 else rotated_nan(k_rot, dtype, R)
    nan_v = torch.isnan(v16.view(dtype).float()) if fp8 else torch.zeros(v16.shape, dtype=torch.bool)
    ref.place_tokens(place, loose_k, nan_k.to(cache_k.dtype), k_lens, token, table)
    ref.place_tokens(place, loose_v, nan_v.to(cache_v.dtype), k_lens, token, table)
    return n, loose_k.bool(), loose_v.bool()


def call(mm, dev, dtype, q16, k16, v16, cos, sin, k, v, k_lens, table=None, **kw):
    """The fused call on device copies of the CPU operands (q16, k16, v16 int16 bits; k, v device tensors); returns q_out."""
    q, kn, vn = (x.to(dev).view(dtype) for x in (q16, k16, v16))
    lens = k_lens if isinstance(k_lens, torch.Tensor) else lens_tensor(k_lens, dev)
    if table is None:
        return mm.rope_kv_cache_append(q, kn, vn, cos.to(dev), sin.to(dev), k, v, lens, **kw)
    return mm.rope_kv_cache_append_paged(q, kn, vn, cos.to(dev), sin.to(dev), k, v, table.to(dev), lens, **kw)


# ---- 1. all forms ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("inter", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", WIDTHS)
def test_1_all_forms_into_a_flat_two_byte_cache(mm, dev, dtype, D, inter):
    B, Hkv, Hq, T, Smax, k_lens = 2, 2, 4, 3, 256, [200, 65]
    cos, sin = tables(Smax, D)
    q16, k16 = values(2510 + D, dtype, B, Hq, T, D), values(2511 + D, dtype, B, Hkv, T, D)
    v16 = patterns(2512 + D, dtype, B, Hkv, T, D)                                   # NaN payloads, −0, ±inf: bit copies
    cache_k, cache_v = patterns(2513 + D, dtype, B, Hkv, Smax, D), patterns(2514 + D, dtype, B, Hkv, Smax, D)
    k, v = cache_k.to(dev).view(dtype), cache_v.to(dev).view(dtype)
    out = call(mm, dev, dtype, q16, k16, v16, cos, sin, k, v, k_lens, interleaved=inter)
    assert out.shape == (B, Hq, T, D) and out.dtype == dtype and out.is_contiguous() and not out.requires_grad
    want_q, k_rot, token = yardstick(dtype, q16, k16, cos, sin, k_lens, D, inter)
    assert token.all() and not torch.equal(want_q, q16)
    n, loose_k, _ = expected_cache(mm, dtype, cache_k, cache_v, k_rot, v16, k_lens, token, D)
    assert n == 6 and not loose_k.any()
    same(out.view(torch.int16), want_q, f"{dtype} D={D} interleaved={inter}: q_out")
    same(k.view(torch.int16), cache_k, f"{dtype} D={D} interleaved={inter}: k")
    same(v.view(torch.int16), cache_v, f"{dtype} D={D} interleaved={inter}: v")
    assert torch.equal(cache_k[0, :, 197:200], k_rot[0]) and torch.equal(cache_v[1, :, 62:65], v16[1])


# ---- 2. the float32 arithmetic ----------------------------------------------------------------------------------------------------------

def contraction_rows(dtype, want=16):
    """Searched on the host among 32 768 seeded rows (D = 128, NeoX pairs, positions < 512): `want` rows on which
    fma(a, c, −fl(b·s)) / fma(b, c, fl(a·s)) changes an output, and `want` on which fma(−b, s, fl(a·c)) / fma(a, s, fl(b·c))
    does — the two places a compiler can contract the rotation, emulated in float64.  Returns (x [N, 128] of dtype,
    pos [N], indices of the first kind, indices of the second, cos, sin)."""
    g = torch.Generator().manual_seed(2520)
    N, D = 32768, 128
    x = torch.randn(N, D, generator=g).to(dtype)
    pos = torch.randint(0, 512, (N,), generator=g)
    cos, sin = tables(512, D)
    c, s = cos[pos], sin[pos]
    a, b = x[:, :64].float(), x[:, 64:].float()
    bits = lambda t: t.to(dtype).view(torch.int16)  # noqa: E731
    ya, yb = bits(a * c - b * s), bits(b * c + a * s)
    a64, b64, c64, s64 = a.double(), b.double(), c.double(), s.double()
    first = (bits((a64 * c64 - (b * s).double()).float()) != ya) | (bits((b64 * c64 + (a * s).double()).float()) != yb)
    second = (bits(((a * c).double() - b64 * s64).float()) != ya) | (bits(((b * c).double() + a64 * s64).float()) != yb)
    kinds = [torch.nonzero(m.any(1)).reshape(-1) for m in (first, second)]
    assert all(k.numel() >= want for k in kinds), [k.numel() for k in kinds]
    return x, pos, kinds[0][:want], kinds[1][:want], cos, sin


@pytest.mark.parametrize("dtype", DTYPES)
def test_2_two_products_and_one_sum_each_rounded_no_fma(mm, dev, dtype):
    """After the narrowing a contracted rotation differs from the yardstick on about 1 element in 60 000 (bfloat16) or 10 000
    (float16) of random data, so the rows that tell are searched for: 16 of each kind.  Eight of them at a time are head 0 of
    q and the k row of the 8 items of a call (T = 1, the item's position the row's); the other q heads hold further rows of
    the search at that position.  Both pair forms: the interleaved row holds the same pairs."""
    x, pos, first, second, cos, sin = contraction_rows(dtype)
    rows = torch.cat([first, second])
    assert rows.numel() == 32
    B, Hq, D, Smax = 8, 8, 128, 512
    for inter in (False, True):
        for lo in range(0, 32, B):
            sel = rows[lo:lo + B]
            k_lens = (pos[sel] + 1).tolist()
            special = x[sel].view(torch.int16)                                             # [8, 128]
            filler = x[(sel[:, None] + torch.arange(1, Hq)[None, :]) % x.shape[0]].view(torch.int16)     # [8, 7, 128]
            q16 = torch.cat([special[:, None], filler], 1)[:, :, None, :].contiguous()     # [8, 8, 1, 128]
            if inter:                                                                      # (x[i], x[i + 64]) → (x[2i], x[2i + 1])
                q16 = torch.stack([q16[..., :64], q16[..., 64:]], -1).reshape(q16.shape)
            k16 = q16[:, :1].clone()
            v16 = values(2521 + lo, dtype, B, 1, 1, D)
            cache_k, cache_v = values(2522, dtype, B, 1, Smax, D), values(2523, dtype, B, 1, Smax, D)
            k, v = cache_k.to(dev).view(dtype), cache_v.to(dev).view(dtype)
            out = call(mm, dev, dtype, q16, k16, v16, cos, sin, k, v, k_lens, interleaved=inter)
            want_q, k_rot, token = yardstick(dtype, q16, k16, cos, sin, k_lens, D, inter)
            assert expected_cache(mm, dtype, cache_k, cache_v, k_rot, v16, k_lens, token, D)[0] == B
            what = f"{dtype} interleaved={inter} rows {lo}..{lo + B - 1} ({'first' if lo < 16 else 'second'} product fused)"
            same(out.view(torch.int16), want_q, what + ": q_out")
            same(k.view(torch.int16), cache_k, what + ": k")
            same(v.view(torch.int16), cache_v, what + ": v")


# ---- 3. every source pattern --------------------------------------------------------------------------------------------------------------

ALL = i16(range(65536))
PARTNERS = [0.0, 1.0, -0.5, 3.0, -2.0 ** -10, 60000.0, 2.0 ** -20]      # finite in both types, 7 of them: every pair index meets each
POSITIONS3, PMAX3 = [0, 1, 77, 95], 96


@pytest.mark.parametrize("inter", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_3_every_bit_pattern_of_the_source_at_four_positions(mm, dev, dtype, inter):
    """All 65 536 patterns of `dtype` as the `a` of a pair — subnormals (float32 subnormal products with bfloat16), −0, ±inf,
    NaN, overflow at the narrowing —, the partner `b` from PARTNERS, at each of the positions 0, 1, 77 and Pmax − 1: 4096 rows of
    64 pairs.  Within the shapes of this file that is 512 calls of B = 8 items with one k row and 8 q rows each (T = 1), on
    slices of buffers uploaded once, into a 2-byte and then an fp8 cache.  q_out is downloaded once; the whole cache is
    compared ON THE DEVICE after every call with the expected cache, kept there by index assignments of rows computed on the
    CPU, every NaN of either side mapped to one code first (all of k is rotated here: R = D)."""
    D, B, Hq, Smax = 128, 8, 8, PMAX3
    cos, sin = tables(PMAX3, D)
    a = ALL.reshape(1, 1024, 64).expand(4, 1024, 64)
    partner = torch.tensor(PARTNERS)[torch.arange(65536) % len(PARTNERS)].to(dtype).view(torch.int16).reshape(1, 1024, 64).expand(4, 1024, 64)
    rows = torch.stack([a, partner], -1).reshape(4, 1024, D) if inter else torch.cat([a, partner], -1)       # [position, row, D]
    rows = rows.contiguous()
    rot = torch.stack([ref.rotate(rows[i], dtype, cos[p], sin[p], D, inter) for i, p in enumerate(POSITIONS3)])
    nan = torch.isnan(rot.view(dtype).float())
    assert nan.float().mean() <= 0.035, float(nan.float().mean())
    assert (2046 if dtype == torch.float16 else 254) * 4 * 2 <= int(nan.sum())             # every NaN pattern of `a` reaches a' and b'
    rows, rot = rows.reshape(4096, D), rot.reshape(4096, D)
    g = torch.arange(4096)                                                  # row g: item g % 8 of call g // 8, position block g // 1024
    q_rows = (g // 1024 * 1024)[:, None] + (g % 1024)[:, None].add(64 * torch.arange(Hq)[None, :]) % 1024       # [4096, 8]: the block's own rows
    lens_all = (torch.tensor(POSITIONS3)[g // 1024] + 1).to(torch.int32).reshape(512, B).to(dev)
    K = rows.to(dev).view(dtype).reshape(512, B, 1, 1, D)
    Q = rows[q_rows].to(dev).view(dtype).reshape(512, B, Hq, 1, D)
    q_out = torch.full((512, B, Hq, 1, D), 0x5555, dtype=torch.int16, device=dev).view(dtype)
    v16 = values(2530, dtype, B, 1, 1, D)
    vn, dcos, dsin = v16.to(dev).view(dtype), cos.to(dev), sin.to(dev)
    items = torch.arange(B, device=dev)
    one_nan = torch.tensor(0x7FFF, dtype=torch.int16, device=dev)
    for fp8 in (False, True):
        if fp8:
            ks, vs = torch.tensor([0.5], device=dev), torch.tensor(2.0, device=dev)
            want_rows = quantised(mm, rot.reshape(4096, 1, 1, D), dtype, ks).reshape(512, B, D)
            want_rows = torch.where(want_rows & 0x7F == NANB, torch.tensor(NANB, dtype=torch.uint8), want_rows).to(dev)
            v_row = quantised(mm, v16, dtype, vs).reshape(B, D).to(dev)
            cache_k, cache_v = codes(2531, B, 1, Smax, D).to(dev), codes(2532, B, 1, Smax, D).to(dev)
            one_code = torch.tensor(NANB, dtype=torch.uint8, device=dev)
            view, canon, kw = (lambda t: t.view(F8)), (lambda t: torch.where(t & 0x7F == NANB, one_code, t)), dict(k_scale=ks, v_scale=vs)
        else:
            want_rows = torch.where(nan.reshape(4096, D), torch.tensor(0x7FFF, dtype=torch.int16), rot).reshape(512, B, D).to(dev)
            v_row = v16.reshape(B, D).to(dev)
            cache_k, cache_v = values(2531, dtype, B, 1, Smax, D).to(dev), values(2532, dtype, B, 1, Smax, D).to(dev)
            view, canon, kw = (lambda t: t.view(dtype)), (lambda t: torch.where(torch.isnan(t.view(dtype)), one_nan, t)), {}
        want_k, want_v = cache_k.clone(), cache_v.clone()
        bad = torch.zeros((), dtype=torch.int64, device=dev)
        for c in range(512):
            got = mm.rope_kv_cache_append(Q[c], K[c], vn, dcos, dsin, view(cache_k), view(cache_v), lens_all[c], interleaved=inter,
                                          q_out=q_out[c], **kw)
            assert got is not None and got.data_ptr() == q_out[c].data_ptr()
            row = lens_all[c].long() - 1
            want_k[items, 0, row], want_v[items, 0, row] = want_rows[c], v_row
            bad += (canon(cache_k) != want_k).sum() + (cache_v != want_v).sum()
        assert int(bad) == 0, f"{dtype} interleaved={inter} fp8={fp8}: {int(bad)} cache elements differ over the 512 calls"
        want_q = rot[q_rows].reshape(512, B, Hq, 1, D)
        same(q_out.view(torch.int16), want_q, f"{dtype} interleaved={inter} fp8={fp8}: q_out", loose=torch.isnan(want_q.view(dtype).float()),
             dtype=dtype)
        q_out.view(torch.int16).fill_(0x5555)


# ---- 4. partial rotation ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R,D", [(16, 128), (32, 128), (64, 128), (48, 96)])
def test_4_partial_rotation_copies_the_tail_bit_for_bit(mm, dev, R, D):
    B, Hkv, Hq, T, Smax, k_lens = 2, 2, 4, 3, 128, [100, 3]
    for n, (dtype, inter) in enumerate([(torch.bfloat16, False), (torch.float16, True), (torch.float16, False), (torch.bfloat16, True)]):
        cos, sin = tables(Smax, R)
        q16, k16, v16 = (values(2540 + R + i, dtype, B, H, T, D) for i, H in enumerate((Hq, Hkv, Hkv)))
        q16[..., R:] = patterns(2543 + R, dtype, B, Hq, T, D - R)
        k16[..., R:] = patterns(2544 + R, dtype, B, Hkv, T, D - R)
        for x in (q16, k16):                                                            # −0 at both ends of the tail
            x[1:, ..., R], x[..., D - 1] = -32768, -32768
        assert torch.isnan(q16[..., R:].view(dtype).float()).sum() >= 3 and torch.isnan(k16[..., R:].view(dtype).float()).sum() >= 3
        cache_k, cache_v = values(2545, dtype, B, Hkv, Smax, D), values(2546, dtype, B, Hkv, Smax, D)
        k, v = cache_k.to(dev).view(dtype), cache_v.to(dev).view(dtype)
        out = call(mm, dev, dtype, q16, k16, v16, cos, sin, k, v, k_lens, interleaved=inter, rotary_dim=R)
        want_q, k_rot, token = yardstick(dtype, q16, k16, cos, sin, k_lens, R, inter)
        assert torch.equal(want_q[..., R:], q16[..., R:]) and not torch.equal(want_q[..., :R], q16[..., :R])
        assert expected_cache(mm, dtype, cache_k, cache_v, k_rot, v16, k_lens, token, R)[0] == 6
        what = f"R={R} D={D} {dtype} interleaved={inter}"
        same(out.view(torch.int16), want_q, what + ": q_out")          # (strict: the rotated part is finite, the tail's NaNs keep their bits)
        same(k.view(torch.int16), cache_k, what + ": k")
        same(v.view(torch.int16), cache_v, what + ": v")


# ---- 5. strides and outputs ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,D,inter", [(torch.bfloat16, 128, False), (torch.float16, 96, True)])
def test_5_strides_of_every_operand_and_every_form_of_the_outputs(mm, dev, dtype, D, inter):
    """q, k_new and v_new are slices of ONE fused projection [B, T, Hq + 2·Hkv, D]; the cache a [B, Smax, Hkv, D] buffer through
    .transpose(1, 2), then a buffer with a row stride of D + 8 whose gaps hold sentinels; cos / sin have a padded row stride.
    q_out fresh, given (a [B, T, Hq, D] buffer transposed) and in place; k_out given and in place.  Whole buffers compared."""
    B, Hkv, Hq, T, Smax, k_lens = 2, 2, 4, 3, 128, [100, 3]
    H = Hq + 2 * Hkv
    qkv = values(2550 + D, dtype, B, T, H, D)
    q16, k16, v16 = (qkv[:, :, lo:hi].transpose(1, 2) for lo, hi in ((0, Hq), (Hq, Hq + Hkv), (Hq + Hkv, H)))
    cos, sin = tables(Smax, D)
    wide = torch.full((2, Smax, D // 2 + 12), float("nan"))
    wide[0, :, :D // 2], wide[1, :, :D // 2] = cos, sin
    dwide = wide.to(dev)
    dcos, dsin = dwide[0, :, :D // 2], dwide[1, :, :D // 2]
    assert dcos.stride() == (D // 2 + 12, 1) and not dcos.is_contiguous()
    want_q, k_rot, token = yardstick(dtype, q16.contiguous(), k16.contiguous(), cos, sin, k_lens, D, inter)
    lens = lens_tensor(k_lens, dev)

    def operands():
        d = qkv.clone().to(dev).view(dtype)
        return (d,) + tuple(d[:, :, lo:hi].transpose(1, 2) for lo, hi in ((0, Hq), (Hq, Hq + Hkv), (Hq + Hkv, H)))

    def buffers(form):
        """The two cache buffers before the call, int16 on the CPU, and the logical [B, Hkv, Smax, D] view of one."""
        if form == "BSHD":
            return [values(2551 + i, dtype, B, Smax, Hkv, D) for i in range(2)], (lambda t: t.transpose(1, 2))
        bufs = [values(2553 + i, dtype, B, Hkv, Smax, D + 8) for i in range(2)]
        for t in bufs:
            t[..., D:] = 0x5555
        return bufs, (lambda t: t[..., :D])

    for form in ("BSHD", "padded rows"):
        bufs, logical = buffers(form)
        assert expected_cache(mm, dtype, logical(bufs[0]), logical(bufs[1]), k_rot, v16, k_lens, token, D)[0] == 6
        for outputs in ("fresh", "given", "in place"):
            dqkv, q, kn, vn = operands()
            assert not q.is_contiguous() and not kn.is_contiguous()
            dbufs = [t.to(dev) for t in buffers(form)[0]]
            k, v = (logical(t.view(dtype)) for t in dbufs)
            assert not k.is_contiguous()
            want_src = qkv.clone()
            what = f"{form}, outputs {outputs}, {dtype}"
            if outputs == "fresh":
                out = mm.rope_kv_cache_append(q, kn, vn, dcos, dsin, k, v, lens, interleaved=inter)
                assert out.is_contiguous() and out.data_ptr() != q.data_ptr()
                same(out.view(torch.int16), want_q, what + ": q_out")
            elif outputs == "given":
                qo_buf = torch.full((B, T, Hq, D + 8), 0x5555, dtype=torch.int16, device=dev)
                ko_buf = torch.full((B, Hkv, T, D), 0x5555, dtype=torch.int16, device=dev)
                qo, ko = qo_buf.view(dtype)[..., :D].transpose(1, 2), ko_buf.view(dtype)
                out = mm.rope_kv_cache_append(q, kn, vn, dcos, dsin, k, v, lens, interleaved=inter, q_out=qo, k_out=ko)
                assert out is qo
                want_buf = torch.full((B, T, Hq, D + 8), 0x5555, dtype=torch.int16)
                want_buf[..., :D] = want_q.transpose(1, 2)
                same(qo_buf, want_buf, what + ": the q_out buffer, gaps included")
                same(ko_buf, k_rot, what + ": k_out")
            else:
                out = mm.rope_kv_cache_append(q, kn, vn, dcos, dsin, k, v, lens, interleaved=inter, q_out=q, k_out=kn)
                assert out is q
                want_src[:, :, :Hq], want_src[:, :, Hq:Hq + Hkv] = want_q.transpose(1, 2), k_rot.transpose(1, 2)
            same(dqkv.view(torch.int16), want_src, what + ": the source buffer (only what is rotated in place changes)")
            same(dbufs[0], bufs[0], what + ": the k buffer")
            same(dbufs[1], bufs[1], what + ": the v buffer")
    assert torch.isnan(dwide[:, :, D // 2:]).all()


# ---- 6. drops and ragged batches -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,page", [(torch.bfloat16, 0), (torch.float16, 16)])
def test_6_dropped_tokens_keep_their_q_and_slots_without_a_token_are_zeros(mm, dev, dtype, page):
    """Smax = 64 rows of cache, Pmax rows of table.  pos < 0 and pos ≥ Pmax: no token — zero rows in q_out and k_out, nothing
    stored (also where the row would still lie inside Smax: Pmax = 40 < Smax); pos ≥ Smax with pos < Pmax = 80: q rotated, k and v
    dropped; paged, table entries −1 and P drop k and v as well."""
    Hkv, Hq, T, D, Smax, B = 2, 4, 3, 64, 64, 4
    # (Pmax, k_lens, slots that hold a token, rows stored in the flat cache, rows stored in the pool), counted by hand:
    #  [2, 66, 81, 40]: item 0 at −1, 0, 1 (2 tokens); item 1 at 63, 64, 65 (3 tokens, 63 stored); item 2 at 78, 79, 80 (2 tokens,
    #  none stored); item 3 at 37, 38, 39 (all stored).  Paged, item 0's page 0 is −1 and item 3's page 2 is P: only row 63 is stored.
    #  [41, 30, 2³¹ − 1, −5] with Pmax = 40: item 0 at 38, 39, 40 — 40 has no table row though it lies inside Smax —; item 1 at 27, 28, 29.
    #  [64, 65, 80, 79]: every slot holds a token; 61, 62, 63 of item 0 and 62, 63 of item 1 are stored.
    cases = ((80, [2, 66, 81, 40], 10, 6, 1), (40, [41, 30, 2 ** 31 - 1, -5], 5, 5, 5), (80, [64, 65, 80, 79], 12, 5, 5))
    for pmax, k_lens, tokens, stored_flat, stored_paged in cases:
        cos, sin = tables(pmax, D)
        q16, k16, v16 = (values(2560 + i, dtype, B, H, T, D) for i, H in enumerate((Hq, Hkv, Hkv)))
        flat_k, flat_v = values(2563, dtype, B, Hkv, Smax, D), values(2564, dtype, B, Hkv, Smax, D)
        table = None
        if page:
            W = Smax // page
            P = B * W + 2
            table = torch.randperm(P, generator=torch.Generator().manual_seed(2565))[:B * W].reshape(B, W).to(torch.int32)
            cache_k, cache_v = (torch.full((P, Hkv, page, D), 0x7FFF, dtype=torch.int16) for _ in range(2))
            scatter(cache_k, table, flat_k)
            scatter(cache_v, table, flat_v)
            table[0, 0], table[3, (k_lens[3] - 1) // page % W] = -1, P                  # item 0's first page, the page of item 3's last token
        else:
            cache_k, cache_v = flat_k, flat_v
        k, v = cache_k.to(dev).view(dtype), cache_v.to(dev).view(dtype)
        k_out = torch.full((B, Hkv, T, D), 0x5555, dtype=torch.int16, device=dev)
        out = call(mm, dev, dtype, q16, k16, v16, cos, sin, k, v, k_lens, table, k_out=k_out.view(dtype))
        want_q, k_rot, token = yardstick(dtype, q16, k16, cos, sin, k_lens, D, False)
        pos, _ = ref.token_slots(B, T, k_lens, pmax)
        n = expected_cache(mm, dtype, cache_k, cache_v, k_rot, v16, k_lens, token, D, table)[0]
        stored = token & (pos < Smax)
        if page:
            entry = table.long().gather(1, (pos.clamp(0, Smax - 1) // page))
            stored &= (entry >= 0) & (entry < cache_k.shape[0])
        assert n == int(stored.sum()) == (stored_paged if page else stored_flat) and int(token.sum()) == tokens, (n, int(token.sum()))
        what = f"Pmax={pmax} k_lens={k_lens} page={page}"
        same(out.view(torch.int16), want_q, what + ": q_out")
        same(k_out, k_rot, what + ": k_out")
        same(k.view(torch.int16), cache_k, what + ": k")
        same(v.view(torch.int16), cache_v, what + ": v")
        assert (want_q[~token[:, None, :].expand(B, Hq, T)] == 0).all() and (want_q[token[:, None, :].expand(B, Hq, T)] != 0).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_6_ragged_batches_are_right_aligned_and_compose_with_the_decode_call(mm, dev, dtype):
    """new_lens = [1, 3, 0] with T = 3: item 0's token stands in the last slot, item 2 has none — zero rows, nothing stored; −2
    and 9 are clamped to 0 and 3.  Then block_sparse_attention_decode on all T slots: the rows of the slots that hold a token
    are those of the decode call made for that item alone with T = new_lens[b]."""
    B, Hkv, Hq, T, D, Smax, k_lens = 3, 2, 4, 3, 64, 512, [200, 65, 130]
    cos, sin = tables(Smax, D)
    q16, k16, v16 = (values(2570 + i, dtype, B, H, T, D, amp=1.0) for i, H in enumerate((Hq, Hkv, Hkv)))
    layout = layout_from_rows(ROWS, dev)
    for new_lens, lens_dtype in (([1, 3, 0], torch.int32), ([1, 9, -2], torch.int64)):
        cache_k, cache_v = values(2573, dtype, B, Hkv, Smax, D, amp=1.0), values(2574, dtype, B, Hkv, Smax, D, amp=1.0)
        k, v = cache_k.to(dev).view(dtype), cache_v.to(dev).view(dtype)
        out = call(mm, dev, dtype, q16, k16, v16, cos, sin, k, v, k_lens, new_lens=torch.tensor(new_lens, device=dev, dtype=lens_dtype))
        want_q, k_rot, token = yardstick(dtype, q16, k16, cos, sin, k_lens, D, False, new_lens)
        assert token.tolist() == [[False, False, True], [True, True, True], [False, False, False]]
        assert expected_cache(mm, dtype, cache_k, cache_v, k_rot, v16, k_lens, token, D)[0] == 4
        same(out.view(torch.int16), want_q, f"new_lens {new_lens}: q_out")
        same(k.view(torch.int16), cache_k, f"new_lens {new_lens}: k")
        same(v.view(torch.int16), cache_v, f"new_lens {new_lens}: v")
        assert torch.equal(cache_k[0, :, 199], k_rot[0, :, 2]) and (want_q[2] == 0).all() and (want_q[0, :, :2] == 0).all()
    lens = lens_tensor(k_lens, dev)
    full, full_lse = mm.block_sparse_attention_decode(out, k, v, layout, lens, chunk=2, return_lse=True)
    for b, n in enumerate([1, 3, 0]):
        if n == 0:
            continue
        alone, alone_lse = mm.block_sparse_attention_decode(out[b:b + 1, :, T - n:].contiguous(), k[b:b + 1], v[b:b + 1], layout, lens[b:b + 1],
                                                            chunk=2, return_lse=True)
        assert_same_bits(full[b:b + 1, :, T - n:], alone, f"item {b}: the rows of its {n} tokens")
        assert_same_bits(full_lse[b:b + 1, :, T - n:], alone_lse, f"item {b}: lse")
        assert torch.isfinite(alone.float()).all() and alone.float().abs().max() > 0


# ---- 7. paged --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("page,dtype,inter", [(16, torch.bfloat16, True), (64, torch.float16, False)])
def test_7_the_paged_call_is_the_flat_call_on_the_gathered_cache(mm, dev, page, dtype, inter):
    """Three items whose tokens straddle rows 15|16, 63|64 and 255|256, a shuffled pool with three pages more than are
    referenced; items share no written page.  q_out and the gathered pool equal the flat call's; unreferenced pages keep
    their bits; and both equal the CPU's."""
    B, Hkv, Hq, T, D, Smax, k_lens = 3, 2, 4, 3, 64, 512, [18, 66, 258]
    W = Smax // page
    P = B * W + 3
    table = torch.randperm(P, generator=torch.Generator().manual_seed(2580 + page))[:B * W].reshape(B, W).to(torch.int32)
    cos, sin = tables(Smax, D)
    q16, k16, v16 = (values(2581 + i, dtype, B, H, T, D) for i, H in enumerate((Hq, Hkv, Hkv)))
    flat_k, flat_v = values(2584, dtype, B, Hkv, Smax, D), values(2585, dtype, B, Hkv, Smax, D)
    pool_k, pool_v = (torch.full((P, Hkv, page, D), 0x7FFF, dtype=torch.int16) for _ in range(2))
    scatter(pool_k, table, flat_k)
    scatter(pool_v, table, flat_v)
    kp, vp = pool_k.to(dev), pool_v.to(dev)
    k, v = flat_k.to(dev), flat_v.to(dev)
    out_p = call(mm, dev, dtype, q16, k16, v16, cos, sin, kp.view(dtype), vp.view(dtype), k_lens, table, interleaved=inter)
    out_f = call(mm, dev, dtype, q16, k16, v16, cos, sin, k.view(dtype), v.view(dtype), k_lens, interleaved=inter)
    same(out_p.view(torch.int16), out_f.view(torch.int16), f"page={page}: q_out of the paged and the flat call")
    same(gathered(kp.cpu(), table), k, f"page={page}: the gathered k pool and the flat cache")
    same(gathered(vp.cpu(), table), v, f"page={page}: the gathered v pool and the flat cache")
    want_q, k_rot, token = yardstick(dtype, q16, k16, cos, sin, k_lens, D, inter)
    assert expected_cache(mm, dtype, pool_k, pool_v, k_rot, v16, k_lens, token, D, table)[0] == 9
    same(out_p.view(torch.int16), want_q, f"page={page}: q_out")
    same(kp, pool_k, f"page={page}: the k pool")
    same(vp, pool_v, f"page={page}: the v pool")
    unreferenced = [e for e in range(P) if e not in table.reshape(-1).tolist()]
    assert len(unreferenced) == 3 and (pool_k[unreferenced] == 0x7FFF).all()


# ---- 8. fp8, and the relation to kv_cache_append ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("page", [0, 16])
def test_8_every_cache_form_is_what_kv_cache_append_leaves_for_the_rounded_rotated_k(mm, dev, dtype, page):
    """fp8 with per-head tensor scales and with a float scale, and the 2-byte form: the cache after the fused call equals, byte
    for byte, the one kv_cache_append(k_rot.to(dev), v_new, …) leaves on a copy of the same cache — k_rot the yardstick's
    rotated k, rounded to the source dtype — and the one built on the CPU."""
    B, Hkv, Hq, T, D, Smax, k_lens = 2, 2, 4, 3, 128, 128, [100, 17]
    cos, sin = tables(Smax, D)
    q16 = values(2590, dtype, B, Hq, T, D, amp=40.0)
    k16, v16 = values(2591, dtype, B, Hkv, T, D, amp=40.0), values(2592, dtype, B, Hkv, T, D, amp=40.0)
    want_q, k_rot, token = yardstick(dtype, q16, k16, cos, sin, k_lens, D, False)
    table = None
    if page:
        W = Smax // page
        P = B * W + 3
        table = torch.randperm(P, generator=torch.Generator().manual_seed(2593))[:B * W].reshape(B, W).to(torch.int32)
    per_head = (torch.tensor([0.3, 7.0], device=dev), torch.tensor([2.5, 0.11], device=dev))
    for scales in (per_head, (0.37, 3), None):
        fp8 = scales is not None
        if fp8:
            flat_k, flat_v, view = codes(2594, B, Hkv, Smax, D), codes(2595, B, Hkv, Smax, D), (lambda t: t.view(F8))
            kw = dict(k_scale=scales[0], v_scale=scales[1])
        else:
            flat_k, flat_v, view, kw = values(2594, dtype, B, Hkv, Smax, D), values(2595, dtype, B, Hkv, Smax, D), (lambda t: t.view(dtype)), {}
        if page:
            cache_k, cache_v = (torch.full((P, Hkv, page, D), NANB if fp8 else 0x7FFF, dtype=flat_k.dtype) for _ in range(2))
            scatter(cache_k, table, flat_k)
            scatter(cache_v, table, flat_v)
        else:
            cache_k, cache_v = flat_k, flat_v
        k, v, k2, v2 = cache_k.to(dev), cache_v.to(dev), cache_k.to(dev), cache_v.to(dev)
        out = call(mm, dev, dtype, q16, k16, v16, cos, sin, view(k), view(v), k_lens, table, **kw)
        lens = lens_tensor(k_lens, dev)
        if page:
            mm.kv_cache_append_paged(k_rot.to(dev).view(dtype), v16.to(dev).view(dtype), view(k2), view(v2), table.to(dev), lens, **kw)
        else:
            mm.kv_cache_append(k_rot.to(dev).view(dtype), v16.to(dev).view(dtype), view(k2), view(v2), lens, **kw)
        what = f"{dtype} page={page} scales={'none' if not fp8 else scales}"
        same(k, k2, what + ": k against kv_cache_append of the yardstick's rotated k")
        same(v, v2, what + ": v against kv_cache_append")
        assert expected_cache(mm, dtype, cache_k, cache_v, k_rot, v16, k_lens, token, D, table, scales if fp8 else None)[0] == 6
        same(k, cache_k, what + ": k against the CPU's")
        same(v, cache_v, what + ": v against the CPU's")
        same(out.view(torch.int16), want_q, what + ": q_out")
        if fp8:   # the scales matter and the bytes are no copy of a 2-byte pattern
            assert not torch.equal(quantised(mm, k_rot, dtype, scales[0]), quantised(mm, k_rot, dtype, None))


# ---- 9. one graph per step ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fp8,dtype", [(False, torch.bfloat16), (True, torch.float16)])
def test_9_one_captured_graph_advances_rotates_appends_and_attends(mm, dev, fp8, dtype):
    """`lens += 1; rope_kv_cache_append_paged; decode` captured ONCE (page 16).  Three replays take one item through 63 → 64 (a
    page and a block boundary) and the other through 127 → 128, the table entry of a page the new token opens assigned in
    place; a fourth replay follows rows of cos / sin changed in place.  After every replay q_out, out, lse and the pool equal,
    bit for bit, those of the eager sequence on copies of the state before it, and the pool the CPU's mirror."""
    B, Hkv, G, T, D, Smax, page, start = 2, 2, 2, 1, 64, 512, 16, [62, 126]
    layout = layout_from_rows(ROWS, dev)
    scales = dict(k_scale=torch.tensor([0.02, 0.03], device=dev), v_scale=torch.tensor([0.025], device=dev)) if fp8 else {}
    raw = torch.uint8 if fp8 else torch.int16
    fill = (lambda seed, *shape: codes(seed, *shape)) if fp8 else (lambda seed, *shape: values(seed, dtype, *shape, amp=1.0))
    view = (lambda t: t.view(F8)) if fp8 else (lambda t: t.view(dtype))
    W, P = Smax // page, 24
    free = [int(e) for e in torch.randperm(P, generator=torch.Generator().manual_seed(2600))]
    table = torch.full((B, W), -1, dtype=torch.int32)
    for b, n in enumerate(start):
        for lp in range((n + page - 1) // page):
            table[b, lp] = free.pop(0)
    mirror_k, mirror_v = (torch.full((P, Hkv, page, D), NANB if fp8 else 0, dtype=raw) for _ in range(2))
    for b, n in enumerate(start):      # the state before the first step: n rows per item
        for x, seed in ((mirror_k, 2601), (mirror_v, 2602)):
            rows = fill(seed + 10 * b, 1, Hkv, n, D)
            for j in range(n):
                x[int(table[b, j // page]), :, j % page] = rows[0, :, j]
    cos, sin = tables(Smax, D)
    dcos, dsin = cos.to(dev), sin.to(dev)
    k, v, dtable = mirror_k.to(dev), mirror_v.to(dev), table.to(dev)
    lens = lens_tensor(start, dev, torch.int64 if fp8 else torch.int32)
    q = torch.zeros((B, Hkv * G, T, D), device=dev, dtype=dtype)
    new_k, new_v = (torch.zeros((B, Hkv, T, D), device=dev, dtype=dtype) for _ in range(2))
    q_out = torch.zeros_like(q)

    def step(k, v, lens, q_out):
        lens.add_(1)
        mm.rope_kv_cache_append_paged(q, new_k, new_v, dcos, dsin, view(k), view(v), dtable, lens, q_out=q_out, **scales)
        return _decode(mm, fp8, page, q_out, k, v, dtable, layout, lens, scales)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(k, v, lens, q_out)  # warm-up on the side stream: the layout's lists are built here; undone below
    torch.cuda.current_stream().wait_stream(s)
    lens.copy_(torch.tensor(start))
    k.copy_(mirror_k)
    v.copy_(mirror_v)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # a host synchronisation in here would fail the capture
        out, lse = step(k, v, lens, q_out)
    torch.cuda.synchronize()
    same(k, mirror_k, "a capture runs nothing")
    lens.copy_(torch.tensor(start))     # (whatever the capture did to it)
    ptrs = (k.data_ptr(), v.data_ptr(), lens.data_ptr(), q.data_ptr(), new_k.data_ptr(), dcos.data_ptr(), q_out.data_ptr())
    host_lens, opened = list(start), 0
    for n in range(4):
        host_lens = [x + 1 for x in host_lens]
        if n == 3:     # the tables are read at every replay: the rows of the next positions are given other angles, in place
            other = tables(Smax, D, base=500.0)
            for b, x in enumerate(host_lens):
                cos[x - 1], sin[x - 1] = other[0][x - 1], other[1][x - 1]
                dcos[x - 1].copy_(cos[x - 1])
                dsin[x - 1].copy_(sin[x - 1])
        q16, k16, v16 = (values(2610 + 10 * i + n, dtype, B, H, T, D, amp=1.0) for i, H in enumerate((Hkv * G, Hkv, Hkv)))
        q.copy_(q16.view(dtype))
        new_k.copy_(k16.view(dtype))
        new_v.copy_(v16.view(dtype))
        for b, x in enumerate(host_lens):
            if (x - 1) % page == 0:  # the new token opens a logical page
                assert int(table[b, (x - 1) // page]) == -1
                table[b, (x - 1) // page] = free.pop(0)
                dtable[b, (x - 1) // page] = int(table[b, (x - 1) // page])
                opened += 1
        k2, v2, lens2, q_out2 = k.clone(), v.clone(), lens.clone(), torch.zeros_like(q_out)
        for t in (out, lse, q_out):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert lens.tolist() == host_lens and ptrs == (k.data_ptr(), v.data_ptr(), lens.data_ptr(), q.data_ptr(), new_k.data_ptr(),
                                                       dcos.data_ptr(), q_out.data_ptr())
        out2, lse2 = step(k2, v2, lens2, q_out2)      # the eager sequence on the copies
        same(q_out.view(torch.int16), q_out2.view(torch.int16), f"replay {n}: q_out of the eager call")
        same(k, k2, f"replay {n}: k of the eager call")
        same(v, v2, f"replay {n}: v of the eager call")
        assert_same_bits(out, out2, f"replay {n}: out of the eager sequence")
        assert_same_bits(lse, lse2, f"replay {n}: lse of the eager sequence")
        want_q, k_rot, token = yardstick(dtype, q16, k16, cos, sin, host_lens, D, False)
        sc = (scales["k_scale"], scales["v_scale"]) if fp8 else None
        assert expected_cache(mm, dtype, mirror_k, mirror_v, k_rot, v16, host_lens, token, D, table, sc)[0] == B
        same(q_out.view(torch.int16), want_q, f"replay {n}, k_lens {host_lens}: q_out")
        same(k, mirror_k, f"replay {n}, k_lens {host_lens}: k")
        same(v, mirror_v, f"replay {n}, k_lens {host_lens}: v")
        assert torch.isfinite(out.float()).all() and out.float().abs().max() > 0
        if n == 3:
            stale = yardstick(dtype, q16, k16, *tables(Smax, D), host_lens, D, False)[0]
            assert not torch.equal(stale, want_q)
    assert host_lens == [66, 130] and opened == 2
