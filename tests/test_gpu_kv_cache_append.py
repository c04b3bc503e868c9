"""matmuls.kv_cache_append and kv_cache_append_paged on the MI355X: the write side of the four decode calls.
The contract is on bits.  A 2-byte cache receives bit copies; an fp8 cache the bytes of kv_to_fp8 as torch computes them ON
THE CPU (no fp8 operator of torch runs on the device: fp8 data moves through uint8 views); token t of item b goes to
k_lens[b] − T + t or nowhere; and everything else keeps its bytes — so every test compares the WHOLE cache, pool or underlying
buffer with one built on the CPU by `place` below, which knows the rule and nothing of the kernel.

B · Hkv ≤ 8, Smax ≤ 512."""
import ctypes

import pytest
import torch

from gpu_helpers import SENTINEL, assert_same_bits, padded
from test_gpu_block_attention_decode import ROWS, layout_from_rows, lens_tensor
from test_gpu_block_attention_decode_paged import gathered, scatter

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn
NANB = 0x7F
WIDTHS = [32, 64, 96, 128]
DTYPES = [torch.bfloat16, torch.float16]
SPECIALS = {torch.bfloat16: [0x7FC1, 0xFFFF, 0x7F81, 0x8000, 0x0001, 0x7F80, 0xFF80],   # NaN payloads, −0, a subnormal, ±inf
            torch.float16: [0x7E01, 0xFFFF, 0x7C01, 0x8000, 0x0001, 0x7C00, 0xFC00]}


def i16(values):
    """Python ints 0 … 65535 as the int16 of those bits."""
    t = torch.as_tensor(values, dtype=torch.int64)
    return (t - 65536 * (t >= 32768)).to(torch.int16)


def patterns(seed, dtype, *shape):
    """Raw 16-bit patterns, int16 on the CPU: uniform over all 65 536, the specials of `dtype` in front."""
    x = torch.randint(-32768, 32768, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.int16)
    x.reshape(-1)[:len(SPECIALS[dtype])] = i16(SPECIALS[dtype])
    return x


def values(seed, dtype, *shape, amp=3.0):
    """Finite values of moderate size in `dtype`, as int16 bits on the CPU."""
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * amp).to(dtype).view(torch.int16)


def codes(seed, *shape):
    """Random e4m3fn bytes that are no NaN code, uint8 on the CPU: what an fp8 cache holds before the append."""
    c = torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.int16).to(torch.uint8)
    return torch.where(c & 0x7F == NANB, torch.tensor(0x3A, dtype=torch.uint8), c)


def quantised(mm, rows16, dtype, scale=None):
    """The bytes of kv_to_fp8 on the CPU for the int16 bits rows16 [B, Hkv, T, D] of `dtype`; scale None: 1."""
    s = 1.0 if scale is None else (scale.cpu() if isinstance(scale, torch.Tensor) else scale)
    return mm.kv_to_fp8(rows16.view(dtype), s)[0].view(torch.uint8)


def place(cache, rows, k_lens, table=None):
    """The rule, on CPU tensors of raw integers: rows [B, Hkv, T, D] written into cache [B, Hkv, Smax, D] — or, with a table
    [B, W], into the pool [P, Hkv, page, D] — in place; returns the number of (item, token) pairs written."""
    B, _, T, _ = rows.shape
    page = cache.shape[2]
    smax = page if table is None else page * table.shape[1]
    lens = [k_lens] * B if isinstance(k_lens, int) else list(k_lens)
    written = 0
    for b in range(B):
        for t in range(T):
            pos = lens[b] - T + t
            if not 0 <= pos < smax:
                continue
            if table is None:
                cache[b, :, pos] = rows[b, :, t]
            else:
                e = int(table[b, pos // page])
                if not 0 <= e < cache.shape[0]:
                    continue
                cache[e, :, pos % page] = rows[b, :, t]
            written += 1
    return written


def same_raw(got, want, what):
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = torch.nonzero(got != want)
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} of {got.numel()} elements differ, first at {bad[:4].tolist()}: got " \
                             f"{[int(got[tuple(i)]) for i in bad[:4]]} want {[int(want[tuple(i)]) for i in bad[:4]]}"


# ---- 1. copy bits, flat --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", WIDTHS)
def test_1_a_two_byte_cache_receives_bit_copies(mm, dev, dtype, D):
    B, Hkv, T, Smax, k_lens = 2, 2, 3, 256, [200, 65]
    cache_k, cache_v = patterns(2310 + D, dtype, B, Hkv, Smax, D), patterns(2311 + D, dtype, B, Hkv, Smax, D)
    new_k, new_v = patterns(2312 + D, dtype, B, Hkv, T, D), patterns(2313 + D, dtype, B, Hkv, T, D)
    assert torch.isnan(new_k.view(dtype).float()).sum() >= 3 and (new_k == -32768).any()        # NaN payloads and −0 are in
    k, v = cache_k.to(dev).view(dtype), cache_v.to(dev).view(dtype)
    assert mm.kv_cache_append(new_k.to(dev).view(dtype), new_v.to(dev).view(dtype), k, v, lens_tensor(k_lens, dev)) is None
    assert place(cache_k, new_k, k_lens) == 6 and place(cache_v, new_v, k_lens) == 6
    same_raw(k.view(torch.int16), cache_k, f"{dtype} D={D}: k")
    same_raw(v.view(torch.int16), cache_v, f"{dtype} D={D}: v")
    assert torch.equal(cache_k[0, :, 197:200], new_k[0]) and torch.equal(cache_v[1, :, 62:65], new_v[1])


# ---- 2. strides ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,D,fp8", [(torch.bfloat16, 128, False), (torch.float16, 96, False), (torch.bfloat16, 64, True),
                                         (torch.float16, 32, True)])
def test_2_source_and_cache_are_read_through_their_own_strides(mm, dev, dtype, D, fp8):
    """k_new and v_new are slices of ONE fused projection [B, T, Hq + 2·Hkv, D]; the cache is a [B, Smax, Hkv, D] buffer seen
    through .transpose(1, 2), then a buffer with a row stride of D + 8 (16 for fp8) whose gaps hold sentinels.  The whole
    underlying buffers are compared: the gaps stay untouched."""
    B, Hkv, Hq, T, Smax, k_lens = 2, 2, 4, 3, 128, [100, 3]
    qkv = values(2320 + D, dtype, B, T, Hq + 2 * Hkv, D)
    new_k, new_v = (qkv[:, :, lo:lo + Hkv].transpose(1, 2) for lo in (Hq, Hq + Hkv))
    dqkv = qkv.to(dev).view(dtype)
    dk, dv = (dqkv[:, :, lo:lo + Hkv].transpose(1, 2) for lo in (Hq, Hq + Hkv))
    assert not dk.is_contiguous() and dk.data_ptr() != dv.data_ptr()
    raw, pad = (torch.uint8, 16) if fp8 else (torch.int16, 8)
    ks, vs = (torch.tensor([0.5, 3.0], device=dev), torch.tensor(0.3, device=dev)) if fp8 else (None, None)
    rows_k = quantised(mm, new_k.contiguous(), dtype, ks) if fp8 else new_k
    rows_v = quantised(mm, new_v.contiguous(), dtype, vs) if fp8 else new_v
    scales = dict(k_scale=ks, v_scale=vs) if fp8 else {}
    fill = (lambda seed, *shape: codes(seed, *shape)) if fp8 else (lambda seed, *shape: values(seed, dtype, *shape))
    view = (lambda t: t.view(F8)) if fp8 else (lambda t: t.view(dtype))
    for form in ("BSHD", "padded rows"):
        if form == "BSHD":
            bufs = [fill(2321 + i, B, Smax, Hkv, D) for i in range(2)]
            logical = lambda t: t.transpose(1, 2)  # noqa: E731
        else:
            bufs = [fill(2323 + i, B, Hkv, Smax, D + pad) for i in range(2)]
            for t in bufs:
                t[..., D:] = 0x55
            logical = lambda t: t[..., :D]  # noqa: E731
        dbufs = [t.to(dev) for t in bufs]
        k, v = (logical(view(t)) for t in dbufs)
        assert not k.is_contiguous()
        mm.kv_cache_append(dk, dv, k, v, lens_tensor(k_lens, dev), **scales)
        assert place(logical(bufs[0]), rows_k, k_lens) == 6 and place(logical(bufs[1]), rows_v, k_lens) == 6
        same_raw(dbufs[0], bufs[0], f"{form} {dtype} fp8={fp8}: the k buffer")
        same_raw(dbufs[1], bufs[1], f"{form} {dtype} fp8={fp8}: the v buffer")
    same_raw(dqkv.view(torch.int16), qkv, "the source is only read")


# ---- 3. edges ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fp8", [False, True])
def test_3_lengths_at_and_beyond_both_ends_drop_tokens_and_move_nothing(mm, dev, fp8):
    Hkv, T, D, Smax, dtype = 2, 3, 64, 64, torch.float16
    cases = [([0, 1, Smax, Smax + 2], torch.int32, [0, 1, 3, 1]),          # nothing; the last token at row 0; the last rows; one of three
             ([2, Smax + 1, Smax + 3, 3], torch.int64, [2, 2, 0, 3]),
             ([-5, 2 ** 31 - 1, Smax + 40, -2 ** 31], torch.int32, [0, 0, 0, 0]),      # no wrap at either end of int32
             (5, torch.int32, [3, 3, 3, 3]), (Smax + 1, torch.int64, [2, 2, 2, 2])]    # 0-d: one length for every item
    for n, (k_lens, lens_dtype, written) in enumerate(cases):
        B = 4
        new_k, new_v = values(2330 + n, dtype, B, Hkv, T, D), values(2340 + n, dtype, B, Hkv, T, D)
        if fp8:
            cache_k, cache_v = codes(2350 + n, B, Hkv, Smax, D), codes(2360 + n, B, Hkv, Smax, D)
            rows_k, rows_v = quantised(mm, new_k, dtype), quantised(mm, new_v, dtype)
            k, v = cache_k.to(dev).view(F8), cache_v.to(dev).view(F8)
        else:
            cache_k, cache_v = values(2350 + n, dtype, B, Hkv, Smax, D), values(2360 + n, dtype, B, Hkv, Smax, D)
            rows_k, rows_v = new_k, new_v
            k, v = cache_k.to(dev).view(dtype), cache_v.to(dev).view(dtype)
        lens = torch.tensor(k_lens, device=dev, dtype=lens_dtype)
        assert lens.dim() == (0 if isinstance(k_lens, int) else 1)
        before = cache_k.clone()
        mm.kv_cache_append(new_k.to(dev).view(dtype), new_v.to(dev).view(dtype), k, v, lens)
        assert place(cache_k, rows_k, k_lens) == sum(written) == place(cache_v, rows_v, k_lens)
        changed = (cache_k != before).any(-1).any(1).sum(-1).tolist()       # rows per item that the rule rewrote
        assert changed == written, (k_lens, changed)
        raw = torch.uint8 if fp8 else torch.int16
        same_raw(k.view(raw), cache_k, f"k_lens {k_lens} fp8={fp8}: k")
        same_raw(v.view(raw), cache_v, f"k_lens {k_lens} fp8={fp8}: v")
    assert torch.equal(cache_k[0, :, Smax - 2:], rows_k[0, :, :2])         # (the last case: tokens 0 and 1 at the last rows)


# ---- 4. paged ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("page,D,dtype", [(page, D, DTYPES[(i + j) % 2]) for i, page in enumerate([16, 64, 256]) for j, D in enumerate(WIDTHS)])
def test_4_pages_tables_and_entries_outside_the_pool(mm, dev, page, D, dtype):
    """Three items whose three tokens straddle rows 15|16, 63|64 and 255|256; a shuffled table; three pages more than are
    referenced.  Both cache types.  Then the table entry of a written position is −1 for one item and P for another: those
    tokens are dropped.  An int64 table and a [B, Wmax][:, :W] slice give the same pool."""
    B, Hkv, T, Smax, k_lens = 3, 2, 3, 512, [18, 66, 258]
    W = Smax // page
    P = B * W + 3
    table = torch.randperm(P, generator=torch.Generator().manual_seed(2370 + page))[:B * W].reshape(B, W).to(torch.int32)
    holes = table.clone()
    holes[0, 15 // page], holes[1, 65 // page] = -1, P
    new_k, new_v = values(2371 + D, dtype, B, Hkv, T, D), values(2372 + D, dtype, B, Hkv, T, D)
    ks, vs = torch.tensor([0.7, 2.5], device=dev), torch.tensor([0.11], device=dev)
    dnew_k, dnew_v = new_k.to(dev).view(dtype), new_v.to(dev).view(dtype)
    for fp8 in (False, True):
        if fp8:
            pool_k, pool_v = (torch.full((P, Hkv, page, D), NANB, dtype=torch.uint8) for _ in range(2))
            scatter(pool_k, table, codes(2373 + D, B, Hkv, Smax, D))
            scatter(pool_v, table, codes(2374 + D, B, Hkv, Smax, D))
            rows_k, rows_v, view, raw = quantised(mm, new_k, dtype, ks), quantised(mm, new_v, dtype, vs), (lambda t: t.view(F8)), torch.uint8
            scales = dict(k_scale=ks, v_scale=vs)
        else:
            pool_k, pool_v = (torch.full((P, Hkv, page, D), 0x7FFF, dtype=torch.int16) for _ in range(2))    # a NaN of both types
            scatter(pool_k, table, values(2373 + D, dtype, B, Hkv, Smax, D))
            scatter(pool_v, table, values(2374 + D, dtype, B, Hkv, Smax, D))
            rows_k, rows_v, view, raw, scales = new_k, new_v, (lambda t: t.view(dtype)), torch.int16, {}
        wide = torch.full((B, W + 5), -1, dtype=torch.int32)
        wide[:, :W] = table
        for what, tab, dtab in (("int32", table, table.to(dev)), ("holes", holes, holes.to(dev)), ("int64", table, table.to(dev).long()),
                                ("a slice", table, wide.to(dev)[:, :W])):
            want_k, want_v = pool_k.clone(), pool_v.clone()
            kp, vp = pool_k.to(dev), pool_v.to(dev)
            assert mm.kv_cache_append_paged(dnew_k, dnew_v, view(kp), view(vp), dtab, lens_tensor(k_lens, dev), **scales) is None
            n = place(want_k, rows_k, k_lens, tab)
            place(want_v, rows_v, k_lens, tab)
            dropped = 0
            if what == "holes":   # item 0 loses the tokens of the logical page of row 15, item 1 those of the page of row 65
                dropped = sum(1 for p in (15, 16, 17) if p // page == 15 // page) + sum(1 for p in (63, 64, 65) if p // page == 65 // page)
            assert n == 9 - dropped and (what != "holes" or dropped >= 2)
            same_raw(kp, want_k, f"page={page} D={D} {dtype} fp8={fp8} {what}: the k pool")
            same_raw(vp, want_v, f"page={page} D={D} {dtype} fp8={fp8} {what}: the v pool")
        unreferenced = [e for e in range(P) if e not in table.reshape(-1).tolist()]
        assert len(unreferenced) == 3 and (want_k[unreferenced] == (NANB if fp8 else 0x7FFF)).all()


# ---- 5. every input, fp8 -------------------------------------------------------------------------------------------------------------

ALL = i16(range(65536))
SCALES = (1.0, 3.0, 0.3, 2.0 ** -7)


@pytest.mark.parametrize("dtype", DTYPES)
def test_5_the_cpu_reference_covers_every_code_every_tie_and_tells_rounding_from_truncation(mm, dtype):
    """What makes test 5 a test, checked on the CPU: at each scale the reference bytes of the 65 536 patterns take all 256
    values; at scale 1 the patterns hold every midpoint of two neighbouring codes, and the reference sends it to the even
    one; and round-to-nearest differs from truncation on thousands of patterns."""
    x = ALL.reshape(1, 1, 65536, 1)
    nan = torch.isnan(x.view(dtype).float()).reshape(-1)
    for s in SCALES:
        b = quantised(mm, x, dtype, s).reshape(-1)
        assert b.unique().numel() == 256 and (b[nan] & 0x7F == NANB).all() and not (b[~nan] & 0x7F == NANB).any(), s
    b = quantised(mm, x, dtype).reshape(-1)
    grid = torch.arange(127, dtype=torch.uint8).view(F8).float()        # the codes 0x00 … 0x7E: 0 … 448, ascending
    y = x.view(dtype).float().reshape(-1)[~nan].clamp(-448.0, 448.0)
    truncated = (torch.searchsorted(grid, y.abs(), right=True) - 1).to(torch.uint8) | (torch.signbit(y).to(torch.uint8) << 7)
    differ = int((truncated != b[~nan]).sum())
    assert differ > (2000 if dtype == torch.bfloat16 else 17000), differ
    mids = (grid[1:] + grid[:-1]) / 2
    ties = torch.cat([mids, -mids])
    assert torch.equal(ties.to(dtype).float(), ties) and torch.isin(ties.to(dtype).view(torch.int16), ALL).all()
    at_ties = quantised(mm, ties.to(dtype).view(torch.int16).reshape(1, 1, -1, 1), dtype).reshape(-1)
    assert (at_ties & 1 == 0).all() and ties.numel() == 252


@pytest.mark.parametrize("page", [0, 16])
@pytest.mark.parametrize("dtype", DTYPES)
def test_5_every_bit_pattern_of_the_source_at_four_scales(mm, dev, dtype, page):
    """All 65 536 patterns of `dtype` as k_new [1, 2, 256, 128] — head 0 the positive half, head 1 the negative — and as v_new
    with the heads swapped and each head shuffled, in ONE call; two calls with per-head scales chosen so that every pattern
    meets 1, 3, 0.3 and 2⁻⁷.  Bytes equal the CPU's wherever the source is no NaN; a NaN code stands where it is one."""
    Hkv, T, D = 2, 256, 128
    new_k = ALL.reshape(1, Hkv, T, D).clone()
    perm = torch.randperm(32768, generator=torch.Generator().manual_seed(2380))
    new_v = torch.stack([ALL[32768:][perm], ALL[:32768][perm]]).reshape(1, Hkv, T, D)
    dnew_k, dnew_v = new_k.to(dev).view(dtype), new_v.to(dev).view(dtype)
    lens = lens_tensor([T], dev)
    met = torch.zeros(65536, 4, dtype=torch.bool)
    for call, (ks, vs) in enumerate((([1.0, 3.0], [0.3, 2.0 ** -7]), ([0.3, 2.0 ** -7], [1.0, 3.0]))):
        if page:
            P = T // page + 3
            table = torch.randperm(P, generator=torch.Generator().manual_seed(2381 + call))[:T // page].reshape(1, -1).to(torch.int32)
            k, v = (torch.full((P, Hkv, page, D), NANB, dtype=torch.uint8, device=dev) for _ in range(2))
            mm.kv_cache_append_paged(dnew_k, dnew_v, k.view(F8), v.view(F8), table.to(dev), lens, k_scale=torch.tensor(ks, device=dev),
                                     v_scale=torch.tensor(vs, device=dev))
            assert (k[[e for e in range(P) if e not in table.reshape(-1).tolist()]] == NANB).all()
            got_k, got_v = gathered(k.cpu(), table), gathered(v.cpu(), table)
        else:
            k, v = (torch.full((1, Hkv, T, D), NANB, dtype=torch.uint8, device=dev) for _ in range(2))
            mm.kv_cache_append(dnew_k, dnew_v, k.view(F8), v.view(F8), lens, k_scale=torch.tensor(ks, device=dev),
                               v_scale=torch.tensor(vs, device=dev))
            got_k, got_v = k.cpu(), v.cpu()
        for what, got, new, scale in (("k", got_k, new_k, ks), ("v", got_v, new_v, vs)):
            want = quantised(mm, new, dtype, torch.tensor(scale))
            nan = torch.isnan(new.view(dtype).float())
            assert (got[nan] & 0x7F == NANB).all(), f"{dtype} page={page} call {call}: a NaN of {what}_new is a NaN code"
            bad = torch.nonzero((got != want) & ~nan)
            first = [(hex(int(new[tuple(i)]) & 0xFFFF), scale[int(i[1])], int(got[tuple(i)]), int(want[tuple(i)])) for i in bad[:6]]
            assert bad.numel() == 0, f"{dtype} page={page} call {call} {what}: {bad.shape[0]} bytes differ; (pattern, scale, got, want): {first}"
            for h in range(Hkv):
                met[new[0, h].reshape(-1).long() & 0xFFFF, SCALES.index(scale[h])] = True
    assert met.all()


# ---- 6. scale forms ------------------------------------------------------------------------------------------------------------------

def test_6_every_form_of_a_scale_and_a_scale_changed_in_place(mm, dev):
    B, Hkv, T, D, Smax, dtype, k_lens = 2, 2, 3, 64, 64, torch.bfloat16, [10, 64]
    new_k, new_v = values(2390, dtype, B, Hkv, T, D, amp=40.0), values(2391, dtype, B, Hkv, T, D, amp=40.0)
    dnew_k, dnew_v, lens = new_k.to(dev).view(dtype), new_v.to(dev).view(dtype), lens_tensor(k_lens, dev)
    per_head = torch.tensor([0.3, 7.0], device=dev)
    forms = [(None, None), (0.3, 3), (torch.tensor(0.3, device=dev), torch.tensor([7.0], device=dev)), (per_head, None),
             (None, per_head.flip(0).contiguous())]
    for ks, vs in forms:
        base_k, base_v = codes(2392, B, Hkv, Smax, D), codes(2393, B, Hkv, Smax, D)
        k, v = base_k.to(dev), base_v.to(dev)
        mm.kv_cache_append(dnew_k, dnew_v, k.view(F8), v.view(F8), lens, k_scale=ks, v_scale=vs)
        place(base_k, quantised(mm, new_k, dtype, ks), k_lens)
        place(base_v, quantised(mm, new_v, dtype, vs), k_lens)
        same_raw(k, base_k, f"k_scale {ks}")
        same_raw(v, base_v, f"v_scale {vs}")
    # the scale is read on the device at every call: a tensor changed in place is followed
    first = k.clone()
    mm.kv_cache_append(dnew_k, dnew_v, k.view(F8), v.view(F8), lens, k_scale=per_head)
    per_head.mul_(2.5)
    ptr = per_head.data_ptr()
    mm.kv_cache_append(dnew_k, dnew_v, k.view(F8), v.view(F8), lens, k_scale=per_head)
    assert per_head.data_ptr() == ptr
    place(base_k, quantised(mm, new_k, dtype, per_head), k_lens)
    same_raw(k, base_k, "after k_scale.mul_(2.5)")
    assert not torch.equal(first, k)


# ---- 7. round trip -------------------------------------------------------------------------------------------------------------------

def _decode(mm, fp8, page, q, k, v, table, layout, lens, scales):
    """The decode call that matches the cache form; k, v raw device tensors (int16 / uint8); returns (out, lse)."""
    kk, vv = (k.view(F8), v.view(F8)) if fp8 else (k.view(q.dtype), v.view(q.dtype))
    kw = dict(chunk=2, return_lse=True, **(scales if fp8 else {}))
    if page:
        f = mm.block_sparse_attention_decode_paged_fp8 if fp8 else mm.block_sparse_attention_decode_paged
        return f(q, kk, vv, table, layout, lens, **kw)
    f = mm.block_sparse_attention_decode_fp8 if fp8 else mm.block_sparse_attention_decode
    return f(q, kk, vv, layout, lens, **kw)


@pytest.mark.parametrize("fp8,page,dtype", [(False, 0, torch.bfloat16), (False, 64, torch.float16), (True, 0, torch.float16),
                                            (True, 16, torch.bfloat16)])
def test_7_append_then_decode_has_the_bits_of_decode_on_the_cpu_built_cache(mm, dev, fp8, page, dtype):
    B, Hkv, G, T, D, Smax, k_lens = 2, 2, 2, 3, 64, 512, [200, 65]
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q = torch.randn((B, Hkv * G, T, D), generator=torch.Generator().manual_seed(2400)).to(dtype).to(dev)
    new_k, new_v = values(2401, dtype, B, Hkv, T, D, amp=1.0), values(2402, dtype, B, Hkv, T, D, amp=1.0)
    scales = dict(k_scale=torch.tensor([0.02, 0.03], device=dev), v_scale=torch.tensor(0.025, device=dev))
    if fp8:
        flat_k, flat_v = codes(2403, B, Hkv, Smax, D), codes(2404, B, Hkv, Smax, D)
        rows_k, rows_v = quantised(mm, new_k, dtype, scales["k_scale"]), quantised(mm, new_v, dtype, scales["v_scale"])
    else:
        flat_k, flat_v = values(2403, dtype, B, Hkv, Smax, D, amp=1.0), values(2404, dtype, B, Hkv, Smax, D, amp=1.0)
        rows_k, rows_v = new_k, new_v
    table = dtable = None
    if page:
        W = Smax // page
        P = B * W + 3
        table = torch.randperm(P, generator=torch.Generator().manual_seed(2405))[:B * W].reshape(B, W).to(torch.int32)
        dtable = table.to(dev)
        cpu_k, cpu_v = (torch.zeros((P, Hkv, page, D), dtype=flat_k.dtype) for _ in range(2))
        scatter(cpu_k, table, flat_k)
        scatter(cpu_v, table, flat_v)
    else:
        cpu_k, cpu_v = flat_k, flat_v
    k, v = cpu_k.to(dev), cpu_v.to(dev)
    view = (lambda t: t.view(F8)) if fp8 else (lambda t: t.view(dtype))
    args = (new_k.to(dev).view(dtype), new_v.to(dev).view(dtype), view(k), view(v))
    if page:
        mm.kv_cache_append_paged(*args, dtable, lens, **(scales if fp8 else {}))
    else:
        mm.kv_cache_append(*args, lens, **(scales if fp8 else {}))
    got = _decode(mm, fp8, page, q, k, v, dtable, layout, lens, scales)
    assert place(cpu_k, rows_k, k_lens, table) == 6 and place(cpu_v, rows_v, k_lens, table) == 6
    same_raw(k, cpu_k, "the cache after the append")
    want = _decode(mm, fp8, page, q, cpu_k.to(dev), cpu_v.to(dev), dtable, layout, lens, scales)
    assert_same_bits(got[0], want[0], f"fp8={fp8} page={page}: out")
    assert_same_bits(got[1], want[1], f"fp8={fp8} page={page}: lse")
    assert torch.isfinite(got[0].float()).all() and got[0].float().abs().max() > 0


# ---- 8. one graph per step ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fp8,page,dtype", [(False, 0, torch.bfloat16), (True, 16, torch.float16)])
def test_8_one_captured_graph_advances_appends_and_attends(mm, dev, fp8, page, dtype):
    """`lens += 1; append; decode` captured ONCE.  Before a replay q, k_new and v_new are refilled in place — and, paged, the
    table entry of a page that the new token opens is assigned in place —; three replays take one item through 63 → 64 and
    the other through 127 → 128.  After every replay the cache equals a CPU mirror bit for bit and out, lse are those of the
    eager decode call on the uploaded mirror."""
    B, Hkv, G, T, D, Smax, start = 2, 2, 2, 1, 64, 512, [62, 126]
    layout = layout_from_rows(ROWS, dev)
    scales = dict(k_scale=torch.tensor([0.02, 0.03], device=dev), v_scale=torch.tensor([0.025], device=dev)) if fp8 else {}
    raw = torch.uint8 if fp8 else torch.int16
    fill = (lambda seed, *shape: codes(seed, *shape)) if fp8 else (lambda seed, *shape: values(seed, dtype, *shape, amp=1.0))
    table = free = None
    if page:
        W, P = Smax // page, 24
        free = [int(e) for e in torch.randperm(P, generator=torch.Generator().manual_seed(2410))]
        table = torch.full((B, W), -1, dtype=torch.int32)
        for b, n in enumerate(start):
            for lp in range((n + page - 1) // page):
                table[b, lp] = free.pop(0)
        mirror_k, mirror_v = (torch.full((P, Hkv, page, D), NANB, dtype=torch.uint8) for _ in range(2))
    else:
        mirror_k, mirror_v = (torch.zeros((B, Hkv, Smax, D), dtype=raw) for _ in range(2))
    for b, n in enumerate(start):      # the state before the first step: n rows per item
        for x, seed in ((mirror_k, 2411), (mirror_v, 2412)):
            rows = fill(seed + 10 * b, 1, Hkv, n, D)
            if page:
                for j in range(n):
                    x[int(table[b, j // page]), :, j % page] = rows[0, :, j]
            else:
                x[b, :, :n] = rows[0]
    view = (lambda t: t.view(F8)) if fp8 else (lambda t: t.view(dtype))
    k, v = mirror_k.to(dev), mirror_v.to(dev)
    dtable = table.to(dev) if page else None
    lens = lens_tensor(start, dev, torch.int64 if fp8 else torch.int32)
    q = torch.zeros((B, Hkv * G, T, D), device=dev, dtype=dtype)
    new_k, new_v = (torch.zeros((B, Hkv, T, D), device=dev, dtype=dtype) for _ in range(2))

    def step():
        lens.add_(1)
        if page:
            mm.kv_cache_append_paged(new_k, new_v, view(k), view(v), dtable, lens, **scales)
        else:
            mm.kv_cache_append(new_k, new_v, view(k), view(v), lens)
        return _decode(mm, fp8, page, q, k, v, dtable, layout, lens, scales)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()  # warm-up on the side stream: the layout's lists are built here; it appends a zero row, undone below
    torch.cuda.current_stream().wait_stream(s)
    lens.copy_(torch.tensor(start))
    k.copy_(mirror_k)
    v.copy_(mirror_v)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # a host synchronisation in here would fail the capture
        out, lse = step()
    torch.cuda.synchronize()
    same_raw(k, mirror_k, "a capture runs nothing")
    lens.copy_(torch.tensor(start))     # (whatever the capture did to it)
    ptrs = (k.data_ptr(), v.data_ptr(), lens.data_ptr(), q.data_ptr(), new_k.data_ptr())
    host_lens, opened = list(start), 0
    for n in range(3):
        host_lens = [x + 1 for x in host_lens]
        rows_k16, rows_v16 = values(2420 + n, dtype, B, Hkv, T, D, amp=1.0), values(2430 + n, dtype, B, Hkv, T, D, amp=1.0)
        new_k.copy_(rows_k16.view(dtype))
        new_v.copy_(rows_v16.view(dtype))
        q.copy_(torch.randn((B, Hkv * G, T, D), generator=torch.Generator().manual_seed(2440 + n)).to(dtype))
        if page:
            for b, x in enumerate(host_lens):
                if (x - 1) % page == 0:  # the new token opens a logical page
                    assert int(table[b, (x - 1) // page]) == -1
                    table[b, (x - 1) // page] = free.pop(0)
                    dtable[b, (x - 1) // page] = int(table[b, (x - 1) // page])
                    opened += 1
        rows_k = quantised(mm, rows_k16, dtype, scales["k_scale"]) if fp8 else rows_k16
        rows_v = quantised(mm, rows_v16, dtype, scales["v_scale"]) if fp8 else rows_v16
        assert place(mirror_k, rows_k, host_lens, table) == B and place(mirror_v, rows_v, host_lens, table) == B
        out.fill_(float("nan"))
        lse.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert lens.tolist() == host_lens and (k.data_ptr(), v.data_ptr(), lens.data_ptr(), q.data_ptr(), new_k.data_ptr()) == ptrs
        same_raw(k, mirror_k, f"replay {n}, k_lens {host_lens}: k")
        same_raw(v, mirror_v, f"replay {n}, k_lens {host_lens}: v")
        want = _decode(mm, fp8, page, q, mirror_k.to(dev), mirror_v.to(dev), dtable, layout, lens_tensor(host_lens, dev), scales)
        assert_same_bits(out, want[0], f"replay {n}: out of the eager decode on the uploaded mirror")
        assert_same_bits(lse, want[1], f"replay {n}: lse")
        assert torch.isfinite(out.float()).all() and out.float().abs().max() > 0
    assert host_lens == [65, 129] and opened == (2 if page else 0)


# ---- 9. the C ABI --------------------------------------------------------------------------------------------------------------------

def _append_entry(capi, name):
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    fn = getattr(capi, name)
    table = [vp, i64, i32, i32] if "paged" in name else []
    scales = [vp, i32, vp, i32] if "fp8" in name else []
    fn.argtypes = 4 * [i32] + table + [i32] + 4 * [vp, i64, i64, i64] + [vp, i32] + scales + [vp]
    fn.restype = ctypes.c_int
    return fn


@pytest.mark.parametrize("name,dtype,D", [("mi_kv_append_b16", torch.bfloat16, 96), ("mi_kv_append_paged_b16", torch.float16, 32),
                                          ("mi_kv_append_fp8_f16", torch.float16, 128), ("mi_kv_append_paged_fp8_bf16", torch.bfloat16, 64)])
def test_9_c_abi_refusals_and_one_padded_call(mm, capi, dev, name, dtype, D):
    """MI_EINVAL without a launch (the cache keeps its bytes), then one call with every pointer inside an allocation of its
    own: leading dimensions and strides different for every operand, SENTINEL bits around the source rows, the cache rows,
    the table and the lengths — the padded buffers equal the CPU's, inside and outside."""
    paged, fp8 = "paged" in name, "fp8" in name
    B, Hkv, T, k_lens = 2, 2, 3, [18, 66]
    page = 16 if paged else 0
    Smax = 128
    W = Smax // page if paged else 0
    outer = B * W + 3 if paged else B
    rows = page if paged else Smax
    items = B * Hkv
    fn = _append_entry(capi, name)
    new_k, new_v = values(2450 + D, dtype, B, Hkv, T, D), values(2451 + D, dtype, B, Hkv, T, D)
    pnk, pnv = (padded(x.to(dev).view(dtype).reshape(items, T, D), i, SENTINEL) for i, x in ((0, new_k), (1, new_v)))
    if fp8:
        cache = [codes(2452 + D + i, outer, Hkv, rows, D) for i in range(2)]
        pk, pv = (padded(x.to(dev).reshape(outer * Hkv, rows, D), 2 + i, 0x55, step=16) for i, x in enumerate(cache))
        ks, vs = torch.tensor([0.4, 2.0], device=dev), torch.tensor([1.5], device=dev)
        rows_k, rows_v = quantised(mm, new_k, dtype, ks), quantised(mm, new_v, dtype, vs)
        scales = (ks.data_ptr(), Hkv, vs.data_ptr(), 1)
    else:
        cache = [values(2452 + D + i, dtype, outer, Hkv, rows, D) for i in range(2)]
        pk, pv = (padded(x.to(dev).view(dtype).reshape(outer * Hkv, rows, D), 2 + i, SENTINEL) for i, x in enumerate(cache))
        rows_k, rows_v, scales = new_k, new_v, ()
    table = None
    ptable = torch.full((B, W + 3), 2 ** 31 - 1, dtype=torch.int32, device=dev)
    if paged:
        table = torch.randperm(outer, generator=torch.Generator().manual_seed(2454))[:B * W].reshape(B, W).to(torch.int32)
        ptable[:, :W] = table.to(dev)
    lens_buf = torch.full((B + 8,), 2 ** 31 - 1, dtype=torch.int32, device=dev)
    lens_buf[4:4 + B] = torch.tensor(k_lens, dtype=torch.int32, device=dev)
    lens_ptr = lens_buf.data_ptr() + 16
    stream = torch.cuda.current_stream().cuda_stream
    before = (pk.buf.clone(), pv.buf.clone())

    def call(items=items, heads=Hkv, T=T, Smax=Smax, D=D, k_new=pnk.buf.data_ptr(), ldkn=pnk.ld, headKn=pnk.stride, k=pk.buf.data_ptr(),
             ldk=pk.ld, headK=pk.stride, lens_count=B, page=page, pages=outer, table_ld=W + 3):
        tab = (ptable.data_ptr(), table_ld, pages, page) if paged else ()
        return fn(items, heads, T, Smax, *tab, D, k_new, ldkn, headKn, Hkv * pnk.stride, pnv.buf.data_ptr(), pnv.ld, pnv.stride,
                  Hkv * pnv.stride, k, ldk, headK, Hkv * pk.stride, pv.buf.data_ptr(), pv.ld, pv.stride, Hkv * pv.stride, lens_ptr,
                  lens_count, *scales, stream)

    unit = 16 if fp8 else 8
    assert pk.ld % unit == 0 and pk.stride % unit == 0 and pv.stride % unit == 0 and pnk.stride % 8 == 0
    for kw in ({"D": 48}, {"items": -1}, {"items": 65536}, {"heads": 3}, {"T": -1}, {"Smax": -16}, {"lens_count": 3}, {"lens_count": 0},
               {"k_new": pnk.buf.data_ptr() + 2}, {"ldkn": pnk.ld + 4}, {"headKn": pnk.stride + 4}, {"k": pk.buf.data_ptr() + 8},
               {"ldk": D - unit}, {"ldk": pk.ld + unit // 2}, {"headK": pk.stride + unit // 2}):
        assert call(**kw) == -1, kw   # MI_EINVAL
    if paged:
        for kw in ({"page": 8}, {"page": 24}, {"pages": -1}, {"table_ld": W - 1}):
            assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert torch.equal(pk.buf, before[0]) and torch.equal(pv.buf, before[1]), "a refused call launches nothing"
    assert call() == 0
    torch.cuda.synchronize()
    raw = torch.uint8 if fp8 else torch.int16
    for p, x, r, what in ((pk, cache[0], rows_k, "k"), (pv, cache[1], rows_v, "v")):
        assert place(x, r, k_lens, table) == 6
        want = p.buf.cpu().view(raw).clone()
        want.as_strided(p.x.shape, p.x.stride()).copy_(x.reshape(p.x.shape))     # the CPU's logical region inside the device's padding …
        same_raw(p.buf.view(raw), want, f"{name}: the padded {what} buffer")       # … equals the buffer: inside the rule, outside untouched
    same_raw(torch.cat([b[~_inside(p)] for b, p in zip(before, (pk, pv))]).view(raw),
             torch.cat([p.buf[~_inside(p)] for p in (pk, pv)]).view(raw), "outside the logical regions")


def _inside(p):
    inside = torch.zeros(p.buf.shape, dtype=torch.bool, device=p.buf.device)
    inside.as_strided(p.x.shape, p.x.stride()).fill_(True)
    return inside
