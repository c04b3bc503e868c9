"""matmuls.key_block_bounds[_paged]_fp8 on the GPU: the bits of key_block_bounds on the cache widened to the
bounds' dtype — and of a CPU reference that takes minimum and maximum on the ordered 16-bit patterns —, signed zeros and
extremes, the paged form, last=T, and unseen memory."""
import pytest
import torch

from test_gpu_block_attention_decode import SMAX, lens_tensor
from test_gpu_block_attention_decode_fp8 import F8, FINITE, NANB, fp8, pools, wide
from test_gpu_block_attention_decode_paged import gathered

pytestmark = pytest.mark.gpu

WIDTHS = [32, 64, 96, 128]
LOWP = [torch.bfloat16, torch.float16]
SENT = 0x5A5A  # the pattern a block without a seen key keeps
B, HKV = 2, 2
BLOCKS = SMAX // 64


def any_codes(seed, *shape):
    """Random codes out of all 254 finite ones (±0, the subnormals, ±448 included), uint8 on the CPU."""
    return FINITE[torch.randint(254, shape, generator=torch.Generator().manual_seed(seed))]


def sentinel(dev, dtype, D, b=B):
    return torch.full((b, HKV, BLOCKS, 2, D), SENT, dtype=torch.int16, device=dev).view(dtype)


def bits(x):
    return x.cpu().view(torch.int16).to(torch.int32) & 0xFFFF


def reference(c, seen, dtype, refresh=None):
    """int32 patterns [B, Hkv, blocks, 2, D] on the CPU from the contract alone: the codes widened by torch (exact), minimum and
    maximum over the seen rows of every block in the order of the 16-bit patterns (−0 < +0); a block without a seen key — or,
    with `refresh` [B, blocks] given, one it does not name — holds SENT.  `seen`: bool [B, Smax]."""
    w = c.view(F8).to(dtype).view(torch.int16).to(torch.int32) & 0xFFFF
    o = torch.where((w & 0x8000) != 0, ~w & 0xFFFF, w | 0x8000)
    b, h, smax, D = c.shape
    out = torch.full((b, h, smax // 64, 2, D), SENT, dtype=torch.int32)
    for i in range(b):
        for J in range(smax // 64):
            rows = seen[i, 64 * J:64 * J + 64].nonzero().flatten() + 64 * J
            if len(rows) == 0 or (refresh is not None and not refresh[i, J]):
                continue
            lo, hi = o[i][:, rows].amin(1), o[i][:, rows].amax(1)
            for slot, x in ((0, lo), (1, hi)):
                out[i, :, J, slot] = torch.where((x & 0x8000) != 0, x & 0x7FFF, ~x & 0xFFFF)
    return out


def seen_rows(k_lens, smax=SMAX):
    return torch.arange(smax)[None, :] < torch.tensor(k_lens)[:, None]


# ---- 1. the bits of key_block_bounds on the widened cache --------------------------------------------------------------------

@pytest.mark.parametrize("k_lens", [[512, 131], [1, 65]])
@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("D", WIDTHS)
def test_1_the_bits_of_the_call_on_the_widened_cache(mm, dev, D, dtype, k_lens):
    kc = any_codes(3201 + D + k_lens[0], B, HKV, SMAX, D)
    lens = lens_tensor(k_lens, dev)
    pre = sentinel(dev, dtype, D)
    got = mm.key_block_bounds_fp8(fp8(kc, dev), lens, pre)
    assert got is pre and got.dtype == dtype and not got.requires_grad
    want = mm.key_block_bounds(wide(kc, dtype, dev), lens, sentinel(dev, dtype, D))
    assert torch.equal(bits(got), bits(want)), f"D={D} {dtype} {k_lens}: the 2-byte call on the widened cache"
    assert torch.equal(bits(got), reference(kc, seen_rows(k_lens), dtype)), f"D={D} {dtype} {k_lens}: the CPU reference"
    assert (bits(got)[1, :, (k_lens[1] + 63) // 64:] == SENT).all()      # blocks without a key keep the sentinel
    # allocated by the call: dtype decides, the same bits where a block holds a key
    fresh = mm.key_block_bounds_fp8(fp8(kc, dev), lens, dtype=dtype)
    assert fresh.dtype == dtype and fresh.is_contiguous() and tuple(fresh.shape) == (B, HKV, BLOCKS, 2, D)
    for b, n in enumerate(k_lens):
        nb = (n + 63) // 64
        assert torch.equal(bits(fresh[b, :, :nb]), bits(got[b, :, :nb]))


# ---- 2. signed zeros and extremes ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
def test_2_signed_zeros_extremes_a_single_key_and_every_code(mm, dev, dtype):
    D = 64
    kc = any_codes(3210, B, HKV, SMAX, D)
    g = torch.Generator().manual_seed(3211)
    # item 0, block 0: only −0 and +0, both in every column
    zeros = torch.where(torch.rand((HKV, 64, D), generator=g) < 0.5, 0x80, 0x00).to(torch.uint8)
    zeros[:, 5], zeros[:, 40] = 0x80, 0x00
    kc[0, :, 0:64] = zeros
    # item 0, block 1: ±448 once in every column, at a row of its own
    rows = torch.randint(0, 32, (D,), generator=g)
    for d in range(D):
        kc[0, :, 64 + int(rows[d]), d], kc[0, :, 96 + int(rows[d]), d] = 0x7E, 0xFE
    # item 0, block 2: a single seen key (k_len = 129); item 1, block 0: every finite code once, the rest +0
    every = torch.zeros(64 * D, dtype=torch.uint8)
    every[:254] = FINITE[torch.randperm(254, generator=g)]
    kc[1, :, 0:64] = every[torch.randperm(64 * D, generator=g)].reshape(64, D)
    k_lens = [129, 64]
    got = bits(mm.key_block_bounds_fp8(fp8(kc, dev), lens_tensor(k_lens, dev), sentinel(dev, dtype, D)))
    assert (got[0, :, 0, 0] == 0x8000).all() and (got[0, :, 0, 1] == 0x0000).all(), "−0 is the minimum, +0 the maximum"
    w448 = int(bits(torch.tensor([448.0]).to(dtype))[0])
    assert (got[0, :, 1, 0] == (w448 | 0x8000)).all() and (got[0, :, 1, 1] == w448).all(), "±448"
    one = bits(kc[0, :, 128].view(F8).to(dtype))
    assert torch.equal(got[0, :, 2, 0], one) and torch.equal(got[0, :, 2, 1], one), "a single key is its own minimum and maximum"
    assert torch.equal(got, reference(kc, seen_rows(k_lens), dtype))
    assert (got[0, :, 3:] == SENT).all() and (got[1, :, 1:] == SENT).all()


# ---- 3. paged ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("page", [16, 128])
@pytest.mark.parametrize("dtype", LOWP)
def test_3_the_paged_form_hidden_pages_and_shared_pages(mm, dev, dtype, page):
    D, k_lens = 96, [512, 131]
    kc = any_codes(3220 + page, B, HKV, SMAX, D)
    kp, _, table = pools(kc, kc, page, 3221 + page)
    lens = lens_tensor(k_lens, dev)
    k8p = fp8(kp, dev)
    got = mm.key_block_bounds_paged_fp8(k8p, table.to(dev), lens, sentinel(dev, dtype, D))
    flat = mm.key_block_bounds_fp8(fp8(gathered(kp, table), dev), lens, sentinel(dev, dtype, D))
    assert torch.equal(bits(got), bits(flat)), f"page {page}: the contiguous call on the gathered bytes"
    assert torch.equal(bits(got), reference(kc, seen_rows(k_lens), dtype))
    assert torch.equal(bits(mm.key_block_bounds_paged_fp8(k8p, table.to(dev).long(), lens, sentinel(dev, dtype, D))), bits(got))
    # a −1 (and a P) entry hides its page's keys; blocks 2 and 3 of item 0 are hidden wholly and are not written
    hidden, seen = table.clone(), seen_rows(k_lens)
    per = max(128 // page, 1)
    for lp, entry in [(128 // page + i, -1 if i % 2 == 0 else kp.shape[0]) for i in range(per if page < 128 else 1)]:
        hidden[0, lp] = entry
        seen[0, lp * page:(lp + 1) * page] = False
    if page < 128:   # … and one page of item 1's block 0: the rest of the block is counted
        hidden[1, 1] = -1
        seen[1, page:2 * page] = False
    got = bits(mm.key_block_bounds_paged_fp8(k8p, hidden.to(dev), lens, sentinel(dev, dtype, D)))
    assert torch.equal(got, reference(kc, seen, dtype)), f"page {page}: hidden pages are left out"
    assert (got[0, :, 2:4] == SENT).all() and (got[0, :, 4] != SENT).any()
    # items sharing pages: item 1 reads item 0's
    shared = table.clone()
    shared[1] = table[0]
    got = bits(mm.key_block_bounds_paged_fp8(k8p, shared.to(dev), lens, sentinel(dev, dtype, D)))
    assert torch.equal(got, reference(kc[:1].expand(2, -1, -1, -1), seen_rows(k_lens), dtype)), f"page {page}: shared pages"


# ---- 4. last = T ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,k_len", [(1, 64), (1, 65), (3, 127), (64, 127), (64, 130), (70, 127)])
def test_4_last_refreshes_exactly_the_blocks_of_the_newest_positions(mm, dev, T, k_len):
    D, dtype = 64, torch.bfloat16 if T % 2 else torch.float16
    kc = any_codes(3230 + T + k_len, B, HKV, SMAX, D)
    k_lens = [k_len, k_len + 192]
    refresh = torch.zeros(B, BLOCKS, dtype=torch.bool)
    for b, n in enumerate(k_lens):
        refresh[b, max(n - T, 0) // 64:(n - 1) // 64 + 1] = True
    assert refresh.sum() >= 2
    got = bits(mm.key_block_bounds_fp8(fp8(kc, dev), lens_tensor(k_lens, dev), sentinel(dev, dtype, D), last=T))
    assert torch.equal(got, reference(kc, seen_rows(k_lens), dtype, refresh)), f"last={T}, k_len={k_len}"
    kp, _, table = pools(kc, kc, 32, 3231)
    got = bits(mm.key_block_bounds_paged_fp8(fp8(kp, dev), table.to(dev), lens_tensor(k_lens, dev), sentinel(dev, dtype, D), last=T))
    assert torch.equal(got, reference(kc, seen_rows(k_lens), dtype, refresh)), f"paged, last={T}, k_len={k_len}"


# ---- 5. nothing outside is read ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["BSHD", "pool"])
def test_5_nothing_outside_is_read(mm, dev, form):
    """The NaN code at the rows at or beyond k_len, between the rows of a [B, Smax, Hkv, D + 16].transpose(1, 2) view and in the
    unreferenced pages of a pool: the bits of the clean call, and no NaN."""
    D, dtype, k_lens = 64, torch.float16, [130, 449]
    kc = any_codes(3240, B, HKV, SMAX, D)
    lens = lens_tensor(k_lens, dev)
    want = bits(mm.key_block_bounds_fp8(fp8(kc, dev), lens, sentinel(dev, dtype, D)))
    dirty = kc.clone()
    for b, n in enumerate(k_lens):
        dirty[b, :, n:] = NANB
    if form == "BSHD":
        buf = torch.full((B, SMAX, HKV, D + 16), NANB, device=dev, dtype=torch.uint8)
        view = buf[..., :D].transpose(1, 2)
        view.copy_(dirty.to(dev))
        assert not view.is_contiguous()
        got = mm.key_block_bounds_fp8(view.view(F8), lens, sentinel(dev, dtype, D))
    else:
        kp, _, table = pools(dirty, dirty, 32, 3241)          # the unreferenced pages hold the NaN code
        got = mm.key_block_bounds_paged_fp8(fp8(kp, dev), table.to(dev), lens, sentinel(dev, dtype, D))
    assert torch.equal(bits(got), want), form
    for b, n in enumerate(k_lens):
        assert not torch.isnan(got[b, :, :(n + 63) // 64].float()).any()
