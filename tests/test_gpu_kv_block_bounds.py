"""matmuls.key_block_bounds / key_block_bounds_paged on the GPU: the per-block key bounds against
torch.amin / torch.amax over the seen rows, for every D, both dtypes, contiguous and paged; blocks without a key untouched;
unseen memory unread; the refresh of the newest T positions; an out-of-range table entry under seen keys."""
import pytest
import torch

from gpu_helpers import SENTINEL, assert_same_bits
from test_gpu_block_attention_decode_paged import gathered, paged

pytestmark = pytest.mark.gpu

SMAX = 512
NAN = float("nan")
WIDTHS = [32, 64, 96, 128]
K_LENS = [512, 200, 65, 0]


def keys(dev, B, Hkv, D, dtype, seed, smax=SMAX):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn((B, Hkv, smax, D), device=dev, generator=g).to(dtype)


def reference(k, k_lens, base):
    """torch.amin / torch.amax over the seen rows of every block, on `base` (the bytes a block without a key keeps)."""
    ref = base.clone()
    for b, n in enumerate(k_lens):
        for J in range(k.shape[2] // 64):
            hi = min(64 * J + 64, n)
            if hi > 64 * J:
                ref[b, :, J, 0] = torch.amin(k[b, :, 64 * J:hi], 1)
                ref[b, :, J, 1] = torch.amax(k[b, :, 64 * J:hi], 1)
    return ref


def sentinel_bounds(k, smax=SMAX):
    B, Hkv, _, D = k.shape
    return torch.full((B, Hkv, smax // 64, 2, D), SENTINEL, device=k.device, dtype=k.dtype)


# ---- 1. every D, both dtypes, contiguous and paged ---------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", WIDTHS)
def test_1_bounds_are_amin_and_amax_of_the_seen_rows(mm, dev, D, dtype):
    B, Hkv = 4, 2
    k = keys(dev, B, Hkv, D, dtype, 1000 + D)
    lens = torch.tensor(K_LENS, device=dev, dtype=torch.int32)
    bounds = sentinel_bounds(k)
    ref = reference(k, K_LENS, bounds)
    out = mm.key_block_bounds(k, lens, bounds)
    assert out is bounds and not out.requires_grad
    assert torch.equal(out, ref), "contiguous: bounds differ from amin / amax of the seen rows (or a block without a key was written)"
    assert (out[3] == SENTINEL).all() and (out[2, :, 2:] == SENTINEL).all() and (out[1, :, 4:] == SENTINEL).all()
    fresh = mm.key_block_bounds(k, lens)
    assert fresh.shape == ref.shape and fresh.dtype == dtype
    for b, n in enumerate(K_LENS):
        nb = (n + 63) // 64
        assert_same_bits(fresh[b, :, :nb], ref[b, :, :nb], f"allocated bounds, item {b}")
    for page in (16, 64, 256):
        kp, _, table = paged(k, k, page, 7 + page)
        got = mm.key_block_bounds_paged(kp, table, lens, sentinel_bounds(k))
        assert_same_bits(got, out, f"page {page}: the paged call against the contiguous call")
    assert_same_bits(mm.key_block_bounds(k, lens.long(), sentinel_bounds(k)), out, "int64 k_lens")


# ---- 2. unseen memory ----------------------------------------------------------------------------------------------------

def test_2_unseen_memory_is_never_read(mm, dev):
    B, Hkv, D, dtype = 4, 2, 64, torch.float16
    k = keys(dev, B, Hkv, D, dtype, 2001)
    lens = torch.tensor(K_LENS, device=dev, dtype=torch.int32)
    want = mm.key_block_bounds(k, lens, sentinel_bounds(k))
    buf = torch.full((B, SMAX, Hkv, D + 8), NAN, device=dev, dtype=dtype)   # NaN between the rows …
    ks = buf[..., :D].transpose(1, 2)
    for b, n in enumerate(K_LENS):
        ks[b, :, :n] = k[b, :, :n]                                           # … and in every row at or beyond k_len
    before = buf.clone()
    got = mm.key_block_bounds(ks, lens, sentinel_bounds(k))
    assert not torch.isnan(got.float()).any()
    assert_same_bits(got, want, "the poisoned strided cache")
    assert_same_bits(buf, before, "the cache's bytes")
    poisoned = k.clone()
    for b, n in enumerate(K_LENS):
        poisoned[b, :, n:] = NAN
    for page in (16, 128):
        kp, _, table = paged(poisoned, poisoned, page, 31 + page)            # unreferenced pool pages are NaN
        snap = kp.clone()
        got = mm.key_block_bounds_paged(kp, table, lens, sentinel_bounds(k))
        assert not torch.isnan(got.float()).any()
        assert_same_bits(got, want, f"page {page}: the poisoned pool")
        assert_same_bits(kp, snap, "the pool's bytes")


# ---- 3. last=T -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("start", [130, 127])
@pytest.mark.parametrize("T", [1, 3, 64, 70])
def test_3_last_refreshes_the_blocks_of_the_newest_positions_only(mm, dev, T, start):
    B, Hkv, D, dtype = 2, 2, 96, torch.bfloat16
    k = keys(dev, B, Hkv, D, dtype, 3000 + T)
    n = start + T                                     # an append of T tokens from k_len 130 (127: every T crosses a boundary)
    lens = torch.tensor([n, n], device=dev, dtype=torch.int32)
    full = mm.key_block_bounds(k, lens, sentinel_bounds(k))
    pre = torch.full_like(full, 3.25)
    got = mm.key_block_bounds(k, lens, pre, last=T)
    assert got is pre
    first, last = start // 64, (n - 1) // 64         # the blocks that hold a position of [k_len − T, k_len)
    assert (last > first) == (T >= 64 or (start == 127 and T >= 2)), "which appends cross a block boundary"
    assert_same_bits(pre[:, :, first:last + 1], full[:, :, first:last + 1], "the refreshed blocks against the full recomputation")
    assert (pre[:, :, :first] == 3.25).all() and (pre[:, :, last + 1:] == 3.25).all(), "every other block keeps its bytes"
    kp, _, table = paged(k, k, 32, 77)
    pre2 = torch.full_like(full, 3.25)
    mm.key_block_bounds_paged(kp, table, lens, pre2, last=T)
    assert_same_bits(pre2, pre, "the paged refresh")
    # a refresh longer than the cache is the full call
    assert_same_bits(mm.key_block_bounds(k, lens, sentinel_bounds(k), last=SMAX + 5), full, "last beyond k_len")


# ---- 4. an out-of-range table entry under seen keys --------------------------------------------------------------------------

def test_4_an_invalid_entry_hides_exactly_its_page(mm, dev):
    B, Hkv, D, dtype, page = 2, 2, 128, torch.float16, 16
    k = keys(dev, B, Hkv, D, dtype, 4001)
    k_lens = [300, 512]
    lens = torch.tensor(k_lens, device=dev, dtype=torch.int32)
    kp, _, table = paged(k, k, page, 41)
    table[0, 5] = -1                                  # keys 80 … 95 of item 0: in block 1, under seen keys
    table[1, 8:12] = kp.shape[0]                      # keys 128 … 191 of item 1: the whole of block 2
    table[0, 20] = -7                                 # keys 320 … 335 of item 0: beyond k_len, never consulted
    got = mm.key_block_bounds_paged(kp, table, lens, sentinel_bounds(k))
    ref = reference(k, k_lens, sentinel_bounds(k))
    rest = torch.cat([k[0, :, 64:80], k[0, :, 96:128]], 1)
    ref[0, :, 1, 0], ref[0, :, 1, 1] = torch.amin(rest, 1), torch.amax(rest, 1)
    ref[1, :, 2] = SENTINEL                           # a block whose every seen key is invisible is not written
    assert torch.equal(got, ref)
    assert not torch.isnan(got.float()).any()
    assert torch.equal(gathered(kp, table)[1, :, :128], k[1, :, :128])
