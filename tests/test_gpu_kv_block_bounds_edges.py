"""matmuls.key_block_bounds / key_block_bounds_paged on the GPU, where random normal keys and one k_len for
every item do not reach: special bit patterns as the minimum and the maximum of their column, in the rows of the last pass;
negative, oversized and 0-d k_lens with three heads per item; and the refresh of the newest T positions with another k_len
per item.  Everything is exact (assert_same_bits)."""
import numpy as np
import pytest
import torch

from gpu_helpers import SENTINEL, assert_same_bits
from test_gpu_block_attention_decode_paged import paged
from test_gpu_kv_block_bounds import keys, reference

pytestmark = pytest.mark.gpu

NAN = float("nan")


def sentinel_bounds(k, smax):
    B, Hkv, _, D = k.shape
    return torch.full((B, Hkv, smax // 64, 2, D), SENTINEL, device=k.device, dtype=k.dtype)


# ---- 1. special patterns ---------------------------------------------------------------------------------------------------------

def ladder(dtype):
    """The values planted, in the contract's order (−0 < +0): ±inf, the largest finite value, the smallest subnormal of each
    sign, both zeros and ordinary values."""
    big, tiny = float(torch.finfo(dtype).max), float(torch.finfo(dtype).smallest_normal) * float(torch.finfo(dtype).eps)
    return [-np.inf, -big, -2.25, -tiny, -0.0, 0.0, tiny, 1.5, big, np.inf]


def min_max_f64(rows):
    """float64 amin / amax over axis 0 with the contract's one extra rule: −0 < +0."""
    neg0, pos0 = (rows == 0) & np.signbit(rows), (rows == 0) & ~np.signbit(rows)
    lo, hi = rows.min(0), rows.max(0)
    lo = np.where(lo == 0, np.where(neg0.any(0), -0.0, 0.0), lo)
    hi = np.where(hi == 0, np.where(pos0.any(0), 0.0, -0.0), hi)
    return lo, hi


# the row of the special in blocks 0 … 4: row 63 (D = 96: the fourth pass of thread row 0; D = 128: the last of 16 rows of the
# fourth pass), 62 and 48 (other rows of the last pass), 0, 21 (D = 96: the first row of the second pass), and in the partial
# block 5 its last seen row 36
SPECIAL_ROWS = [63, 62, 0, 21, 48, 36]
SEEN_LAST = 37


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [32, 96, 128])
def test_1_special_patterns_as_the_minimum_and_the_maximum(mm, dev, D, dtype):
    """Column 2i holds ladder value i as its minimum — every other row drawn from the ladder at or above it — and column
    2i + 1 holds it as its maximum; column 20 holds only the two zeros (min −0, max +0), column 21 only −0 (both −0); the
    other columns draw from the whole ladder.  No NaN among the seen keys (unspecified); NaN in every unseen row."""
    B, Hkv, smax = 1, 2, 64 * len(SPECIAL_ROWS)
    lad = ladder(dtype)
    assert D >= 22 and float(torch.tensor(lad[3], dtype=dtype)) == lad[3] != 0
    g = np.random.default_rng(500 + D)
    k64 = np.zeros((B, Hkv, smax, D))
    for col in range(D):
        i, as_max = col // 2, col % 2
        pool = (lad[:i + 1] if as_max else lad[i:]) if col < 20 else [-0.0, 0.0] if col == 20 else [-0.0] if col == 21 else lad
        k64[..., col] = np.asarray(pool)[g.integers(0, len(pool), (B, Hkv, smax))]
        if col < 20:
            for J, r in enumerate(SPECIAL_ROWS):
                others = [v for v in pool if not (v == lad[i] and np.signbit(v) == np.signbit(lad[i]))] or [lad[i]]
                k64[:, :, 64 * J:64 * J + 64, col] = np.asarray(others)[g.integers(0, len(others), (B, Hkv, 64))]
                k64[:, :, 64 * J + r, col] = lad[i]                    # the special stands in exactly one row of the block
    k_len = smax - 64 + SEEN_LAST
    want = np.full((B, Hkv, smax // 64, 2, D), SENTINEL)
    for J in range(smax // 64):
        rows = k64[:, :, 64 * J:min(64 * J + 64, k_len)]
        for b in range(B):
            for h in range(Hkv):
                want[b, h, J, 0], want[b, h, J, 1] = min_max_f64(rows[b, h])
    for J, r in enumerate(SPECIAL_ROWS):                              # the reference holds what the construction claims
        for i in range(10):
            for slot in (0, 1):
                w = want[0, 0, J, slot, 2 * i + slot]
                assert w == lad[i] and np.signbit(w) == np.signbit(lad[i]), (J, i, slot)
    assert np.signbit(want[..., 0, 20]).all() and not np.signbit(want[..., 1, 20]).any() and np.signbit(want[..., 21]).all()
    k = torch.from_numpy(k64).to(dtype)
    assert torch.equal(k.double(), torch.from_numpy(k64)), "a planted value does not fit the type"
    k[:, :, k_len:] = NAN
    k = k.to(dev)
    lens = torch.tensor([k_len], device=dev, dtype=torch.int32)
    want = torch.from_numpy(want).to(dtype)
    got = mm.key_block_bounds(k, lens, sentinel_bounds(k, smax))
    assert_same_bits(got, want, f"D={D} {dtype}: contiguous")
    kp, _, table = paged(k, k, 16, 600 + D)
    assert_same_bits(mm.key_block_bounds_paged(kp, table, lens, sentinel_bounds(k, smax)), want, f"D={D} {dtype}: pages of 16")


# ---- 2. k_lens forms -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,dtype", [(32, torch.float16), (96, torch.bfloat16)])
def test_2_negative_oversized_and_zero_dim_k_lens_with_three_heads(mm, dev, D, dtype):
    """Hkv = 3, so that item c's batch index c / heads and head c % heads both differ from c.  A negative k_len writes
    nothing; one above Smax is clamped — every block from its 64 rows; a 0-d k_lens serves every item."""
    B, Hkv, smax = 3, 3, 256
    k = keys(dev, B, Hkv, D, dtype, 7100 + D, smax)
    for k_lens, dt in (([-5, smax + 100, 70], torch.int32), ([smax + 1, -1, 129], torch.int64)):
        base = sentinel_bounds(k, smax)
        want = reference(k, [min(max(n, 0), smax) for n in k_lens], base)
        got = mm.key_block_bounds(k, torch.tensor(k_lens, device=dev, dtype=dt), sentinel_bounds(k, smax))
        assert_same_bits(got, want, f"k_lens {k_lens}")
        kp, _, table = paged(k, k, 32, 71)
        assert_same_bits(mm.key_block_bounds_paged(kp, table, torch.tensor(k_lens, device=dev, dtype=dt), sentinel_bounds(k, smax)),
                         want, f"k_lens {k_lens}: pages of 32")
        empty = k_lens.index(min(k_lens))
        assert (got[empty] == SENTINEL).all()
    for n in (130, -3, smax + 7):
        want = reference(k, [min(max(n, 0), smax)] * B, sentinel_bounds(k, smax))
        got = mm.key_block_bounds(k, torch.tensor(n, device=dev, dtype=torch.int32), sentinel_bounds(k, smax))
        assert_same_bits(got, want, f"0-d k_lens = {n}")
        clamped, part = min(max(n, 0), smax), sentinel_bounds(k, smax)
        if clamped > 0:
            first, last = max(clamped - 3, 0) // 64, (clamped - 1) // 64
            part[:, :, first:last + 1] = want[:, :, first:last + 1]
        got = mm.key_block_bounds(k, torch.tensor(n, device=dev, dtype=torch.int32), sentinel_bounds(k, smax), last=3)
        assert_same_bits(got, part, f"0-d k_lens = {n}, last=3")


# ---- 3. per-item refresh ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [1, 3, 70])
def test_3_last_refreshes_each_item_from_its_own_length(mm, dev, T):
    """k_lens [130, 64, 3, 0]: for every item exactly the blocks that hold a position of [max(k_len − T, 0), k_len) get the
    bits of the full call; every other block keeps the sentinel.  Contiguous and in pages of 16."""
    B, Hkv, D, dtype, smax = 4, 3, 64, torch.float16, 256
    k_lens = [130, 64, 3, 0]
    k = keys(dev, B, Hkv, D, dtype, 7300 + T, smax)
    lens = torch.tensor(k_lens, device=dev, dtype=torch.int32)
    full = mm.key_block_bounds(k, lens, sentinel_bounds(k, smax))
    assert_same_bits(full, reference(k, k_lens, sentinel_bounds(k, smax)), "the full call")
    want = sentinel_bounds(k, smax)
    refreshed = []
    for b, n in enumerate(k_lens):
        if n > 0:
            first, last = max(n - T, 0) // 64, (n - 1) // 64
            want[b, :, first:last + 1] = full[b, :, first:last + 1]
            refreshed.append(list(range(first, last + 1)))
    assert refreshed == {1: [[2], [0], [0]], 3: [[1, 2], [0], [0]], 70: [[0, 1, 2], [0], [0]]}[T]
    got = mm.key_block_bounds(k, lens, sentinel_bounds(k, smax), last=T)
    assert_same_bits(got, want, f"last={T}: contiguous")
    kp, _, table = paged(k, k, 16, 73 + T)
    assert_same_bits(mm.key_block_bounds_paged(kp, table, lens, sentinel_bounds(k, smax), last=T), want, f"last={T}: pages of 16")
