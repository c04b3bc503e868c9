"""matmuls.select_key_blocks on the GPU, from bounds tensors given directly: exact integer cases with ties
at the K-th place, real-valued cases under the derived fp32 summation bound, the shapes of the selection itself up to the
cap of 16 384 blocks, the upper-bound property on real caches, poisoned non-candidates, and batch independence."""
import numpy as np
import pytest
import torch

from gpu_helpers import assert_same_bits

pytestmark = pytest.mark.gpu

NAN = float("nan")
WIDTHS = [32, 64, 96, 128]
U = 2.0 ** -24


def reference(q, bounds, k_lens, K, sink, local):
    """The contract in float64 / integers on the CPU: (ids [B, Hkv, T, K], counts, scores [B, Hkv, T, blocks], s_abs) — s_abs
    the largest Σ_d max(|q·lo|, |q·hi|) over (g, J) per token, for the summation bound."""
    q, bounds = q.cpu().double(), bounds.cpu().double()
    B, Hq, T, D = q.shape
    Hkv, blocks = bounds.shape[1], bounds.shape[2]
    G = Hq // Hkv
    ids, counts = np.full((B, Hkv, T, K), -1, np.int64), np.zeros((B, Hkv, T), np.int64)
    scores, s_abs = np.full((B, Hkv, T, blocks), -np.inf), np.zeros((B, Hkv, T))
    for b in range(B):
        for h in range(Hkv):
            lo, hi = bounds[b, h, :, 0], bounds[b, h, :, 1]                      # [blocks, D]
            for t in range(T):
                pos = min(max(int(k_lens[b]), 0), blocks * 64) - T + t
                if pos < 0:
                    continue
                n = pos // 64 + 1
                qg = q[b, h * G:(h + 1) * G, t]                                   # [G, D]
                a, c = qg[:, None, :] * lo[None, :n], qg[:, None, :] * hi[None, :n]
                s = torch.maximum(a, c).sum(-1).amax(0).numpy()                  # [n]
                s_abs[b, h, t] = float(torch.maximum(a.abs(), c.abs()).sum(-1).max())
                scores[b, h, t, :n] = s
                forced = np.zeros(n, bool)
                forced[:min(sink, n)] = True
                forced[max(n - local, 0):] = True
                rest = [J for J in np.lexsort((np.arange(n), -s)) if not forced[J]]   # score descending, index ascending
                cnt = min(K, n)
                chosen = np.sort(np.concatenate([np.nonzero(forced)[0], np.array(rest[:cnt - int(forced.sum())], np.int64)]))
                assert len(chosen) == cnt
                ids[b, h, t, :cnt], counts[b, h, t] = chosen, cnt
    return ids, counts, scores, s_abs


def kth_gap(scores, ids, counts, sink, local, b, h, t):
    """(score of the last chosen, of the first unchosen) unforced candidate of a token, or None where there is no such pair."""
    n = int(np.isfinite(scores[b, h, t]).sum())
    unforced = [J for J in range(n) if not (J < sink or J >= n - local)]
    chosen = set(ids[b, h, t, :counts[b, h, t]].tolist())
    inside = [scores[b, h, t, J] for J in unforced if J in chosen]
    outside = [scores[b, h, t, J] for J in unforced if J not in chosen]
    return (min(inside), max(outside)) if inside and outside else None


def integer_operands(B, Hkv, G, T, D, blocks, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(-4, 5, (B, Hkv * G, T, D), generator=g).to(dtype)
    lo = torch.randint(-8, 9, (B, Hkv, blocks, D), generator=g)
    hi = torch.minimum(lo + torch.randint(0, 6, (B, Hkv, blocks, D), generator=g), torch.tensor(8))
    return q, torch.stack([lo, hi], 3).to(dtype)


def run(mm, dev, q, bounds, k_lens, K, sink, local):
    ids, counts, scores = mm.select_key_blocks(q.to(dev), bounds.to(dev), torch.tensor(k_lens, device=dev, dtype=torch.int32), K,
                                               sink=sink, local=local, return_scores=True)
    assert ids.dtype == torch.int32 and counts.dtype == torch.int32 and scores.dtype == torch.float32
    return ids.cpu().numpy().astype(np.int64), counts.cpu().numpy().astype(np.int64), scores.cpu().numpy().astype(np.float64)


# ---- 1. exact cases ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [1, 4, 16])
@pytest.mark.parametrize("D", WIDTHS)
def test_1_exact_integer_cases_with_ties_at_the_kth_place(mm, dev, D, G):
    """Integer q in [−4, 4] and bounds in [−8, 8]: every partial sum is an integer below 2²⁴, so the fp32 scores are exact in
    any order and ids, counts and scores equal the integer computation exactly.  Item 0's unforced blocks hold only two
    distinct bounds (blocks 1, 3, 5 and 2, 4), so the K-th place falls among equal scores: the lower index wins."""
    B, Hkv, T, blocks = 2, 2, 3, 8
    dtype = torch.bfloat16 if (D // 32 + G) % 2 else torch.float16
    q, bounds = integer_operands(B, Hkv, G, T, D, blocks, 100 * D + G, dtype)
    bounds[0, :, 3], bounds[0, :, 5] = bounds[0, :, 1], bounds[0, :, 1]
    bounds[0, :, 4] = bounds[0, :, 2]
    k_lens = [512, 449]                      # item 0: 8 candidates; item 1: pos 446, 447, 448 — 7, 7 and 8 candidates
    ties = 0
    for K, sink, local in ((4, 1, 2), (5, 1, 2), (6, 1, 2), (1, 0, 1), (3, 0, 1), (8, 2, 3), (13, 1, 2)):
        r_ids, r_counts, r_scores, _ = reference(q, bounds, k_lens, K, sink, local)
        ids, counts, scores = run(mm, dev, q, bounds, k_lens, K, sink, local)
        assert np.array_equal(scores, r_scores), (K, sink, local)
        assert np.array_equal(counts, r_counts), (K, sink, local)
        assert np.array_equal(ids, r_ids), (K, sink, local, ids[0, 0], r_ids[0, 0])
        for h in range(Hkv):
            for t in range(T):
                gap = kth_gap(r_scores, r_ids, r_counts, sink, local, 0, h, t)
                ties += gap is not None and gap[0] == gap[1]
    assert ties > 0, "no tie at the K-th place: the tie rule went untested"


# ---- 2. real-valued cases ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", WIDTHS)
def test_2_real_valued_cases_under_the_summation_bound(mm, dev, D):
    """Random normal q and bounds.  An fp32 sum of D exact products in any order lies within γ_D·Σ|terms| ≤ 2·D·2⁻²⁴·Σ|terms|
    of the float64 sum; where the gap between the last chosen and the first unchosen unforced candidate exceeds twice that
    (asserted here, on the CPU), the chosen SET is the reference's."""
    B, Hkv, G, T, blocks, dtype = 2, 2, 4, 3, 8, (torch.bfloat16 if D % 64 else torch.float16)
    g = torch.Generator().manual_seed(7000 + D)
    q = torch.randn((B, Hkv * G, T, D), generator=g).to(dtype)
    a, c = torch.randn((B, Hkv, blocks, D), generator=g), torch.randn((B, Hkv, blocks, D), generator=g)
    bounds = torch.stack([torch.minimum(a, c), torch.maximum(a, c)], 3).to(dtype)
    k_lens = [512, 449]
    for K, sink, local in ((4, 1, 2), (5, 0, 1), (2, 0, 1)):
        r_ids, r_counts, r_scores, s_abs = reference(q, bounds, k_lens, K, sink, local)
        tol = 2 * D * U * s_abs                                         # per token
        for b in range(B):
            for h in range(Hkv):
                for t in range(T):
                    gap = kth_gap(r_scores, r_ids, r_counts, sink, local, b, h, t)
                    assert gap is not None and gap[0] - gap[1] > 2 * tol[b, h, t], "precondition: choose another seed"
        ids, counts, scores = run(mm, dev, q, bounds, k_lens, K, sink, local)
        assert np.array_equal(counts, r_counts)
        assert np.array_equal(ids, r_ids), (K, sink, local)             # ascending lists of equal sets
        fin = np.isfinite(r_scores)
        assert np.array_equal(np.isneginf(scores), ~fin)
        err = np.abs(np.where(fin, scores - np.where(fin, r_scores, 0.0), 0.0))
        print(f"D={D} K={K}: max score error {err.max():.3e}, bound {tol.min():.3e}")
        assert (err <= tol[..., None]).all()


# ---- 3. the shapes of the selection itself -------------------------------------------------------------------------------------

@pytest.mark.parametrize("blocks", [1, 8, 300, 16384])
def test_3_block_counts_and_every_k(mm, dev, blocks):
    """T = 3 across a block boundary (three candidate sets), a token with pos < 0 (count 0) for one block, K ≥ candidates
    lists every candidate; integer operands, so everything is exact."""
    D, G, T, dtype = (32, 2, 3, torch.bfloat16) if blocks > 8 else (96, 3, 3, torch.float16)
    q, bounds = integer_operands(1, 1, G, T, D, blocks, 31 + blocks, dtype)
    k_lens = [64 * (blocks - 1) + 2]            # pos 64(blocks − 1) − 1, …, + 1; one block: pos −1, 0, 1
    for K in sorted({1, 3, blocks, blocks + 5}):
        sink, local = (0, 1) if K < 3 else (1, 2)
        r_ids, r_counts, r_scores, _ = reference(q, bounds, k_lens, K, sink, local)
        ids, counts, scores = run(mm, dev, q, bounds, k_lens, K, sink, local)
        assert np.array_equal(scores, r_scores) and np.array_equal(counts, r_counts), K
        assert np.array_equal(ids, r_ids), K
        if blocks == 1:
            assert counts[0, 0, 0] == 0 and (ids[0, 0, 0] == -1).all()        # pos < 0
        if K >= blocks:
            n = int(counts[0, 0, T - 1])
            assert n == blocks and np.array_equal(ids[0, 0, T - 1, :n], np.arange(blocks)) and (ids[0, 0, T - 1, n:] == -1).all()


def test_3_one_block_above_the_cap_is_refused(mm, dev):
    q = torch.zeros((1, 1, 1, 32), device=dev, dtype=torch.bfloat16)
    bounds = torch.empty((1, 1, 16385, 2, 32), device=dev, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="16385 blocks per item exceed the 16384"):
        mm.select_key_blocks(q, bounds, torch.tensor(5, device=dev), 4)
    assert mm.select_key_blocks_takes(torch.bfloat16, 32, 1, 16384) and not mm.select_key_blocks_takes(torch.bfloat16, 32, 1, 16385)


# ---- 4. the upper-bound property ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [1, 4])
def test_4_a_score_bounds_every_seen_key_of_its_block(mm, dev, G):
    """Bounds from key_block_bounds of a random cache: score(J) = max_g s_g(J) ≥ q_g·k_j in float64 for every seen key j of a
    candidate block and every head g of the group (G = 1: s_g itself), minus the fp32 summation bound."""
    B, Hkv, T, D, smax, dtype = 4, 2, 1, 64, 512, torch.float16
    k_lens = [512, 200, 65, 0]
    g = torch.Generator(device=dev).manual_seed(4100 + G)
    k = torch.randn((B, Hkv, smax, D), device=dev, generator=g).to(dtype)
    q = torch.randn((B, Hkv * G, T, D), device=dev, generator=g).to(dtype)
    lens = torch.tensor(k_lens, device=dev, dtype=torch.int32)
    bounds = mm.key_block_bounds(k, lens, torch.zeros((B, Hkv, smax // 64, 2, D), device=dev, dtype=dtype))
    _, counts, scores = mm.select_key_blocks(q, bounds, lens, 3, return_scores=True)
    scores, kd, qd = scores.cpu().double(), k.cpu().double(), q.cpu().double()
    checked = 0
    for b, n in enumerate(k_lens):
        for h in range(Hkv):
            if n == 0:
                assert counts[b, h, 0] == 0 and torch.isinf(scores[b, h, 0]).all()
                continue
            dots = qd[b, h * G:(h + 1) * G, 0] @ kd[b, h, :n].T                                # [G, n]
            terms = (qd[b, h * G:(h + 1) * G, 0].abs()[:, None, :] * kd[b, h, :n].abs()[None]).sum(-1).max()
            for J in range((n - 1) // 64 + 1):
                best = float(dots[:, 64 * J:min(64 * J + 64, n)].max())
                assert float(scores[b, h, 0, J]) >= best - 2 * D * U * float(terms), (b, h, J)
                checked += 1
    assert checked == 2 * (8 + 4 + 2)


# ---- 5. poisoned non-candidates ------------------------------------------------------------------------------------------------

def test_5_bounds_of_non_candidates_are_never_read(mm, dev):
    B, Hkv, G, T, D, blocks, dtype = 2, 2, 4, 2, 128, 8, torch.bfloat16
    q, bounds = integer_operands(B, Hkv, G, T, D, blocks, 5001, dtype)
    k_lens = [130, 321]
    clean = mm.select_key_blocks(q.to(dev), bounds.to(dev), torch.tensor(k_lens, device=dev), 4, return_scores=True)
    poisoned = bounds.clone()
    for b, n in enumerate(k_lens):
        poisoned[b, :, (n - 1) // 64 + 1:] = NAN
    got = mm.select_key_blocks(q.to(dev), poisoned.to(dev), torch.tensor(k_lens, device=dev), 4, return_scores=True)
    for x, y, what in zip(got, clean, ("block_ids", "block_counts", "scores")):
        assert torch.equal(x, y), what
    assert not torch.isnan(got[2]).any()


# ---- 6. independence -------------------------------------------------------------------------------------------------------------

def test_6_an_item_of_a_batch_is_the_call_on_it_alone(mm, dev):
    B, Hkv, G, T, D, blocks, dtype = 4, 2, 4, 3, 96, 8, torch.float16
    g = torch.Generator().manual_seed(6001)
    q = torch.randn((B, Hkv * G, T, D), generator=g).to(dtype).to(dev)
    a, c = torch.randn((B, Hkv, blocks, D), generator=g), torch.randn((B, Hkv, blocks, D), generator=g)
    bounds = torch.stack([torch.minimum(a, c), torch.maximum(a, c)], 3).to(dtype).to(dev)
    lens = torch.tensor([512, 66, 300, 2], device=dev, dtype=torch.int32)
    ids, counts, scores = mm.select_key_blocks(q, bounds, lens, 4, return_scores=True)
    for b in range(B):
        one = mm.select_key_blocks(q[b:b + 1], bounds[b:b + 1], lens[b:b + 1], 4, return_scores=True)
        assert torch.equal(ids[b:b + 1], one[0]) and torch.equal(counts[b:b + 1], one[1]), f"item {b} alone"
        assert_same_bits(scores[b:b + 1], one[2], f"item {b} alone: scores")
    # q through its own strides: a [B, T, Hq, D] buffer seen as [B, Hq, T, D]
    qs = q.transpose(1, 2).contiguous().transpose(1, 2)
    assert not qs.is_contiguous()
    again = mm.select_key_blocks(qs, bounds, lens, 4, return_scores=True)
    assert torch.equal(again[0], ids) and torch.equal(again[1], counts)
    assert_same_bits(again[2], scores, "a strided q")
