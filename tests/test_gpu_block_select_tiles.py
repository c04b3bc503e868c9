"""matmuls.select_key_blocks_tiles on the GPU: the K best key blocks of every 64-position tile of a prefill
chunk, scored on the matrix cores as [q⁻ | q⁺] · [lo | hi]ᵀ.

1. planted scores: every token's q has one non-zero coordinate, so a tile score is a max of single exact products — the
   returned scores bit for bit, the lists against the written-out ordering, ties across the K-th place;
2. real operands: scores within 4·D·2⁻²⁴·s_abs of float64, lists the exact ordering of the returned scores, the chosen set
   that of float64 outside a ±2·tol band;
3. the upper bound: no key a token of the tile sees has a larger q·k than its block's score;
4. invariance: B, T / new_lens, a strided q;
5. non-finite bounds: the structure holds and nothing is stored outside the rows.

THE BOUND OF 2.  An fp32 sum of the 2·D exact products of a score in ANY summation tree under round-to-nearest lies within
(2·D − 1)·2⁻²⁴·s_abs of the exact sum, s_abs the sum of the terms' absolute values.  The MFMA's internal adder is not documented
to round to nearest per addition, hence a margin of about 2: 4·D·2⁻²⁴·s_abs.  A tile score is a max over tokens and heads, so
it lies within the LARGEST such bound over the tile's tokens and heads of the float64 max.  The largest measured error ÷ bound
is printed (profiles/r37_block_attention_prefill_selected.log keeps it)."""
import ctypes

import numpy as np
import pytest
import torch

from gpu_helpers import assert_same_bits, padded

pytestmark = pytest.mark.gpu

NAN = float("nan")
KB = 64
U = 2.0 ** -24
WIDTHS = [32, 64, 96, 128]
GUARD = -7  # around the int32 outputs of the C-ABI call of test 5


def clamp(n, lo, hi):
    return min(max(int(n), lo), hi)


def tiles_of(T):
    return -(-T // KB) + 1


def tile_slots(T, k_len, new_len, x, blocks):
    """(r, [slots]) of tile x: the slots that hold a token whose pos lies in [64r, 64r + 64)."""
    n = clamp(k_len, 0, blocks * KB)
    start = n - T
    first = max(n - (T if new_len is None else clamp(new_len, 0, T)), 0)
    r = start // KB + x
    return r, [p - start for p in range(max(first, r * KB), min(n, r * KB + KB))]


def select_from_scores(s, K, sink, local):
    """The written-out ordering: (ascending list, count) from the scores of the n candidates — forced blocks, then score
    descending / index ascending with −0 as +0 and NaN lowest."""
    n = len(s)
    forced = np.zeros(n, bool)
    forced[:min(sink, n)] = True
    forced[max(n - local, 0):] = True
    key = np.where(np.isnan(s), -np.inf, s + 0.0)
    order = np.lexsort((np.arange(n), np.isnan(s), -key))
    rest = [J for J in order if not forced[J]]
    cnt = min(K, n)
    chosen = np.sort(np.concatenate([np.nonzero(forced)[0], np.array(rest[:cnt - int(forced.sum())], np.int64)]))
    assert len(chosen) == cnt
    return chosen, cnt


def reference(q, bounds, k_lens, new_lens, K, sink, local):
    """The contract in float64 on the CPU: (ids [B, Hkv, X, K], counts, scores [B, Hkv, X, blocks], tol) — tol = 4·D·2⁻²⁴ · the
    largest Σ|terms| over the tile's tokens and heads, per (tile, block)."""
    q, bounds = q.cpu().double(), bounds.cpu().double()
    B, Hq, T, D = q.shape
    Hkv, blocks = bounds.shape[1], bounds.shape[2]
    G, X = Hq // Hkv, tiles_of(T)
    ids, counts = np.full((B, Hkv, X, K), -1, np.int64), np.zeros((B, Hkv, X), np.int64)
    scores, tol = np.full((B, Hkv, X, blocks), -np.inf), np.zeros((B, Hkv, X, blocks))
    for b in range(B):
        for x in range(X):
            r, slots = tile_slots(T, k_lens[b], None if new_lens is None else new_lens[b], x, blocks)
            if not slots:
                continue
            n = r + 1
            assert 0 < n <= blocks
            for h in range(Hkv):
                qt = q[b, h * G:(h + 1) * G][:, slots].reshape(-1, D)            # [G · tokens, D]
                lo, hi = bounds[b, h, :n, 0], bounds[b, h, :n, 1]                # [n, D]
                qm, qp = qt.clamp(max=0), qt.clamp(min=0)
                s = (qm @ lo.T + qp @ hi.T).amax(0).numpy()
                s_abs = (qm.abs() @ lo.abs().T + qp @ hi.abs().T).amax(0).numpy()
                scores[b, h, x, :n], tol[b, h, x, :n] = s, 4 * D * U * s_abs
                chosen, cnt = select_from_scores(s, K, sink, local)
                ids[b, h, x, :cnt], counts[b, h, x] = chosen, cnt
    return ids, counts, scores, tol


def run(mm, dev, q, bounds, k_lens, K, sink, local, new_lens=None):
    news = None if new_lens is None else torch.tensor(new_lens, device=dev, dtype=torch.int32)
    ids, counts, scores = mm.select_key_blocks_tiles(q.to(dev), bounds.to(dev), torch.tensor(k_lens, device=dev, dtype=torch.int32), K,
                                                     sink=sink, local=local, new_lens=news, return_scores=True)
    assert ids.dtype == torch.int32 and counts.dtype == torch.int32 and scores.dtype == torch.float32
    T = q.shape[2]
    assert ids.shape[2] == counts.shape[2] == scores.shape[2] == mm.block_attention_prefill_tiles(T) == tiles_of(T)
    return ids.cpu().numpy().astype(np.int64), counts.cpu().numpy().astype(np.int64), scores.cpu().numpy()


def assert_lists_follow_scores(ids, counts, scores, T, k_lens, new_lens, K, sink, local, what):
    """The selection is an exact function of the float32 scores the call returns."""
    B, Hkv, X, blocks = scores.shape
    for b in range(B):
        for x in range(X):
            r, slots = tile_slots(T, k_lens[b], None if new_lens is None else new_lens[b], x, blocks)
            for h in range(Hkv):
                if not slots:
                    assert counts[b, h, x] == 0 and (ids[b, h, x] == -1).all() and np.isneginf(scores[b, h, x]).all(), (what, b, h, x)
                    continue
                chosen, cnt = select_from_scores(scores[b, h, x, :r + 1].astype(np.float64), K, sink, local)
                assert counts[b, h, x] == cnt and np.array_equal(ids[b, h, x, :cnt], chosen), (what, b, h, x)
                assert (ids[b, h, x, cnt:] == -1).all() and np.isneginf(scores[b, h, x, r + 1:]).all(), (what, b, h, x)


# ---- 1. exact planted scores -------------------------------------------------------------------------------------------------------

def planted(B, Hkv, G, T, D, blocks, seed, dtype):
    """q with one non-zero coordinate per (token, head) — ±(1 … 4)·2⁻ᵏ, exact in both dtypes — and bounds of non-zero multiples
    of 1/8 in [−8, 8] with lo ≤ hi; a third of the blocks share the rows of blocks 2, 5 and 8, so scores tie.  Item 1's q is
    positive and every fourth block's bounds are negative: there every score of item 1 is NEGATIVE, and a slot without a token
    (item 1's tiles are partial) that took part with its zero row would raise it to 0."""
    g = torch.Generator().manual_seed(seed)
    q = torch.zeros((B, Hkv * G, T, D))
    d = torch.randint(0, D, (B, Hkv * G, T), generator=g)
    val = torch.randint(1, 5, d.shape, generator=g).float() * (torch.randint(0, 2, d.shape, generator=g) * 2 - 1) * 0.5 ** torch.randint(0, 3, d.shape, generator=g)
    val[1] = val[1].abs()
    q.scatter_(3, d[..., None], val[..., None])
    a = (torch.randint(-64, 65, (B, Hkv, blocks, D), generator=g).float() / 8)
    c = (torch.randint(-64, 65, (B, Hkv, blocks, D), generator=g).float() / 8)
    a, c = torch.where(a == 0, torch.tensor(0.125), a), torch.where(c == 0, torch.tensor(-0.125), c)
    lo, hi = torch.minimum(a, c), torch.maximum(a, c)
    for J in range(2, blocks, 3):
        lo[:, :, J], hi[:, :, J] = lo[:, :, 2 + 3 * (J // 3 % 3)], hi[:, :, 2 + 3 * (J // 3 % 3)]
    lo[:, :, 1::4], hi[:, :, 1::4] = -hi[:, :, 1::4].abs().maximum(lo[:, :, 1::4].abs()), -hi[:, :, 1::4].abs().minimum(lo[:, :, 1::4].abs())
    return q.to(dtype), torch.stack([lo, hi], 3).to(dtype)


@pytest.mark.parametrize("G", [1, 4, 16])
@pytest.mark.parametrize("n", [9, 64, 257, 513])
def test_1_exact_planted_scores_and_ties_at_the_kth_place(mm, dev, n, G):
    """T = 130 behind start = 64(n − 2) + 40: tile n − 2 holds 24 tokens, tile n − 1 all 64 (n candidates: 513 needs a third
    turn of the 16 waves × 16 blocks), tile n 42, the fourth none.  Item 1's new_lens = 50 empties its first tile and leaves
    8 tokens in the second.  Every product but one of a score is an exact zero: the float32 score is known on the CPU."""
    i = [9, 64, 257, 513].index(n) + [1, 4, 16].index(G)
    D, dtype = WIDTHS[i % 4], (torch.bfloat16, torch.float16)[(i // 2) % 2]
    B, Hkv, T, blocks = 2, 2, 130, n + 2
    k_lens, new_lens = [KB * (n - 2) + 40 + T] * 2, [T, 50]
    q, bounds = planted(B, Hkv, G, T, D, blocks, 1000 * n + G, dtype)
    ties = 0
    for sink, local in ((0, 1), (1, 2), (3, 5)):
        for K in sorted({sink + local + 1, max(n // 2, sink + local), n - 1}):
            r_ids, r_counts, r_scores, _ = reference(q, bounds, k_lens, new_lens, K, sink, local)
            ids, counts, scores = run(mm, dev, q, bounds, k_lens, K, sink, local, new_lens)
            what = f"n={n} G={G} D={D} K={K} sink={sink} local={local}"
            assert_same_bits(torch.from_numpy(scores), torch.from_numpy(r_scores.astype(np.float32)), what + ": scores")
            assert np.array_equal(counts, r_counts), what
            assert np.array_equal(ids, r_ids), what
            assert (counts[1, :, 0] == 0).all() and (counts[:, :, 3] == 0).all() and (counts[0, :, 1] == min(K, n)).all(), what
            assert (r_scores[1, :, 1:3, 1:n:4] < 0).all(), "precondition: item 1's scores of the negative blocks are negative"
            for b in range(B):
                for h in range(Hkv):
                    for x in range(3):
                        cnt, m = int(r_counts[b, h, x]), n - 1 + x
                        if cnt == 0 or cnt == m:
                            continue
                        unforced = [J for J in range(m) if not (J < sink or J >= m - local)]
                        chosen = set(r_ids[b, h, x, :cnt].tolist())
                        inside = [r_scores[b, h, x, J] for J in unforced if J in chosen]
                        if not inside:
                            continue
                        kth = min(inside)
                        tied = [J for J in unforced if r_scores[b, h, x, J] == kth]
                        ties += len(tied) >= 2 and any(J not in chosen for J in tied)
    assert ties > 0, "no tie across the K-th place: the tie rule went untested"


# ---- 2, 3. real operands ---------------------------------------------------------------------------------------------------------------

REAL = dict(B=1, Hkv=2, G=4, T=130, D=128, smax=32768, k_len=32700, K=32, sink=1, local=2, seed=2002)


@pytest.fixture(scope="module")
def real(mm, dev):
    """Normal keys and queries, the bounds of key_block_bounds, the float64 reference — taken once — and the device call."""
    p = REAL
    g = torch.Generator().manual_seed(p["seed"])
    k = torch.randn((p["B"], p["Hkv"], p["smax"], p["D"]), generator=g).to(torch.bfloat16)
    q = torch.randn((p["B"], p["Hkv"] * p["G"], p["T"], p["D"]), generator=g).to(torch.bfloat16)
    lens = torch.tensor([p["k_len"]], device=dev, dtype=torch.int32)
    bounds = mm.key_block_bounds(k.to(dev), lens, torch.zeros((p["B"], p["Hkv"], p["smax"] // KB, 2, p["D"]), device=dev, dtype=torch.bfloat16))
    ref = reference(q, bounds, [p["k_len"]], None, p["K"], p["sink"], p["local"])
    # the band: a condition on the inputs, asserted from the float64 reference BEFORE the device call
    r_ids, r_counts, r_scores, tol = ref
    for h in range(p["Hkv"]):
        for x in range(3):
            m, cnt = int(np.isfinite(r_scores[0, h, x]).sum()), int(r_counts[0, h, x])
            unforced = [J for J in range(m) if not (J < p["sink"] or J >= m - p["local"])]
            chosen = set(r_ids[0, h, x, :cnt].tolist())
            kth = min(r_scores[0, h, x, J] for J in unforced if J in chosen)
            band = [J for J in unforced if abs(r_scores[0, h, x, J] - kth) <= 2 * tol[0, h, x, J]]
            assert len(band) <= 0.02 * m, f"precondition: {len(band)} of {m} candidates in the band: choose another seed"
    got = run(mm, dev, q, bounds, [p["k_len"]], p["K"], p["sink"], p["local"])
    return q, k, bounds, ref, got


def test_2_real_scores_lie_within_the_summation_bound(real):
    _, _, _, (_, _, r_scores, tol), (_, _, scores) = real
    fin = np.isfinite(r_scores)
    assert np.array_equal(np.isneginf(scores), ~fin) and fin.sum() == 2 * (509 + 510 + 511)
    ratio = np.abs(scores[fin].astype(np.float64) - r_scores[fin]) / tol[fin]
    print(f"select_key_blocks_tiles D=128 G=4: largest score error / bound = {ratio.max():.4f} (bound 4·D·2^-24·s_abs)")
    assert ratio.max() <= 1.0, f"a score lies {ratio.max():.3f} bounds from float64"


def test_2_real_lists_are_the_ordering_of_the_returned_scores_and_close_on_float64(real):
    p = REAL
    _, _, _, (r_ids, r_counts, r_scores, tol), (ids, counts, scores) = real
    assert_lists_follow_scores(ids, counts, scores, p["T"], [p["k_len"]], None, p["K"], p["sink"], p["local"], "real operands")
    assert np.array_equal(counts, r_counts)
    for h in range(p["Hkv"]):
        for x in range(3):
            m, cnt = int(np.isfinite(r_scores[0, h, x]).sum()), int(r_counts[0, h, x])
            unforced = [J for J in range(m) if not (J < p["sink"] or J >= m - p["local"])]
            ref_chosen, chosen = set(r_ids[0, h, x, :cnt].tolist()), set(ids[0, h, x, :cnt].tolist())
            kth = min(r_scores[0, h, x, J] for J in unforced if J in ref_chosen)
            for J in range(m):
                if J not in unforced:
                    assert J in chosen, (h, x, J)
                elif r_scores[0, h, x, J] > kth + 2 * tol[0, h, x, J]:
                    assert J in chosen, (h, x, J)
                elif r_scores[0, h, x, J] < kth - 2 * tol[0, h, x, J]:
                    assert J not in chosen, (h, x, J)


def test_3_a_score_bounds_every_key_a_token_of_the_tile_sees(real):
    p = REAL
    q, k, _, (_, _, _, tol), (_, _, scores) = real
    G, D, T = p["G"], p["D"], p["T"]
    qd, kd = q.double(), k.double()
    checked = 0
    for x in range(3):
        r, slots = tile_slots(T, p["k_len"], None, x, p["smax"] // KB)
        pos = torch.tensor([p["k_len"] - T + t for t in slots])
        for h in range(p["Hkv"]):
            qt = qd[0, h * G:(h + 1) * G][:, slots]                                        # [G, tokens, D]
            dots = qt @ kd[0, h, :(r + 1) * KB].T                                          # [G, tokens, keys]
            seen = torch.arange((r + 1) * KB)[None, :] <= pos[:, None]                     # key j ≤ pos (pos < k_len)
            best = dots.masked_fill(~seen[None], -float("inf")).amax((0, 1)).reshape(r + 1, KB).amax(1).numpy()
            assert (best <= scores[0, h, x, :r + 1].astype(np.float64) + tol[0, h, x, :r + 1]).all(), (x, h)
            checked += r + 1
    assert checked == 2 * (509 + 510 + 511)


# ---- 4. invariance -----------------------------------------------------------------------------------------------------------------------

def test_4_a_tile_depends_on_its_own_item_and_positions_only(mm, dev):
    B, Hkv, G, T, D, blocks, dtype, K = 3, 2, 4, 130, 96, 24, torch.float16, 6
    g = torch.Generator().manual_seed(4004)
    q = torch.randn((B, Hkv * G, T, D), generator=g).to(dtype).to(dev)
    a, c = torch.randn((B, Hkv, blocks, D), generator=g), torch.randn((B, Hkv, blocks, D), generator=g)
    bounds = torch.stack([torch.minimum(a, c), torch.maximum(a, c)], 3).to(dtype).to(dev)
    k_lens = [1500, 131, 700]
    lens = torch.tensor(k_lens, device=dev, dtype=torch.int32)
    whole = mm.select_key_blocks_tiles(q, bounds, lens, K, return_scores=True)
    for b in range(B):  # B = 1 against inside B = 3
        one = mm.select_key_blocks_tiles(q[b:b + 1], bounds[b:b + 1], lens[b:b + 1], K, return_scores=True)
        assert torch.equal(whole[0][b:b + 1], one[0]) and torch.equal(whole[1][b:b + 1], one[1]), f"item {b} alone"
        assert_same_bits(whole[2][b:b + 1], one[2], f"item {b} alone: scores")
    # a strided q: a [B, T, Hq, D] buffer seen as [B, Hq, T, D]
    qs = q.transpose(1, 2).contiguous().transpose(1, 2)
    assert not qs.is_contiguous()
    again = mm.select_key_blocks_tiles(qs, bounds, lens, K, return_scores=True)
    assert torch.equal(again[0], whole[0]) and torch.equal(again[1], whole[1])
    assert_same_bits(again[2], whole[2], "a strided q")
    # T = 100 against the last 100 of 130 slots under new_lens = 100: the same tokens, so the same rows r
    news = torch.full((B,), 100, device=dev, dtype=torch.int32)
    long = mm.select_key_blocks_tiles(q, bounds, lens, K, new_lens=news, return_scores=True)
    short = mm.select_key_blocks_tiles(q[:, :, 30:], bounds, lens, K, return_scores=True)
    rows = 0
    for b, n in enumerate(k_lens):
        for xs in range(tiles_of(100)):
            r, slots = tile_slots(100, n, None, xs, blocks)
            xl = r - (n - 130) // KB
            if not slots:
                continue
            assert tile_slots(130, n, 100, xl, blocks) == (r, [t + 30 for t in slots])
            assert torch.equal(long[0][b, :, xl], short[0][b, :, xs]) and torch.equal(long[1][b, :, xl], short[1][b, :, xs]), (b, r)
            assert_same_bits(long[2][b, :, xl], short[2][b, :, xs], f"item {b} row {r}: scores")
            rows += 1
    assert rows == 3 + 3 + 2   # positions 1400 … 1499: rows 21, 22, 23; 31 … 130: 0, 1, 2; 600 … 699: 9, 10
    assert not torch.equal(long[2], whole[2])  # (the 30 slots without a token took part in `whole`)


# ---- 5. non-finite bounds ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_5_non_finite_bounds_keep_the_structure_and_nothing_outside_is_written(mm, capi, dev, dtype):
    """inf and NaN in the bounds, through the C entry: q inside a NaN buffer (read through its strides), the three outputs
    inside guarded buffers.  Only the structure is promised: the count, ascending distinct candidates, every forced block, −1
    from the count on, no store outside the rows."""
    B, Hkv, G, T, D, blocks, K, sink, local = 2, 2, 4, 130, 64, 40, 7, 2, 3
    g = torch.Generator().manual_seed(5005)
    q = torch.randn((B, Hkv * G, T, D), generator=g).to(dtype).to(dev)
    a, c = torch.randn((B, Hkv, blocks, D), generator=g), torch.randn((B, Hkv, blocks, D), generator=g)
    bounds = torch.stack([torch.minimum(a, c), torch.maximum(a, c)], 3)
    bounds[:, :, 1::4, 1, ::5] = float("inf")
    bounds[:, :, 2::4, 0, 1::7] = -float("inf")
    bounds[:, :, 3::4, :, 3::9] = NAN
    bounds = bounds.to(dtype).to(dev)
    k_lens = [2300, 131]
    lens = torch.tensor(k_lens, device=dev, dtype=torch.int32)
    X, items, pad = tiles_of(T), B * Hkv, 64
    pq = padded(q.reshape(B * Hkv * G, T, D), 0, NAN)
    ids = torch.full((pad + items * X * K + pad,), GUARD, dtype=torch.int32, device=dev)
    counts = torch.full((pad + items * X + pad,), GUARD, dtype=torch.int32, device=dev)
    scores = torch.full((pad + items * X * blocks + pad,), -7.5, dtype=torch.float32, device=dev)
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    fn = getattr(capi, "mi_block_select_tiles_" + ("bf16" if dtype == torch.bfloat16 else "f16"))
    fn.argtypes, fn.restype = 6 * [i32] + [vp, i64, i64, i64, vp, vp, i32, vp, i32] + 3 * [i32] + 4 * [vp], ctypes.c_int
    st = fn(items, Hkv, T, blocks * KB, D, G, pq.buf.data_ptr(), pq.ld, pq.stride, pq.stride * Hkv * G, bounds.data_ptr(), lens.data_ptr(), B,
            None, 0, K, sink, local, ids[pad:].data_ptr(), counts[pad:].data_ptr(), scores[pad:].data_ptr(),
            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0
    for buf, fill in ((ids, GUARD), (counts, GUARD), (scores, -7.5)):
        assert (buf[:pad] == fill).all() and (buf[-pad:] == fill).all(), "a store outside the outputs"
    ids, counts = ids[pad:-pad].reshape(B, Hkv, X, K).cpu().numpy(), counts[pad:-pad].reshape(B, Hkv, X).cpu().numpy()
    scores = scores[pad:-pad].reshape(B, Hkv, X, blocks).cpu().numpy()
    seen_nan = False
    for b in range(B):
        for x in range(X):
            r, slots = tile_slots(T, k_lens[b], None, x, blocks)
            for h in range(Hkv):
                n = r + 1 if slots else 0
                cnt = min(K, n)
                row = ids[b, h, x]
                assert counts[b, h, x] == cnt and (row[cnt:] == -1).all(), (b, h, x)
                assert (np.diff(row[:cnt]) > 0).all() and (row[:cnt] >= 0).all() and (row[:cnt] < max(n, 1)).all(), (b, h, x, row)
                forced = [J for J in range(n) if J < sink or J >= n - local]
                assert set(forced[:cnt] if len(forced) > cnt else forced) <= set(row[:cnt].tolist()), (b, h, x, row)
                assert np.isneginf(scores[b, h, x, n:]).all()
                seen_nan = seen_nan or bool(np.isnan(scores[b, h, x, :n]).any())
    assert seen_nan, "no NaN score: the inputs were to give some"
