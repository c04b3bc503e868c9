"""matmuls.select_key_blocks on the GPU at the sizes where its threshold search and its emission run:
planted scores — any float32 bit pattern, exact — from one wave's worth of candidates to the cap of 16 384, with 0 < R < U in
every case so that neither shortcut is taken; real operands at ~3000 candidates in a three-part check; a NaN head; the null
scores pointer at scale; and the append → bounds → select → decode loop from an empty cache.

R is the number of slots left for the unforced candidates and U the number of unforced candidates.  Every condition a case
claims (0 < R < U, ties at the R-th place that are not all taken, ties across thread ranges and waves, the band of part B) is
computed from the numpy reference alone and asserted on the CPU before the device call."""
import numpy as np
import pytest
import torch

from gpu_helpers import assert_same_bits
from test_gpu_block_attention_decode import check_rule, lens_tensor
from test_gpu_block_attention_decode_selected import vis_of_lists
from test_gpu_block_select import integer_operands

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
NS = [9, 64, 65, 1023, 1024, 1025, 2049, 16384]   # one wave, one pass of the 1024-thread loop, per = 1 → 2 → 3, the cap
NANS = [0x7FC00000, 0xFFC00000, 0x7FFF0000, 0xFF810000]   # quiet and signalling NaN patterns of both signs (bfloat16 pieces)
BASE = 0x4B000000                                 # 2²³: its six low hex digits are mantissa bits


def bits_f32(b):
    return np.asarray(b, np.uint32).view(np.float32)


# ---- planting --------------------------------------------------------------------------------------------------------------

def pieces(x, low_bits):
    """x (float32) as three float32 pieces a, b, c with ((0 + a) + b) + c == x in float32: a is x with its `low_bits` low
    pattern bits cleared, b the same truncation of x − a, c the rest.  low_bits = 16: the pieces are bfloat16 values;
    13: float16 values (11 + 11 + 2 significant bits) for |x| in [2¹⁰, 2¹⁵).  Non-finite x and 0: a = x, b = c = 0."""
    x = np.asarray(x, np.float32)
    mask = np.uint32((0xFFFFFFFF >> low_bits) << low_bits)
    fin = np.isfinite(x)
    xf = np.where(fin, x, np.float32(0))
    a = (xf.view(np.uint32) & mask).view(np.float32)
    r = xf - a
    b = (r.view(np.uint32) & mask).view(np.float32)
    c = r - b
    a = np.where(fin, a, x)
    return a, b, c


def planted(x, dtype):
    """bounds rows [n, 2, 32] in `dtype` whose score against q = (1, 1, 1, 0, …) is x bit for bit — checked here on the CPU:
    every piece survives the narrowing, and the kernel's order ((+0 + a) + b) + c gives x in float32."""
    x = np.asarray(x, np.float32)
    a, b, c = pieces(x, 16 if dtype == torch.bfloat16 else 13)
    rows = np.zeros((len(x), 32), np.float32)
    rows[:, 0], rows[:, 1], rows[:, 2] = a, b, c
    if dtype == torch.bfloat16:                                        # the high half-words as they are: a NaN keeps its sign
        assert not (rows.view(np.uint32) & 0xFFFF).any(), "a planted piece does not fit bfloat16"
        narrow = torch.from_numpy((rows.view(np.uint32) >> 16).astype(np.uint16).view(np.int16)).view(torch.bfloat16)
    else:
        narrow = torch.from_numpy(rows).to(dtype)
    assert_same_bits(narrow.float(), torch.from_numpy(rows), "a planted piece does not fit the operand type")
    assert not ((np.abs(rows) < (2.0 ** -126 if dtype == torch.bfloat16 else 2.0 ** -14)) & (rows != 0)).any(), "a subnormal piece"
    with np.errstate(invalid="ignore"):
        total = ((np.float32(0) + a) + b) + c
    assert_same_bits(total, x, "the pieces do not sum to the planted score")
    return torch.stack([narrow, narrow], 1)


def launch(mm, dev, xs, k_lens, K, sink, local, dtype=torch.bfloat16, return_scores=True, T=3):
    """One call with B = len(xs) items, Hkv = 1, G = 1, D = 32: item b's block J scores xs[b][J] for every token."""
    n = len(xs[0])
    q = torch.zeros((len(xs), 1, T, 32), dtype=dtype)
    q[..., :3] = 1
    bounds = torch.stack([planted(x, dtype) for x in xs])[:, None]
    assert bounds.shape == (len(xs), 1, n, 2, 32)
    got = mm.select_key_blocks(q.to(dev), bounds.to(dev), torch.tensor(k_lens, device=dev, dtype=torch.int32), K, sink=sink,
                               local=local, return_scores=return_scores)
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.int32
    return [g.cpu().numpy() for g in got]


# ---- the reference: plain numpy on the float32 scores ---------------------------------------------------------------------------

def order_of(s):
    """Candidate indices in the contract's order: numbers before NaN, value descending (−0 == +0), index ascending."""
    nan = np.isnan(s)
    with np.errstate(invalid="ignore"):                               # (widening a signalling NaN raises the flag)
        v = np.where(nan, 0.0, s.astype(np.float64))
    return np.lexsort((np.arange(len(s)), -v, nan))


def same_place(x, y):
    return (np.isnan(x) & np.isnan(y)) | (x == y)


def token(s, K, sink, local):
    """The contract for one token with candidate scores s: (ascending list, count, facts about the R-th place)."""
    n = len(s)
    sink_n = min(sink, n)
    local_from = max(n - local, sink_n)
    forced = np.zeros(n, bool)
    forced[:sink_n], forced[local_from:] = True, True
    order = order_of(s)
    rest = order[~forced[order]]
    count = min(K, n)
    R, U = count - int(forced.sum()), len(rest)
    chosen = np.sort(np.concatenate([np.nonzero(forced)[0], rest[:max(R, 0)]]))
    assert len(chosen) == count
    facts = dict(n=n, R=R, U=U, tied=np.zeros(0, np.int64), open_tie=False)
    if 0 < R < U:
        tied = rest[same_place(s[rest], s[rest[R - 1]])]
        facts.update(tied=np.sort(tied), open_tie=bool(same_place(s[rest[R]], s[rest[R - 1]])))
    return chosen, count, facts


def expected(xs, k_lens, K, sink, local, T=3):
    """(ids [B, 1, T, K], counts [B, 1, T], scores [B, 1, T, n] float32, facts[b][t]) of a planted launch."""
    B, n = len(xs), len(xs[0])
    ids, counts = np.full((B, 1, T, K), -1, np.int32), np.zeros((B, 1, T), np.int32)
    scores, facts = np.full((B, 1, T, n), -np.inf, np.float32), []
    for b in range(B):
        facts.append([])
        for t in range(T):
            pos = min(max(k_lens[b], 0), 64 * n) - T + t
            cand = pos // 64 + 1 if pos >= 0 else 0
            chosen, count, f = token(np.asarray(xs[b][:cand], np.float32), K, sink, local)
            ids[b, 0, t, :count], counts[b, 0, t] = chosen, count
            scores[b, 0, t, :cand] = xs[b][:cand]
            facts[b].append(f)
    return ids, counts, scores, facts


def lens_of(n):
    """Item 0: tokens with n − 1, n and n candidates; item 1: three tokens with max(n // 3, 1) candidates."""
    return [64 * (n - 1) + 2, 64 * (max(n // 3, 1) - 1) + 3]


def pairs_of(n):
    """(sink, local); at n = 9 the pair (3, 5) would leave one unforced candidate, so (2, 3) stands in for it."""
    return [(0, 1), (1, 2), (3, 5) if n > 9 else (2, 3)]


def ks_of(n, sink, local):
    """forced + 1, about n / 2, n − 2 and n − 1.  At K = n − 1 item 0's first token (n − 1 candidates) lists everything — the
    `all` shortcut — and its other two tokens search; at every other K all three search."""
    forced = sink + local
    return sorted({forced + 1, max(n // 2, forced + 1), max(n - 2, forced + 1), n - 1})


def conditions(facts0, n, K, ties):
    """None if item 0's tokens exercise what the case claims, else the reason (conditions on the inputs alone)."""
    per = -(-n // 1024)
    for t, f in enumerate(facts0):
        if t == 0 and K == n - 1:
            continue                                                   # n − 1 candidates, K of them: documented in ks_of
        if not 0 < f["R"] < f["U"]:
            return f"token {t}: R = {f['R']}, U = {f['U']}: a shortcut is taken"
        if ties:
            if len(f["tied"]) < 2 or not f["open_tie"]:
                return f"token {t}: {len(f['tied'])} candidates tie with the R-th, or all of them are taken"
            if n >= 2049 and not (f["tied"][-1] // (64 * per) > f["tied"][0] // (64 * per)):
                return f"token {t}: the ties stay inside one wave's span of {64 * per} indices"   # (a wave holds 64 ranges)
    return None


def run_fixed(mm, dev, xs, n, K, sink, local, dtype, tag, want):
    """The device call on planted scores against `want` = expected(…): score bits first, then counts and lists, exactly."""
    r_ids, r_counts, r_scores, _ = want
    ids, counts, scores = launch(mm, dev, xs, lens_of(n), K, sink, local, dtype)
    assert_same_bits(scores, r_scores, f"{tag}: the scores are not the planted bits")
    assert np.array_equal(counts, r_counts), tag
    bad = np.argwhere(ids != r_ids)
    assert len(bad) == 0, (tag, f"{len(bad)} list entries differ, first at {bad[:3].tolist()}: got "
                           f"{[int(ids[tuple(i)]) for i in bad[:3]]} want {[int(r_ids[tuple(i)]) for i in bad[:3]]}")
    return ids, counts, scores


def seeds_of(n):
    return range(4000 if n <= 100 else 100)


def run_case(mm, dev, make, n, K, sink, local, ties, dtype=torch.bfloat16, what=""):
    """make(seed) → the planted scores of item 0; the first seed that meets the conditions is used (a search on the CPU, over
    the inputs alone).  Item 1 gets the same family under another seed."""
    for seed in seeds_of(n):
        xs = [make(seed), make(seed + 7919)]
        want = expected(xs, lens_of(n), K, sink, local)
        why = conditions(want[3][0], n, K, ties)
        if why is None:
            break
    else:
        raise AssertionError(f"{what} n={n} K={K} ({sink}, {local}): no seed meets the conditions: {why}")
    got = run_fixed(mm, dev, xs, n, K, sink, local, dtype, f"{what} n={n} K={K} sink={sink} local={local} seed={seed}", want)
    return xs, got, want[3]


def sweep(mm, dev, maker, n, ties, dtype=torch.bfloat16, what=""):
    for sink, local in pairs_of(n):
        for K in ks_of(n, sink, local):
            run_case(mm, dev, maker, n, K, sink, local, ties, dtype, what)


# ---- A. score families ------------------------------------------------------------------------------------------------------------

def random_bits(n, seed, lo_exp=32, hi_exp=254):
    g = np.random.default_rng(seed)
    sign = g.integers(0, 2, n, dtype=np.uint32) << 31
    return bits_f32(sign | (g.integers(lo_exp, hi_exp + 1, n, dtype=np.uint32) << 23) | g.integers(0, 1 << 23, n, dtype=np.uint32))


@pytest.mark.parametrize("n", NS)
def test_a1_random_bits(mm, dev, n):
    """Uniform 32-bit patterns of both signs with exponent field in [32, 254]: every round of the search meets a random digit."""
    sweep(mm, dev, lambda seed: random_bits(n, 1000 * n + seed), n, ties=False, what="random bits")


@pytest.mark.parametrize("r", range(6))
@pytest.mark.parametrize("n", NS)
def test_a2_one_digit_decides(mm, dev, n, r):
    """Every key is 2²³ except hex digit r (r = 0: the last round), drawn from 0 … 15: ties everywhere, and the R-th and the
    (R + 1)-th key can differ at digit r only — asserted on the patterns — and here tie."""
    def make(seed):
        g = np.random.default_rng(100000 * r + 10 * n + seed)
        b = np.uint32(BASE) | (g.integers(0, 16, n, dtype=np.uint32) << np.uint32(4 * r))
        assert not ((b ^ np.uint32(BASE)) & ~np.uint32(0xF << (4 * r))).any()
        return bits_f32(b)
    sweep(mm, dev, make, n, ties=True, what=f"digit {r}")


@pytest.mark.parametrize("value", [bits_f32(0xC2F6E979), -np.inf, np.nan, None], ids=["finite", "neg_inf", "nan", "nan_patterns"])
@pytest.mark.parametrize("n", NS)
def test_a3_all_equal(mm, dev, n, value):
    """Every unforced candidate ties (n = 16 384, (0, 1): 16 383 ties in the packed high half-word): the list is the forced
    blocks and the lowest R unforced indices.  NaN patterns of both signs, quiet and signalling, are one place in the order."""
    for sink, local in pairs_of(n):
        for K in ks_of(n, sink, local):
            def make(seed):                                            # None: every score a NaN, of four patterns: all one place
                return np.full(n, value, np.float32) if value is not None else bits_f32([NANS[(J + seed) % 4] for J in range(n)])
            _, (ids, counts, _), _ = run_case(mm, dev, make, n, K, sink, local, True, what="all equal")
            for t, cand in enumerate((n - 1, n, n)):
                forced = sink + local
                want = list(range(sink + K - forced)) + list(range(cand - local, cand)) if K < cand else list(range(cand))
                assert ids[0, 0, t, :counts[0, 0, t]].tolist() == want, (n, K, sink, local, t)


@pytest.mark.parametrize("side", ["fewer_high_than_slots", "more_high_than_slots"])
@pytest.mark.parametrize("n", NS)
def test_a4_two_values(mm, dev, n, side):
    """m copies of a high value at seeded positions, a low value elsewhere.  m < R: the threshold is the low value and R − m of
    its many ties are taken; m > R: the threshold is the high value."""
    hi, lo = bits_f32(0x4E9A3C71), bits_f32(0xBD0F00A5)
    for sink, local in pairs_of(n):
        for K in ks_of(n, sink, local):
            R, U = K - sink - local, n - sink - local
            m = R // 2 if side[0] == "f" else min(U, R + max(2, (U - R) // 2))

            def make(seed):
                g = np.random.default_rng(31 * n + 7 * K + seed)
                x = np.full(n, lo, np.float32)
                x[sink + g.permutation(U)[:m]] = hi                    # among the unforced candidates of the n-candidate tokens
                return x
            _, _, facts = run_case(mm, dev, make, n, K, sink, local, True, what=f"two values, m = {m}")
            for f in facts[0][1:]:
                assert f["R"] == R and f["U"] == U and len(f["tied"]) == (U - m if m < R else m)


@pytest.mark.parametrize("n", NS)
def test_a5_specials(mm, dev, n):
    """+inf, −inf, NaN patterns of both signs, +0, negative and positive numbers and a repeated lowest finite value L, shuffled.  Three K put the
    threshold on L (the last finite above the −inf's), inside the −inf's, and inside the NaNs (the search ends at key 0); K is
    worked out from the planted classes among the unforced candidates.  (−0 cannot be planted: a sum that starts at +0 never
    gives −0.)  At n = 9 only (0, 1) leaves the eight unforced candidates that the seven L / −inf / NaN copies need."""
    L = bits_f32(0xFE9C4B21)                                           # a large negative number below every other finite one
    for sink, local in pairs_of(n)[:1 if n == 9 else 3]:
        forced, U = sink + local, n - sink - local
        n_l, n_ninf, n_nan = max(2, U // 9), max(2, U // 9), max(3, U // 9)
        extra = n - n_l - n_ninf - n_nan
        for where in range(3):
            for seed in seeds_of(n):
                rnd = random_bits(extra, 977 * n + seed, 100, 150)   # |x| < 2²⁴: above L, below +inf
                fill = [np.float32(np.inf), np.float32(0), None, None]
                xs = []
                for s in (seed, seed + 7919):
                    x = np.array([L] * n_l + [-np.inf] * n_ninf + [bits_f32(NANS[i % 4]) for i in range(n_nan)] +
                                 [rnd[i] if fill[i % 4] is None else fill[i % 4] for i in range(extra)], np.float32)
                    xs.append(x[np.random.default_rng(53 * n + s).permutation(n)])
                u = xs[0][sink:n - local]                              # the unforced candidates of the n-candidate tokens
                at_l, at_ninf, at_nan = int((u == L).sum()), int(np.isneginf(u).sum()), int(np.isnan(u).sum())
                above = len(u) - at_l - at_ninf - at_nan
                K = forced + [above + max(1, at_l // 2), above + at_l + max(1, at_ninf // 2), above + at_l + at_ninf + max(1, at_nan // 2)][where]
                if K > n - 2:
                    continue
                want = expected(xs, lens_of(n), K, sink, local)
                tied_at = [xs[0][f["tied"][0]] if len(f["tied"]) else np.float32(1) for f in want[3][0]]
                in_class = all([v == L, np.isneginf(v), np.isnan(v)][where] for v in tied_at)
                if conditions(want[3][0], n, K, ties=True) is None and in_class:
                    break
            else:
                raise AssertionError(f"specials n={n} ({sink}, {local}) where={where}: no seed meets the conditions")
            run_fixed(mm, dev, xs, n, K, sink, local, torch.bfloat16, f"specials {where} n={n} K={K} ({sink}, {local}) seed={seed}", want)


def test_a6_float16_entry(mm, dev):
    """mi_block_select_f16 on planted scores: float16 pieces of 11 + 11 + 2 bits, magnitudes in [2¹⁰, 2¹⁵), both signs (the
    split is verified in planted()); a pool of n // 8 patterns, so the R-th place ties.  The selection code is shared."""
    n = 2049

    def make(seed):
        g = np.random.default_rng(4242 + seed)
        return random_bits(n // 8, 99 + seed, 137, 141)[g.integers(0, n // 8, n)]
    sweep(mm, dev, make, n, ties=True, dtype=torch.float16, what="float16")


def test_a7_a_nan_head_is_passed_over(mm, dev):
    """G = 2 with head 0's q NaN at d = 0: every s_0 is NaN and fmaxf passes it over — lists, counts and score bits are the
    G = 1 call on head 1 alone.  Both heads NaN: every score is NaN, the list is the forced blocks and the lowest unforced."""
    B, Hkv, T, D, blocks, K, sink, local = 2, 2, 3, 32, 300, 150, 1, 2
    q, bounds = integer_operands(B, Hkv, 2, T, D, blocks, 777, torch.bfloat16)
    q[:, 0::2, :, 0] = float("nan")
    lens = torch.tensor([64 * (blocks - 1) + 2, 64 * 100 + 3], device=dev, dtype=torch.int32)
    got = mm.select_key_blocks(q.to(dev), bounds.to(dev), lens, K, sink=sink, local=local, return_scores=True)
    alone = mm.select_key_blocks(q[:, 1::2].contiguous().to(dev), bounds.to(dev), lens, K, sink=sink, local=local, return_scores=True)
    assert not torch.isnan(got[2]).any()
    assert torch.equal(got[0], alone[0]) and torch.equal(got[1], alone[1])
    assert_same_bits(got[2], alone[2], "a NaN head: the scores of the other head alone")
    s = alone[2].cpu().numpy()
    for b, cands in enumerate(((299, 300, 300), (101, 101, 101))):     # … and the call alone is the contract on its own scores
        for h in range(Hkv):
            for t, cand in enumerate(cands):
                chosen, count, f = token(s[b, h, t, :cand], K, sink, local)
                assert (0 < f["R"] < f["U"]) == (cand > K)
                assert got[0][b, h, t, :count].tolist() == chosen.tolist() and int(got[1][b, h, t]) == count
    q[:, 1::2, :, 0] = float("nan")
    ids, counts, scores = mm.select_key_blocks(q.to(dev), bounds.to(dev), lens, K, sink=sink, local=local, return_scores=True)
    for b, cands in enumerate(((299, 300, 300), (101, 101, 101))):
        for t, cand in enumerate(cands):
            assert torch.isnan(scores[b, :, t, :cand]).all() and torch.isneginf(scores[b, :, t, cand:]).all()
            want = list(range(K - local)) + list(range(cand - local, cand)) if cand > K else list(range(cand))
            for h in range(Hkv):
                assert ids[b, h, t, :int(counts[b, h, t])].tolist() == want, (b, h, t)


def test_a8_lists_without_scores_are_the_lists_with_scores(mm, dev):
    """The null `scores` pointer at n = 2049 (three passes of the emission's ranges), random bits."""
    n, k_lens = 2049, lens_of(2049)
    xs = [random_bits(n, 5), random_bits(n, 6)]
    for K, sink, local in ((4, 1, 2), (1024, 3, 5), (2047, 0, 1)):
        r_ids, r_counts, _, facts = expected(xs, k_lens, K, sink, local)
        assert conditions(facts[0], n, K, ties=False) is None
        with_scores = launch(mm, dev, xs, k_lens, K, sink, local)
        without = launch(mm, dev, xs, k_lens, K, sink, local, return_scores=False)
        assert len(without) == 2
        for got in (with_scores, without):
            assert np.array_equal(got[0], r_ids) and np.array_equal(got[1], r_counts), K


# ---- B. real operands at scale ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,G,dtype", [(64, 1, torch.bfloat16), (64, 4, torch.float16), (64, 16, torch.bfloat16),
                                       (128, 1, torch.float16), (128, 4, torch.bfloat16), (128, 16, torch.float16)])
def test_b_real_operands_at_three_thousand_candidates(mm, dev, D, G, dtype):
    """Random normal q and bounds (as test_2 of test_gpu_block_select.py), ~3000 candidates.  No seed gives a clean K-th gap at
    this size, so the check has three parts, none of which takes the code under test for the truth:
      1. scores within 2·D·2⁻²⁴·s_abs of the float64 scores (the bound derived in that test_2's docstring);
      2. lists and counts are the contract's ordering of the float32 scores the call returned — selection is an exact function
         of those bits;
      3. closure against float64: with tol that bound and v the float64 score of the R-th unforced candidate, every unforced
         candidate above v + 2·tol is listed and every one below v − 2·tol is not.  The candidates within ±2·tol of v are left
         unjudged; that they are at most 2 % of a token's candidates is a condition on the inputs, asserted from the float64
         reference before the device call (normal data meets it as it is: no wider spread of the bounds was needed)."""
    B, Hkv, T, blocks, sink, local = 2, 1, 3, 3001, 1, 2
    g = torch.Generator().manual_seed(8000 + D + G)
    q = torch.randn((B, Hkv * G, T, D), generator=g).to(dtype)
    a, c = torch.randn((B, Hkv, blocks, D), generator=g), torch.randn((B, Hkv, blocks, D), generator=g)
    bounds = torch.stack([torch.minimum(a, c), torch.maximum(a, c)], 3).to(dtype)
    k_lens = [64 * (blocks - 1) + 2, 64 * 2000 + 3]
    cands = [[blocks - 1, blocks, blocks], [2001, 2001, 2001]]
    q64, lo64, hi64 = q.double().numpy(), bounds[:, 0, :, 0].double().numpy(), bounds[:, 0, :, 1].double().numpy()
    s64, tol = np.full((B, T, blocks), -np.inf), np.zeros((B, T))
    for b in range(B):
        for t in range(T):
            n = cands[b][t]
            per_head = [np.maximum(q64[b, h, t] * lo64[b, :n], q64[b, h, t] * hi64[b, :n]).sum(-1) for h in range(G)]
            s_abs = max(np.maximum(np.abs(q64[b, h, t] * lo64[b, :n]), np.abs(q64[b, h, t] * hi64[b, :n])).sum(-1).max() for h in range(G))
            s64[b, t, :n], tol[b, t] = np.max(per_head, 0), 2 * D * EPS * s_abs
    for K in (16, blocks // 16, blocks // 2):
        judged = []
        for b in range(B):
            for t in range(T):
                n, R = cands[b][t], K - sink - local
                unforced = np.arange(sink, n - local)
                v = np.sort(s64[b, t, unforced])[::-1][R - 1]
                band = np.abs(s64[b, t, unforced] - v) <= 2 * tol[b, t]
                assert 0 < R < len(unforced) and band.sum() <= 0.02 * n, f"precondition: {band.sum()} of {n} candidates in the band"
                judged.append((b, t, unforced[s64[b, t, unforced] > v + 2 * tol[b, t]], unforced[s64[b, t, unforced] < v - 2 * tol[b, t]], band.sum() / n))
        ids, counts, scores = (x.cpu().numpy() for x in mm.select_key_blocks(
            q.to(dev), bounds.to(dev), torch.tensor(k_lens, device=dev, dtype=torch.int32), K, sink=sink, local=local, return_scores=True))
        worst = 0.0
        for b, t, must, must_not, share in judged:
            n = cands[b][t]
            assert np.isneginf(scores[b, 0, t, n:]).all()
            err = np.abs(scores[b, 0, t, :n].astype(np.float64) - s64[b, t, :n]).max()
            worst = max(worst, err / tol[b, t])
            assert err <= tol[b, t], (b, t, err, tol[b, t])                                    # 1
            chosen, count, _ = token(scores[b, 0, t, :n], K, sink, local)
            assert counts[b, 0, t] == count == K and np.array_equal(ids[b, 0, t], chosen), (b, t)  # 2
            listed = set(ids[b, 0, t].tolist())
            assert all(J in listed for J in must.tolist()) and not any(J in listed for J in must_not.tolist()), (b, t)  # 3
        print(f"D={D} G={G} {dtype} K={K}: max score error / bound {worst:.3f}; band shares " + " ".join(f"{j[4]:.4f}" for j in judged))


# ---- D. the loop --------------------------------------------------------------------------------------------------------------------

def test_d_seventy_steps_from_an_empty_cache(mm, dev):
    """append → key_block_bounds(last=T) → select_key_blocks → block_sparse_attention_decode_selected, eagerly, T alternating 1
    and 3, from k_lens [0, 61]: item 0 starts empty and both items cross block boundaries at different steps.  After every
    step the incrementally kept bounds have the bits of a full recomputation and the lists are the contract's ordering of the
    returned scores; every tenth step out and lse meet float64 attention over the listed blocks."""
    B, Hkv, G, D, dtype, smax, K, sink, local = 2, 2, 4, 64, torch.float16, 512, 3, 1, 1
    g = torch.Generator(device=dev).manual_seed(9701)
    k, v = (torch.zeros((B, Hkv, smax, D), device=dev, dtype=dtype) for _ in range(2))
    prefix = torch.randn((Hkv, 61, D), device=dev, generator=g).to(dtype)
    k[1, :, :61], v[1, :, :61] = prefix, prefix.flip(1)
    host_lens = [0, 61]
    lens = lens_tensor(host_lens, dev)
    bounds = torch.full((B, Hkv, smax // 64, 2, D), 3.25, device=dev, dtype=dtype)
    mm.key_block_bounds(k, lens, bounds)                                # the prefix of item 1; item 0 has no key yet
    crossings = [0, 0]
    for step in range(70):
        T = 1 if step % 2 == 0 else 3
        q = torch.randn((B, Hkv * G, T, D), device=dev, generator=g).to(dtype)
        k_new, v_new = (torch.randn((B, Hkv, T, D), device=dev, generator=g).to(dtype) for _ in range(2))
        for b in range(B):
            crossings[b] += (host_lens[b] + T - 1) // 64 > max(host_lens[b] - 1, 0) // 64
        host_lens = [x + T for x in host_lens]
        lens += T
        mm.kv_cache_append(k_new, v_new, k, v, lens)
        mm.key_block_bounds(k, lens, bounds, last=T)
        ids, counts, scores = mm.select_key_blocks(q, bounds, lens, K, sink=sink, local=local, return_scores=True)
        out, lse = mm.block_sparse_attention_decode_selected(q, k, v, ids, counts, lens, return_lse=True)
        full = mm.key_block_bounds(k, lens)
        s, h_ids, h_counts = scores.cpu().numpy(), ids.cpu().numpy(), counts.cpu().numpy()
        for b, n in enumerate(host_lens):
            nb = (n + 63) // 64
            assert_same_bits(bounds[b, :, :nb], full[b, :, :nb], f"step {step}, item {b}: the kept bounds")
            assert (bounds[b, :, nb:] == 3.25).all(), f"step {step}, item {b}: a block without a key was written"
            for h in range(Hkv):
                for t in range(T):
                    cand = (n - T + t) // 64 + 1
                    chosen, count, _ = token(s[b, h, t, :cand], K, sink, local)
                    assert h_counts[b, h, t] == count and h_ids[b, h, t, :count].tolist() == chosen.tolist(), (step, b, h, t)
                    assert (h_ids[b, h, t, count:] == -1).all() and np.isneginf(s[b, h, t, cand:]).all()
        if step % 10 == 9 or step == 69:
            check_rule(f"loop step {step}", out, q, k, v, vis_of_lists(ids, counts, host_lens, T, smax), G, lse)
    assert host_lens == [140, 201] and crossings[0] >= 2 and crossings[1] >= 2
