"""The decode calls of DESIGN.md §3.18 – §3.20 at the lengths they were written for: lists of 16 and 64 entries, so that a
wave walks 3 … 16 entries in a row — the steady state of the walk: the transposed LDS image rewritten turn after turn, the
rescale of the online softmax between turns, in the paged forms the tile whose column and table entries the in-loop
look-ahead fetched, skipped entries in a row — and the combine kernel merges 4 … 64 partials.  The neighbouring files
(test_gpu_block_attention_decode{,_paged,_fp8}.py) stay at Smax = 512 with at most two turns per wave.

Shapes: MEDIUM Smax = 1024 (16 blocks), LONG Smax = 4096 (64 blocks); B = 2, Hkv = 2, G = 4 unless stated.  The layouts are
built here, seeded, unsorted, the diagonal never last: the last block row lists every block; one middle row (39 of 64, 9 of
16) lists every block up to its diagonal plus entries above the diagonal, placed so that a wave skips two entries in a row,
another skips the first entry of its chunk and another its last ones; the row below it is sparse (13 entries: one
workgroup's waves take 4, 3, 3, 3 turns); rows 15 and 16 of the long layout are fully causal (16 and 17 entries: a growing
cache goes from one non-empty default chunk to two); the other rows are short.  Every test asserts on the host, from the
layout, how many turns its waves take and how many partials its combine merges.

Accuracy is the project's rule e_dev ≤ 8 · e_ref, but PER CLASS: a class is the G rows of one (k / v item, token), and
scaled_err of the device result and of the yardstick (dense_step in fp32 narrowed, against dense_step in float64) is taken
over that class alone, with no floor from other classes.  On the whole tensor an item with a short list, whose outputs are
about 30 × larger than those of a 64-entry list, would set the scale, and a lost block of the long item would stay under the
bound.  lse keeps its bound of 1e-5 relative to float64.

THE SENSITIVITY PROOF.  Before it calls the device, every rule-based test shows on the CPU, in float64, on its own inputs,
for the classes of the longest list and of the skip row, that the two checks see ONE wrong list entry: (1) the lse with any
one computed entry dropped, or taken twice, differs from the true lse by at least 100 × the lse bound; (2) the output with
any one entry's V block replaced by the V block its wave held one turn earlier (list position p − 4, or the computed one
before that) has a class error of at least 1.5 · 8 · e_ref of the class; (3) so has the output with any one entry dropped.
These are conditions on the inputs (seed, G), not tolerances on the device; the minima are printed.  Where the diagonal
block of a token holds only a key or two (k_len = 64 · 39 + 2 with T = 3) the new tokens' keys point along their own
token's first query head with a score of 5, so that dropping that entry is visible too."""
import math
import os
import random

import pytest
import torch

from sparse_attention_helpers import FACTOR, rel_err, scaled_err
from test_gpu_block_attention_decode import (layout_from_rows, lens_tensor, operands, poison_unseen, references, stack_layouts,
                                             visible)
from test_gpu_block_attention_decode_fp8 import F8, codes, fp8, pools, queries, same, wide
from test_gpu_block_attention_decode_paged import paged, same_as_contiguous

pytestmark = pytest.mark.gpu

NAN = float("nan")
KB = 64                 # keys of a block
WAVES = 4               # waves of a workgroup: wave w walks entries w, w + 4, … of its chunk
MEDIUM, LONG = 1024, 4096
LSE_BOUND = 1e-5        # check_rule's bound on lse, relative to float64
LSE_MARGIN = 100.0      # a dropped or repeated entry moves lse by at least this many bounds
OUT_MARGIN = 1.5        # a stale V tile or a dropped entry gives at least OUT_MARGIN · FACTOR · e_ref
LOUD = 5.0              # score of a new token's own key where its diagonal block holds fewer than 32 visible keys


# ---- the layouts --------------------------------------------------------------------------------------------------------

def _unsorted(rng, cols, diag):
    """`cols` in a seeded order that is not ascending and does not end on the diagonal (one with a block below the diagonal)."""
    cols = list(cols)
    rng.shuffle(cols)
    while len(cols) > 1 and (cols == sorted(cols) or cols[-1] == diag):
        rng.shuffle(cols)
    return cols


def build_rows(blocks, skip_row, skip_at, sparse_len, causal_rows, seed):
    """The lists of the `blocks` layout rows: the last row full, `skip_row` every block up to its diagonal with entries
    above the diagonal at the list positions `skip_at`, the row below it `sparse_len` entries, `causal_rows` fully causal,
    the others the diagonal and up to two blocks below it, some with one entry above the diagonal."""
    rng = random.Random(seed)
    rows = []
    for i in range(blocks):
        if i == blocks - 1 or i in causal_rows:
            row = _unsorted(rng, range(i + 1), i)
        elif i == skip_row:
            below = _unsorted(rng, range(i + 1), i)
            above = rng.sample(range(i + 1, blocks), len(skip_at))
            row = [above.pop() if p in skip_at else below.pop(0) for p in range(i + 1 + len(skip_at))]
        elif i == skip_row - 1:
            row = _unsorted(rng, [i] + rng.sample(range(i), sparse_len - 1), i)
        else:
            row = [i] + rng.sample(range(i), min(i, rng.randrange(3)))
            if len(row) > 1 and rng.random() < 0.3:
                row.append(rng.randrange(i + 1, blocks))
            row = _unsorted(rng, row, i)
        rows.append(row)
    return rows


SKIP_ROW = {LONG: 39, MEDIUM: 9}
# list positions of the entries above the diagonal.  LONG, chunks of 16 (and one chunk of 64 alike): wave 1's first entry
# (1), wave 2 twice in a row (6, 10), wave 3's last two of the second chunk (27, 31), wave 0's first two of the third
# (32, 36), wave 1's last ones (45, 49).  MEDIUM, one chunk: wave 2's first two (2, 6), wave 1's last two (9, 13).
SKIP_AT = {LONG: (1, 6, 10, 20, 27, 31, 32, 36, 45, 49), MEDIUM: (2, 6, 9, 13)}
ROWS = {LONG: build_rows(64, 39, SKIP_AT[LONG], 13, (15, 16), 4096), MEDIUM: build_rows(16, 9, SKIP_AT[MEDIUM], 5, (), 1024)}
K_LENS = {1: {LONG: [LONG, KB * 39 + 40], MEDIUM: [MEDIUM, KB * 9 + 37]},   # T = 1: the second item inside the skip row
          3: {LONG: [LONG, KB * 39 + 2]}}                                  # T = 3: its tokens on rows 38, 39, 39


def computed(lst, p, pos, blocks):
    return 0 <= lst[p] < blocks and lst[p] * KB <= pos


def walk(lst, pos, chunk, blocks):
    """What the kernel does with the list `lst` of the row of pos under `chunk`: per launched chunk (⌈blocks / chunk⌉ of
    them, whatever the list's length) and wave, the list positions the wave visits, each with whether it is computed."""
    out = []
    for c in range(max(1, -(-blocks // chunk))):
        beg, end = min(len(lst), c * chunk), min(len(lst), (c + 1) * chunk)
        out.append([[(p, computed(lst, p, pos, blocks)) for p in range(beg + w, end, WAVES)] for w in range(WAVES)])
    return out


def turns(lst, pos, chunk, blocks):
    """Per launched chunk the four waves' numbers of computed entries."""
    return [[sum(ok for _, ok in wave) for wave in ch] for ch in walk(lst, pos, chunk, blocks)]


def assert_long(what, rows, k_len, T, chunk, smax):
    """A call is long when a wave takes ≥ 3 turns in one chunk or the combine merges ≥ 16 partials."""
    blocks = smax // KB
    most = max(max(max(ch) for ch in turns(rows[(k_len - T + t) // KB], k_len - T + t, chunk, blocks)) for t in range(T))
    partials = -(-blocks // chunk)
    assert most >= 3 or partials >= 16, f"{what}: chunk={chunk} gives {most} turns and {partials} partials"
    return most, partials


def assert_layout(smax):
    """The facts about the layout that the tests rely on, from the lists alone."""
    rows, blocks, r = ROWS[smax], smax // KB, SKIP_ROW[smax]
    assert len(rows) == blocks and sorted(rows[-1]) == list(range(blocks))
    for i, row in enumerate(rows):
        assert i in row and len(set(row)) == len(row) and all(0 <= j < blocks for j in row)
        assert len(row) == 1 or (row[-1] != i and row != sorted(row)), f"row {i}: unsorted, the diagonal not last"
        assert len(row) <= 5 or i in (blocks - 1, r, r - 1, 15, 16), f"row {i} is short"
    lst, pos = rows[r], KB * r + 1
    assert sorted(j for j in lst if j <= r) == list(range(r + 1)) and len(lst) == r + 1 + len(SKIP_AT[smax])
    assert [p for p in range(len(lst)) if not computed(lst, p, pos, blocks)] == list(SKIP_AT[smax])
    for chunk in (16, 64):  # the three skip cases, in chunks of 16 and in one chunk
        waves = [[ok for _, ok in wave] for ch in walk(lst, pos, chunk, blocks) for wave in ch if wave]
        assert any(not a and not b for wave in waves for a, b in zip(wave, wave[1:])), "two skipped entries in a row"
        assert any(not wave[0] and any(wave) for wave in waves), "a wave's first entry of a chunk is skipped"
        assert any(len(wave) > 2 and not wave[-1] and not wave[-2] and any(wave) for wave in waves), "a wave's last entries are skipped"
    if smax == LONG:
        assert len(rows[38]) == 13 and turns(rows[38], KB * 38 + 63, 16, blocks)[0] == [4, 3, 3, 3]
        assert sorted(rows[15]) == list(range(16)) and sorted(rows[16]) == list(range(17))


# ---- the inputs, the references and the two checks --------------------------------------------------------------------------------

def note(line):
    print(line)
    path = os.environ.get("MI_SOFTMAX_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


class Case:
    """The CPU side of one call: q [B, Hq, T, D], the clean cache k, v [B, Hkv, Smax, D] (any float type: what the device
    reads, widened or dequantised), the visibility mask, and the float64 reference, the yardstick and the float64 lse —
    computed once and shared by every call of the test."""

    def __init__(self, q, k, v, rows, k_lens, vis=None):
        self.q, self.k, self.v, self.rows, self.k_lens = q, k, v, rows, list(k_lens)
        (self.B, Hq, self.T, self.D), self.Hkv, self.smax = q.shape, k.shape[1], k.shape[2]
        self.G = Hq // self.Hkv
        self.vis = visible([rows], self.B, self.Hkv, self.T, self.k_lens, smax=self.smax) if vis is None else vis
        self.ref, self.yard, self.lse64 = references(q, k, v, self.vis, self.G)

    def pos(self, b, t):
        return self.k_lens[b] - self.T + t

    def classes(self):
        return [(b, h, t) for b in range(self.B) for h in range(self.Hkv) for t in range(self.T)]

    def rows_of(self, x, b, h, t):
        return x[b, h * self.G:(h + 1) * self.G, t]


def make_loud(q, k, k_lens, G):
    """Where the diagonal block of a token holds fewer than 32 visible keys, the token's own key points along the query of
    the first head of each group, at a score of LOUD under scale = 1 / √D: dropping the block moves lse and out visibly."""
    B, Hq, T, D = q.shape
    for b in range(B):
        for t in range(T):
            pos = k_lens[b] - T + t
            if pos >= 0 and pos % KB + 1 < 32:
                for h in range(k.shape[1]):
                    own = q[b, h * G, t].double()
                    k[b, h, pos] = (own * (LOUD * math.sqrt(D) / float(own @ own))).to(k.dtype)


def make_case(smax, G, T, D, dtype, seed, B=2, Hkv=2, k_lens=None):
    """Operands from the neighbours' `operands`, drawn on the CPU (the proof runs there before the device sees them)."""
    k_lens = K_LENS[T][smax] if k_lens is None else k_lens
    q, k, v = operands("cpu", B, Hkv, G, T, D, dtype, seed, smax=smax)
    make_loud(q, k, k_lens, G)
    return Case(q, k, v, ROWS[smax], k_lens)


def prove(what, case, classes):
    """The sensitivity proof of the module's docstring for the classes (b, h, t) given; returns the minimum ratios
    (lse change / bound, stale-tile error / e_ref, dropped-entry error / e_ref)."""
    nb, D, G = case.smax // KB, case.D, case.G
    worst = [float("inf")] * 3
    for b, h, t in classes:
        pos = case.pos(b, t)
        lst = case.rows[pos // KB]
        qc, kc, vc = case.rows_of(case.q, b, h, t).double(), case.k[b, h].double(), case.v[b, h].double()
        mask = case.vis[b, h, t]
        s = ((qc @ kc.T) / math.sqrt(D)).masked_fill(~mask, -float("inf"))
        m = s.max(-1, keepdim=True).values
        e = torch.exp(s - m).reshape(G, nb, KB)
        vb = vc.reshape(nb, KB, D)
        w = e.sum(-1)                                   # [G, nb]: the blocks' shares of the row sum
        o = torch.einsum("gjs,jsd->gjd", e, vb)         # [G, nb, D]: … and of the unnormalised output
        L, O = w.sum(-1, keepdim=True), o.sum(1)
        out, lse = O / L, (m + torch.log(L)).squeeze(-1)
        ref, yard = case.rows_of(case.ref, b, h, t), case.rows_of(case.yard, b, h, t)
        assert float((out - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), "the proof's float64 result is the reference's"
        assert float((lse - case.rows_of(case.lse64, b, h, t)).abs().max()) <= 1e-9
        e_ref = scaled_err(yard.numpy(), ref.numpy())
        assert e_ref > 0
        live = [(p, j) for p, j in enumerate(lst) if computed(lst, p, pos, nb) and bool(mask[j * KB:(j + 1) * KB].any())]
        assert len(live) >= 10, (what, b, h, t)
        for p, j in live:
            share = w[:, j:j + 1] / L
            for moved in (torch.log1p(-share), torch.log1p(share)):   # the entry dropped, the entry taken twice
                worst[0] = min(worst[0], float((moved.squeeze(-1) / lse).abs().max()) / LSE_BOUND)
            dropped = (O - o[:, j]) / (L - w[:, j:j + 1])
            worst[2] = min(worst[2], scaled_err(dropped.numpy(), ref.numpy()) / e_ref)
            before = [j2 for p2, j2 in live if p2 < p and (p - p2) % WAVES == 0]   # the wave's earlier tiles
            if p >= WAVES and before:
                stale = (O - o[:, j] + torch.einsum("gs,sd->gd", e[:, j], vb[before[-1]])) / L
                worst[1] = min(worst[1], scaled_err(stale.numpy(), ref.numpy()) / e_ref)
    note(f"{what}: sensitivity over {len(classes)} classes: a dropped / repeated entry moves lse by ≥ {worst[0]:.0f} bounds, "
         f"a stale V tile gives ≥ {worst[1]:.1f} · e_ref, a dropped entry ≥ {worst[2]:.1f} · e_ref")
    assert worst[0] >= LSE_MARGIN, f"{what}: the lse check would miss an entry ({worst[0]:.0f} bounds): another seed"
    assert worst[1] >= OUT_MARGIN * FACTOR, f"{what}: the rule would miss a stale V tile ({worst[1]:.1f} · e_ref): another seed"
    assert worst[2] >= OUT_MARGIN * FACTOR, f"{what}: the rule would miss a dropped entry ({worst[2]:.1f} · e_ref): another seed"
    return worst


def prove_long_and_skip(what, case):
    """… for the classes of the longest list (item 0, the last token) and of the skip row (item 1, its tokens on that row)."""
    r = SKIP_ROW[case.smax]
    classes = [(0, h, case.T - 1) for h in range(case.Hkv)]
    assert len(case.rows[case.pos(0, case.T - 1) // KB]) == case.smax // KB
    if len(case.k_lens) > 1 and any(case.pos(1, t) // KB == r for t in range(case.T)):
        classes += [(1, h, t) for h in range(case.Hkv) for t in range(case.T) if case.pos(1, t) // KB == r]
        assert len(classes) > case.Hkv
    return prove(what, case, classes)


def check_classes(what, out, lse, case):
    """The rule e_dev ≤ FACTOR · e_ref on every class (b, h, t) alone — none left out, no floor from the others —, zero rows
    and lse −inf where a token sees nothing, lse to LSE_BOUND of float64."""
    assert out.dtype == case.q.dtype and tuple(out.shape) == tuple(case.q.shape), what
    out, lse = out.cpu(), lse.cpu()
    assert torch.isfinite(out.float()).all(), what
    assert lse.dtype == torch.float32 and tuple(lse.shape) == tuple(case.q.shape[:3]), what
    ratios, refs = [], []
    for b, h, t in case.classes():
        got, ref, yard = (case.rows_of(x, b, h, t) for x in (out, case.ref, case.yard))
        if not bool(case.vis[b, h, t].any()):
            assert (got == 0).all() and (case.rows_of(lse, b, h, t) == -float("inf")).all(), f"{what}: class {(b, h, t)} sees nothing"
            continue
        e_ref, e_dev = scaled_err(yard.numpy(), ref.numpy()), scaled_err(got.double().numpy(), ref.numpy())
        assert e_dev <= FACTOR * e_ref, f"{what}: class {(b, h, t)} (pos {case.pos(b, t)}): e_dev {e_dev:.3e} > {FACTOR:g} · e_ref {e_ref:.3e}"
        ratios.append(e_dev / e_ref if e_ref > 0 else 0.0)
        refs.append(e_ref)
    seen = case.vis.any(-1).repeat_interleave(case.G, 1)
    e_lse = rel_err(lse[seen].double().numpy(), case.lse64[seen].numpy())
    note(f"block attention decode long, {what}: {len(ratios)} classes, e_dev / e_ref {min(ratios):.2f} … {max(ratios):.2f} "
         f"(e_ref {min(refs):.2e} … {max(refs):.2e}); lse max rel err {e_lse:.2e}")
    assert e_lse <= LSE_BOUND, f"{what}: lse differs from float64 by {e_lse:.3e} relative"


def on(dev, *xs):
    return [x.to(dev) for x in xs]


# ---- 1. contiguous, medium ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [32, 64, 96, 128])
def test_1_contiguous_medium_lists_of_sixteen(mm, dev, dtype, D):
    """16 entries (k_len = 1024) and the skip row (k_len = 613: 10 computed entries among 14) under chunk None (one chunk
    of 4 turns per wave, no combine), 12 (3 turns, then a chunk of 4 single turns) and 5; NaN in every key no token sees."""
    smax, blocks, T, k_lens = MEDIUM, MEDIUM // KB, 1, K_LENS[1][MEDIUM]
    assert_layout(smax)
    case = make_case(smax, 4, T, D, dtype, 3100 + D)
    full = ROWS[smax][-1]
    default = mm._decode_chunk(smax, D)
    assert_long("medium", ROWS[smax], k_lens[0], T, default, smax)
    assert turns(full, smax - 1, 16, blocks) == [[4, 4, 4, 4]]
    assert turns(full, smax - 1, 12, blocks) == [[3, 3, 3, 3], [1, 1, 1, 1]]
    assert [sum(ch) for ch in turns(full, smax - 1, 5, blocks)] == [5, 5, 5, 1]
    prove_long_and_skip(f"medium {dtype} D={D}", case)
    layout, lens = layout_from_rows(ROWS[smax], dev), lens_tensor(k_lens, dev)
    q, k, v = on(dev, case.q, poison_unseen(case.k, case.vis), poison_unseen(case.v, case.vis))
    for chunk in (None, 12, 5):
        out, lse = mm.block_sparse_attention_decode(q, k, v, layout, lens, chunk=chunk, return_lse=True)
        check_classes(f"medium {dtype} D={D} chunk={chunk}", out, lse, case)


# ---- 2. contiguous, long --------------------------------------------------------------------------------------------------------------

# (the seeds: where the first one did not meet the proof's margins in bfloat16, a later one of the same sequence + 1000 · i)
LONG_FORMS = [(D, (torch.bfloat16, torch.float16)[j % 2], seed) for j, (D, seed) in enumerate([(32, 8232), (64, 3264), (96, 5296), (128, 3328)])]


def assert_long_chunks(mm, D):
    """The walks of the 64-entry list under the long chunk values, and that each is long."""
    rows, blocks, full = ROWS[LONG], LONG // KB, ROWS[LONG][-1]
    default = mm._decode_chunk(LONG, D)
    assert_long("chunk=None", rows, LONG, 1, default, LONG)
    assert turns(full, LONG - 1, 16, blocks) == 4 * [[4, 4, 4, 4]]                       # None today: 4 chunks of 4 turns
    assert turns(full, LONG - 1, 64, blocks) == [[16, 16, 16, 16]]                        # one chunk, no combine launch
    assert assert_long("chunk=1", rows, LONG, 1, 1, LONG) == (1, 64)                       # 64 partials
    assert turns(full, LONG - 1, 7, blocks) == 9 * [[2, 2, 2, 1]] + [[1, 0, 0, 0]]        # 10 chunks, the last ragged
    return default


@pytest.mark.parametrize("D,dtype,seed", LONG_FORMS)
def test_2_contiguous_long_lists_of_sixty_four(mm, dev, D, dtype, seed):
    """k_lens 4096 and 64 · 39 + 2 with T = 3: the tokens of item 0 walk the 64-entry list, those of item 1 stand on rows
    38 (13 entries), 39 and 39 (the skip row).  chunk None, 64, 1 and 7, each under the per-class rule; one chunk is one
    chunk (64 against 4096), None is the module's constant."""
    smax, T, k_lens = LONG, 3, K_LENS[3][LONG]
    assert_layout(smax)
    default = assert_long_chunks(mm, D)
    assert [(k_lens[1] - T + t) // KB for t in range(T)] == [38, 39, 39]
    case = make_case(smax, 4, T, D, dtype, seed)
    prove_long_and_skip(f"long {dtype} D={D}", case)
    layout, lens = layout_from_rows(ROWS[smax], dev), lens_tensor(k_lens, dev)
    q, k, v = on(dev, case.q, poison_unseen(case.k, case.vis), poison_unseen(case.v, case.vis))
    got = {}
    for chunk in (None, 64, 1, 7, 4096, default):
        got[chunk] = mm.block_sparse_attention_decode(q, k, v, layout, lens, chunk=chunk, return_lse=True)
    for chunk in (None, 64, 1, 7):
        check_classes(f"long {dtype} D={D} chunk={chunk}", got[chunk][0], got[chunk][1], case)
    same(got[64], got[4096], "one chunk either way")
    same(got[None], got[default], "chunk=None")


# ---- 3. groups ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G,D,dtype,seed", [(1, 64, torch.float16, 3301), (16, 96, torch.bfloat16, 7316)])
def test_3_group_sizes(mm, dev, G, D, dtype, seed):
    """One query head per k / v head (a class is one row: float16, whose e_ref lets the rule see one entry of 64) and the
    full tile of 16, at the long shape with T = 3 under the default chunk."""
    smax, T, k_lens = LONG, 3, K_LENS[3][LONG]
    default = assert_long_chunks(mm, D)
    case = make_case(smax, G, T, D, dtype, seed)
    prove_long_and_skip(f"long G={G} {dtype} D={D}", case)
    layout, lens = layout_from_rows(ROWS[smax], dev), lens_tensor(k_lens, dev, torch.int64)
    q, k, v = on(dev, case.q, poison_unseen(case.k, case.vis), poison_unseen(case.v, case.vis))
    out, lse = mm.block_sparse_attention_decode(q, k, v, layout, lens, return_lse=True)
    check_classes(f"long G={G} {dtype} D={D} chunk=None ({default})", out, lse, case)


# ---- 4. bit relations at the long shape ----------------------------------------------------------------------------------------------------

BIT_CHUNKS = (None, 7)


def test_4_an_item_of_a_batch_is_the_call_on_it_alone(mm, dev):
    smax, T, D, dtype, k_lens = LONG, 3, 64, torch.bfloat16, [LONG, KB * 39 + 2, KB * 16 + 5]
    assert_long_chunks(mm, D)
    layout = layout_from_rows(ROWS[smax], dev)
    q, k, v = operands(dev, 3, 2, 4, T, D, dtype, 3401, smax=smax)
    lens = lens_tensor(k_lens, dev)
    for chunk in BIT_CHUNKS:
        out, lse = mm.block_sparse_attention_decode(q, k, v, layout, lens, chunk=chunk, return_lse=True)
        assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
        for b in range(3):
            one = mm.block_sparse_attention_decode(q[b:b + 1], k[b:b + 1], v[b:b + 1], layout, lens[b:b + 1], chunk=chunk, return_lse=True)
            same((out[b:b + 1], lse[b:b + 1]), one, f"chunk={chunk}: item {b} alone")


def test_4_shared_layout_against_the_layout_repeated_per_item(mm, dev):
    smax, B, Hkv, T, D, dtype, k_lens = LONG, 2, 2, 3, 96, torch.float16, K_LENS[3][LONG]
    assert_long_chunks(mm, D)
    layout = layout_from_rows(ROWS[smax], dev)
    repeated = stack_layouts([layout] * (B * Hkv), (B, Hkv), dev)
    q, k, v = operands(dev, B, Hkv, 4, T, D, dtype, 3402, smax=smax)
    lens = lens_tensor(k_lens, dev)
    for chunk in BIT_CHUNKS:
        shared = mm.block_sparse_attention_decode(q, k, v, layout, lens, chunk=chunk, return_lse=True)
        assert torch.isfinite(shared[0].float()).all()
        same(mm.block_sparse_attention_decode(q, k, v, repeated, lens, chunk=chunk, return_lse=True), shared,
             f"chunk={chunk}: the layout repeated per item")


@pytest.mark.parametrize("form,D,dtype", [("BHSD", 32, torch.float16), ("BSHD", 128, torch.bfloat16)])
def test_4_a_strided_cache_against_its_contiguous_clone(mm, dev, form, D, dtype):
    """Row stride D + 8 in a buffer of NaN, [B, Hkv, Smax, D] and the transposed view of [B, Smax, Hkv, D], NaN in every
    key no token sees."""
    smax, B, Hkv, T, k_lens = LONG, 2, 2, 3, K_LENS[3][LONG]
    assert_long_chunks(mm, D)
    layout = layout_from_rows(ROWS[smax], dev)
    q, k, v = operands(dev, B, Hkv, 4, T, D, dtype, 3403 + D, smax=smax)
    vis = visible([ROWS[smax]], B, Hkv, T, k_lens, smax=smax)

    def strided(x):
        shape = (B, Hkv, smax, D + 8) if form == "BHSD" else (B, smax, Hkv, D + 8)
        buf = torch.full(shape, NAN, device=dev, dtype=dtype)
        view = buf[..., :D] if form == "BHSD" else buf[..., :D].transpose(1, 2)
        view.copy_(poison_unseen(x, vis))
        return view

    ks, vs = strided(k), strided(v)
    assert not ks.is_contiguous() and ks.stride(2) > D and ks.shape == k.shape
    lens = lens_tensor(k_lens, dev)
    for chunk in BIT_CHUNKS:
        out, lse = mm.block_sparse_attention_decode(q, ks, vs, layout, lens, chunk=chunk, return_lse=True)
        assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
        clone = mm.block_sparse_attention_decode(q, ks.contiguous(), vs.contiguous(), layout, lens, chunk=chunk, return_lse=True)
        same((out, lse), clone, f"chunk={chunk} {form}: the strided cache against its contiguous clone")


# ---- 5. paged, long ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("page,D,dtype,seed", [(16, 128, torch.bfloat16, 7516), (32, 96, torch.float16, 3532), (64, 64, torch.bfloat16, 3564),
                                               (256, 32, torch.float16, 3756)])
def test_5_paged_long(mm, dev, page, D, dtype, seed):
    """From a wave's third turn on the tile comes from the column and the table entries the in-loop look-ahead read: 16
    turns under chunk=64, 4 under the default.  A shuffled table, three unreferenced NaN pages, NaN in every unseen key: the
    bits of the contiguous call on the gathered cache, and the per-class rule."""
    smax, T, k_lens = LONG, 3, K_LENS[3][LONG]
    assert_long_chunks(mm, D)
    case = make_case(smax, 4, T, D, dtype, seed)
    prove_long_and_skip(f"paged long page={page} {dtype} D={D}", case)
    layout, lens = layout_from_rows(ROWS[smax], dev), lens_tensor(k_lens, dev)
    q, k, v = on(dev, case.q, poison_unseen(case.k, case.vis), poison_unseen(case.v, case.vis))
    kp, vp, table = paged(k, v, page, 3501 + page)
    assert kp.shape[0] == 2 * (smax // page) + 3 and not torch.equal(table.flatten().sort().values, table.flatten())
    for chunk in (None, 64):
        out, lse = same_as_contiguous(mm, f"page {page} chunk={chunk}", q, kp, vp, table, layout, lens, chunk=chunk)
        check_classes(f"paged long page={page} {dtype} D={D} chunk={chunk}", out, lse, case)


# ---- 6. paged, holes met in steady state ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("page,D,dtype,seed", [(16, 64, torch.float16, 3616), (128, 128, torch.bfloat16, 6728)])
def test_6_paged_holes_in_steady_state(mm, dev, page, D, dtype, seed):
    """Table entries −1 and P under seen keys of the 64-entry list, in blocks at list positions ≥ 8 — met in a wave's turn
    ≥ 3 under chunk=64 — and the pool pages they named NaN: finite, and the rule and lse hold with those keys removed from
    the mask.  A page of 16 keys takes a quarter of a tile away, a page of 128 two whole tiles."""
    smax, T, k_lens, blocks = LONG, 3, K_LENS[3][LONG], LONG // KB
    full = ROWS[smax][-1]
    at = {j: p for p, j in enumerate(full)}
    per = max(1, page // KB)     # blocks of a logical page
    pages = [lp for lp in range(smax // page) if all(at[(lp * page) // KB + i] >= 8 for i in range(per))]
    holes = [pages[1], pages[len(pages) // 2], pages[-2]]
    assert turns(full, smax - 1, 64, blocks) == [[16, 16, 16, 16]]
    for lp in holes:   # with every entry computed, list position p is turn p // 4 + 1 of wave p % 4
        assert all(at[(lp * page) // KB + i] // WAVES + 1 >= 3 for i in range(per))
    q, k, v = operands("cpu", 2, 2, 4, T, D, dtype, seed, smax=smax)
    make_loud(q, k, k_lens, 4)
    vis = visible([ROWS[smax]], 2, 2, T, k_lens, smax=smax)
    unseen = ~vis.any(2)
    for lp in holes:
        assert vis[0, :, :, lp * page:(lp + 1) * page].all(), "a page of seen keys"
        vis[0, :, :, lp * page:(lp + 1) * page] = False
    case = Case(q, k, v, ROWS[smax], k_lens, vis)
    prove_long_and_skip(f"holes page={page}", case)
    layout, lens = layout_from_rows(ROWS[smax], dev), lens_tensor(k_lens, dev)
    qd, kd, vd = on(dev, q, k, v)
    kd[unseen.to(dev)] = NAN
    vd[unseen.to(dev)] = NAN
    kp, vp, table = paged(kd, vd, page, 3601 + page)
    P = kp.shape[0]
    for i, lp in enumerate(holes):
        kp[int(table[0, lp])] = NAN
        vp[int(table[0, lp])] = NAN
        table[0, lp] = (-1, P)[i % 2]
    out, lse = mm.block_sparse_attention_decode_paged(q=qd, k_pages=kp, v_pages=vp, block_table=table, layout=layout, k_lens=lens,
                                                      chunk=64, return_lse=True)
    check_classes(f"holes page={page} {dtype} D={D} chunk=64", out, lse, case)


# ---- 7. fp8, long -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("page,D,dtype,seed", [(0, 128, torch.bfloat16, 6828), (0, 32, torch.float16, 3732), (16, 64, torch.bfloat16, 3780),
                                               (16, 96, torch.float16, 3812), (64, 32, torch.bfloat16, 5796), (64, 128, torch.float16, 3892)])
def test_7_fp8_long(mm, dev, page, D, dtype, seed):
    """The e4m3fn cache, contiguous (page = 0) and paged, under the default chunk and chunk=64: without scales the bits of
    the 2-byte call on the widened cache; with per-head scales, none a power of two, the per-class rule against float64 on
    the dequantised cache."""
    smax, B, Hkv, G, T, k_lens = LONG, 2, 2, 4, 1, K_LENS[1][LONG]
    assert_long_chunks(mm, D)
    layout, lens = layout_from_rows(ROWS[smax], dev), lens_tensor(k_lens, dev)
    q = queries(seed, "cpu", B, Hkv * G, T, D, dtype)
    kc, vc = codes(seed + 1, B, Hkv, smax, D), codes(seed + 2, B, Hkv, smax, D)
    ks, vs = torch.tensor([0.37, 0.9]), torch.tensor([0.11, 3.3])
    kd, vd = (c.view(F8).to(torch.float32).double() * s.double().reshape(1, Hkv, 1, 1) for c, s in ((kc, ks), (vc, vs)))
    case = Case(q, kd, vd, ROWS[smax], k_lens)
    prove_long_and_skip(f"fp8 long page={page} {dtype} D={D}", case)
    qd = q.to(dev)
    if page:
        kp, vp, table = pools(kc, vc, page, 3703 + page)
        tab = table.to(dev)
        call8 = lambda **kw: mm.block_sparse_attention_decode_paged_fp8(qd, fp8(kp, dev), fp8(vp, dev), tab, layout, lens,  # noqa: E731
                                                                        return_lse=True, **kw)
        kw_, vw_ = wide(kp, dtype, dev), wide(vp, dtype, dev)
        call16 = lambda **kw: mm.block_sparse_attention_decode_paged(qd, kw_, vw_, tab, layout, lens, return_lse=True, **kw)  # noqa: E731
    else:
        call8 = lambda **kw: mm.block_sparse_attention_decode_fp8(qd, fp8(kc, dev), fp8(vc, dev), layout, lens,  # noqa: E731
                                                                  return_lse=True, **kw)
        kw_, vw_ = wide(kc, dtype, dev), wide(vc, dtype, dev)
        call16 = lambda **kw: mm.block_sparse_attention_decode(qd, kw_, vw_, layout, lens, return_lse=True, **kw)  # noqa: E731
    for chunk in (None, 64):
        got = call8(chunk=chunk)
        assert torch.isfinite(got[0].float()).all()
        same(got, call16(chunk=chunk), f"fp8 page={page} {dtype} D={D} chunk={chunk}: the 2-byte call on the widened cache")
    out, lse = call8(k_scale=ks.to(dev), v_scale=vs.to(dev))
    check_classes(f"fp8 long page={page} {dtype} D={D} per-head scales", out, lse, case)


# ---- 8. graph capture ---------------------------------------------------------------------------------------------------------------------------------

def test_8_one_graph_replayed_while_long_caches_grow(mm, dev):
    """One capture of the long contiguous call under the default chunk.  Item 0 grows 1023 → 1026: its token goes from row
    15 (16 entries: one non-empty chunk) to row 16 (17 entries: the second chunk stops being empty); item 1 grows
    4093 → 4096 on the 64-entry list.  Before each replay the new k / v rows and q are written in place; after it the
    replay has the bits of the eager call and is under the per-class rule."""
    smax, B, Hkv, G, T, D, dtype = LONG, 2, 2, 4, 1, 128, torch.float16
    default = assert_long_chunks(mm, D)
    rows = ROWS[smax]
    assert default == 16 and len(rows[15]) == 16 and len(rows[16]) == 17
    assert [sum(ch) for ch in turns(rows[15], 1023, default, smax // KB)] == [16, 0, 0, 0]
    assert [sum(ch) for ch in turns(rows[16], 1024, default, smax // KB)] == [16, 1, 0, 0]
    layout = layout_from_rows(rows, dev)
    q_host, k_host, v_host = operands("cpu", B, Hkv, G, T, D, dtype, 3801, smax=smax)
    q, k, v = on(dev, q_host, k_host, v_host)
    lens = lens_tensor([1023, 4093], dev, torch.int64)
    g = torch.Generator().manual_seed(3802)
    run = lambda: mm.block_sparse_attention_decode(q, k, v, layout, lens, return_lse=True)  # noqa: E731
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()  # warm-up on the side stream: the layout's lists are built here
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # a host synchronisation in here would fail the capture
        out, lse = run()
    previous = None
    for step, host_lens in enumerate(([1024, 4094], [1025, 4095], [1026, 4096])):
        for b, n in enumerate(host_lens):
            k_host[b, :, n - 1] = torch.randn((Hkv, D), generator=g).to(dtype)
            v_host[b, :, n - 1] = torch.randn((Hkv, D), generator=g).to(dtype)
        q_host = torch.randn(q.shape, generator=g).to(dtype)
        case = Case(q_host, k_host, v_host, rows, host_lens)
        prove(f"replay {step}", case, [(1, h, 0) for h in range(Hkv)])
        with torch.no_grad():
            lens += 1
            for b, n in enumerate(host_lens):
                k[b, :, n - 1] = k_host[b, :, n - 1].to(dev)
                v[b, :, n - 1] = v_host[b, :, n - 1].to(dev)
            q.copy_(q_host.to(dev))
        assert lens.tolist() == host_lens
        want = run()
        out.fill_(NAN)
        lse.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        same((out, lse), want, f"replay {step}, k_lens {host_lens}")
        check_classes(f"replay {step}, k_lens {host_lens}", out, lse, case)
        assert previous is None or not torch.equal(previous, out)
        previous = out.clone()
