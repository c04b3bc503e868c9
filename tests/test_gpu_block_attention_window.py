"""window= and sink= of the sixteen reading calls on the MI355X: the token at pos sees key j iff the call's own
rule holds and (j > pos − W or j < S).  Accuracy is the project's rule e_dev ≤ 8 · e_ref against dense masked float64 attention
under a mask built here from the rule alone; everything else is bit for bit: a window that hides nothing against the plain call,
the forms against each other, block-aligned windows against today's list kernel with the hidden ids struck out, unaligned windows
against today's kernel on a cache whose hidden slots underflow, NaN in hidden keys, the prefill decompositions, a graph replay.

Smax = 512, B ≤ 4, Hkv = 2, chunk=2.  The caches hold e4m3fn-representable values, so one set of operands serves the 2-byte and the
fp8 forms.  The window's two edges are PLANTED so that an off-by-one cannot hide under the rule: the query of a planted row points
along an axis of its own; in k / v head 0 the keys pos − W and pos − W + 1, in head 1 the keys S and S − 1 point along that axis —
a key the rule hides with a score about 20, one it shows with about 16, the rest below 3 — with a value row of +128 where hidden
and −128 where shown (a row holds one edge: with both shown plants in one row, hiding either would move nothing).  Every other row
has its own key as its one high score, so that no row weighs a ±128 row like an ordinary key.  Checked on the
CPU before a kernel runs: the float64 reference of the row moves by ≥ 100 × the rule's allowance 8 · e_ref · max |ref| when a
hidden plant is shown and when a shown plant is hidden.  A planted row is −128 · (1 − 10⁻⁴): e_ref is set by the other rows."""
import functools

import pytest
import torch

from gpu_helpers import assert_same_bits
from sparse_attention_helpers import FACTOR, assert_tensor_under_rule, rel_err, scaled_err
from test_gpu_block_attention_decode import SMAX, check_rule, layout_from_rows, lens_tensor, references, visible
from test_gpu_block_attention_decode_fp8 import F8, codes, pools
from test_gpu_block_attention_decode_paged import paged

pytestmark = pytest.mark.gpu

NAN = float("nan")
TOP = 2 ** 31 - 1
BLOCKS, KB, K_SLOTS = SMAX // 64, 64, 8
CALLS = [(lists, page, f8) for lists in (False, True) for page in (0, 16) for f8 in (False, True)]  # the 8 calls of a kind
PAGES64 = [(lists, 64, f8) for lists in (False, True) for f8 in (False, True)]
DTYPES = [torch.bfloat16, torch.float16]
WINDOWS, SINKS = (1, 5, 64, 65, 100), (0, 4, 70)
FULL = [list(range(r + 1)) for r in range(BLOCKS)]  # the fully kept causal layout
form_id = lambda f: f"{'lists' if f[0] else 'layout'}-page{f[1]}-{'fp8' if f[2] else '2byte'}"  # noqa: E731


def banded(mm, W, S):
    """The rows of matmuls.sliding_window_layout(Smax, W, S)."""
    keep = mm.sliding_window_layout(SMAX, W, S)
    assert keep.dtype == torch.bool and tuple(keep.shape) == (BLOCKS, BLOCKS)
    return [[c for c in range(BLOCKS) if keep[r, c]] for r in range(BLOCKS)]


def clamp(n, lo, hi):
    return min(max(int(n), lo), hi)


def window_visible(rows, B, Hkv, T, k_lens, W, S, new_lens=None):
    """The plain rule's mask [B, Hkv, T, Smax] of `visible`, cut by the window: key j stays iff j > pos − W or j < S."""
    vis = visible([rows], B, Hkv, T, k_lens)
    j = torch.arange(SMAX)
    for b in range(B):
        for t in range(T):
            pos = clamp(k_lens[b], 0, SMAX) - T + t
            vis[b, :, t] &= (j > pos - W) | (j < S)
        if new_lens is not None:
            vis[b, :, :T - clamp(new_lens[b], 0, T)] = False
    return vis


# ---- operands: e4m3fn-representable caches, planted edges ------------------------------------------------------------------------

def amplitudes(D):
    """(the shown plant's key element, the hidden plant's): scores of about 16 and 20 under q's 4 and the scale 1 / √D, rounded to
    e4m3fn."""
    return tuple(float(torch.tensor(x * D ** 0.5).to(F8).float()) for x in (4.0, 5.0))


def planted(B, Hkv, G, T, D, k_lens, W, S, rows_of_item, seed):
    """(q, k, v, plants) float32 on the CPU.  The cache is random finite e4m3fn values with |x| < 4.  Every row of q is
    4 · e_axis + 0.02 · noise: the planted rows rows_of_item(b) = [(t, axis)] on axes of their own, every other row t on axis
    3 + t mod (D − 3).  For a planted row at pos: in head 0 the keys pos − W (where the rule hides it) and pos − W + 1, in head 1 —
    for the item's FIRST planted row only, the sink keys being every row's — the keys S (where the rule hides it) and S − 1 are zero
    but for `axis`: the hidden plant's element or the shown plant's; the value row is +128 or −128 likewise.  So a planted row holds at
    most one shown and one hidden plant per head.  Every (row, head) WITHOUT a shown plant gets its own key — which it always sees —
    as its one high score, with the value row the key has: no row weighs a ±128 row like an ordinary key, which keeps e_ref at the size
    of the rest's weight.  plants: [(b, h, t, j, hidden)]."""
    assert Hkv == 2 and min(T, W + 1) <= D - 3  # rows that see each other's own keys stand on axes of their own
    g = torch.Generator().manual_seed(seed)
    q = 0.02 * torch.randn((B, Hkv * G, T, D), generator=g)
    k = codes(seed + 1, B, Hkv, SMAX, D).view(F8).float()
    v = codes(seed + 2, B, Hkv, SMAX, D).view(F8).float()
    shown, hid = amplitudes(D)
    plants = []
    for b in range(B):
        start = clamp(k_lens[b], 0, SMAX) - T
        axes = {t: 3 + t % (D - 3) for t in range(T)}
        axes.update(dict(rows_of_item(b)))
        has_shown, plant_keys = set(), set()
        for n, (t, axis) in enumerate(rows_of_item(b)):
            pos = start + t
            if pos < 0:
                continue
            for h, keys in ((0, (pos - W, pos - W + 1)), (1, (S, S - 1) if n == 0 else ())):
                for first_hidden, j in zip((True, False), keys):
                    hidden = not (j > pos - W or j < S)
                    if not 0 <= j <= pos or hidden != first_hidden:  # (pos − W may be a sink key, S may lie inside the window)
                        continue
                    k[b, h, j] = 0.0
                    k[b, h, j, axis] = hid if hidden else shown
                    v[b, h, j] = 128.0 if hidden else -128.0
                    plants.append((b, h, t, j, hidden))
                    plant_keys.add((h, j))
                    if not hidden:
                        has_shown.add((t, h))
        for t in range(T):
            pos = start + t
            if pos < 0:
                continue
            q[b, :, t, axes[t]] += 4.0
            for h in range(Hkv):
                if (t, h) not in has_shown:
                    if (h, pos) not in plant_keys:
                        k[b, h, pos] = 0.0
                    k[b, h, pos, axes[t]] = shown
    return q, k, v, plants


def assert_the_edges_would_show(what, q, k, v, vis, plants, G, dtype, refs):
    """On the CPU, before the kernel: for every plant, the float64 reference of its row with that ONE key's visibility flipped — a
    hidden plant shown, a shown plant hidden — differs from the true row by ≥ 100 × the rule's allowance 8 · e_ref · max |ref|."""
    ref, yard, _ = refs
    e_ref = scaled_err(yard.double().numpy(), ref.numpy())
    need = 100.0 * FACTOR * e_ref * float(ref.abs().max())
    qd, kd, vd = q.to(dtype).double(), k.to(dtype).double(), v.to(dtype).double()
    kinds = {True: float("inf"), False: float("inf")}
    for b, h, t, j, hidden in plants:
        mask = vis[b, h, t].clone()
        assert bool(mask[j]) != hidden, (what, b, h, t, j)
        mask[j] = hidden  # flipped
        s = (qd[b, h * G:(h + 1) * G, t] @ kd[b, h].T) / q.shape[-1] ** 0.5  # [G, Smax]
        if mask.any():
            row = torch.softmax(s.masked_fill(~mask, -float("inf")), -1) @ vd[b, h]
        else:
            row = torch.zeros_like(ref[b, h * G:(h + 1) * G, t])
        move = float((row - ref[b, h * G:(h + 1) * G, t]).abs().amax(-1).min())
        kinds[hidden] = min(kinds[hidden], move)
        assert move >= need, f"{what}: plant {(b, h, t, j)} ({'hidden' if hidden else 'shown'}) flipped moves the reference by {move:.3e} < {need:.3e}"
    print(f"{what}: e_ref {e_ref:.3e}, needed {need:.3e}; the smallest move of a hidden plant shown {kinds[True]:.3e}, of a shown plant "
          f"hidden {kinds[False]:.3e}")
    return kinds


def check_under_rule(what, got, q, refs, vis, G):
    """check_rule of the decode tests on references taken once per case: the rule on out, zero rows and lse −inf where nothing is seen,
    lse against float64."""
    out, lse = got
    ref, yard, lse64 = refs
    assert out.dtype == q.dtype and out.shape == q.shape and torch.isfinite(out.float()).all(), what
    assert_tensor_under_rule(f"window {what} out", out, yard, ref)
    seen = vis.any(-1).repeat_interleave(G, 1)
    assert (out.cpu()[~seen] == 0).all(), f"{what}: a token that sees nothing is a zero row"
    lse = lse.cpu()
    assert lse.dtype == torch.float32 and (lse[~seen] == -float("inf")).all(), what
    if seen.any():
        e = rel_err(lse[seen].double().numpy(), lse64[seen].numpy())
        assert e <= 1e-5, f"{what}: lse differs from float64 by {e:.3e} relative"


# ---- the sixteen calls on float32 CPU operands -----------------------------------------------------------------------------------

def decode_lists(rows, B, Hkv, T, k_lens):
    """block_ids / block_counts naming, for every token, the blocks of its layout row in their order."""
    ids = torch.full((B, Hkv, T, K_SLOTS), -1, dtype=torch.int32)
    counts = torch.zeros((B, Hkv, T), dtype=torch.int32)
    for b in range(B):
        for t in range(T):
            pos = clamp(k_lens[b], 0, SMAX) - T + t
            if pos >= 0:
                row = rows[pos // KB]
                ids[b, :, t, :len(row)] = torch.tensor(row, dtype=torch.int32)
                counts[b, :, t] = len(row)
    return ids, counts


def prefill_lists(rows, B, Hkv, T, k_lens):
    """… for every position tile: tile x of item b is layout row ⌊(k_len − T) / 64⌋ + x."""
    X = -(-T // KB) + 1
    ids = torch.full((B, Hkv, X, K_SLOTS), -1, dtype=torch.int32)
    counts = torch.zeros((B, Hkv, X), dtype=torch.int32)
    for b in range(B):
        for x in range(X):
            r = (clamp(k_lens[b], 0, SMAX) - T) // KB + x
            if 0 <= r < BLOCKS:
                ids[b, :, x, :len(rows[r])] = torch.tensor(rows[r], dtype=torch.int32)
                counts[b, :, x] = len(rows[r])
    return ids, counts


def run(mm, kind, form, q, k, v, k_lens, dev, dtype, rows, *, lists=None, seed=7, hole=None, **kw):
    """One of the 8 calls of `kind` ("decode" / "prefill") on float32 CPU operands of e4m3fn-representable values, its blocks from
    `rows` — as a shared layout or as lists (`lists`: the caller's own ids / counts) —; hole (b, logical page): that table entry
    becomes −1.  Returns (out, lse)."""
    listed, page, f8 = form
    B, Hq, T, D = q.shape
    Hkv = k.shape[1]
    qd, lens = q.to(dtype).to(dev), lens_tensor(k_lens, dev)
    kw = dict(return_lse=True, **kw)
    if kind == "decode":
        kw.setdefault("chunk", 2)
    if f8:
        kc, vc = k.to(F8).view(torch.uint8), v.to(F8).view(torch.uint8)
        if page:
            kp, vp, table = pools(kc, vc, page, seed)
            cache, table = (kp.to(dev).view(F8), vp.to(dev).view(F8)), table.to(dev)
        else:
            cache = (kc.to(dev).view(F8), vc.to(dev).view(F8))
    else:
        kd, vd = k.to(dtype).to(dev), v.to(dtype).to(dev)
        if page:
            kp, vp, table = paged(kd, vd, page, seed)
            cache = (kp, vp)
        else:
            cache = (kd, vd)
    if page and hole is not None:
        table[hole[0], hole[1]] = -1
    tab = (table,) if page else ()
    suffix = ("_paged" if page else "") + ("_fp8" if f8 else "")
    if listed:
        ids, counts = lists if lists is not None else (decode_lists if kind == "decode" else prefill_lists)(rows, B, Hkv, T, k_lens)
        return getattr(mm, f"block_sparse_attention_{kind}_selected{suffix}")(qd, *cache, *tab, ids.to(dev), counts.to(dev), lens, **kw)
    return getattr(mm, f"block_sparse_attention_{kind}{suffix}")(qd, *cache, *tab, layout_from_rows(rows, dev), lens, **kw)


def same(got, want, what):
    assert_same_bits(got[0], want[0], f"{what}: out")
    assert_same_bits(got[1], want[1], f"{what}: lse")


def random_case(B, Hkv, G, T, D, seed, q0=None):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn((B, Hkv * G, T, D), generator=g)
    if q0 is not None:
        q[..., 0] = q0
    return q, codes(seed + 1, B, Hkv, SMAX, D).view(F8).float(), codes(seed + 2, B, Hkv, SMAX, D).view(F8).float()


# ---- 1. the rule, with planted edges -----------------------------------------------------------------------------------------------

DECODE_LENS = [512, 200, 130, 3]
# (T, k_lens): a chunk of 70 across one and two tile edges (50 … 119, 60 … 129), one of 130 across two and three (70 … 199, 382 … 511)
PREFILL_SHAPES = {70: [120, 130], 130: [200, 512]}


def decode_shape(T):
    return dict(B=4, Hkv=2, G=4 if T == 1 else 1, D=64 if T == 1 else 128)


def prefill_shape(T):  # (D = 128: the rows of a chunk stand on axes of their own)
    return dict(B=2, Hkv=2, G=2 if T == 70 else 1, D=128)


def prefill_rows(T, k_len):
    """The planted rows of a chunk: the first, the last, and one in the middle of a tile — on axes 0, 1, 2."""
    mid = [t for t in range(2, T - 2) if (k_len - T + t) % KB == 31][-1]
    return [(T - 1, 1), (0, 0), (mid, 2)]


@functools.lru_cache(maxsize=None)
def rule_case(kind, T, W, S, banded_rows, dtype):
    """(q, k, v, vis, references, G, k_lens, rows) of one case of test 1, its edges proven to show; shared by the 8 calls."""
    rows = [list(r) for r in banded_rows] if banded_rows else FULL
    if kind == "decode":
        shape, k_lens = decode_shape(T), DECODE_LENS
        rows_of_item = lambda b: [(b % T, b % T)]  # noqa: E731  (one planted token per item)
    else:
        shape, k_lens = prefill_shape(T), PREFILL_SHAPES[T]
        rows_of_item = lambda b: prefill_rows(T, k_lens[b])  # noqa: E731
    B, Hkv, G, D = shape["B"], shape["Hkv"], shape["G"], shape["D"]
    q, k, v, plants = planted(B, Hkv, G, T, D, k_lens, W, S, rows_of_item, 1000 + 7 * W + S + T)
    vis = window_visible(rows, B, Hkv, T, k_lens, W, S)
    refs = references(q.to(dtype), k.to(dtype), v.to(dtype), vis, G)
    what = f"{kind} T={T} W={W} S={S} {'banded' if banded_rows else 'full'} {dtype}"
    kinds = assert_the_edges_would_show(what, q, k, v, vis, plants, G, dtype, refs)
    assert kinds[False] < float("inf"), what  # every case has a shown plant; a hidden one wherever the window hides a key
    return q, k, v, vis, refs, G, k_lens, rows


def all_rule_cases(mm, kind, Ts, dtype):
    for T in Ts:
        for W in WINDOWS:
            for S in SINKS:
                for rows in (None, tuple(tuple(r) for r in banded(mm, W, S))):
                    yield T, W, S, rule_case(kind, T, W, S, rows, dtype)


@pytest.mark.parametrize("form", CALLS, ids=form_id)
@pytest.mark.parametrize("dtype", DTYPES)
def test_1_decode_under_the_rule_with_planted_edges(mm, dev, form, dtype):
    """All 16 forms (8 calls × 2 dtypes): T ∈ {1, 3}, k_lens [512, 200, 130, 3], W ∈ {1, 5, 64, 65, 100}, S ∈ {0, 4, 70}, on the fully
    kept causal layout and on sliding_window_layout's."""
    hidden_somewhere = False
    for T, W, S, (q, k, v, vis, refs, G, k_lens, rows) in all_rule_cases(mm, "decode", (1, 3), dtype):
        got = run(mm, "decode", form, q, k, v, k_lens, dev, dtype, rows, window=W, sink=S)
        check_under_rule(f"decode {form_id(form)} {dtype} T={T} W={W} S={S} rows={len(rows[-1])}", got, q.to(dtype), refs, vis, G)
        hidden_somewhere |= not vis[0, 0, -1, :k_lens[0] - 1].all()
    assert hidden_somewhere


@pytest.mark.parametrize("form", CALLS, ids=form_id)
@pytest.mark.parametrize("dtype", DTYPES)
def test_1_prefill_under_the_rule_with_planted_edges(mm, dev, form, dtype):
    """The 8 prefill calls × 2 dtypes: chunks of 70 and 130 tokens across one, two and three tile edges, three planted rows each."""
    for T, W, S, (q, k, v, vis, refs, G, k_lens, rows) in all_rule_cases(mm, "prefill", (70, 130), dtype):
        got = run(mm, "prefill", form, q, k, v, k_lens, dev, dtype, rows, window=W, sink=S)
        check_under_rule(f"prefill {form_id(form)} {dtype} T={T} W={W} S={S} rows={len(rows[-1])}", got, q.to(dtype), refs, vis, G)


@pytest.mark.parametrize("D,G,form", [(32, 16, (False, 0, False)), (96, 4, (True, 16, True))])
def test_1_other_widths_and_a_group_of_16(mm, dev, D, G, form):
    B, Hkv, T, W, S, dtype = 4, 2, 3, 65, 4, torch.float16
    rows = banded(mm, W, S)
    q, k, v, plants = planted(B, Hkv, G, T, D, DECODE_LENS, W, S, lambda b: [(b % T, b % T)], 1500 + D)
    vis = window_visible(rows, B, Hkv, T, DECODE_LENS, W, S)
    refs = references(q.to(dtype), k.to(dtype), v.to(dtype), vis, G)
    assert_the_edges_would_show(f"D={D} G={G}", q, k, v, vis, plants, G, dtype, refs)
    check_under_rule(f"decode D={D} G={G}", run(mm, "decode", form, q, k, v, DECODE_LENS, dev, dtype, rows, window=W, sink=S), q.to(dtype),
                     refs, vis, G)
    if G <= 4:
        Tp, lens = 70, [120, 130, 512, 70]
        q, k, v, plants = planted(B, Hkv, G, Tp, D, lens, W, S, lambda b: prefill_rows(Tp, lens[b]), 1600 + D)
        vis = window_visible(rows, B, Hkv, Tp, lens, W, S)
        refs = references(q.to(dtype), k.to(dtype), v.to(dtype), vis, G)
        assert_the_edges_would_show(f"prefill D={D} G={G}", q, k, v, vis, plants, G, dtype, refs)
        check_under_rule(f"prefill D={D} G={G}", run(mm, "prefill", form, q, k, v, lens, dev, dtype, rows, window=W, sink=S), q.to(dtype),
                         refs, vis, G)


# ---- 2. bit for bit where nothing is hidden ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", CALLS, ids=form_id)
def test_2_a_window_that_hides_nothing_is_the_plain_call(mm, dev, form):
    """W = 2³¹ − 1, and sink = Smax under any W: out and lse of the plain call, in the 16 + 16 forms."""
    from test_gpu_block_attention_decode import ROWS
    for dtype, D in ((torch.bfloat16, 64), (torch.float16, 128)):
        for kind, T, k_lens in (("decode", 3, DECODE_LENS), ("prefill", 70, [130, 512, 70, 3])):
            q, k, v = random_case(4, 2, 4, T, D, 2000 + D + T)
            for rows in (ROWS, FULL):
                plain = run(mm, kind, form, q, k, v, k_lens, dev, dtype, rows)
                what = f"{kind} {form_id(form)} {dtype}"
                same(run(mm, kind, form, q, k, v, k_lens, dev, dtype, rows, window=TOP), plain, f"{what}: W = 2^31 - 1")
                same(run(mm, kind, form, q, k, v, k_lens, dev, dtype, rows, window=TOP, sink=TOP), plain, f"{what}: W = S = 2^31 - 1")
                same(run(mm, kind, form, q, k, v, k_lens, dev, dtype, rows, window=1, sink=SMAX), plain, f"{what}: sink = Smax")
                same(run(mm, kind, form, q, k, v, k_lens, dev, dtype, rows, window=SMAX), plain, f"{what}: W = Smax")


# ---- 3. bit for bit between forms --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,T,k_lens,dtype,D", [("decode", 3, [512, 200, 130, 3], torch.bfloat16, 128),
                                                   ("prefill", 70, [512, 200, 130, 70], torch.float16, 64)])
def test_3_the_forms_against_each_other(mm, dev, kind, T, k_lens, dtype, D):
    """Paged = contiguous on the gathered cache (pages of 16 and 64, shuffled, one entry −1 behind the window), fp8 without scales =
    2-byte on the widened cache, a list = the layout row that lists the same blocks in the same order."""
    W, S = 100, 4
    q, k, v = random_case(4, 2, 4, T, D, 3000 + T)
    for rows in (FULL, banded(mm, W, S)):
        base = run(mm, kind, (False, 0, False), q, k, v, k_lens, dev, dtype, rows, window=W, sink=S)
        for form in CALLS[1:] + PAGES64:
            # item 0 (positions up to 511): the keys 64 … 127 are behind every token's window and no sink keys
            hole = (0, 80 // form[1]) if form[1] else None
            same(run(mm, kind, form, q, k, v, k_lens, dev, dtype, rows, window=W, sink=S, hole=hole), base,
                 f"{kind} {form_id(form)} against the contiguous 2-byte layout call")


# ---- 4. block-aligned edges against today's kernel ---------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [0, 64])
@pytest.mark.parametrize("form", [(True, 0, False), (True, 16, True), (True, 64, False), (True, 0, True)], ids=form_id)
def test_4_block_aligned_windows_are_the_plain_list_call_with_the_hidden_ids_struck_out(mm, dev, form, S):
    """pos − W + 1 a multiple of 64: every listed block is wholly shown or wholly hidden, and the windowed list call is the PLAIN list
    call whose wholly hidden ids are −1 at the same list positions — in two-entry chunks and in one chunk."""
    B, Hkv, G, D, dtype, W = 3, 2, 4, 64, torch.bfloat16, 192
    k_lens = [512, 448, 256]  # pos − W + 1 = 320, 256, 64
    q, k, v = random_case(B, Hkv, G, 1, D, 4000 + S)
    order = [3, 7, 0, 5, 1, 6, 2, 4]
    ids = torch.tensor(order, dtype=torch.int32).repeat(B, Hkv, 1, 1)
    counts = torch.full((B, Hkv, 1), 8, dtype=torch.int32)
    struck = ids.clone()
    for b in range(B):
        pos = k_lens[b] - 1
        assert (pos - W + 1) % KB == 0
        for p, J in enumerate(order):
            if KB * J >= S and KB * J + 63 <= pos - W:
                struck[b, :, 0, p] = -1
        assert (struck[b] == -1).sum() == Hkv * ((pos - W + 1 - S) // KB), (b, struck[b])
    for chunk in (2, 8):
        got = run(mm, "decode", form, q, k, v, k_lens, dev, dtype, None, lists=(ids, counts), window=W, sink=S, chunk=chunk)
        want = run(mm, "decode", form, q, k, v, k_lens, dev, dtype, None, lists=(struck, counts), chunk=chunk)
        same(got, want, f"decode {form_id(form)} S={S} chunk={chunk}")
    # prefill: one tile of 64 tokens on a tile edge, W = 128; block r − 2 — shown to some rows, hidden from others — is not listed
    T, W, k_lens = 64, 128, [512, 448, 320]
    q, k, v = random_case(B, Hkv, G, T, D, 4100 + S)
    ids = torch.full((B, Hkv, 2, K_SLOTS), -1, dtype=torch.int32)
    counts = torch.zeros((B, Hkv, 2), dtype=torch.int32)
    for b in range(B):
        r = (k_lens[b] - T) // KB
        lst = [J for J in order if J <= r and J != r - 2]
        ids[b, :, 0, :len(lst)], counts[b, :, 0] = torch.tensor(lst, dtype=torch.int32), len(lst)
    struck = ids.clone()
    for b in range(B):
        r = (k_lens[b] - T) // KB
        for p in range(int(counts[b, 0, 0])):
            J = int(ids[b, 0, 0, p])
            if KB * J >= S and KB * J + 63 <= KB * r - W:
                struck[b, :, 0, p] = -1
        assert (struck[b, 0, 0] == -1).sum() == K_SLOTS - int(counts[b, 0, 0]) + max(r - 2 - S // KB, 0)
    got = run(mm, "prefill", form, q, k, v, k_lens, dev, dtype, None, lists=(ids, counts), window=W, sink=S)
    want = run(mm, "prefill", form, q, k, v, k_lens, dev, dtype, None, lists=(struck, counts))
    same(got, want, f"prefill {form_id(form)} S={S}")


# ---- 5. unaligned edges against today's kernel -------------------------------------------------------------------------------------

def underflowing(k, v, hid, low):
    """Copies of the caches whose slots `hid` [B, Hkv, Smax] hold v = 0 and the key (low, 0, …)."""
    kt, vt = k.clone(), v.clone()
    kt[hid] = 0.0
    kt[..., 0][hid] = low
    vt[hid] = 0.0
    return kt, vt


def assert_the_hidden_slots_underflow(q, kt, vis_t, hid, G, D):
    """The condition, in float32 on the CPU: every planted score ≥ 120 below its row's maximum, a normal key in every row."""
    s = (q[:, :, None] @ kt.repeat_interleave(G, 1).transpose(-1, -2)).squeeze(-2) / D ** 0.5  # [B, Hq, Smax]
    seen, planted_ = vis_t.repeat_interleave(G, 1), hid.repeat_interleave(G, 1)
    top = s.masked_fill(~seen, -float("inf")).amax(-1)
    assert torch.isfinite(top).all() and (top > -50).all()
    assert planted_.any() and (s.masked_fill(~planted_, -float("inf")).amax(-1)[planted_.any(-1)] <= top[planted_.any(-1)] - 120).all()


@pytest.mark.parametrize("form", [(False, 0, False), (False, 16, False), (False, 64, True), (True, 0, False), (True, 16, True)], ids=form_id)
def test_5_an_unaligned_window_has_the_bits_of_todays_kernel_on_a_cache_whose_hidden_slots_underflow(mm, dev, form):
    """Row t of the windowed call = row t of the PLAIN call on a cache copy whose slots hidden from t hold v = 0 and a key that
    underflows: element 0 of every q is +16, element 0 of the planted key −4096 (−448 in fp8), its other elements 0.  The weight
    __expf gives such a key is exactly 0, and a partial wiped by a later maximum is 0 · finite.  Decode at T = 3 (every token),
    prefill for 6 rows of a 70-token chunk."""
    B, Hkv, G, D, dtype, W, S = 2, 2, 4, 64, torch.bfloat16, 100, 4
    low = -448.0 if form[2] else -4096.0
    for kind, T, k_lens, rows_t in (("decode", 3, [130, 512], (0, 1, 2)), ("prefill", 70, [130, 512], (0, 3, 9, 40, 63, 69))):
        q, k, v = random_case(B, Hkv, G, T, D, 5000 + T, q0=16.0)
        q = q.to(dtype).float()
        plain_vis = visible([FULL], B, Hkv, T, k_lens)
        vis = window_visible(FULL, B, Hkv, T, k_lens, W, S)
        got = run(mm, kind, form, q, k, v, k_lens, dev, dtype, FULL, window=W, sink=S)
        for t in rows_t:
            hid = (plain_vis & ~vis)[:, :, t]
            kt, vt = underflowing(k, v, hid, low)
            assert_the_hidden_slots_underflow(q[:, :, t], kt, vis[:, :, t], hid, G, D)
            want = run(mm, kind, form, q, kt, vt, k_lens, dev, dtype, FULL)
            assert_same_bits(got[0][:, :, t], want[0][:, :, t], f"{kind} {form_id(form)}: row {t}: out")
            assert_same_bits(got[1][:, :, t], want[1][:, :, t], f"{kind} {form_id(form)}: row {t}: lse")


# ---- 6. decode never loads a hidden key --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", CALLS, ids=form_id)
def test_6_nan_in_every_key_hidden_from_all_tokens_of_the_item(mm, dev, form):
    """k and v hold NaN in every key that no token of the item sees — the keys behind every token's window that are no sink keys among
    them, in wholly hidden blocks and in the two straddling ones: a finite output, bit for bit the clean run."""
    B, Hkv, G, T, D, dtype = 4, 2, 4, 3, 64, torch.float16
    q, k, v = random_case(B, Hkv, G, T, D, 6000)
    for W, S, rows in ((100, 4, FULL), (65, 70, FULL), (5, 0, banded(mm, 5, 0)), (64, 4, banded(mm, 64, 4))):
        vis = window_visible(rows, B, Hkv, T, DECODE_LENS, W, S)
        unseen = ~vis.any(2)  # [B, Hkv, Smax]
        behind = visible([FULL], B, Hkv, T, DECODE_LENS).any(2) & unseen
        assert behind[0].any() and behind[1].any()
        kn, vn = k.clone(), v.clone()
        kn[unseen], vn[unseen] = NAN, NAN
        clean = run(mm, "decode", form, q, k, v, DECODE_LENS, dev, dtype, rows, window=W, sink=S)
        dirty = run(mm, "decode", form, q, kn, vn, DECODE_LENS, dev, dtype, rows, window=W, sink=S)
        assert torch.isfinite(dirty[0].float()).all()
        same(dirty, clean, f"decode {form_id(form)} W={W} S={S}: NaN in the hidden keys")


# ---- 7. the prefill decompositions -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", [(False, 0, False), (True, 16, True), (False, 64, True), (True, 0, False)], ids=form_id)
def test_7_chunks_ragged_items_and_decode_against_prefill(mm, dev, form):
    B, Hkv, G, D, dtype, W, S = 3, 2, 4, 64, torch.bfloat16, 100, 4
    k_lens = [512, 230, 130]
    rows = banded(mm, W, S)
    q, k, v = random_case(B, Hkv, G, 100, D, 7000)
    kw = dict(window=W, sink=S)
    # 100 tokens = 60 + 40 (the chunks cut the tiles differently; a tile's list is its layout row's either way)
    whole = run(mm, "prefill", form, q, k, v, k_lens, dev, dtype, rows, **kw)
    first = run(mm, "prefill", form, q[:, :, :60], k, v, [n - 40 for n in k_lens], dev, dtype, rows, **kw)
    last = run(mm, "prefill", form, q[:, :, 60:], k, v, k_lens, dev, dtype, rows, **kw)
    same((torch.cat([first[0], last[0]], 2), torch.cat([first[1], last[1]], 2)), whole, f"{form_id(form)}: 100 = 60 + 40")
    # ragged new_lens = each item alone with its own chunk
    news = [100, 37, 70]
    ragged = run(mm, "prefill", form, q, k, v, k_lens, dev, dtype, rows, new_lens=torch.tensor(news, device=dev, dtype=torch.int32), **kw)
    for b, n in enumerate(news):
        one = run(mm, "prefill", (form[0], 0, form[2]), q[b:b + 1, :, 100 - n:], k[b:b + 1], v[b:b + 1], k_lens[b:b + 1], dev, dtype, rows, **kw)
        same((ragged[0][b:b + 1, :, 100 - n:], ragged[1][b:b + 1, :, 100 - n:]), one, f"{form_id(form)}: item {b} alone")
        assert (ragged[0][b, :, :100 - n] == 0).all() and (ragged[1][b, :, :100 - n] == -float("inf")).all()
    # decode at T = 3 and prefill at T = 3: the same rule, each under the accuracy rule
    q3 = q[:, :, :3].contiguous()
    vis = window_visible(rows, B, Hkv, 3, k_lens, W, S)
    for kind in ("decode", "prefill"):
        out, lse = run(mm, kind, form, q3, k, v, k_lens, dev, dtype, rows, **kw)
        check_rule(f"{kind} T=3 {form_id(form)}", out, q3.to(dtype), k.to(dtype), v.to(dtype), vis, G, lse)


# ---- 8. graph capture --------------------------------------------------------------------------------------------------------------

def test_8_one_graph_of_lens_append_and_windowed_decode(mm, dev):
    """lens += 1; kv_cache_append; decode(window=100, sink=4) captured once and replayed while k_lens crosses a block edge (198 → 202
    for item 0): the window's edge moves with pos, the two ints are baked in."""
    B, Hkv, G, D, dtype, W, S = 2, 2, 4, 64, torch.float16, 100, 4
    rows = banded(mm, W, S)
    layout = layout_from_rows(rows, dev)
    g = torch.Generator(device=dev).manual_seed(8000)
    q = torch.randn((B, Hkv * G, 1, D), device=dev, generator=g).to(dtype)
    k, v = (torch.randn((B, Hkv, SMAX, D), device=dev, generator=g).to(dtype) for _ in range(2))
    k_new, v_new = (torch.randn((B, Hkv, 1, D), device=dev, generator=g).to(dtype) for _ in range(2))
    lens = lens_tensor([198, 300], dev, torch.int64)

    def step():
        lens.add_(1)
        mm.kv_cache_append(k_new, v_new, k, v, lens)
        return mm.block_sparse_attention_decode(q, k, v, layout, lens, chunk=2, return_lse=True, window=W, sink=S)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()  # warm-up on the side stream: the layout's lists are built here
    torch.cuda.current_stream().wait_stream(s)
    lens.sub_(1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # (a capture does not run: lens stays)
        out, lse = step()
    kc, vc, lc = k.clone(), v.clone(), lens.clone()  # the eager sequence runs on copies of the state
    for n in range(4):  # 199, 200, 201, 202
        for t in (q, k_new, v_new):
            t.copy_(torch.randn(t.shape, device=dev, generator=g).to(dtype))
        lc.add_(1)
        mm.kv_cache_append(k_new, v_new, kc, vc, lc)
        want = mm.block_sparse_attention_decode(q, kc, vc, layout, lc, chunk=2, return_lse=True, window=W, sink=S)
        out.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        host = [199 + n, 301 + n]
        assert lens.tolist() == host and lc.tolist() == host
        same((out, lse), want, f"replay {n}, k_lens {host}")
        check_rule(f"replay {n}", out, q, k, v, window_visible(rows, B, Hkv, 1, host, W, S), G, lse)


# ---- 9. the parent's tree tests, unchanged -----------------------------------------------------------------------------------------

def test_9_the_tree_calls_pass_an_empty_window(mm, dev):
    """The tree entries run on the same kernels with W = 2³¹ − 1 and S = 0; tests/test_gpu_block_attention_decode_tree.py covers them and
    is left as it is.  Here: one tree call beside the windowed call that hides the same keys — a chain's word hides nothing, so the
    tree call, the plain call and the call under the widest window are one result."""
    from test_gpu_block_attention_decode import ROWS
    from test_gpu_block_attention_decode_tree import mask_tensor
    B, Hkv, G, T, D, dtype = 4, 2, 4, 3, 64, torch.bfloat16
    q, k, v = random_case(B, Hkv, G, T, D, 9000)
    chain = mask_tensor([[(2 << t) - 1 for t in range(T)]] * B, dev)
    for form in CALLS:
        plain = run(mm, "decode", form, q, k, v, DECODE_LENS, dev, dtype, ROWS)
        same(run(mm, "decode", form, q, k, v, DECODE_LENS, dev, dtype, ROWS, tree_mask=chain), plain, f"{form_id(form)}: the chain")
        same(run(mm, "decode", form, q, k, v, DECODE_LENS, dev, dtype, ROWS, window=TOP), plain, f"{form_id(form)}: the widest window")
