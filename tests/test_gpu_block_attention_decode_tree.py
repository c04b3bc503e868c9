"""tree_mask= of the eight decode calls on the MI355X: the T new tokens of an item are the nodes of a drafted
tree, token t sees the cached prefix, itself and the draft keys its int64 word names.  Accuracy is the project's rule
e_dev ≤ 8 · e_ref against dense masked float64 attention under a mask built here from the rule alone; everything else is bit for
bit: the causal and the all-ones words against the call without a mask, garbage in the bits never looked at, NaN in hidden
slots, the forms against each other, and a real tree against TODAY's kernel on a cache whose hidden slots underflow.

Smax = 512, B · Hkv ≤ 8, chunk=2.  The caches hold e4m3fn-representable values, so one set of operands serves the 2-byte and
the fp8 forms.  The draft keys are planted: the queries of an item's tokens stand along distinct axes and draft key i points
along the axes of the tokens it is hidden from, with a value row of ±128 that spells i — checked on the CPU before a kernel runs: the
float64 reference with ANY ONE hidden key made visible moves by at least 100 × the rule's allowance.  That bound decides the
shapes: in bfloat16 (allowance ≈ 0.03 of the largest output) a leak has to outweigh every true row three times over, so every
row of a bfloat16 case sees at least 60 cached keys; the rows that see draft keys only — k_len < T, or a layout row that lists
the window's block alone — stand in the float16 cases (allowance ≈ 0.004), as stars, where a row is its own value row."""
import functools

import numpy as np
import pytest
import torch

from gpu_helpers import assert_same_bits
from sparse_attention_helpers import FACTOR, scaled_err
from test_gpu_block_attention_decode import ROWS, SMAX, check_rule, layout_from_rows, lens_tensor, references, visible
from test_gpu_block_attention_decode_fp8 import F8, codes, pools
from test_gpu_block_attention_decode_paged import gathered, paged

pytestmark = pytest.mark.gpu

NAN = float("nan")
K_SLOTS = 8
LAYOUT_FORMS = [(False, page, f8) for page in (0, 16, 64) for f8 in (False, True)]
FORMS = LAYOUT_FORMS + [(True, page, f8) for page in (0, 16, 64) for f8 in (False, True)]  # (lists, page, fp8)


# ---- trees and their words, from the rule alone ---------------------------------------------------------------------------------

def tree_parents(kind, T, seed=0):
    if kind == "chain":
        return [t - 1 for t in range(T)]
    if kind == "star":
        return [-1] * T
    if kind == "two":
        return [-1, -1][:T] + [t - 2 for t in range(2, T)]
    g = np.random.Generator(np.random.PCG64(seed))
    return [int(g.integers(-1, t)) for t in range(T)]


def words_of(parents):
    """Python ints (unsigned): bit i of word t iff i is t or an ancestor of t."""
    w = []
    for t, p in enumerate(parents):
        w.append((w[p] if p >= 0 else 0) | (1 << t))
    return w


def mask_tensor(words, dev):
    """Unsigned words [B][T] or [T] as the int64 tensor of the call."""
    signed = lambda x: x - (1 << 64) if x >= (1 << 63) else x  # noqa: E731
    rows = [[signed(x) for x in r] for r in words] if isinstance(words[0], list) else [signed(x) for x in words]
    return torch.tensor(rows, dtype=torch.int64, device=dev)


def tree_visible(vis, words, k_lens, T, smax=SMAX):
    """The plain rule's mask [B, Hkv, T, Smax] minus the draft keys base + i, i < t, whose bit of word (b, t) is clear."""
    vis = vis.clone()
    for b in range(vis.shape[0]):
        base = min(max(k_lens[b], 0), smax) - T
        for t in range(T):
            for i in range(t):
                if not (words[b][t] >> i) & 1 and base + i >= 0:
                    vis[b, :, t, base + i] = False
    return vis


# ---- operands: e4m3fn-representable caches, axis queries, planted draft keys -------------------------------------------------------

def planted(B, Hkv, G, T, D, k_lens, words, seed, amp=4.0, key=32.0, value=128.0):
    """(q, k, v) float32 on the CPU.  q[b, :, t] = amp · e_axis(t) + 0.02 · noise (axis(t) = t mod D; T ≤ D: distinct axes);
    the cache is random finite e4m3fn values with |x| < 4; draft key i of item b is key · Σ e_axis(t) over the tokens t > i it
    is hidden from (a key hidden from nobody stays random) — a score of amp · key / √D ≥ 11 above the rest for them, an ordinary
    one for the tokens that see it —, its value row ±value with the sign of element d spelling bit d mod 6 of i: two draft
    keys differ by 2 · value in some element."""
    g = torch.Generator().manual_seed(seed)
    q = 0.02 * torch.randn((B, Hkv * G, T, D), generator=g)
    for t in range(T):
        q[:, :, t, t % D] += amp
    k = codes(seed + 1, B, Hkv, SMAX, D).view(F8).float()
    v = codes(seed + 2, B, Hkv, SMAX, D).view(F8).float()
    for b in range(B):
        base = min(max(k_lens[b], 0), SMAX) - T
        for i in range(T):
            hidden_from = [t for t in range(i + 1, T) if not (words[b][t] >> i) & 1]
            if hidden_from and base + i >= 0:
                k[b, :, base + i] = 0.0
                for t in hidden_from:
                    k[b, :, base + i, t % D] = key
                v[b, :, base + i] = torch.tensor([value if (i >> (d % 6)) & 1 else -value for d in range(D)])
    return q, k, v


def assert_a_leak_would_show(what, q, k, v, vis_tree, vis_plain, G, dtype):
    """On the CPU, before the kernel: for every row and every key the tree hides from it (and the plain rule shows), the float64
    reference with that one key visible differs from the true one by ≥ 100 × the rule's allowance 8 · e_ref, in the rule's own
    measure (max |difference| / max |reference|)."""
    ref, yard, lse = references(q.to(dtype), k.to(dtype), v.to(dtype), vis_tree, G)
    e_ref = scaled_err(yard.double().numpy(), ref.numpy())
    need = 100.0 * FACTOR * e_ref * float(ref.abs().max())
    hidden = (vis_plain & ~vis_tree).repeat_interleave(G, 1)  # [B, Hq, T, Smax]
    assert hidden.any(), what
    qd, kd, vd = q.to(dtype).double(), k.to(dtype).double().repeat_interleave(G, 1), v.to(dtype).double().repeat_interleave(G, 1)
    s = (qd @ kd.transpose(-1, -2)) / q.shape[-1] ** 0.5
    w = torch.exp(s - lse[..., None])  # the leaked key's weight against the row's true sum
    share = torch.where(torch.isinf(w), torch.ones_like(w), w / (1 + w))
    worst = float("inf")
    for b in range(q.shape[0]):
        cols = hidden[b].any(0).any(0).nonzero().flatten()  # the window's slots that are hidden from some row
        move = (share[b][:, :, cols, None] * (vd[b][:, None, cols] - ref[b][:, :, None])).abs().amax(-1)  # [Hq, T, cols]
        worst = min(worst, float(move[hidden[b][:, :, cols]].min()))
    print(f"{what}: e_ref {e_ref:.3e}, the smallest move of a leaked key {worst:.3e}, needed {need:.3e}")
    assert worst >= need, f"{what}: a leaked key would move the reference by {worst:.3e} < {need:.3e}"


def lists_of_rows(B, Hkv, T, k_lens, dev):
    """block_ids / block_counts naming, for every token, the blocks of its layout row of ROWS in their order."""
    ids = torch.full((B, Hkv, T, K_SLOTS), -1, dtype=torch.int32)
    counts = torch.zeros((B, Hkv, T), dtype=torch.int32)
    for b in range(B):
        for t in range(T):
            pos = min(max(k_lens[b], 0), SMAX) - T + t
            if pos >= 0:
                row = ROWS[pos // 64]
                ids[b, :, t, :len(row)] = torch.tensor(row, dtype=torch.int32)
                counts[b, :, t] = len(row)
    return ids.to(dev), counts.to(dev)


def run(mm, form, q, k, v, k_lens, dev, dtype, tree_mask, chunk=2, seed=7, table_edit=None):
    """One of the 16 forms on float32 CPU operands of e4m3fn-representable values; returns (out, lse)."""
    lists, page, f8 = form
    B, Hq, T, D = q.shape
    Hkv = k.shape[1]
    qd, lens = q.to(dtype).to(dev), lens_tensor(k_lens, dev)
    kw = dict(chunk=chunk, return_lse=True, tree_mask=tree_mask)
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
    tab = (table,) if page else ()
    if lists:
        ids, counts = lists_of_rows(B, Hkv, T, k_lens, dev)
        name = "block_sparse_attention_decode_selected" + ("_paged" if page else "") + ("_fp8" if f8 else "")
        return getattr(mm, name)(qd, *cache, *tab, ids, counts, lens, **kw)
    name = "block_sparse_attention_decode" + ("_paged" if page else "") + ("_fp8" if f8 else "")
    return getattr(mm, name)(qd, *cache, *tab, layout_from_rows(ROWS, dev), lens, **kw)


@functools.lru_cache(maxsize=None)
def _case(B, Hkv, G, T, D, k_lens, kinds, seed):
    return case(B, Hkv, G, T, D, list(k_lens), list(kinds), seed)


def case(B, Hkv, G, T, D, k_lens, kinds, seed):
    """(words [B][T], q, k, v, plain mask, tree mask) of a batch whose item b carries the tree kinds[b % len]."""
    words = [words_of(tree_parents(kinds[b % len(kinds)], T, seed + b)) for b in range(B)]
    q, k, v = planted(B, Hkv, G, T, D, k_lens, words, seed)
    plain = visible([ROWS], B, Hkv, T, k_lens)
    return words, q, k, v, plain, tree_visible(plain, words, k_lens, T)


# ---- 1. the rule of 8, every form ----------------------------------------------------------------------------------------------

# k_len 130 with T = 7: the window straddles a block edge and two layout rows; T = 64: k_len 200 straddles (window 136 … 199),
# k_len 192 and 320 cover a block exactly.  float16 only (see the top): k_len 3 and 40 < T — tokens that do not exist —, and
# k_len 71, whose layout row [1, 4] shows the window alone.  (T, k_lens, the items' trees)
SHAPES = {
    (torch.bfloat16, "short"): (7, (130, 258, 512, 200), ("star", "two", "random", "random")),
    (torch.bfloat16, "long"): (64, (200, 192, 320, 512), ("two", "random", "star", "random")),
    (torch.float16, "short"): (7, (130, 3, 512, 71), ("random", "star", "two", "star")),
    (torch.float16, "long"): (64, (200, 192, 40, 512), ("two", "random", "star", "random")),
}
SHORT = dict(T=7, k_lens=[130, 3, 512, 71])
LONG = dict(T=64, k_lens=[200, 192, 40, 512])


@pytest.mark.parametrize("form", FORMS, ids=lambda f: f"{'lists' if f[0] else 'layout'}-page{f[1]}-{'fp8' if f[2] else '2byte'}")
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_1_rule_of_8_in_all_16_forms(mm, dev, form, dtype):
    """All 16 forms (8 calls × 2 dtypes), D = 64 with T = 7 and D = 128 with T = 64, star / two branches / random trees."""
    for D, G, shape in ((64, 5, "short"), (128, 1, "long")):
        B, Hkv, (T, k_lens, kinds) = 4, 2, SHAPES[dtype, shape]
        words, q, k, v, plain, vis = _case(B, Hkv, G, T, D, k_lens, kinds, 900 + D)
        k_lens = list(k_lens)
        assert_a_leak_would_show(f"{form} {dtype} D={D}", q, k, v, vis, plain, G, dtype)
        out, lse = run(mm, form, q, k, v, k_lens, dev, dtype, mask_tensor(words, dev))
        check_rule(f"tree {form} {dtype} D={D} T={T}", out, q.to(dtype), k.to(dtype), v.to(dtype), vis, G, lse)


@pytest.mark.parametrize("D,G,form", [(32, 16, (False, 0, False)), (96, 16, (True, 16, True)), (64, 16, (False, 64, False)),
                                      (128, 5, (True, 0, False))])
def test_1_rule_of_8_other_widths_and_groups(mm, dev, D, G, form):
    B, Hkv, dtype = 4, 1, (torch.bfloat16, torch.float16)[D in (96, 128)]
    T, k_lens, kinds = SHAPES[dtype, "short"]
    words, q, k, v, plain, vis = case(B, Hkv, G, T, D, list(k_lens), list(kinds), 940 + D)
    k_lens = list(k_lens)
    assert_a_leak_would_show(f"D={D} G={G}", q, k, v, vis, plain, G, dtype)
    out, lse = run(mm, form, q, k, v, k_lens, dev, dtype, mask_tensor(words, dev))
    check_rule(f"tree D={D} G={G} {form}", out, q.to(dtype), k.to(dtype), v.to(dtype), vis, G, lse)


# ---- 2. bit for bit ---------------------------------------------------------------------------------------------------------------

def same(got, want, what):
    assert_same_bits(got[0], want[0], f"{what}: out")
    assert_same_bits(got[1], want[1], f"{what}: lse")


@pytest.mark.parametrize("form", FORMS, ids=lambda f: f"{'lists' if f[0] else 'layout'}-page{f[1]}-{'fp8' if f[2] else '2byte'}")
def test_2_the_causal_and_the_all_ones_words_are_the_plain_call(mm, dev, form):
    for dtype, D, shape in ((torch.bfloat16, 64, LONG), (torch.float16, 128, SHORT)):
        B, Hkv, G, T, k_lens = 4, 2, 4, shape["T"], shape["k_lens"]
        words, q, k, v, _, _ = case(B, Hkv, G, T, D, k_lens, ["random"], 960 + D)
        plain = run(mm, form, q, k, v, k_lens, dev, dtype, None)
        causal = [[(2 << t) - 1 for t in range(T)]] * B
        same(run(mm, form, q, k, v, k_lens, dev, dtype, mask_tensor(causal, dev)), plain, f"{form} {dtype}: the causal words")
        same(run(mm, form, q, k, v, k_lens, dev, dtype, torch.full((B, T), -1, dtype=torch.int64, device=dev)), plain,
             f"{form} {dtype}: all ones")


@pytest.mark.parametrize("form", [(False, 0, False), (False, 16, True), (True, 64, False), (True, 0, True)])
def test_2_garbage_above_t_the_shared_mask_and_an_item_alone(mm, dev, form):
    B, Hkv, G, D, dtype, T, k_lens = 4, 2, 4, 64, torch.float16, LONG["T"], LONG["k_lens"]
    kinds = ["random"]
    words, q, k, v, plain, vis = case(B, Hkv, G, T, D, k_lens, kinds, 975)
    words = [words[0]] * B  # one tree for the batch: the [T] form below
    q, k, v = planted(B, Hkv, G, T, D, k_lens, words, 975)
    vis = tree_visible(plain, words, k_lens, T)
    mask = mask_tensor(words, dev)
    clean = run(mm, form, q, k, v, k_lens, dev, dtype, mask)
    # bits at or above t are never looked at (the token's own bit included: it always sees itself)
    g = torch.Generator().manual_seed(5)
    junk = torch.randint(-2 ** 63, 2 ** 63 - 1, (B, T), generator=g, dtype=torch.int64)
    low = torch.tensor([(1 << t) - 1 for t in range(T)], dtype=torch.int64)
    dirty = ((mask.cpu() & low) | (junk & ~low)).to(dev)
    same(run(mm, form, q, k, v, k_lens, dev, dtype, dirty), clean, f"{form}: garbage in the bits >= t")
    # a [T] mask is the repeated [B, T] one
    same(run(mm, form, q, k, v, k_lens, dev, dtype, mask[0].contiguous()), clean, f"{form}: the shared [T] mask")
    # an item alone against the item in the batch
    for b in (0, 2):
        one = run(mm, (form[0], 0, form[2]), q[b:b + 1], k[b:b + 1], v[b:b + 1], k_lens[b:b + 1], dev, dtype, mask[b:b + 1].contiguous())
        ref = run(mm, (form[0], 0, form[2]), q, k, v, k_lens, dev, dtype, mask)
        same(one, (ref[0][b:b + 1], ref[1][b:b + 1]), f"{form}: item {b} alone")


def test_2_nan_in_every_hidden_slot_of_a_star(mm, dev):
    """A star hides every draft key from every other token: each slot holds NaN for all tokens but its own.  Token t is
    run alone through its word — T calls of one item whose other slots are NaN — against the clean batch call."""
    B, Hkv, G, D, dtype, T, k_lens = 1, 2, 4, 64, torch.bfloat16, 7, [130]
    words, q, k, v, plain, vis = case(B, Hkv, G, T, D, k_lens, ["star"], 981)
    mask = mask_tensor(words, dev)
    for form in ((False, 0, False), (False, 16, False), (True, 0, True)):
        clean = run(mm, form, q, k, v, k_lens, dev, dtype, mask)
        for t in range(T):
            kn, vn = k.clone(), v.clone()
            others = [130 - T + i for i in range(T) if i != t]
            kn[:, :, others], vn[:, :, others] = NAN, NAN
            got = run(mm, form, q, kn, vn, k_lens, dev, dtype, mask)
            assert_same_bits(got[0][:, :, t], clean[0][:, :, t], f"{form}: token {t} with NaN in every other draft slot")
            assert_same_bits(got[1][:, :, t], clean[1][:, :, t], f"{form}: token {t}: lse")


def test_2_the_forms_against_each_other(mm, dev):
    B, Hkv, G, D, dtype, T, k_lens = 4, 2, 4, 128, torch.bfloat16, LONG["T"], LONG["k_lens"]
    words, q, k, v, _, _ = case(B, Hkv, G, T, D, k_lens, ["two", "random"], 990)
    mask = mask_tensor(words, dev)
    base = run(mm, (False, 0, False), q, k, v, k_lens, dev, dtype, mask)
    for form in FORMS[1:]:  # paged against contiguous, fp8 without scales against 2-byte, a list against the layout row
        same(run(mm, form, q, k, v, k_lens, dev, dtype, mask), base, f"{form} against the contiguous 2-byte layout call")


def test_2_a_graph_replay_follows_the_mask_in_place(mm, dev):
    B, Hkv, G, D, dtype, T, k_lens = 2, 2, 4, 64, torch.bfloat16, 7, [130, 71]
    words, q, k, v, _, _ = case(B, Hkv, G, T, D, k_lens, ["random"], 995)
    qd, kd, vd, lens = q.to(dtype).to(dev), k.to(dtype).to(dev), v.to(dtype).to(dev), lens_tensor(k_lens, dev)
    layout = layout_from_rows(ROWS, dev)
    mask = mask_tensor(words, dev)
    call = lambda: mm.block_sparse_attention_decode(qd, kd, vd, layout, lens, chunk=2, return_lse=True, tree_mask=mask)  # noqa: E731
    call()  # (the layout's record, the allocator's pools)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse = call()
    for kind in ("star", "two"):
        mask.copy_(mask_tensor([words_of(tree_parents(kind, T))] * B, dev))
        graph.replay()
        torch.cuda.synchronize()
        same((out, lse), call(), f"replay after the mask became a {kind}")


# ---- 3. a real tree against today's kernel -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", [(False, 0, False), (False, 16, False), (False, 64, True), (True, 0, False), (True, 16, True)])
def test_3_a_real_tree_has_the_bits_of_todays_kernel_on_a_cache_whose_hidden_slots_underflow(mm, dev, form):
    """Row t of the tree call = row t of the PLAIN call on a cache copy whose slots hidden from t hold v = 0 and a key that
    underflows: element 0 of every q is +16, element 0 of the planted key −4096 (−448 in fp8), its other elements 0.  The
    weight __expf gives such a key is exactly 0, and a partial wiped by a later maximum is 0 · finite."""
    B, Hkv, G, D, dtype, T, k_lens = 2, 2, 4, 64, torch.bfloat16, 7, [130, 71]
    low = -448.0 if form[2] else -4096.0
    words = [words_of(tree_parents("random", T, 31)), words_of(tree_parents("two", T))]
    g = torch.Generator().manual_seed(77)
    q = torch.randn((B, Hkv * G, T, D), generator=g).to(dtype).float()
    q[..., 0] = 16.0
    k = codes(78, B, Hkv, SMAX, D).view(F8).float()
    v = codes(79, B, Hkv, SMAX, D).view(F8).float()
    plain_vis = visible([ROWS], B, Hkv, T, k_lens)
    vis = tree_visible(plain_vis, words, k_lens, T)
    tree = run(mm, form, q, k, v, k_lens, dev, dtype, mask_tensor(words, dev))
    for t in range(T):
        kt, vt = k.clone(), v.clone()
        hid = (plain_vis & ~vis)[:, :, t]  # [B, Hkv, Smax]
        kt[hid] = 0.0
        kt[..., 0][hid] = low
        vt[hid] = 0.0
        # the condition, in float32 on the CPU: every planted score ≥ 120 below its row's maximum, a normal key in every row
        s = (q[:, :, t, None] @ kt.repeat_interleave(G, 1).transpose(-1, -2)).squeeze(-2) / D ** 0.5  # [B, Hq, Smax]
        seen, planted_ = vis[:, :, t].repeat_interleave(G, 1), hid.repeat_interleave(G, 1)
        top = s.masked_fill(~seen, -float("inf")).amax(-1)
        assert torch.isfinite(top).all() and (top > -50).all()
        if planted_.any():
            assert (s.masked_fill(~planted_, -float("inf")).amax(-1) <= top - 120).all()
        want = run(mm, form, q, kt, vt, k_lens, dev, dtype, None)
        assert_same_bits(tree[0][:, :, t], want[0][:, :, t], f"{form}: token {t}: out")
        assert_same_bits(tree[1][:, :, t], want[1][:, :, t], f"{form}: token {t}: lse")


# ---- the helper on the device ----------------------------------------------------------------------------------------------------

def test_tree_attention_mask_on_the_device(mm, dev):
    for T in (1, 7, 64):
        parents = [tree_parents(kind, T, 3) for kind in ("chain", "star", "two", "random")]
        mask, depth = mm.tree_attention_mask(torch.tensor(parents, device=dev, dtype=torch.int32))
        assert mask.device.type == "cuda" and mask.dtype == torch.int64 and depth.dtype == torch.int32
        assert torch.equal(mask.cpu(), mask_tensor([words_of(p) for p in parents], "cpu"))
        assert depth.cpu().tolist() == [[bin(w).count("1") - 1 for w in words_of(p)] for p in parents]
