"""matmuls.block_sparse_attention on the MI355X, where the suite could stay green over a wrong kernel: every compiled form,
blocks above 64, the item loops behind the 65 535-item grid cap, graph capture and the lists kept on a layout tensor.  The
instruments are the project's own: the rule e_dev ≤ 8 · e_ref against dense masked attention in float64
(sparse_attention_helpers: the yardstick is the same computation in fp32 narrowed to T per stage), bit-for-bit
invariances, exact zeros.
  1. every form: T ∈ {bf16, fp16} × D ∈ {32, 64, 96, 128} × causal × lengths — the 32 instantiations of each of the forward,
     dq and dk/dv kernels (Tile<D> on 2·D of 256 threads, LDS strides D + 8, the register budget of each D) — one 2-d call
     at S = 192 on an unsorted lower-triangular layout, lengths 150 / 170 inside a block with NaN in the padding, under the
     rule; exact zeros at and beyond the lengths;
  2. block = 64·f: the bits of the block = 64 call on a layout expanded here in plain Python (sub-block order), and the
     rule against the coarse mask —
       a. f = 3, an unsorted and an empty coarse row (square), a rectangular layout: _expand_block_layout on the device;
       b. f = 2, three per-head layouts of different order, one with a coarse column nobody keeps: csr_transpose_batched
          and the ascending re-sort of _block_layout_transposed on expanded lists; every item the bits of its 2-d call;
       c. f = 2, causal: fine blocks above the diagonal inside a coarse diagonal block, and a coarse block above the
          diagonal, are skipped by next_block on the query and on the key side;
       d. f = 2, grouped heads, causal, lengths on a fine boundary inside a coarse block, inside a fine block and full,
          poisoned padding: the length cut of the walk on expanded lists;
  3. more than 65 535 items: the loops `for (b = blockIdx.y; b < batch; b += gridDim.y)` of the three kernels, with the
     LDS restaged per item, the layout taken by item % layouts and the lengths by b / lens_div past the wrap — the call
     against the same call in two launches of at most 65 535 items, the items around the wrap against their 2-d calls,
     the last item under the rule —
       a. per-head layouts L = 2 (the 65 535 stride is odd: the second pass meets the other layout), a key block that
          nobody sees; b. grouped G = 2 with lengths 0 … 65 and the causal mask (b / group, b / lens_div);
  4. a. forward + backward in one graph capture (plain with block = 128 and causal; grouped with int64 lengths): the
        replay gives the eager bits, again after q, k, v, the incoming gradient and the lengths changed in place;
     b. the lists kept on the layout tensor (_block_layout per f, _bsr_layout): after the indices are rewritten in place
        every call gives the bits of a freshly built layout tensor — block_sparse_attention with block = 64 and 128 in
        turn on one tensor, block_sparse_mm, block_sparse_linear.
"""
import pytest
import torch

from block_attention_gqa_helpers import fill_padding, length_mask
from gpu_helpers import assert_same_bits
from sparse_attention_helpers import assert_tensor_under_rule, dense_step

pytestmark = pytest.mark.gpu

NAMES = ("out", "dq", "dk", "dv")
LOWP = (torch.bfloat16, torch.float16)
NAN = float("nan")


def layout_from_rows(rows_cols, cols, dev):
    """A 2-d CSR block layout (values 1) from per-block-row column lists, kept in the order given (unsorted allowed)."""
    crow = [0]
    for c in rows_cols:
        crow.append(crow[-1] + len(c))
    col = [j for c in rows_cols for j in c]
    return torch.sparse_csr_tensor(torch.tensor(crow, device=dev), torch.tensor(col, device=dev), torch.ones(len(col), device=dev),
                                   size=(len(rows_cols), cols))


def stack_layouts(items, dev):
    """2-d layouts of equal entry counts as one batched layout [len(items), rows, cols]."""
    crow = torch.stack([l.crow_indices() for l in items])
    col = torch.stack([l.col_indices() for l in items])
    return torch.sparse_csr_tensor(crow, col, torch.ones(col.shape, device=dev), size=(len(items),) + tuple(items[0].shape))


def expanded(rows_cols, f):
    """The layout in blocks of 64·f as one in 64-blocks, in sub-block order, on lists: sub-row a of block row I lists, for
    the entries c of row I in their stored order, the columns c·f … c·f + f − 1."""
    return [[c * f + b for c in row for b in range(f)] for row in rows_cols for _ in range(f)]


def block_mask(layout, block, causal=False):
    """Boolean CPU mask [*l_lead, Sq, Sk] of a block layout."""
    vals = torch.ones_like(torch.Tensor.values(layout), dtype=torch.float32)
    m = torch.sparse_csr_tensor(torch.Tensor.crow_indices(layout), torch.Tensor.col_indices(layout), vals, size=layout.shape)
    m = (m.cpu().to_dense() != 0).repeat_interleave(block, -2).repeat_interleave(block, -1)
    return m & torch.ones(m.shape[-2:], dtype=torch.bool).tril() if causal else m


def operands(dev, lead, kv_lead, Sq, Sk, D, dtype, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    q = torch.randn(lead + (Sq, D), device=dev, generator=g).to(dtype)
    k, v = (torch.randn(kv_lead + (Sk, D), device=dev, generator=g).to(dtype) for _ in range(2))
    w = torch.randn(lead + (Sq, D), device=dev, generator=g).to(dtype)
    return q, k, v, w


def step(mm, q, k, v, layout, w, **kw):
    """(out, dq, dk, dv) of one forward + backward on fresh leaves (aliases of the operands: nothing is copied)."""
    q, k, v = (t.detach().requires_grad_(True) for t in (q, k, v))
    out = mm.block_sparse_attention(q, k, v, layout, **kw)
    return (out.detach(),) + torch.autograd.grad(out, (q, k, v), grad_outputs=w)


def reference(q, k, v, w, mask, G, wide, narrow=None):
    """dense_step on k, v repeated G times along the head dimension, dk and dv summed over each group in `wide`."""
    scale = 1.0 / q.shape[-1] ** 0.5
    if G == 1:
        return dense_step(q, k, v, w, mask, scale, wide, narrow=narrow)
    out, dq, dk, dv = dense_step(q, k.repeat_interleave(G, -3), v.repeat_interleave(G, -3), w, mask, scale, wide, narrow=narrow)
    fold = lambda t: t.reshape(t.shape[:-3] + (t.shape[-3] // G, G) + t.shape[-2:]).sum(-3)  # noqa: E731
    return out, dq, fold(dk), fold(dv)


def check_rule(what, got, q, k, v, w, mask, G=1):
    ref = reference(q, k, v, w, mask, G, torch.float64)
    yard = reference(q, k, v, w, mask, G, torch.float32, narrow=q.dtype)
    for name, g, r, y in zip(NAMES, got, ref, yard):
        assert g.dtype == q.dtype and g.shape == r.shape, (what, name)
        assert_tensor_under_rule(f"block attention forms {what} {name}", g, y, r)


def assert_same_step(got, want, what):
    for name, g, x in zip(NAMES, got, want):
        assert_same_bits(g, x, f"{what}: {name}")


def assert_padding_is_zero(got, q_lens, k_lens, what):
    """got [B, …, S, D]: finite everywhere, exact zeros in out, dq at and beyond q_lens[b] and in dk, dv beyond k_lens[b]."""
    for name, g in zip(NAMES, got):
        assert torch.isfinite(g.float()).all(), (what, name)
    for b, (nq, nk) in enumerate(zip(q_lens, k_lens)):
        assert (got[0][b, ..., nq:, :] == 0).all() and (got[1][b, ..., nq:, :] == 0).all(), (what, b)
        assert (got[2][b, ..., nk:, :] == 0).all() and (got[3][b, ..., nk:, :] == 0).all(), (what, b)


def poisoned(q, k, v, w, q_lens, k_lens):
    """(the operands with zeros in the padding — what the references read —, the same with NaN there — what the device reads)."""
    clean = tuple(fill_padding(t, n, 0) for t, n in ((q, q_lens), (k, k_lens), (v, k_lens), (w, q_lens)))
    return clean, tuple(fill_padding(t, n, NAN) for t, n in zip(clean, (q_lens, k_lens, k_lens, q_lens)))


# ---- 1. every compiled form ------------------------------------------------------------------------------------------

FORMS_ROWS = [[0], [1, 0], [0, 2, 1]]  # lower-triangular in blocks; unsorted: the diagonal block is not last in the walk


@pytest.mark.parametrize("lens", [False, True], ids=["no lengths", "lengths"])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("D", [32, 64, 96, 128])
@pytest.mark.parametrize("dtype", LOWP)
def test_1_every_compiled_form_under_the_rule(mm, dev, dtype, D, causal, lens):
    S, q_len, k_len = 192, 150, 170
    assert mm.block_attention_takes(dtype, D, 64)
    layout = layout_from_rows(FORMS_ROWS, 3, dev)
    q, k, v, w = operands(dev, (), (), S, S, D, dtype, 100 + D + 2 * causal + lens)
    mask = block_mask(layout, 64, causal)
    what = f"{dtype} D={D} causal={causal} lengths={lens}"
    if not lens:
        check_rule(what, step(mm, q, k, v, layout, w, causal=causal), q, k, v, w, mask)
        return
    clean, nan = poisoned(*(t[None] for t in (q, k, v, w)), [q_len], [k_len])
    got = step(mm, *(t[0] for t in nan[:3]), layout, nan[3][0], causal=causal, q_lens=torch.tensor(q_len, device=dev),
               k_lens=torch.tensor(k_len, device=dev))
    assert_padding_is_zero([g[None] for g in got], [q_len], [k_len], what)
    check_rule(what, got, *(t[0] for t in clean), length_mask(mask[None], [q_len], [k_len])[0])


# ---- 2. blocks above 64 ----------------------------------------------------------------------------------------------

def coarse_against_fine(mm, what, ops, coarse, fine, f, mask, G=1, clean=None, **kw):
    """The call with block = 64·f: the bits of the block = 64 call on the hand-expanded layout, and the rule against the
    coarse mask (on `clean`, the operands the references read, where the device's are poisoned)."""
    q, k, v, w = ops
    got = step(mm, q, k, v, coarse, w, block=64 * f, **kw)
    assert_same_step(got, step(mm, q, k, v, fine, w, block=64, **kw), f"{what}: the hand-expanded block = 64 call")
    check_rule(what, got, *(clean or ops), mask, G)
    return got


def test_2a_block_192_unsorted_and_empty_coarse_rows(mm, dev):
    S, f, rows = 384, 3, [[1, 0], []]
    coarse, fine = layout_from_rows(rows, 2, dev), layout_from_rows(expanded(rows, f), 6, dev)
    ops = operands(dev, (), (), S, S, 96, torch.float16, 201)
    got = coarse_against_fine(mm, "block = 192, fp16 D=96", ops, coarse, fine, f, block_mask(coarse, 64 * f))
    assert (got[0][192:] == 0).all() and (got[1][192:] == 0).all()  # the empty coarse row
    assert got[2].abs().sum() > 0 and got[3].abs().sum() > 0


def test_2a_block_192_rectangular(mm, dev):
    Sq, Sk, f, rows = 384, 576, 3, [[2, 0], [1]]
    coarse, fine = layout_from_rows(rows, 3, dev), layout_from_rows(expanded(rows, f), 9, dev)
    ops = operands(dev, (), (), Sq, Sk, 32, torch.bfloat16, 202)
    coarse_against_fine(mm, "block = 192, 2 x 3, bf16 D=32", ops, coarse, fine, f, block_mask(coarse, 64 * f))


PER_HEAD_128 = [[[0, 1], []], [[0], [0]], [[1, 0], []]]  # two entries each; head 1: coarse column 1 is kept by nobody


def test_2b_block_128_per_head_layouts(mm, dev):
    S, f, D, dtype = 256, 2, 128, torch.float16
    coarse = stack_layouts([layout_from_rows(r, 2, dev) for r in PER_HEAD_128], dev)
    fine = stack_layouts([layout_from_rows(expanded(r, f), 4, dev) for r in PER_HEAD_128], dev)
    q, k, v, w = ops = operands(dev, (2, 3), (2, 3), S, S, D, dtype, 203)
    got = coarse_against_fine(mm, "block = 128, per head, fp16 D=128", ops, coarse, fine, f,
                              block_mask(coarse, 64 * f).expand(2, 3, S, S))
    for b in range(2):
        for h in range(3):
            want = step(mm, q[b, h], k[b, h], v[b, h], layout_from_rows(PER_HEAD_128[h], 2, dev), w[b, h], block=64 * f)
            assert_same_step([g[b, h] for g in got], want, f"item {b, h} alone")
    assert (got[2][:, 1, 128:] == 0).all() and (got[3][:, 1, 128:] == 0).all()  # head 1's coarse column nobody keeps
    assert (got[0][:, 0, 128:] == 0).all() and (got[1][:, 2, 128:] == 0).all()  # the empty coarse rows of heads 0 and 2


def test_2c_block_128_causal_pair(mm, dev):
    S, f, D, dtype = 256, 2, 128, torch.bfloat16
    ops = operands(dev, (), (), S, S, D, dtype, 204)
    results = {}
    for name, rows in (("tril", [[0], [0, 1]]), ("above", [[0, 1], [1, 0]]), ("above, cut", [[0], [1, 0]])):
        coarse, fine = layout_from_rows(rows, 2, dev), layout_from_rows(expanded(rows, f), 4, dev)
        results[name] = coarse_against_fine(mm, f"block = 128 causal ({name})", ops, coarse, fine, f,
                                            block_mask(coarse, 64 * f, causal=True), causal=True)
    assert_same_step(results["above"], results["above, cut"], "a coarse block above the diagonal contributes nothing")


def test_2d_block_128_grouped_causal_lengths_poison(mm, dev):
    S, f, D, dtype, lens = 256, 2, 32, torch.float16, [64, 100, 256]
    rows = [[0], [1, 0]]
    coarse, fine = layout_from_rows(rows, 2, dev), layout_from_rows(expanded(rows, f), 4, dev)
    clean, nan = poisoned(*operands(dev, (3, 4), (3, 2), S, S, D, dtype, 205), lens, lens)
    dev_lens = torch.tensor(lens, device=dev)
    mask = length_mask(block_mask(coarse, 64 * f, causal=True).expand(3, 4, S, S), lens, lens)
    got = coarse_against_fine(mm, "block = 128 grouped causal lengths, fp16 D=32", nan, coarse, fine, f, mask, G=2, clean=clean,
                              causal=True, q_lens=dev_lens, k_lens=dev_lens)
    assert_padding_is_zero(got, lens, lens, "block = 128 grouped causal lengths")


# ---- 3. beyond 65 535 items --------------------------------------------------------------------------------------------

def assert_same_bits_on_device(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), what


def against_two_launches(mm, q, k, v, layout, w, lens=None, **kw):
    """The call on all the items, checked per result on the device against the same call in two launches of at most
    65 535 query items each (cut at a whole leading index)."""
    half = (q.shape[0] + 1) // 2
    assert q[:half].numel() // (q.shape[-2] * q.shape[-1]) <= 65535 < q.numel() // (q.shape[-2] * q.shape[-1])
    cut = lambda s: {} if lens is None else {"q_lens": lens[s], "k_lens": lens[s]}  # noqa: E731
    got = step(mm, q, k, v, layout, w, **kw, **cut(slice(None)))
    for s in (slice(0, half), slice(half, None)):
        part = step(mm, q[s], k[s], v[s], layout, w[s], **kw, **cut(s))
        for name, g, x in zip(NAMES, got, part):
            assert_same_bits_on_device(g[s], x, f"{name} of items {s} in a launch of their own")
        del part
    return got


def test_3a_beyond_65535_items_per_head_layouts(mm, dev):
    """65 538 items, Sq = 64, Sk = 128, D = 32, bf16.  Device memory: 0.27 GB per q-sized tensor (q, the incoming gradient,
    out, dq), 0.54 GB per k-sized one (k, v, dk, dv), half of the results again for a launch of the reference, 1.1 GB in
    fp32 while an operand is drawn: under 6 GB in all."""
    B, Sq, Sk, D, dtype = 32769, 64, 128, 32, torch.bfloat16
    rows = [[[0]], [[1]]]  # head 0 keeps key block 0, head 1 key block 1
    layout = stack_layouts([layout_from_rows(r, 2, dev) for r in rows], dev)
    q, k, v, w = operands(dev, (B, 2), (B, 2), Sq, Sk, D, dtype, 301)
    got = against_two_launches(mm, q, k, v, layout, w)
    assert not got[2][:, 0, 64:].any() and not got[3][:, 0, 64:].any()  # the key blocks nobody sees, past the wrap too
    assert not got[2][:, 1, :64].any() and not got[3][:, 1, :64].any()
    flat = lambda t: t.reshape((-1,) + t.shape[-2:])  # noqa: E731
    fq, fk, fv, fw = (flat(t) for t in (q, k, v, w))
    items = 2 * B
    for i in (0, 1, 65534, 65535, 65536, items - 1):
        want = step(mm, fq[i], fk[i], fv[i], layout_from_rows(rows[i % 2], 2, dev), fw[i])
        assert_same_step([flat(g)[i] for g in got], want, f"item {i} alone")
    i = items - 1
    lay = layout_from_rows(rows[i % 2], 2, dev)
    check_rule(f"item {i} of {items}", [flat(g)[i] for g in got], fq[i], fk[i], fv[i], fw[i], block_mask(lay, 64))


def test_3b_beyond_65535_items_grouped_lengths_causal(mm, dev):
    """65 538 query items on 32 769 k / v items, S = 64, D = 32, fp16, lengths 0 … 65 by item.  Device memory: 0.27 GB per
    q-sized tensor, 0.13 GB per k-sized one, half of the results again for a launch of the reference: under 2 GB."""
    B, S, D, dtype = 32769, 64, 32, torch.float16
    layout = layout_from_rows([[0]], 1, dev)
    q, k, v, w = operands(dev, (B, 2), (B, 1), S, S, D, dtype, 302)
    lens = torch.arange(B, device=dev) % 66
    got = against_two_launches(mm, q, k, v, layout, w, lens=lens, causal=True)
    beyond = torch.arange(S, device=dev)[None, :] >= lens[:, None]  # [B, S]: the positions that do not exist
    for name, g in zip(NAMES, got):
        assert torch.isfinite(g).all(), name
        assert not g[beyond[:, None, :].expand(g.shape[:-1])].any(), f"{name}: exact zeros at and beyond the lengths"
    for b in (0, 32767, B - 1):  # query items 0, 1 | 65 534, 65 535 | 65 536, 65 537: lengths 0, 31, 32
        n = torch.tensor(b % 66, device=dev)
        want = step(mm, q[b], k[b], v[b], layout, w[b], causal=True, q_lens=n, k_lens=n)
        assert_same_step([g[b] for g in got], want, f"batch entry {b} alone")
    b, n = B - 1, (B - 1) % 66
    mask = length_mask(block_mask(layout, 64, causal=True).expand(1, 2, S, S), [n], [n])[0]
    check_rule(f"batch entry {b} of {B}, length {n}", [g[b] for g in got], q[b], k[b], v[b], w[b], mask, G=2)


# ---- 4a. graph capture -----------------------------------------------------------------------------------------------

def captured_against_eager(mm, dev, call, statics, fresh):
    """forward + backward of `call` in one capture: the replay into poisoned results gives the eager bits; then `fresh`
    values copied into the static tensors in place, and the replay gives the eager bits for those."""
    def run():
        out = call()
        return (out,) + torch.autograd.grad(out, statics[:3], grad_outputs=statics[3])

    eager = [r.detach().clone() for r in run()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()  # warm-up on the side stream: the layout's lists are built here
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # a host synchronisation in here would fail the capture
        results = [r.detach() for r in run()]  # (plain tensors: the poison below is no business of autograd's)
    for want, what in ((eager, "graph replay"), (None, "graph replay after the operands changed in place")):
        if want is None:
            with torch.no_grad():
                for t, x in zip(statics, fresh):
                    t.copy_(x)
            want = [r.detach().clone() for r in run()]
        for r in results:
            r.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        for name, r, x in zip(NAMES, results, want):
            assert_same_bits(r, x, f"{what}: {name}")
            assert torch.isfinite(r.float()).all(), (what, name)
    assert any(not torch.equal(a, b) for a, b in zip(eager, want)), "the fresh operands change the results"


def test_4a_graph_capture_block_128_causal(mm, dev):
    S, D, dtype = 256, 64, torch.bfloat16
    layout = layout_from_rows([[0], [1, 0]], 2, dev)
    q, k, v, w = operands(dev, (2, 2), (2, 2), S, S, D, dtype, 401)
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    fresh = operands(dev, (2, 2), (2, 2), S, S, D, dtype, 402)
    captured_against_eager(mm, dev, lambda: mm.block_sparse_attention(q, k, v, layout, block=128, causal=True), (q, k, v, w), fresh)


def test_4a_graph_capture_grouped_int64_lengths(mm, dev):
    S, D, dtype = 128, 32, torch.float16
    layout = layout_from_rows([[0, 1], [1, 0]], 2, dev)
    q, k, v, w = operands(dev, (3, 4), (3, 2), S, S, D, dtype, 403)
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    q_lens = torch.tensor([128, 70, 1], device=dev, dtype=torch.int64)
    k_lens = torch.tensor([65, 128, 100], device=dev, dtype=torch.int64)
    fresh = operands(dev, (3, 4), (3, 2), S, S, D, dtype, 404) + (torch.tensor([64, 128, 33], device=dev),
                                                                  torch.tensor([128, 3, 64], device=dev))
    captured_against_eager(mm, dev, lambda: mm.block_sparse_attention(q, k, v, layout, q_lens=q_lens, k_lens=k_lens),
                           (q, k, v, w, q_lens, k_lens), fresh)


# ---- 4b. the lists kept on the layout tensor ---------------------------------------------------------------------------

REWRITES = ([[0], [0, 1]], [[1], [1, 0]], [[0], [1, 0]])  # row 1 reordered; row 0 keeps another block; the first rows again


def rewrite(layout, rows_cols, dev):
    layout.col_indices().copy_(torch.tensor([j for c in rows_cols for j in c], device=dev))


def test_4b_rewritten_indices_rebuild_the_attention_lists(mm, dev):
    """One layout tensor [2, 2], used with block = 64 at S = 128 and with block = 128 at S = 256 in turn (a record per f),
    its column indices rewritten in place between the calls: always the bits of a fresh layout tensor."""
    D, dtype = 64, torch.bfloat16
    ops = {f: operands(dev, (2,), (2,), 128 * f, 128 * f, D, dtype, 410 + f) for f in (1, 2)}
    call = lambda lay, f: step(mm, *ops[f][:3], lay, ops[f][3], block=64 * f)  # noqa: E731
    rows = [[0], [1, 0]]
    layout = layout_from_rows(rows, 2, dev)
    seen = {}
    for new_rows in (None,) + REWRITES:
        if new_rows is not None:
            rows = new_rows
            rewrite(layout, rows, dev)
        for f in (1, 2, 2, 1):  # each f builds its record and then meets it again
            got = call(layout, f)
            assert_same_step(got, call(layout_from_rows(rows, 2, dev), f), f"rows {rows}, block = {64 * f}")
            seen[(str(rows), f)] = got
    for f in (1, 2):  # a rewrite that changes which blocks are kept shows in the bits: a stale list could not pass
        outs = [seen[(str(r), f)][0] for r in REWRITES]
        assert all(not torch.equal(a, b) for a, b in zip(outs, outs[1:])), f


def test_4b_rewritten_indices_rebuild_the_block_product_lists(mm, dev):
    """block_sparse_mm and block_sparse_linear on one layout tensor whose column indices are rewritten in place (the sorted
    lists, the entry ids and the transposed lists of _bsr_layout): always the bits of a fresh layout tensor."""
    dtype, N = torch.bfloat16, 40
    g = torch.Generator(device=dev).manual_seed(420)
    values = torch.randn((3, 64, 64), device=dev, generator=g).to(dtype)
    b, wb = (torch.randn((2, 128, N), device=dev, generator=g).to(dtype) for _ in range(2))
    x, wx = (torch.randn((70, 128), device=dev, generator=g).to(dtype) for _ in range(2))
    bias = torch.randn(128, device=dev, generator=g).to(dtype)

    def products(lay):
        vals, b1, x1, bias1 = (t.detach().requires_grad_(True) for t in (values, b, x, bias))
        out = mm.block_sparse_mm(vals, lay, b1)
        y = mm.block_sparse_linear(x1, vals, lay, bias1)
        return (out.detach(), y.detach()) + torch.autograd.grad(out, (vals, b1), grad_outputs=wb) + \
            torch.autograd.grad(y, (x1, vals, bias1), grad_outputs=wx)

    names = ("mm out", "linear y", "mm d values", "mm d b", "linear d x", "linear d values", "linear d bias")
    rows = [[0], [1, 0]]
    layout = layout_from_rows(rows, 2, dev)
    outs = []
    for new_rows in (None,) + REWRITES:
        if new_rows is not None:
            rows = new_rows
            rewrite(layout, rows, dev)
        for again in range(2):
            got = products(layout)
            for name, r, x_ in zip(names, got, products(layout_from_rows(rows, 2, dev))):
                assert_same_bits(r, x_, f"rows {rows}, call {again}: {name}")
        outs.append(got)
    assert all(not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1]) for a, c in zip(outs, outs[1:]))
