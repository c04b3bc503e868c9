"""CSR row softmax on the MI355X (csrc/csr_softmax.hip through custom_mm.csr_softmax / csr_softmax_backward and
matmuls.sparse_softmax): the exactness DESIGN.md §3.12 promises bit for bit, row sums, accuracy against torch-CPU's float64
COO softmax under the e_dev ≤ 8 · e_ref rule, special values and shapes, batched tensors, stream capture."""
import numpy as np
import pytest
import torch

from gpu_helpers import assert_same_bits
from sparse_attention_helpers import (accuracy_matrix, assert_under_rule, cpu_sparse_softmax, dev_softmax, dev_softmax_backward,
                                      device_pattern, rel_err, row_sums64, scaled_err, with_values)

pytestmark = pytest.mark.gpu

LOWP = (torch.bfloat16, torch.float16)
# lengths around every boundary of the kernel's forms: the lane groups (16 / 32 / 64 lanes × 8 entries), the chains (64),
# the LDS buffer (4096 forward, 2048 backward) and beyond it
PROBE_LENS = (1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047,
              2048, 2049, 4095, 4096, 4097, 5000, 9000)


def rowptr_of(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))]).astype(np.int32)


def probe_values(seed, spread=4.0):
    g = np.random.Generator(np.random.PCG64(seed))
    n = int(sum(PROBE_LENS))
    return (spread * g.standard_normal(n)).astype(np.float32), g.standard_normal(n).astype(np.float32)


def embed(fill_len, fill_rows, x, dy, seed):
    """The probe rows followed by `fill_rows` rows of `fill_len` entries: (rowptr, M, x, dy, probe entry count)."""
    g = np.random.Generator(np.random.PCG64(seed))
    lens = list(PROBE_LENS) + [fill_len] * fill_rows
    extra = fill_len * fill_rows
    return (rowptr_of(lens), len(lens), np.concatenate([x, g.standard_normal(extra).astype(np.float32)]),
            np.concatenate([dy, g.standard_normal(extra).astype(np.float32)]), len(x))


def test_1a_run_to_run_identical(cmm, dev):
    rowptr, cols, v1, _, dy = accuracy_matrix()
    M = len(rowptr) - 1
    y1, y2 = dev_softmax(cmm, dev, v1, rowptr, M), dev_softmax(cmm, dev, v1, rowptr, M)
    assert_same_bits(y1, y2, "forward, run to run")
    g1, g2 = dev_softmax_backward(cmm, dev, y1, dy, rowptr, M), dev_softmax_backward(cmm, dev, y1, dy, rowptr, M)
    assert_same_bits(g1, g2, "backward, run to run")


def test_1b_a_rows_bits_do_not_depend_on_the_group_width_or_the_batch(cmm, dev):
    x, dy = probe_values(11)
    n = len(x)
    total = int(sum(PROBE_LENS))
    # mean row length ≤ 48 → 16 lanes per row, ≤ 160 → 32, beyond → 64 (csr_softmax.hip, group_lanes)
    fills = {16: (1, 4000), 32: (100, 3000), 64: (400, 3000)}
    results = {}
    for lanes, (fill_len, fill_rows) in fills.items():
        rowptr, M, xs, dys, _ = embed(fill_len, fill_rows, x, dy, 12)
        mean = len(xs) // M
        assert {16: mean <= 48, 32: 48 < mean <= 160, 64: mean > 160}[lanes], (lanes, mean)
        y = dev_softmax(cmm, dev, xs, rowptr, M)
        g = dev_softmax_backward(cmm, dev, y, dys, rowptr, M)
        results[lanes] = (y[:n].clone(), g[:n].clone())
    for lanes in (32, 64):
        assert_same_bits(results[lanes][0], results[16][0], f"forward, {lanes} lanes vs 16")
        assert_same_bits(results[lanes][1], results[16][1], f"backward, {lanes} lanes vs 16")
    # the same rows as every item of a batched tensor (offsets [batch, M + 1] with the items' bases)
    batch, M = 3, len(PROBE_LENS)
    base = rowptr_of(PROBE_LENS).astype(np.int64)
    offs = np.stack([base + i * total for i in range(batch)]).astype(np.int32)
    yb = dev_softmax(cmm, dev, np.tile(x, batch), offs, M, batch=batch)
    gb = dev_softmax_backward(cmm, dev, yb, np.tile(dy, batch), offs, M, batch=batch)
    for i in range(batch):
        assert_same_bits(yb[i * n:(i + 1) * n], results[16][0], f"forward, item {i} of a batch")
        assert_same_bits(gb[i * n:(i + 1) * n], results[16][1], f"backward, item {i} of a batch")


@pytest.mark.parametrize("dtype", LOWP)
def test_1c_low_precision_is_the_float32_kernel_narrowed_once(cmm, dev, dtype):
    x, dy = probe_values(13)
    rowptr, M = rowptr_of(PROBE_LENS), len(PROBE_LENS)
    xt, dyt = torch.from_numpy(x).to(dtype), torch.from_numpy(dy).to(dtype)
    y = dev_softmax(cmm, dev, xt, rowptr, M, dtype=dtype)
    assert y.dtype == dtype
    assert_same_bits(y, dev_softmax(cmm, dev, xt.float(), rowptr, M).to(dtype), f"forward {dtype}")
    g = dev_softmax_backward(cmm, dev, y, dyt, rowptr, M)
    assert g.dtype == dtype
    assert_same_bits(g, dev_softmax_backward(cmm, dev, y.float(), dyt.float(), rowptr, M).to(dtype), f"backward {dtype}")
    # … with a scale, and under matmuls.sparse_softmax's rule for the group width of a short-row matrix
    y = dev_softmax(cmm, dev, xt, rowptr, M, scale=0.3, dtype=dtype)
    assert_same_bits(y, dev_softmax(cmm, dev, xt.float(), rowptr, M, scale=0.3).to(dtype), f"forward {dtype}, scale")
    g = dev_softmax_backward(cmm, dev, y, dyt, rowptr, M, scale=0.3)
    assert_same_bits(g, dev_softmax_backward(cmm, dev, y.float(), dyt.float(), rowptr, M, scale=0.3).to(dtype),
                     f"backward {dtype}, scale")


def test_1d_scale_is_one_float32_multiply_before_everything_else(cmm, dev):
    x, dy = probe_values(14)
    rowptr, M = rowptr_of(PROBE_LENS), len(PROBE_LENS)
    for scale in (0.125, 0.3, 1.7):
        pre = (torch.from_numpy(x) * torch.tensor(scale, dtype=torch.float32)).numpy()  # fl32(scale · x)
        assert_same_bits(dev_softmax(cmm, dev, x, rowptr, M, scale=scale), dev_softmax(cmm, dev, pre, rowptr, M),
                         f"scale {scale}")


def test_1e_in_place_gives_the_same_bits(cmm, dev):
    x, dy = probe_values(15)
    rowptr, M = rowptr_of(PROBE_LENS), len(PROBE_LENS)
    for dtype in (torch.float32,) + LOWP:
        xt, dyt = torch.from_numpy(x).to(dtype), torch.from_numpy(dy).to(dtype)
        y = dev_softmax(cmm, dev, xt, rowptr, M, scale=0.7, dtype=dtype)
        assert_same_bits(dev_softmax(cmm, dev, xt.clone(), rowptr, M, scale=0.7, dtype=dtype, in_place=True), y,
                         f"forward in place {dtype}")
        g = dev_softmax_backward(cmm, dev, y, dyt, rowptr, M, scale=0.7)
        assert_same_bits(dev_softmax_backward(cmm, dev, y, dyt.clone(), rowptr, M, scale=0.7, in_place=True), g,
                         f"backward in place {dtype}")


def test_2_row_sums(cmm, dev):
    """|Σ y − 1| ≤ (L + 3)·2⁻²⁴ for every non-empty finite row, the sum taken on the host in float64: any fp32 summation
    order of L positive terms is within (L − 1)·2⁻²⁴ relative, the reciprocal-multiply within 3·2⁻²⁴."""
    rowptr, cols, v1, v2, _ = accuracy_matrix()
    M = len(rowptr) - 1
    for name, v in (("spread 40", v1), ("uniform", v2)):
        y = dev_softmax(cmm, dev, v, rowptr, M).cpu().numpy()
        assert np.isfinite(y).all()
        sums, lens = row_sums64(rowptr, y)
        nz = lens > 0
        used = np.abs(sums[nz] - 1.0) / ((lens[nz] + 3) * 2.0 ** -24)
        print(f"row sums, {name}: largest share of the bound used {used.max():.3f}")
        assert (used <= 1.0).all(), (name, float(used.max()))


@pytest.mark.parametrize("scale", [1.0, 0.125])
def test_3_accuracy_against_float64_torch_cpu(cmm, dev, scale):
    """e_dev ≤ 8 · e_ref, e = max |y − y64| / y64 (gradients: max |dx − dx64| / max |dx64|, dy standard normal), y64 float64
    torch.sparse.softmax on the CPU (COO), e_ref torch-CPU float32 on the same input.  With a scale the reference's input
    is fl32(scale · x)."""
    rowptr, cols, v1, v2, dy = accuracy_matrix()
    M, K = len(rowptr) - 1, 20000
    for name, v in (("4·normal", v1), ("uniform", v2)):
        pre = (torch.from_numpy(v) * torch.tensor(scale, dtype=torch.float32)).numpy()
        y64, g64 = cpu_sparse_softmax(rowptr, cols, pre, M, K, dy, torch.float64)
        y32, g32 = cpu_sparse_softmax(rowptr, cols, pre, M, K, dy, torch.float32)
        y = dev_softmax(cmm, dev, v, rowptr, M, scale=scale)
        g = dev_softmax_backward(cmm, dev, y, dy, rowptr, M, scale=1.0)  # (the reference differentiates softmax(pre) in pre)
        assert_under_rule(f"csr_softmax forward, {name}, scale {scale}", rel_err(y32, y64), rel_err(y.cpu().numpy(), y64))
        assert_under_rule(f"csr_softmax backward, {name}, scale {scale}", scaled_err(g32, g64), scaled_err(g.cpu().numpy(), g64))
        # the backward's own scale: dx = scale · (the gradient at scale 1), one more rounding
        gs = dev_softmax_backward(cmm, dev, y, dy, rowptr, M, scale=scale).cpu().numpy()
        assert scaled_err(gs, scale * g64) <= 8 * scaled_err(g32, g64) + 2.0 ** -23


def torch_rows_softmax(x, rowptr):
    out = torch.empty_like(x)
    for r in range(len(rowptr) - 1):
        s, e = int(rowptr[r]), int(rowptr[r + 1])
        if e > s:
            out[s:e] = torch.softmax(x[s:e], 0)
    return out


def assert_rows_match(y, x, rowptr, what):
    """NaN by position; every other value under the rule of the accuracy check against float64 torch.softmax of the row's
    stored entries, torch-CPU float32 as e_ref."""
    y = y.cpu()
    ref32, ref64 = torch_rows_softmax(x, rowptr), torch_rows_softmax(x.double(), rowptr)
    assert torch.equal(torch.isnan(y), torch.isnan(ref64)), f"{what}: NaN positions differ"
    ok = ~torch.isnan(ref64)
    zero = ok & (ref64 == 0)
    assert (y[zero] == 0).all(), f"{what}: an entry that must be 0 is not"
    e_ref, e_dev = rel_err(ref32[ok].numpy(), ref64[ok].numpy()), rel_err(y[ok].numpy(), ref64[ok].numpy())
    assert e_dev <= 8 * max(e_ref, 2.0 ** -24), (what, e_ref, e_dev)


def test_4_special_values_and_shapes(cmm, dev):
    # empty matrix, all rows empty: nothing is written
    out = torch.full((4,), 7.0, device=dev)
    cmm.csr_softmax(torch.empty(0, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), 0, 1, 0, 1.0, out[:0])
    cmm.csr_softmax(torch.empty(0, device=dev), torch.zeros(6, dtype=torch.int32, device=dev), 0, 1, 5, 1.0, out[:0])
    assert (out == 7.0).all()
    # one row holding the whole matrix
    g = np.random.Generator(np.random.PCG64(21))
    x = torch.from_numpy((4 * g.standard_normal(3000)).astype(np.float32))
    assert_rows_match(dev_softmax(cmm, dev, x, [0, 3000], 1), x, [0, 3000], "one row")
    # the boundary lengths, and one beyond the LDS form's capacity
    lens = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 0, 6000)
    rowptr = rowptr_of(lens)
    x = torch.from_numpy((4 * g.standard_normal(int(rowptr[-1]))).astype(np.float32))
    y = dev_softmax(cmm, dev, x, rowptr, len(lens))
    assert_rows_match(y, x, rowptr, "boundary lengths")
    assert (y.cpu()[:1] == 1.0).all()  # a row of one entry
    # explicit −inf, +inf, NaN, a row of only −inf, explicit zeros — in every form (registers, LDS, streamed)
    inf, nan = float("inf"), float("nan")
    for L in (5, 40, 700, 5000):
        rows = []
        base = (4 * g.standard_normal(L)).astype(np.float32)
        for special in ((-inf,), (inf,), (nan,), (-inf, -inf, 0.0), (0.0, 0.0), (nan, inf), (inf, inf)):
            r = base.copy()
            r[g.choice(L, len(special), replace=False)] = special
            rows.append(r)
        rows.append(np.full(L, -inf, np.float32))
        rows.append(np.zeros(L, np.float32))
        rowptr = rowptr_of([L] * len(rows))
        x = torch.from_numpy(np.concatenate(rows))
        assert_rows_match(dev_softmax(cmm, dev, x, rowptr, len(rows)), x, rowptr, f"special values, rows of {L}")
    # a hub row of 10⁶ entries among short rows
    lens = [3] * 500 + [1_000_000] + [7] * 500
    rowptr = rowptr_of(lens)
    x = torch.from_numpy((4 * g.standard_normal(int(rowptr[-1]))).astype(np.float32))
    dy = torch.from_numpy(g.standard_normal(int(rowptr[-1])).astype(np.float32))
    y = dev_softmax(cmm, dev, x, rowptr, len(lens))
    y64 = torch_rows_softmax(x.double(), rowptr)
    e_ref, e_dev = rel_err(torch_rows_softmax(x, rowptr).numpy(), y64.numpy()), rel_err(y.cpu().numpy(), y64.numpy())
    assert_under_rule("csr_softmax forward, hub row of 1e6", e_ref, e_dev)
    sums, ln = row_sums64(rowptr, y.cpu().numpy())
    assert (np.abs(sums - 1.0) <= (ln + 3) * 2.0 ** -24).all()
    gdev = dev_softmax_backward(cmm, dev, y, dy, rowptr, len(lens)).cpu().double()
    yd, dd = y.cpu().double(), dy.double()
    rows = torch.from_numpy(np.repeat(np.arange(len(lens)), lens))
    dots = torch.zeros(len(lens), dtype=torch.float64).index_add_(0, rows, yd * dd)
    g64 = yd * (dd - dots[rows])
    assert scaled_err(gdev.numpy(), g64.numpy()) <= 2.0 ** -20  # (a 10⁶-term dot product in 64 fp32 chains)


def per_item_values(mm, a, scale):
    """sparse_softmax of every item of a batched CSR tensor as a 2-d call: the values, concatenated."""
    S = a.shape[-2]
    crow = a.crow_indices().reshape(-1, S + 1)
    col = a.col_indices().reshape(crow.shape[0], -1)
    val = a.values().reshape(crow.shape[0], -1)
    out = []
    for i in range(crow.shape[0]):
        item = torch.sparse_csr_tensor(crow[i], col[i], val[i], size=tuple(a.shape[-2:]))
        out.append(mm.sparse_softmax(item, scale).values())
    return torch.cat(out)


@pytest.mark.parametrize("batch_shape,S,keep,index_dtype", [((2, 3), 128, 0.2, torch.int64), ((2, 3), 128, 0.2, torch.int32),
                                                            ((384,), 512, 0.10, torch.int64)])
def test_5_batched_gives_the_bits_of_the_per_item_calls(mm, dev, batch_shape, S, keep, index_dtype):
    a = device_pattern(dev, batch_shape, S, keep, 31, index_dtype)
    g = torch.Generator(device=dev).manual_seed(32)
    a = with_values(a, 4 * torch.randn(a.values().shape, device=dev, generator=g))
    y = mm.sparse_softmax(a, 0.5)
    assert y.layout == torch.sparse_csr and y.shape == a.shape and y.values().shape == a.values().shape
    assert y.crow_indices().dtype == index_dtype
    assert_same_bits(y.values().reshape(-1), per_item_values(mm, a, 0.5), "batched vs per item")
    # and the gradient
    a = a.requires_grad_(True)
    w = with_values(a.detach(), torch.randn(a.values().shape, device=dev, generator=g))
    out = mm.sparse_softmax(a, 0.5)
    (gx,) = torch.autograd.grad(out, a, grad_outputs=w)
    k = a.values().shape[-1] // S
    y2, w2 = out.detach().values().reshape(-1, k).double(), w.values().reshape(-1, k).double()
    ref = 0.5 * y2 * (w2 - (y2 * w2).sum(-1, keepdim=True))
    assert scaled_err(gx.values().reshape(-1, k).cpu().numpy(), ref.cpu().numpy()) <= 2.0 ** -20


def test_6_forward_and_backward_record_into_a_graph(mm, dev):
    a = device_pattern(dev, (4,), 256, 0.15, 41)
    g = torch.Generator(device=dev).manual_seed(42)
    x = (4 * torch.randn(a.values().shape, device=dev, generator=g))
    a = with_values(a, x).requires_grad_(True)
    w = with_values(a.detach(), torch.randn(a.values().shape, device=dev, generator=g))

    def step():
        out = mm.sparse_softmax(a, 0.25)
        (gx,) = torch.autograd.grad(out, a, grad_outputs=w)
        return out.detach().values(), gx.detach().values()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        y_eager, g_eager = (t.clone() for t in step())  # (the pattern is narrowed here, once: it is static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # a host synchronisation in here would fail the capture
        y_cap, g_cap = step()
    for _ in range(2):
        y_cap.fill_(-1.0)
        g_cap.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert_same_bits(y_cap, y_eager, "captured forward")
        assert_same_bits(g_cap, g_eager, "captured backward")
