"""CSR × dense with reduce = sum / mean / amax / amin (torch.sparse.mm's `reduce`) on the shapes the sum path is measured on.

    python tools/bench_spmm_reduce.py [--only TAG] [--log FILE] [--dtype float32|bfloat16|float16]

Shapes: C2 (64 K x 64 K at 0.1 % x 128), C3 (1 M x 1 M at 0.01 % x 256), tools/bench_skew.py's hub-row matrix (100 K rows
of 100 entries plus rows of 10^5, 3·10^5 and 10^6 entries, K = 1 M, N = 256) and the three GNN-like shapes of
tools/bench_degree_skew.py (Pareto row lengths clipped at 8000, its generators).  Per shape, interleaved medians (ms) of:
sum (custom_mm.naive_spmm), mean, amax and amin without arg, amax with arg, and forward + backward through
matmuls.sparse_mm_reduce for sum / mean / amax; the ratios the targets are stated in; algorithmic GB/s of amax
(nnz·(4N+8) + 4(M+1) + 4MN, + 4MN with arg).  Sampled rows (the longest included) of mean and of amax with arg are
compared with torch-CPU's aten::_sparse_mm_reduce_impl on their sub-CSR: amax bit for bit (arg included), mean to 1e-5.
--dtype bfloat16 / float16 runs every entry on operands of that type (bytes nnz·(2N+6) + 4(M+1) + 2MN), times the float32
amax beside them in the same interleaved rounds (the `T/f32` ratio) and checks the sampled rows against torch-CPU on the
widened operands, narrowed.
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "matrix-multiplication_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import custom_mm  # noqa: E402
import matmuls  # noqa: E402
from bench_degree_skew import csr_from_lengths, pareto_lengths  # noqa: E402
from bench_hbm_regime import time_interleaved  # noqa: E402

dev = torch.device("cuda")


def shape_csr(name):
    """(M, K, N, rowptr, col, val) on the device."""
    if name == "C2":
        M, N = 65_536, 128
        return (M, M, N) + csr_from_lengths(torch.full((M,), 66, dtype=torch.int64, device=dev), M, 2)
    if name == "C3":
        M, N = 1_000_000, 256
        return (M, M, N) + csr_from_lengths(torch.full((M,), 100, dtype=torch.int64, device=dev), M, 3)
    if name == "hub":  # tools/bench_skew.py's matrix
        M, K, N = 100_000, 1_000_000, 256
        g = torch.Generator(device=dev).manual_seed(0)
        lens = torch.full((M,), 100, dtype=torch.int64)
        lens[7], lens[5000], lens[99_999] = 1_000_000, 100_000, 300_000
        rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)]).to(torch.int32).to(dev)
        nnz = int(lens.sum())
        col = torch.randint(0, K, (nnz,), device=dev, dtype=torch.int32, generator=g)
        val = torch.rand(nnz, device=dev, generator=g)
        return M, K, N, rowptr, col, val
    M, N, mean = {"arxiv": (170_000, 128, 14), "reddit": (233_000, 602, 490), "products": (2_400_000, 100, 50)}[name]
    return (M, M, N) + csr_from_lengths(pareto_lengths(M, mean, 8000, M, seed=1), M, 5)


def check_rows(rowptr, col, val, B, C_mean, C_max, arg, n=48, seed=0):
    """Sampled rows (the longest three included) vs torch-CPU on their sub-CSR: amax bits + arg, mean to 1e-5."""
    M = rowptr.numel() - 1
    lens = (rowptr[1:] - rowptr[:-1]).long()
    rows = torch.unique(torch.cat([torch.topk(lens, 3).indices.cpu(),
                                   torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).choice(M, n, replace=False))]))
    rows_d = rows.to(dev)
    starts, ls = rowptr[rows_d].long(), lens[rows_d]
    idx = torch.repeat_interleave(starts - torch.cumsum(ls, 0) + ls, ls) + torch.arange(int(ls.sum()), device=dev)
    uniq, inv = torch.unique(col[idx], return_inverse=True)
    rp = torch.zeros(len(rows) + 1, dtype=torch.int64)
    rp[1:] = torch.cumsum(ls.cpu(), 0)
    a = torch.sparse_csr_tensor(rp, inv.long().cpu(), val[idx].float().cpu(), (len(rows), len(uniq))).requires_grad_()
    Bs = B[uniq.long()].float().cpu()
    want_max, want_arg = torch.ops.aten._sparse_mm_reduce_impl(a, Bs, "amax")
    want_mean, _ = torch.ops.aten._sparse_mm_reduce_impl(a, Bs, "mean")
    lowp = C_max.dtype != torch.float32
    want_max = want_max.detach().to(C_max.dtype).float()  # (narrowed once: the low-precision contract)
    nnz = col.numel()
    mapped = torch.where(want_arg == idx.numel(), torch.tensor(nnz),
                         starts.cpu()[:, None] + (want_arg - rp[:-1][:, None]))
    got_max, got_arg = C_max[rows_d].float().cpu(), arg[rows_d].cpu().long()
    same_max = torch.equal(torch.isnan(got_max), torch.isnan(want_max)) and \
        torch.equal(got_max.nan_to_num().view(torch.int32), want_max.nan_to_num().view(torch.int32))
    tol = torch.finfo(C_mean.dtype).eps if lowp else 1e-5
    close_mean = torch.allclose(C_mean[rows_d].float().cpu(), want_mean.detach(), rtol=tol, atol=tol if lowp else 1e-6)
    return same_max and torch.equal(got_arg, mapped), close_mean, len(rows)


def fwd_bwd(a, b, reduce, G):
    def step():
        a.grad = b.grad = None
        matmuls.sparse_mm_reduce(a, b, reduce).backward(G)
    return step


def run(name, out, dtype=torch.float32):
    t0 = time.time()
    M, K, N, rowptr, col, val = shape_csr(name)
    nnz = col.numel()
    g = torch.Generator(device=dev).manual_seed(7)
    B = torch.randn(K, N, device=dev, generator=g)
    lowp = dtype != torch.float32
    if lowp:
        val32, B32, C32 = val, B, torch.empty(M, N, device=dev)
        val, B = val.to(dtype), B.to(dtype)
    C = {k: torch.empty(M, N, device=dev, dtype=dtype) for k in ("sum", "mean", "amax", "amin", "amax_arg")}
    arg = torch.empty(M, N, device=dev, dtype=torch.int32)
    ent = {
        "sum": lambda: custom_mm.naive_spmm(val, col, rowptr, nnz, M, K, B, C["sum"]),
        "mean": lambda: custom_mm.naive_spmm_reduce(val, col, rowptr, nnz, M, K, B, C["mean"], "mean"),
        "amax": lambda: custom_mm.naive_spmm_reduce(val, col, rowptr, nnz, M, K, B, C["amax"], "amax"),
        "amin": lambda: custom_mm.naive_spmm_reduce(val, col, rowptr, nnz, M, K, B, C["amin"], "amin"),
        "amax_arg": lambda: custom_mm.naive_spmm_reduce(val, col, rowptr, nnz, M, K, B, C["amax_arg"], "amax", arg),
    }
    if lowp:
        ent["amax_f32"] = lambda: custom_mm.naive_spmm_reduce(val32, col, rowptr, nnz, M, K, B32, C32, "amax")
    t = time_interleaved(ent)
    ok_max, ok_mean, nrows = check_rows(rowptr, col, val, B, C["mean"], C["amax_arg"], arg)
    same_noarg = torch.equal(C["amax"].view(torch.int16 if lowp else torch.int32),
                             C["amax_arg"].view(torch.int16 if lowp else torch.int32))
    a = torch.sparse_csr_tensor(rowptr, col, val, (M, K)).requires_grad_()
    b = B.clone().requires_grad_()
    Gd = torch.randn(M, N, device=dev, generator=g).to(dtype)
    tb = time_interleaved({r: fwd_bwd(a, b, r, Gd) for r in ("sum", "mean", "amax")}, rounds=2)
    byts = nnz * (2 * N + 6) + 4 * (M + 1) + 2 * M * N if lowp else nnz * (4 * N + 8) + 4 * (M + 1) + 4 * M * N
    longest = int((rowptr[1:] - rowptr[:-1]).max())
    line = (f"{name:9s} M={M} K={K} N={N} nnz={nnz} longest={longest} | ms: sum {t['sum']:.3f} mean {t['mean']:.3f} "
            f"amax {t['amax']:.3f} amin {t['amin']:.3f} amax+arg {t['amax_arg']:.3f} | amax/sum {t['amax'] / t['sum']:.2f} "
            f"arg/noarg {t['amax_arg'] / t['amax']:.2f} mean/sum {t['mean'] / t['sum']:.2f} | amax {byts / t['amax'] / 1e6:.0f} GB/s "
            f"(+arg {(byts + 4 * M * N) / t['amax_arg'] / 1e6:.0f}) | fwd+bwd ms: sum {tb['sum']:.2f} mean {tb['mean']:.2f} "
            f"amax {tb['amax']:.2f} | {nrows} rows vs torch-CPU: amax+arg bits {'ok' if ok_max else 'FAIL'}, "
            f"mean {'ok' if ok_mean else 'FAIL'}; amax without arg = with arg {'ok' if same_noarg else 'FAIL'} "
            f"[{time.time() - t0:.0f} s]")
    if lowp:
        line += f" | float32 amax {t['amax_f32']:.3f} ms, T/f32 {t['amax'] / t['amax_f32']:.2f}"
    print(line, flush=True)
    out.append(line)
    del a, b, Gd, C, arg, B, rowptr, col, val
    torch.cuda.empty_cache()
    return ok_max and ok_mean and same_noarg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--log", default="")
    ap.add_argument("--dtype", default="float32", choices=("float32", "bfloat16", "float16"))
    a = ap.parse_args()
    head = (f"# device {torch.cuda.get_device_name(0)}; interleaved medians, ms per call; algorithmic bytes "
            f"nnz·(4N+8)+4(M+1)+4MN (+4MN arg)")
    if a.dtype != "float32":
        head = (f"# device {torch.cuda.get_device_name(0)}; {a.dtype}; interleaved medians, ms per call; algorithmic bytes "
                f"nnz·(2N+6)+4(M+1)+2MN (+4MN arg)")
    print(head, flush=True)
    out, ok = [head], True
    for name in ("C2", "C3", "hub", "arxiv", "reddit", "products"):
        if a.only and a.only != name:
            continue
        ok = run(name, out, getattr(torch, a.dtype)) and ok
    if a.log:
        Path(a.log).parent.mkdir(parents=True, exist_ok=True)
        Path(a.log).write_text("\n".join(out) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
