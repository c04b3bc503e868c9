"""The CSR row softmax (custom_mm.csr_softmax / csr_softmax_backward) and the sparse attention step built on it.

    python tools/bench_csr_softmax.py [--quick] [--log FILE] [--only softmax|attention]

Softmax alone — forward and backward, float32 — on
  c3        1 M x 1 M at 0.01 % (config C3's pattern: Binomial row lengths, mean 105)
  hub       the hub-row matrix of tools/bench_skew.py (100 K rows of 100 entries; three rows of 10^6, 10^5 and 3·10^5)
  arxiv / reddit / products   the GNN-like Pareto row lengths of tools/bench_degree_skew.py
  attn25 / attn10 / attn5     384 x 512 x 512 batched attention patterns, 25 / 10 / 5 % kept per row
beside, IN THE SAME RUN and interleaved with it (the entries share clock and power state):
  copy      y.copy_(x) of the same values array: the same 8·nnz bytes, the bandwidth yardstick of a one-read one-write kernel
  coo       torch.sparse.softmax on the COO form on the device, if this torch build runs it (the failure is logged if not)
Algorithmic bytes: 8·nnz + 4·(rows + batch) forward, 12·nnz + 4·(rows + batch) backward.

The whole step — sparse_attention forward + backward at the attention shapes (D = 64) — beside
  prune     the existing dense-then-prune route of benchmarks/bert_attention.py: cublasTransbMM scores, dense softmax,
            mask, naiveSpMM (dense → CSR on every step)
  dense     the dense classes: cublasTransbMM, dense softmax, cublasMM

Each figure is the median of `--rounds` interleaved rounds with the spread (min … max) beside it.
"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "matrix-multiplication_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import custom_mm  # noqa: E402
import matmuls  # noqa: E402

dev = torch.device("cuda")


def interleaved(fns, rounds, iters):
    """{name: (median, min, max) ms per call}: every round times each entry once (iters calls between two events), in turn."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / iters)
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in times.items()}


def fmt(t):
    return f"{t[0]:.4f} ms ({t[1]:.4f} … {t[2]:.4f})"


def binomial_offsets(M, K, density, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    lens = torch.binomial(torch.full((M,), float(K), device=dev), torch.full((M,), density, device=dev), generator=g).long()
    return torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), lens.cumsum(0)]).to(torch.int32)


def softmax_shapes(quick):
    from bench_degree_skew import pareto_lengths
    def from_lens(lens):
        return torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), lens.to(dev).cumsum(0)]).to(torch.int32), 1, lens.numel()
    s = 8 if quick else 1
    yield "c3", (binomial_offsets(1_000_000 // s, 1_000_000, 1e-4, 0), 1, 1_000_000 // s)
    lens = torch.full((100_000,), 100, dtype=torch.int64)
    lens[7], lens[5000], lens[99_999] = 1_000_000, 100_000, 300_000
    yield "hub", from_lens(lens)
    for tag, M, mean in (("arxiv", 170_000, 14), ("reddit", 233_000, 490), ("products", 2_400_000 // s, 50)):
        yield tag, from_lens(pareto_lengths(M, mean, 0, M, seed=3))
    nb, S = (48 if quick else 384), 512
    for keep in (25, 10, 5):
        k = round(S * keep / 100)
        offs = (torch.arange(S + 1, device=dev) * k).unsqueeze(0) + (torch.arange(nb, device=dev) * S * k).unsqueeze(1)
        yield f"attn{keep}", (offs.to(torch.int32).contiguous(), nb, S)


def bench_softmax(out, quick, rounds):
    out("# softmax alone, float32: ms per call, median (min … max) of interleaved rounds; GB/s on the algorithmic bytes")
    for tag, (offs, batch, M) in softmax_shapes(quick):
        nnz = int(offs.reshape(-1)[-1])
        g = torch.Generator(device=dev).manual_seed(1)
        x = 4 * torch.randn(nnz, device=dev, generator=g)
        dy = torch.randn(nnz, device=dev, generator=g)
        y, dx, c = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        custom_mm.csr_softmax(x, offs, nnz, batch, M, 1.0, y)
        fns = {"fwd": lambda: custom_mm.csr_softmax(x, offs, nnz, batch, M, 1.0, y),
               "bwd": lambda: custom_mm.csr_softmax_backward(y, dy, offs, nnz, batch, M, 1.0, dx),
               "copy": lambda: c.copy_(x)}
        coo_note = ""
        if batch == 1 and nnz <= 120_000_000:
            try:
                rows = torch.repeat_interleave(torch.arange(M, device=dev), (offs[1:] - offs[:-1]).long())
                pos = torch.arange(nnz, device=dev) - offs[:-1].long()[rows]  # distinct columns: the position in the row
                coo = torch.sparse_coo_tensor(torch.stack([rows, pos]), x, (M, int(pos.max()) + 1)).coalesce()
                torch.sparse.softmax(coo, 1)
                fns["coo"] = lambda: torch.sparse.softmax(coo, 1)
            except Exception as e:  # noqa: BLE001  (recorded, as asked: whether this build runs it on the device)
                coo_note = f"  coo: {type(e).__name__}: {str(e).splitlines()[0][:120]}"
        t = interleaved(fns, rounds, 5)
        fb, bb = 8 * nnz + 4 * (batch * (M + 1)), 12 * nnz + 4 * (batch * (M + 1))
        line = (f"{tag:9s} rows {batch * M:8d} nnz {nnz:10d} mean {nnz / (batch * M):7.1f} | fwd {fmt(t['fwd'])} "
                f"{fb / t['fwd'][0] / 1e6:6.0f} GB/s | bwd {fmt(t['bwd'])} {bb / t['bwd'][0] / 1e6:6.0f} GB/s | copy {fmt(t['copy'])} "
                f"{8 * nnz / t['copy'][0] / 1e6:6.0f} GB/s | fwd/copy {t['fwd'][0] / t['copy'][0]:.2f} bwd/copy {t['bwd'][0] / t['copy'][0]:.2f}")
        if "coo" in t:
            line += f" | coo {fmt(t['coo'])} fwd is {t['coo'][0] / t['fwd'][0]:.1f}x faster"
        out(line + coo_note)
        del x, dy, y, dx, c, fns


def bench_attention(out, quick, rounds):
    out("# sparse_attention forward + backward, float32, D = 64: ms per step, median (min … max); prune = dense scores + dense "
        "softmax + mask + naiveSpMM (benchmarks/bert_attention.py), dense = the dense classes")
    nb, S, D = (48 if quick else 384), 512, 64
    g = torch.Generator(device=dev).manual_seed(2)
    q, k, v = (torch.randn(nb, S, D, device=dev, generator=g, requires_grad=True) for _ in range(3))
    w = torch.randn(nb, S, D, device=dev, generator=g)
    scale = 1.0 / D ** 0.5
    for keep in (25, 10, 5):
        kk = round(S * keep / 100)
        cols = torch.rand(nb, S, S, device=dev, generator=g).topk(kk, dim=-1).indices.sort(dim=-1).values
        crow = (torch.arange(S + 1, device=dev) * kk).expand(nb, S + 1).contiguous()
        pattern = torch.sparse_csr_tensor(crow, cols.reshape(nb, -1).contiguous(), torch.ones(nb, S * kk, device=dev), size=(nb, S, S))
        mask = torch.zeros(nb, S, S, device=dev).scatter_(-1, cols, 1.0)
        neg = (1.0 - mask) * -1e30

        def step(fn):
            def run():
                for t in (q, k, v):
                    t.grad = None
                fn().backward(w)
            return run

        def sparse():
            return matmuls.sparse_attention(q, k, v, pattern)

        def prune():
            s = matmuls.cublasTransbMM.apply(q, k) * scale + neg
            return matmuls.naiveSpMM.apply(torch.softmax(s, -1) * mask, v)

        def dense():
            s = matmuls.cublasTransbMM.apply(q, k) * scale + neg
            return matmuls.cublasMM.apply(torch.softmax(s, -1), v)

        ref = dense()
        err = float((sparse() - ref).abs().max())
        t = interleaved({"sparse": step(sparse), "prune": step(prune), "dense": step(dense)}, rounds, 3)
        out(f"attn{keep:<3d} {nb} x {S} x {S}, {kk} kept per row | sparse_attention {fmt(t['sparse'])} | prune {fmt(t['prune'])} "
            f"({t['prune'][0] / t['sparse'][0]:.2f}x) | dense {fmt(t['dense'])} ({t['dense'][0] / t['sparse'][0]:.2f}x) | "
            f"max |sparse - dense| {err:.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="smaller shapes (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--log", default=None)
    ap.add_argument("--only", choices=("softmax", "attention"), default=None)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the device; there is no fallback"
    log = open(a.log, "a") if a.log else None

    def out(line):
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()

    out(f"# tools/bench_csr_softmax.py{' --quick' if a.quick else ''} on {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    if a.only != "attention":
        bench_softmax(out, a.quick, a.rounds)
    if a.only != "softmax":
        bench_attention(out, a.quick, a.rounds)


if __name__ == "__main__":
    main()
