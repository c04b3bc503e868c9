#!/usr/bin/env python3
"""Block-sparse × dense products on the matrix cores against their two yardsticks, timed side by side in one run
(DESIGN.md §3.15).

    python tools/bench_block_mm.py [--rounds 5] [--iters 5] [--log profiles/r15_block_mm.log]

Per shape (M × K × N, bfloat16, 64 × 64 blocks) and fraction of the blocks kept at random (50 / 25 / 10 / 5 %): forward and
forward + backward (both gradients) of matmuls.block_sparse_mm, of this package's dense product cublasMM on the densified
A, and of naiveSpMM on the element-wise expansion of the same A (the only bfloat16 sparse path before this one).  The
contestants of a case are timed in interleaved rounds (one after the other inside every round, so that clock and cache
state drift over all alike); each figure is the median over the rounds of the mean of `iters` back-to-back calls between
two events, with the spread (min … max over the rounds) beside it.  The block path's MFMA TFLOP/s count the kept blocks'
flops only: 2·64²·N per kept block forward, three times that forward + backward.  The layout is static: its sorted and
transposed lists are built in the warm-up, as in a training loop.
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "matrix-multiplication_amd"))

SHAPES = [(8192, 8192, 8192), (4096, 4096, 16384)]
FRACTIONS = [0.50, 0.25, 0.10, 0.05]
BLOCK = 64


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-csr", action="store_true", help="leave the element-wise CSR contestant out")
    ap.add_argument("--log", default=str(REPO / "profiles" / "r15_block_mm.log"))
    args = ap.parse_args()
    import matmuls
    dev = torch.device("cuda:0")
    lines = [f"# tools/bench_block_mm.py --rounds {args.rounds} --iters {args.iters}: ms, median over the rounds "
             f"[min … max]; bfloat16, block {BLOCK}; {torch.cuda.get_device_name(0)}"]

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    for M, K, N in SHAPES:
        g = torch.Generator(device=dev).manual_seed(8)
        b = torch.randn(K, N, device=dev, generator=g).bfloat16().requires_grad_(True)
        w = torch.randn(M, N, device=dev, generator=g).bfloat16()
        for frac in FRACTIONS:
            rb, cb = M // BLOCK, K // BLOCK
            keep = max(1, round(frac * cb))
            bm = torch.zeros(rb, cb, dtype=torch.bool, device=dev)
            bm.scatter_(1, torch.rand(rb, cb, device=dev, generator=g).topk(keep, dim=-1).indices, True)
            dense = (torch.randn(M, K, device=dev, generator=g) / 8).bfloat16()
            dense = dense * bm.repeat_interleave(BLOCK, 0).repeat_interleave(BLOCK, 1)
            bsr = dense.to_sparse_bsr((BLOCK, BLOCK))
            values, layout = matmuls.bsr_parts(bsr)
            values = values.detach().clone().requires_grad_(True)
            n = values.shape[0]
            a_dense = dense.clone().requires_grad_(True)

            def block_fn():
                return matmuls.block_sparse_mm(values, layout, b)

            def dense_fn():
                return matmuls.cublasMM.apply(a_dense, b)

            def step(fn, leaves):
                def run():
                    torch.autograd.grad(fn(), leaves, grad_outputs=w)
                return run

            runs = {"block bf16 fwd": block_fn, "block bf16 fwd+bwd": step(block_fn, (values, b)),
                    "dense bf16 fwd": dense_fn, "dense bf16 fwd+bwd": step(dense_fn, (a_dense, b))}
            csr_note = ""
            if not args.no_csr:
                try:
                    a_csr = dense.to_sparse_csr().requires_grad_(True)

                    def csr_fn():
                        return matmuls.naiveSpMM.apply(a_csr, b)

                    csr_fn()
                    step(csr_fn, (a_csr, b))()
                    runs["csr bf16 fwd"], runs["csr bf16 fwd+bwd"] = csr_fn, step(csr_fn, (a_csr, b))
                except Exception as e:  # the expansion does not fit, or the path refuses it: said in the log
                    csr_note = f"  element-wise csr: not run ({type(e).__name__}: {str(e)[:120]})"
            del dense
            for fn in runs.values():  # warm-up: every kernel loaded, the layout's kept lists built
                fn()
                fn()
            torch.cuda.synchronize()
            samples = {name: [] for name in runs}
            for _ in range(args.rounds):
                for name, fn in runs.items():
                    samples[name].append(timed(fn, args.iters))
            emit(f"\n{M} x {K} x {N}, {frac:.0%} of the blocks: {n} of {rb * cb} blocks kept ({keep} per block row)")
            med = {}
            for name, xs in samples.items():
                med[name] = statistics.median(xs)
                emit(f"  {name:22s} {med[name]:9.3f}  [{min(xs):.3f} … {max(xs):.3f}]")
            if csr_note:
                emit(csr_note)
            flops = 2.0 * n * BLOCK * BLOCK * N
            emit(f"  block path MFMA TFLOP/s over the kept blocks: fwd {flops / med['block bf16 fwd'] / 1e9:.1f}, "
                 f"fwd+bwd {3 * flops / med['block bf16 fwd+bwd'] / 1e9:.1f}")
            emit(f"  ratio dense / block: fwd {med['dense bf16 fwd'] / med['block bf16 fwd']:.2f}, "
                 f"fwd+bwd {med['dense bf16 fwd+bwd'] / med['block bf16 fwd+bwd']:.2f}")
            if "csr bf16 fwd" in med:
                emit(f"  ratio csr / block: fwd {med['csr bf16 fwd'] / med['block bf16 fwd']:.2f}, "
                     f"fwd+bwd {med['csr bf16 fwd+bwd'] / med['block bf16 fwd+bwd']:.2f}")
            runs.clear()
            del values, layout, bsr, a_dense
            torch.cuda.empty_cache()
    Path(args.log).parent.mkdir(parents=True, exist_ok=True)
    Path(args.log).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
