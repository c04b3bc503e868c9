#!/usr/bin/env python3
"""Block-sparse attention on the matrix cores against its two yardsticks, timed side by side in one run.

    python tools/bench_block_attention.py [--rounds 7] [--iters 10] [--log profiles/r14_block_attention.log]

Per shape (batch × S², D = 64, block 64, bfloat16) and block layout — a sliding window of 3 blocks, the window plus one
global block column, about 25 % of the blocks kept at random, and the window under causal=True —: forward and forward +
backward of matmuls.block_sparse_attention, of torch's dense masked scaled_dot_product_attention, and of
matmuls.fused_sparse_attention on the element-wise expansion of the same layout (the only bfloat16 batch path before this
one).  The contestants of a case are timed in interleaved rounds (one after the other inside every round, so that clock
and cache state drift over all alike); each figure is the median over the rounds of the mean of `iters` back-to-back
calls between two events, with the spread (min … max over the rounds) beside it.  The block path's MFMA TFLOP/s count
the kept blocks' flops only: 4·64²·D per kept block forward, 10·64²·D backward (causal: the blocks at or below the
diagonal, the diagonal ones counted whole).  The layout is static: its narrowed and transposed forms are built in the
warm-up, as in a training loop.
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "matrix-multiplication_amd"))
sys.path.insert(0, str(REPO / "tests"))

SHAPES = [(384, 512), (96, 1024), (48, 2048)]
D, BLOCK = 64, 64


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def block_masks(nb, dev, seed):
    """{name: (boolean [nb, nb] block mask, causal)} of the four cases."""
    i = torch.arange(nb, device=dev)
    window = (i[:, None] - i[None, :]).abs() <= 1
    glob = window.clone()
    glob[:, 0] = True
    g = torch.Generator(device=dev).manual_seed(seed)
    keep = max(1, round(0.25 * nb))
    rand = torch.zeros(nb, nb, dtype=torch.bool, device=dev)
    rand.scatter_(1, torch.rand(nb, nb, device=dev, generator=g).topk(keep, dim=-1).indices, True)
    return {"window 3": (window, False), "window 3 + global column": (glob, False), "random 25 %": (rand, False),
            "window 3, causal": (window, True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--log", default=str(REPO / "profiles" / "r14_block_attention.log"))
    args = ap.parse_args()
    import matmuls
    dev = torch.device("cuda:0")
    lines = [f"# tools/bench_block_attention.py --rounds {args.rounds} --iters {args.iters}: ms, median over the rounds "
             f"[min … max]; bfloat16, D = {D}, block {BLOCK}; {torch.cuda.get_device_name(0)}"]

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    for items, S in SHAPES:
        nb = S // BLOCK
        g = torch.Generator(device=dev).manual_seed(8)
        q, k, v = (torch.randn(items, S, D, device=dev, generator=g).bfloat16().requires_grad_(True) for _ in range(3))
        w = torch.randn(items, S, D, device=dev, generator=g).bfloat16()
        x = (q, k, v)
        for name, (bm, causal) in block_masks(nb, dev, 9).items():
            layout = bm.float().to_sparse_csr()
            mask = bm.repeat_interleave(BLOCK, 0).repeat_interleave(BLOCK, 1)
            if causal:
                mask = mask & torch.ones(S, S, dtype=torch.bool, device=dev).tril()
            counted = (bm & torch.ones(nb, nb, dtype=torch.bool, device=dev).tril()) if causal else bm
            blocks = int(counted.sum()) * items
            # the element-wise pattern of the same mask, one copy of the indices per item (equal counts per item)
            e2 = mask.float().to_sparse_csr()
            nnz = e2.values().numel()
            elementwise = torch.sparse_csr_tensor(e2.crow_indices().expand(items, S + 1).contiguous(),
                                                  e2.col_indices().expand(items, nnz).contiguous(),
                                                  torch.ones(items, nnz, device=dev), size=(items, S, S))

            def block_fn():
                return matmuls.block_sparse_attention(q, k, v, layout, block=BLOCK, causal=causal)

            def sdpa_fn():
                return torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask)

            def fused_fn():
                return matmuls.fused_sparse_attention(q, k, v, elementwise)

            def step(fn):
                def run():
                    torch.autograd.grad(fn(), x, grad_outputs=w)
                return run

            runs = {"block bf16 fwd": block_fn, "block bf16 fwd+bwd": step(block_fn),
                    "dense sdpa bf16 fwd": sdpa_fn, "dense sdpa bf16 fwd+bwd": step(sdpa_fn),
                    "fused csr bf16 fwd": fused_fn, "fused csr bf16 fwd+bwd": step(fused_fn)}
            for fn in runs.values():  # warm-up: every kernel loaded, the layouts' kept forms built
                fn()
                fn()
            torch.cuda.synchronize()
            samples = {n: [] for n in runs}
            for _ in range(args.rounds):
                for n, fn in runs.items():
                    samples[n].append(timed(fn, args.iters))
            emit(f"\n{items} x {S}^2, {name}: {blocks // items} of {nb * nb} blocks counted per item "
                 f"({blocks / items / (nb * nb):.1%}), {nnz} element-wise entries per item")
            med = {}
            for n, xs in samples.items():
                med[n] = statistics.median(xs)
                emit(f"  {n:26s} {med[n]:8.3f}  [{min(xs):.3f} … {max(xs):.3f}]")
            flops = blocks * BLOCK * BLOCK * D
            emit(f"  block path MFMA TFLOP/s over the kept blocks: fwd {4 * flops / med['block bf16 fwd'] / 1e9:.1f}, "
                 f"fwd+bwd {14 * flops / med['block bf16 fwd+bwd'] / 1e9:.1f}")
            emit(f"  ratio dense sdpa / block: fwd {med['dense sdpa bf16 fwd'] / med['block bf16 fwd']:.2f}, "
                 f"fwd+bwd {med['dense sdpa bf16 fwd+bwd'] / med['block bf16 fwd+bwd']:.2f}")
            emit(f"  ratio fused csr / block: fwd {med['fused csr bf16 fwd'] / med['block bf16 fwd']:.2f}, "
                 f"fwd+bwd {med['fused csr bf16 fwd+bwd'] / med['block bf16 fwd+bwd']:.2f}")
            del elementwise, e2, mask
    Path(args.log).parent.mkdir(parents=True, exist_ok=True)
    Path(args.log).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
