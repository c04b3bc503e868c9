#!/usr/bin/env python3
"""Fused against composed sparse attention, timed side by side in one run.

    python tools/bench_fused_attention.py [--rounds 7] [--iters 10] [--log profiles/r13_fused_attention.log]

Per shape (batch × S², share of the entries kept, D = 64): forward and forward + backward of
matmuls.fused_sparse_attention and matmuls.sparse_attention in float32, the fused step in bfloat16, and torch's dense
masked scaled_dot_product_attention in bfloat16 as the outside yardstick.  The contestants of a shape are timed in
interleaved rounds (one after the other inside every round, so that clock and cache state drift over all alike); each
figure is the median over the rounds of the mean of `iters` back-to-back calls between two events, with the spread
(min … max over the rounds) beside it.  Peak allocated memory across one forward + backward is taken for both float32
paths.  The pattern is static: its narrowed and transposed forms are built in the warm-up, as in a training loop.
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "matrix-multiplication_amd"))
sys.path.insert(0, str(REPO / "tests"))

SHAPES = [(384, 512, 0.25), (384, 512, 0.10), (384, 512, 0.05), (96, 1024, 0.10), (48, 2048, 0.10)]
D = 64


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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--log", default=str(REPO / "profiles" / "r13_fused_attention.log"))
    args = ap.parse_args()
    import matmuls
    from sparse_attention_helpers import device_pattern
    dev = torch.device("cuda:0")
    lines = [f"# tools/bench_fused_attention.py --rounds {args.rounds} --iters {args.iters}: ms, median over the rounds "
             f"[min … max]; D = {D}; {torch.cuda.get_device_name(0)}"]

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    for nb, S, keep in SHAPES:
        a = device_pattern(dev, (nb,), S, keep, 7)
        nnz = a.values().numel()
        g = torch.Generator(device=dev).manual_seed(8)
        q, k, v = (torch.randn(nb, S, D, device=dev, generator=g, requires_grad=True) for _ in range(3))
        w = torch.randn(nb, S, D, device=dev, generator=g)
        qb, kb, vb = (t.detach().bfloat16().requires_grad_(True) for t in (q, k, v))
        wb = w.bfloat16()
        mask = torch.zeros(nb, S, S, device=dev, dtype=torch.bool)
        mask.view(nb * S, S).scatter_(1, a.col_indices().reshape(nb * S, -1), True)

        def fwd(fn, x):
            return lambda: fn(*x, a)

        def step(fn, x, g_out):
            def run():
                out = fn(*x, a)
                torch.autograd.grad(out, x, grad_outputs=g_out)
            return run

        def sdpa(*x):
            return torch.nn.functional.scaled_dot_product_attention(*x, attn_mask=mask)

        def sdpa_step():
            out = sdpa(qb, kb, vb)
            torch.autograd.grad(out, (qb, kb, vb), grad_outputs=wb)

        f32, b16 = (q, k, v), (qb, kb, vb)
        runs = {
            "fused f32 fwd": fwd(matmuls.fused_sparse_attention, f32),
            "composed f32 fwd": fwd(matmuls.sparse_attention, f32),
            "fused f32 fwd+bwd": step(matmuls.fused_sparse_attention, f32, w),
            "composed f32 fwd+bwd": step(matmuls.sparse_attention, f32, w),
            "fused bf16 fwd": fwd(matmuls.fused_sparse_attention, b16),
            "fused bf16 fwd+bwd": step(matmuls.fused_sparse_attention, b16, wb),
            "dense sdpa bf16 fwd": lambda: sdpa(qb, kb, vb),
            "dense sdpa bf16 fwd+bwd": sdpa_step,
        }
        peaks = {}
        for name in ("fused f32 fwd+bwd", "composed f32 fwd+bwd"):
            runs[name]()  # (the pattern's kept forms exist before the peak is taken)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            runs[name]()
            torch.cuda.synchronize()
            peaks[name] = torch.cuda.max_memory_allocated() - base
        for fn in runs.values():  # warm-up: every kernel loaded
            fn()
            fn()
        torch.cuda.synchronize()
        samples = {name: [] for name in runs}
        for _ in range(args.rounds):
            for name, fn in runs.items():
                samples[name].append(timed(fn, args.iters))
        emit(f"\n{nb} x {S}^2, {keep:.0%} kept ({nnz} entries, {nnz // (nb * S)} per row)")
        med = {}
        for name, xs in samples.items():
            med[name] = statistics.median(xs)
            emit(f"  {name:26s} {med[name]:8.3f}  [{min(xs):.3f} … {max(xs):.3f}]")
        emit(f"  ratio composed / fused f32: fwd {med['composed f32 fwd'] / med['fused f32 fwd']:.2f}, "
             f"fwd+bwd {med['composed f32 fwd+bwd'] / med['fused f32 fwd+bwd']:.2f}")
        emit(f"  ratio fused f32 / fused bf16: fwd {med['fused f32 fwd'] / med['fused bf16 fwd']:.2f}, "
             f"fwd+bwd {med['fused f32 fwd+bwd'] / med['fused bf16 fwd+bwd']:.2f}")
        emit(f"  ratio dense sdpa bf16 / fused bf16: fwd {med['dense sdpa bf16 fwd'] / med['fused bf16 fwd']:.2f}, "
             f"fwd+bwd {med['dense sdpa bf16 fwd+bwd'] / med['fused bf16 fwd+bwd']:.2f}")
        emit(f"  peak allocated across fwd+bwd, f32: fused {peaks['fused f32 fwd+bwd'] / 2 ** 20:.1f} MiB, "
             f"composed {peaks['composed f32 fwd+bwd'] / 2 ** 20:.1f} MiB")
        del mask
    Path(args.log).parent.mkdir(parents=True, exist_ok=True)
    Path(args.log).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
