#!/usr/bin/env python3
"""Query-aware key-block selection for decoding, measured.

    python tools/bench_block_attention_select.py [--batch 8] [--lens 32768,131072] [--ratio 16] [--rounds 5] [--iters 10]
                                                 [--log profiles/r32_block_attention_select.log] [--append]

bfloat16, D = 128, Hkv = 8 k / v heads, G = 4 query heads each, T = 1 new token at pos = k_len − 1 of a full cache
(Smax = k_len), K = Smax / 64 / ratio, sink = 1, local = 2.  Contestants of a row are timed in interleaved rounds, each
figure the median over the rounds of the mean of `iters` calls, with the spread (min … max) beside it — once as `iters`
back-to-back eager calls between two events (the Python front end's checks included) and once as ONE captured graph of
`iters` calls replayed between two events (the device's share):
  bounds last=1     matmuls.key_block_bounds(k, lens, bounds, last=1): the refresh after an append of one token;
  select            matmuls.select_key_blocks(q, bounds, lens, K, sink=1, local=2);
  decode selected   matmuls.block_sparse_attention_decode_selected on the lists of the select call;
  step              the three in sequence;
  dense decode      matmuls.block_sparse_attention_decode with the dense causal layout: what the step replaces.
Per row the bytes' own time: the bounds read Smax/64 · 4·D bytes and the kept k / v K · 256·D bytes per (b, h), over 8 TB/s,
the HBM rate of §3.18.
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "matrix-multiplication_amd"))
sys.path.insert(0, str(REPO / "tools"))

from bench_block_attention import timed  # noqa: E402
from bench_block_attention_decode import square_layout  # noqa: E402

D, BLOCK, HKV, G = 128, 64, 8, 4
HBM_BYTES_PER_S = 8e12


def graphed(fn, iters):
    """One graph of `iters` calls of fn, captured after a warm-up on a side stream; returns its replay."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(iters):
            fn()
    return graph.replay


def measure(runs, rounds, iters):
    for fn in runs.values():  # warm-up: every kernel loaded, the dense layout's kept form built
        fn()
        fn()
    torch.cuda.synchronize()
    replays = {n: graphed(fn, iters) for n, fn in runs.items()}
    for r in replays.values():
        r()
    torch.cuda.synchronize()
    eager, device = {n: [] for n in runs}, {n: [] for n in runs}
    for _ in range(rounds):
        for n, fn in runs.items():
            eager[n].append(timed(fn, iters))
            device[n].append(timed(replays[n], 1) / iters)
    stat = lambda xs: (statistics.median(xs), min(xs), max(xs))  # noqa: E731
    return {n: (stat(eager[n]), stat(device[n])) for n in runs}


def main():
    ints = lambda s: [int(x) for x in s.split(",") if x]  # noqa: E731
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--lens", type=ints, default=[32768, 131072])
    ap.add_argument("--ratio", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--log", default=str(REPO / "profiles" / "r32_block_attention_select.log"))
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    import matmuls
    dev = torch.device("cuda:0")
    B = args.batch
    lines = [f"# tools/bench_block_attention_select.py --batch {B} --lens {args.lens} --ratio {args.ratio} --rounds {args.rounds} "
             f"--iters {args.iters}: ms per call, median over the rounds [min … max], eager | one graph of {args.iters} calls; "
             f"bfloat16, D = {D}, Hkv = {HKV}, G = {G}, T = 1, sink = 1, local = 2; bytes over 8 TB/s; "
             f"{torch.cuda.get_device_name(0)}"]

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    for klen in args.lens:
        nb = klen // BLOCK
        K = max(3, nb // args.ratio)
        g = torch.Generator(device=dev).manual_seed(32)
        q = torch.randn(B, HKV * G, 1, D, device=dev, generator=g).bfloat16()
        k = torch.randn(B, HKV, klen, D, device=dev, dtype=torch.bfloat16, generator=g)
        v = torch.randn(B, HKV, klen, D, device=dev, dtype=torch.bfloat16, generator=g)
        lens = torch.full((B,), klen, device=dev, dtype=torch.int32)
        bounds = matmuls.key_block_bounds(k, lens)
        ids, counts = matmuls.select_key_blocks(q, bounds, lens, K, sink=1, local=2)
        dense = square_layout(torch.ones(nb, dtype=torch.bool, device=dev), nb)

        def step():
            matmuls.key_block_bounds(k, lens, bounds, last=1)
            i, c = matmuls.select_key_blocks(q, bounds, lens, K, sink=1, local=2)
            return matmuls.block_sparse_attention_decode_selected(q, k, v, i, c, lens)

        runs = {"bounds last=1": lambda: matmuls.key_block_bounds(k, lens, bounds, last=1),
                "select": lambda: matmuls.select_key_blocks(q, bounds, lens, K, sink=1, local=2),
                "decode selected": lambda: matmuls.block_sparse_attention_decode_selected(q, k, v, ids, counts, lens),
                "step (bounds + select + decode)": step,
                "dense decode": lambda: matmuls.block_sparse_attention_decode(q, k, v, dense, lens)}
        res = measure(runs, args.rounds, args.iters)
        bounds_bytes, kept_bytes = B * HKV * nb * 4 * D, B * HKV * K * 256 * D
        floor_ms = (bounds_bytes + kept_bytes) / HBM_BYTES_PER_S * 1e3
        dense_ms = B * HKV * nb * 256 * D / HBM_BYTES_PER_S * 1e3
        emit(f"\nB = {B}, k_len = {klen}: K = {K} of {nb} blocks; bounds {bounds_bytes / 2 ** 20:.1f} MiB + kept k / v "
             f"{kept_bytes / 2 ** 20:.1f} MiB = {floor_ms:.4f} ms at 8 TB/s (the dense cache: {dense_ms:.4f} ms)")
        for n, ((em, el, eh), (dm, dl, dh)) in res.items():
            emit(f"  {n:34s} eager {em:8.4f}  [{el:.4f} … {eh:.4f}]   graph {dm:8.4f}  [{dl:.4f} … {dh:.4f}]")
        parts = sum(res[n][1][0] for n in ("bounds last=1", "select", "decode selected"))
        emit(f"  the three parts' graph medians sum to {parts:.4f} ms; step / dense decode = "
             f"{res['step (bounds + select + decode)'][1][0] / res['dense decode'][1][0]:.2f} (graph), "
             f"{res['step (bounds + select + decode)'][0][0] / res['dense decode'][0][0]:.2f} (eager)")
        del q, k, v, bounds
        torch.cuda.empty_cache()
    path = Path(args.log)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
