#!/usr/bin/env python3
"""Key-block selection over an FP8 KV cache, measured.

    python tools/bench_block_attention_select_fp8.py [--batch 8] [--lens 4096,16384,65536,131072] [--ratio 16] [--rounds 5]
                                                     [--iters 10] [--log profiles/r36_block_attention_select_fp8.log] [--append]

§3.29's shapes: bfloat16 q, D = 128, Hkv = 8 k / v heads, G = 4 query heads each, T = 1 new token at pos = k_len − 1 of a full
cache (Smax = k_len), K = Smax / 64 / ratio, sink = 1, local = 2.  The cache is kv_to_fp8 of normal keys and values with its
per-head scales as device tensors; the 2-byte yardstick runs on the same bytes widened to bfloat16.  All contestants of a row
are timed in the SAME interleaved rounds (tools/bench_block_attention_select.py's measure: the median over the rounds of the
mean of `iters` calls, min … max beside it, eager and as one captured graph of `iters` calls):
  bounds fp8 / bf16   key_block_bounds_fp8(k8, lens, bounds, last=1) / key_block_bounds(kw, lens, bounds, last=1);
  select              select_key_blocks(q, bounds, lens, K, sink=1, local=2) on the fp8 cache's bounds;
  walk fp8 / bf16     block_sparse_attention_decode_selected_fp8 / block_sparse_attention_decode_selected on the lists;
  step fp8 / bf16     bounds, select and walk in sequence: the whole decode step of this tree over either cache;
  dense fp8           block_sparse_attention_decode_fp8 with the dense causal layout: what the fp8 step replaces.
Two expectations are stated, not enforced: walk fp8 / walk bf16 inside 0.68 … 1.11 (§3.20's range of the layout forms), and
the fp8 bounds refresh not slower than the bf16 one beyond the run's own spread.
"""
import argparse
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "matrix-multiplication_amd"))
sys.path.insert(0, str(REPO / "tools"))

from bench_block_attention_decode import square_layout  # noqa: E402
from bench_block_attention_select import BLOCK, D, G, HKV, measure  # noqa: E402


def main():
    ints = lambda s: [int(x) for x in s.split(",") if x]  # noqa: E731
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--lens", type=ints, default=[4096, 16384, 65536, 131072])
    ap.add_argument("--ratio", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--log", default=str(REPO / "profiles" / "r36_block_attention_select_fp8.log"))
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    import matmuls as m
    dev = torch.device("cuda:0")
    B = args.batch
    lines = [f"# tools/bench_block_attention_select_fp8.py --batch {B} --lens {args.lens} --ratio {args.ratio} --rounds {args.rounds} "
             f"--iters {args.iters}: ms per call, median over the rounds [min … max], eager | one graph of {args.iters} calls; "
             f"bfloat16 q, float8_e4m3fn cache with per-head scales, D = {D}, Hkv = {HKV}, G = {G}, T = 1, sink = 1, local = 2; "
             f"{torch.cuda.get_device_name(0)}"]

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    for klen in args.lens:
        nb = klen // BLOCK
        K = max(3, nb // args.ratio)
        g = torch.Generator(device=dev).manual_seed(36)
        q = torch.randn(B, HKV * G, 1, D, device=dev, generator=g).bfloat16()
        caches = []
        for _ in range(2):
            x = torch.randn(B, HKV, klen, D, device=dev, dtype=torch.bfloat16, generator=g)
            caches.append(m.kv_to_fp8(x))
            del x
        (k8, ks), (v8, vs) = caches
        kw, vw = k8.to(torch.bfloat16), v8.to(torch.bfloat16)      # the 2-byte yardstick's cache: the same values, unscaled
        lens = torch.full((B,), klen, device=dev, dtype=torch.int32)
        bounds8 = m.key_block_bounds_fp8(k8, lens, dtype=torch.bfloat16)
        bounds2 = m.key_block_bounds(kw, lens)
        assert torch.equal(bounds8.view(torch.int16), bounds2.view(torch.int16)), "the bounds of the widened cache"
        ids, counts = m.select_key_blocks(q, bounds8, lens, K, sink=1, local=2)
        dense = square_layout(torch.ones(nb, dtype=torch.bool, device=dev), nb)

        def step_fp8():
            m.key_block_bounds_fp8(k8, lens, bounds8, last=1)
            i, c = m.select_key_blocks(q, bounds8, lens, K, sink=1, local=2)
            return m.block_sparse_attention_decode_selected_fp8(q, k8, v8, i, c, lens, k_scale=ks, v_scale=vs)

        def step_bf16():
            m.key_block_bounds(kw, lens, bounds2, last=1)
            i, c = m.select_key_blocks(q, bounds2, lens, K, sink=1, local=2)
            return m.block_sparse_attention_decode_selected(q, kw, vw, i, c, lens)

        runs = {"bounds fp8 last=1": lambda: m.key_block_bounds_fp8(k8, lens, bounds8, last=1),
                "bounds bf16 last=1": lambda: m.key_block_bounds(kw, lens, bounds2, last=1),
                "select": lambda: m.select_key_blocks(q, bounds8, lens, K, sink=1, local=2),
                "walk fp8": lambda: m.block_sparse_attention_decode_selected_fp8(q, k8, v8, ids, counts, lens, k_scale=ks, v_scale=vs),
                "walk bf16": lambda: m.block_sparse_attention_decode_selected(q, kw, vw, ids, counts, lens),
                "step fp8": step_fp8,
                "step bf16": step_bf16,
                "dense fp8": lambda: m.block_sparse_attention_decode_fp8(q, k8, v8, dense, lens, k_scale=ks, v_scale=vs)}
        res = measure(runs, args.rounds, args.iters)
        emit(f"\nB = {B}, k_len = {klen}: K = {K} of {nb} blocks; kept k / v {B * HKV * K * 128 * D / 2 ** 20:.1f} MiB fp8, "
             f"{B * HKV * K * 256 * D / 2 ** 20:.1f} MiB bf16; the dense fp8 cache {B * HKV * nb * 128 * D / 2 ** 20:.1f} MiB")
        for n, ((em, el, eh), (dm, dl, dh)) in res.items():
            emit(f"  {n:20s} eager {em:8.4f}  [{el:.4f} … {eh:.4f}]   graph {dm:8.4f}  [{dl:.4f} … {dh:.4f}]")
        gm = {n: r[1][0] for n, r in res.items()}
        (_, b8lo, b8hi), (_, b2lo, b2hi) = res["bounds fp8 last=1"][1], res["bounds bf16 last=1"][1]
        emit(f"  graph medians: walk fp8 / walk bf16 = {gm['walk fp8'] / gm['walk bf16']:.2f} (expected inside 0.68 … 1.11); "
             f"bounds fp8 / bounds bf16 = {gm['bounds fp8 last=1'] / gm['bounds bf16 last=1']:.2f} (spreads {b8lo:.4f} … {b8hi:.4f} and "
             f"{b2lo:.4f} … {b2hi:.4f}); step fp8 / step bf16 = {gm['step fp8'] / gm['step bf16']:.2f}; step fp8 / dense fp8 = "
             f"{gm['step fp8'] / gm['dense fp8']:.2f}")
        del q, k8, v8, kw, vw, bounds8, bounds2, caches
        torch.cuda.empty_cache()
    path = Path(args.log)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
