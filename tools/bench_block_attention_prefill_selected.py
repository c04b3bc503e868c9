#!/usr/bin/env python3
"""Prefill over selected key blocks, measured: the tile-level selection on the matrix cores and the prefill
walk over its lists, for a chunk of a prompt behind a long cached prefix.

    python tools/bench_block_attention_prefill_selected.py [--batches 1,4] [--chunks 512,2048] [--lens 32768,131072] [--ratio 16]
                                                           [--rounds 5] [--iters 3]
                                                           [--log profiles/r37_block_attention_prefill_selected.log] [--append]

bfloat16, D = 128, Hq = 32, Hkv = 8 (G = 4); the chunk is the last T tokens of a full cache (Smax = k_len), K = Smax / 64 / ratio,
sink = 1, local = 2.  Contestants of a row are timed in interleaved rounds, each figure the median over the rounds of the mean
of `iters` calls, with the spread (min … max) beside it — once as `iters` back-to-back eager calls between two events (the
Python front end's checks included) and once as ONE captured graph of `iters` calls replayed between two events (the device's
share):
  bounds last=T     matmuls.key_block_bounds(k, lens, bounds, last=T): the refresh after the chunk's append;
  select tiles      matmuls.select_key_blocks_tiles(q, bounds, lens, K, sink=1, local=2);
  prefill selected  matmuls.block_sparse_attention_prefill_selected on the lists of the select call;
  step              the three in sequence;
  dense prefill     matmuls.block_sparse_attention_prefill with the dense causal layout — row r lists the blocks 0 … r, so
                    every tile of the chunk walks its whole causal prefix —: what the step replaces;
  select per token  matmuls.select_key_blocks on the same q: the yardstick for the select kernel.
Per row: the select kernel's MFMA rate — B · Hq · 64 · (tiles with a token) · candidates · 4 · D flop over its graph time, the
work of whole 64-row tiles — and the walk's share of the kept k / v bytes' own time, B · Hkv · tiles · K · 256 · D bytes over
8 TB/s, the HBM rate of §3.18 (the G heads of a group read the same bytes: counted once).
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
from bench_block_attention_select import graphed  # noqa: E402

D, BLOCK, HKV, G = 128, 64, 8, 4
HBM_BYTES_PER_S = 8e12


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
    ap.add_argument("--batches", type=ints, default=[1, 4])
    ap.add_argument("--chunks", type=ints, default=[512, 2048])
    ap.add_argument("--lens", type=ints, default=[32768, 131072])
    ap.add_argument("--ratio", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--log", default=str(REPO / "profiles" / "r37_block_attention_prefill_selected.log"))
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    import matmuls
    dev = torch.device("cuda:0")
    lines = [f"# tools/bench_block_attention_prefill_selected.py --batches {args.batches} --chunks {args.chunks} --lens {args.lens} "
             f"--ratio {args.ratio} --rounds {args.rounds} --iters {args.iters}: ms per call, median over the rounds [min … max], "
             f"eager | one graph of {args.iters} calls; bfloat16, D = {D}, Hq = {HKV * G}, Hkv = {HKV}, sink = 1, local = 2; "
             f"bytes over 8 TB/s; {torch.cuda.get_device_name(0)}"]

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    for klen in args.lens:
        nb = klen // BLOCK
        K = max(3, nb // args.ratio)
        dense = torch.tril(torch.ones(nb, nb, device=dev)).to_sparse_csr()  # row r: the blocks 0 … r
        for B in args.batches:
            g = torch.Generator(device=dev).manual_seed(37)
            k = torch.randn(B, HKV, klen, D, device=dev, dtype=torch.bfloat16, generator=g)
            v = torch.randn(B, HKV, klen, D, device=dev, dtype=torch.bfloat16, generator=g)
            lens = torch.full((B,), klen, device=dev, dtype=torch.int32)
            bounds = matmuls.key_block_bounds(k, lens)
            for T in args.chunks:
                q = torch.randn(B, HKV * G, T, D, device=dev, generator=g).bfloat16()
                ids, counts = matmuls.select_key_blocks_tiles(q, bounds, lens, K, sink=1, local=2)

                def step():
                    matmuls.key_block_bounds(k, lens, bounds, last=T)
                    i, c = matmuls.select_key_blocks_tiles(q, bounds, lens, K, sink=1, local=2)
                    return matmuls.block_sparse_attention_prefill_selected(q, k, v, i, c, lens)

                runs = {"bounds last=T": lambda: matmuls.key_block_bounds(k, lens, bounds, last=T),
                        "select tiles": lambda: matmuls.select_key_blocks_tiles(q, bounds, lens, K, sink=1, local=2),
                        "prefill selected": lambda: matmuls.block_sparse_attention_prefill_selected(q, k, v, ids, counts, lens),
                        "step (bounds + select + prefill)": step,
                        "dense prefill": lambda: matmuls.block_sparse_attention_prefill(q, k, v, dense, lens),
                        "select per token": lambda: matmuls.select_key_blocks(q, bounds, lens, K, sink=1, local=2)}
                res = measure(runs, args.rounds, args.iters)
                first = (klen - T) // BLOCK
                rows = [r for r in range(first, first + -(-T // BLOCK) + 1) if max(klen - T, r * BLOCK) < min(klen, r * BLOCK + BLOCK)]
                flop = B * HKV * G * 64 * sum(r + 1 for r in rows) * 4 * D
                kept_bytes = B * HKV * sum(min(K, r + 1) for r in rows) * 256 * D
                floor_ms = kept_bytes / HBM_BYTES_PER_S * 1e3
                emit(f"\nB = {B}, T = {T}, k_len = {klen}: {len(rows)} tiles, K = {K} of {nb} blocks; kept k / v "
                     f"{kept_bytes / 2 ** 20:.1f} MiB = {floor_ms:.4f} ms at 8 TB/s")
                for n, ((em, el, eh), (dm, dl, dh)) in res.items():
                    emit(f"  {n:34s} eager {em:8.4f}  [{el:.4f} … {eh:.4f}]   graph {dm:8.4f}  [{dl:.4f} … {dh:.4f}]")
                sel, walk = res["select tiles"][1][0], res["prefill selected"][1][0]
                stepg, denseg = res["step (bounds + select + prefill)"], res["dense prefill"]
                emit(f"  select tiles: {flop / (sel * 1e-3) / 1e12:.1f} TFLOP/s on the matrix cores, {sel / walk:.2f} of the walk, "
                     f"{sel / res['select per token'][1][0]:.3f} of the per-token select; the walk: the kept bytes' time is "
                     f"{floor_ms / walk:.2f} of it; step / dense prefill = {stepg[1][0] / denseg[1][0]:.3f} (graph), "
                     f"{stepg[0][0] / denseg[0][0]:.3f} (eager)")
                del q, ids, counts
            del k, v, bounds
            torch.cuda.empty_cache()
    path = Path(args.log)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
