#!/usr/bin/env python3
"""window= and sink= of the decode and prefill calls beside the calls without them, measured.

    python tools/bench_block_attention_window.py [--batches 1,8] [--lens 4096,32768,131072] [--window 4096] [--sinks 0,4]
                                                 [--pages 0,16] [--prefill 512,2048] [--rounds 5] [--iters 10]
                                                 [--log profiles/r39_block_attention_window.log] [--append]

The shapes of tools/bench_block_attention_decode.py: bfloat16, D = 128, Hq = 32 query heads over Hkv = 8 k / v heads, block 64,
chunk=None, a full cache (Smax = k_len); the cache contiguous (page 0) or a pool of shuffled pages.  Per row, in the SAME
interleaved rounds:
  decode, T = 1   the windowed call on matmuls.sliding_window_layout(Smax, W, S) beside the PLAIN call on that layout (which reads
                  the same blocks and cuts nothing), and the windowed call on the fully kept causal layout — what the block skip
                  saves of a dense walk, and what its empty chunks cost;
  prefill, T      the windowed call beside the plain call on the banded layout.
Each figure is the median over the rounds of the mean of `iters` back-to-back calls between two events, with the spread
(min … max) beside it.  Expectation, not a test: windowed / plain within the plain call's own spread plus 5 %.  Checked once per
row: the window 2³¹ − 1 gives the bits of the plain call.  The tree calls against their parents are
tools/bench_block_attention_decode_tree.py's rows; run it with --log on the same file and --append.
"""
import argparse
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "matrix-multiplication_amd"))
sys.path.insert(0, str(REPO / "tools"))

from bench_block_attention_decode import BLOCK, D, HKV, HQ, last_row, measure, square_layout  # noqa: E402
from bench_block_attention_decode_paged import scattered  # noqa: E402


def main():
    ints = lambda s: [int(x) for x in s.split(",") if x]  # noqa: E731
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=ints, default=[1, 8])
    ap.add_argument("--lens", type=ints, default=[4096, 32768, 131072])
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--sinks", type=ints, default=[0, 4])
    ap.add_argument("--pages", type=ints, default=[0, 16])
    ap.add_argument("--prefill", type=ints, default=[512, 2048])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--log", default=str(REPO / "profiles" / "r39_block_attention_window.log"))
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    import matmuls
    dev = torch.device("cuda:0")
    W = args.window
    lines = [f"# tools/bench_block_attention_window.py --batches {args.batches} --lens {args.lens} --window {W} --sinks {args.sinks} --pages "
             f"{args.pages} --prefill {args.prefill} --rounds {args.rounds} --iters {args.iters}: ms, median over the rounds [min … max]; "
             f"bfloat16, D = {D}, Hq = {HQ}, Hkv = {HKV}, block {BLOCK}, chunk=None; page 0: the contiguous cache, else a pool of shuffled "
             f"pages; banded: sliding_window_layout(Smax, W, S); ratio: to the plain call of the same rounds; "
             f"{torch.cuda.get_device_name(0)}"]

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    ratios, misses = {"decode": [], "prefill": []}, []

    def row(kind, where, name, res, plain, windowed):
        (pm, plo, phi), (wm, wlo, whi) = res[plain], res[windowed]
        allowed = phi / pm + 0.05
        verdict = "within" if wm / pm <= allowed else "ABOVE"
        emit(f"  {name:26s} plain {pm:9.4f} [{plo:.4f} … {phi:.4f}]  windowed {wm:9.4f} [{wlo:.4f} … {whi:.4f}]  windowed / plain "
             f"{wm / pm:5.3f} ({verdict} the plain call's spread + 5 % = {allowed:5.3f})")
        ratios[kind].append(wm / pm)
        if verdict == "ABOVE":
            misses.append(f"{where}, {name}: {wm / pm:.3f}")

    for klen in args.lens:
        nb = klen // BLOCK
        for B in args.batches:
            g = torch.Generator(device=dev).manual_seed(39)
            k = torch.randn(B, HKV, klen, D, device=dev, dtype=torch.bfloat16, generator=g)
            v = torch.randn(B, HKV, klen, D, device=dev, dtype=torch.bfloat16, generator=g)
            lens = torch.full((B,), klen, device=dev, dtype=torch.int32)
            full = square_layout(last_row("fully kept", nb, dev, 0), nb)  # (decode reads the row of pos alone)
            for page in args.pages:
                if page:
                    Wp = klen // page
                    table = torch.randperm(B * Wp, device=dev, generator=g).reshape(B, Wp).to(torch.int32)
                    cache, name = (scattered(k, page, table), scattered(v, page, table), table), f"page {page}"
                    decode, prefill = matmuls.block_sparse_attention_decode_paged, matmuls.block_sparse_attention_prefill_paged
                else:
                    cache, name = (k, v), "contiguous"
                    decode, prefill = matmuls.block_sparse_attention_decode, matmuls.block_sparse_attention_prefill
                for S in args.sinks:
                    where = f"B = {B}, k_len = {klen}, {name}, W = {W}, S = {S}"
                    emit(f"\n{where}")
                    banded = matmuls.sliding_window_layout(klen, W, S, device=dev).to_sparse_csr()
                    q = torch.randn(B, HQ, 1, D, device=dev, generator=g).bfloat16()
                    runs = {"plain": lambda: decode(q, *cache, banded, lens),
                            "windowed": lambda: decode(q, *cache, banded, lens, window=W, sink=S),
                            "windowed, dense": lambda: decode(q, *cache, full, lens, window=W, sink=S)}
                    want = runs["plain"]()
                    got = decode(q, *cache, banded, lens, window=2 ** 31 - 1)
                    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), "the widest window differs from the plain call"
                    res = measure(runs, args.rounds, args.iters)
                    row("decode", where, "decode T = 1, banded", res, "plain", "windowed")
                    (bm, _, _), (dm, dlo, dhi) = res["windowed"], res["windowed, dense"]
                    emit(f"  {'decode T = 1, dense layout':26s} windowed {dm:9.4f} [{dlo:.4f} … {dhi:.4f}]  dense / banded {dm / bm:5.3f}")
                    for T in args.prefill:
                        if T > klen:
                            continue
                        q = torch.randn(B, HQ, T, D, device=dev, generator=g).bfloat16()
                        runs = {"plain": lambda: prefill(q, *cache, banded, lens),
                                "windowed": lambda: prefill(q, *cache, banded, lens, window=W, sink=S)}
                        want = runs["plain"]()
                        got = prefill(q, *cache, banded, lens, window=2 ** 31 - 1)
                        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), "the widest window differs from the plain call"
                        row("prefill", where, f"prefill T = {T}, banded", measure(runs, args.rounds, args.iters), "plain", "windowed")
                    del q, banded
                del cache
            del k, v
            torch.cuda.empty_cache()
    for kind, xs in ratios.items():
        if xs:
            emit(f"\n# {kind}: windowed / plain over the {len(xs)} rows: {min(xs):.3f} … {max(xs):.3f}")
    emit(f"# above the plain call's spread + 5 % in {len(misses)} rows" + "".join("\n#   " + m for m in misses))
    path = Path(args.log)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
