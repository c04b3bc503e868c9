#!/usr/bin/env python3
"""The speculative step's three calls beside their parents, measured.

    python tools/bench_block_attention_decode_tree.py [--batches 1,8] [--lens 4096,32768,131072] [--tokens 8,64] [--pages 0,16]
                                                      [--rounds 5] [--iters 10]
                                                      [--log profiles/r38_block_attention_decode_tree.log] [--append]

The shapes of tools/bench_block_attention_decode.py: bfloat16, D = 128, Hq = 32 query heads over Hkv = 8 k / v heads, block 64,
chunk=None, the T newest tokens of a full cache (Smax = k_len, a multiple of 64, so the window of T ≤ 64 drafted slots lies in the
last block and all T tokens read the last layout row); layouts: a window of 16 blocks + 1 global block, and fully kept; the cache
contiguous (page 0) or a pool of shuffled pages.  Per row the decode call with tree_mask= of a random tree stands beside the call
without a mask, rope_kv_cache_append(positions=…) beside the call without positions, and kv_cache_compact beside kv_cache_append of
the same T rows (the other call that touches T rows of k and v once) — all in the SAME interleaved rounds; each figure is the
median over the rounds of the mean of `iters` back-to-back calls between two events, with the spread (min … max) beside it.
Expectation, not a test: tree / plain within the plain call's own spread plus 5 %.  Checked once per row: the tree call with the
causal words gives the bits of the plain call.
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
    ap.add_argument("--tokens", type=ints, default=[8, 64])
    ap.add_argument("--pages", type=ints, default=[0, 16])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--log", default=str(REPO / "profiles" / "r38_block_attention_decode_tree.log"))
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    import matmuls
    dev = torch.device("cuda:0")
    lines = [f"# tools/bench_block_attention_decode_tree.py --batches {args.batches} --lens {args.lens} --tokens {args.tokens} --pages "
             f"{args.pages} --rounds {args.rounds} --iters {args.iters}: ms, median over the rounds [min … max]; bfloat16, D = {D}, "
             f"Hq = {HQ}, Hkv = {HKV}, block {BLOCK}, chunk=None; page 0: the contiguous cache, else a pool of shuffled pages; ratio: to "
             f"the parent call of the same rounds; {torch.cuda.get_device_name(0)}"]

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    ratios, misses = [], []
    for klen in args.lens:
        nb = klen // BLOCK
        for B in args.batches:
            for T in args.tokens:
                g = torch.Generator(device=dev).manual_seed(38)
                q = torch.randn(B, HQ, T, D, device=dev, generator=g).bfloat16()
                kn, vn = (torch.randn(B, HKV, T, D, device=dev, generator=g).bfloat16() for _ in range(2))
                k = torch.randn(B, HKV, klen, D, device=dev, dtype=torch.bfloat16, generator=g)
                v = torch.randn(B, HKV, klen, D, device=dev, dtype=torch.bfloat16, generator=g)
                cos, sin = (torch.rand(klen, D // 2, device=dev, generator=g) for _ in range(2))
                lens = torch.full((B,), klen, device=dev, dtype=torch.int32)
                parents = torch.stack([torch.tensor([int(torch.randint(-1, t, (1,), generator=torch.Generator().manual_seed(100 * b + t)))
                                                     if t else -1 for t in range(T)]) for b in range(B)]).to(dev)
                mask, depth = matmuls.tree_attention_mask(parents)
                causal = matmuls.tree_attention_mask(torch.arange(-1, T - 1, device=dev))[0]
                positions = (lens - T)[:, None] + depth
                accept = torch.arange(T, device=dev, dtype=torch.int32).flip(0).repeat(B, 1).contiguous()  # every row moves
                counts = torch.full((B,), T, device=dev, dtype=torch.int32)
                for page in args.pages:
                    if page:
                        W = klen // page
                        table = torch.randperm(B * W, device=dev, generator=g).reshape(B, W).to(torch.int32)
                        kc, vc = scattered(k, page, table), scattered(v, page, table)
                        cache, name = (kc, vc, table), f"page {page}"
                        decode, rope = matmuls.block_sparse_attention_decode_paged, matmuls.rope_kv_cache_append_paged
                        append, compact = matmuls.kv_cache_append_paged, matmuls.kv_cache_compact_paged
                    else:
                        cache, name = (k, v), "contiguous"
                        decode, rope = matmuls.block_sparse_attention_decode, matmuls.rope_kv_cache_append
                        append, compact = matmuls.kv_cache_append, matmuls.kv_cache_compact
                    emit(f"\nB = {B}, T = {T}, k_len = {klen}, {name}")
                    for lname in ("window 16 + global", "fully kept"):
                        layout = square_layout(last_row(lname, nb, dev, 21), nb)
                        runs = {"decode": lambda: decode(q, *cache, layout, lens),
                                "decode, tree_mask": lambda: decode(q, *cache, layout, lens, tree_mask=mask)}
                        want = runs["decode"]()
                        got = decode(q, *cache, layout, lens, tree_mask=causal)
                        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), "the causal words differ from the plain call"
                        res = measure(runs, args.rounds, args.iters)
                        (pm, plo, phi), (tm, tlo, thi) = res["decode"], res["decode, tree_mask"]
                        allowed = phi / pm + 0.05
                        verdict = "within" if tm / pm <= allowed else "ABOVE"
                        emit(f"  {lname:20s} plain {pm:9.4f} [{plo:.4f} … {phi:.4f}]  tree {tm:9.4f} [{tlo:.4f} … {thi:.4f}]  tree / plain "
                             f"{tm / pm:5.3f} ({verdict} the plain call's spread + 5 % = {allowed:5.3f})")
                        ratios.append(tm / pm)
                        if verdict == "ABOVE":
                            misses.append(f"B = {B}, T = {T}, k_len = {klen}, {name}, {lname}: {tm / pm:.3f}")
                    writes = {"rope": lambda: rope(q, kn, vn, cos, sin, *cache, lens),
                              "rope, positions": lambda: rope(q, kn, vn, cos, sin, *cache, lens, positions=positions),
                              "append": lambda: append(kn, vn, *cache, lens),
                              "compact": lambda: compact(*cache, lens, accept, counts, T)}
                    res = measure(writes, args.rounds, args.iters)
                    for parent, child in (("rope", "rope, positions"), ("append", "compact")):
                        (pm, plo, phi), (cm, clo, chi) = res[parent], res[child]
                        emit(f"  {parent:20s} {pm:9.4f} [{plo:.4f} … {phi:.4f}]  {child} {cm:9.4f} [{clo:.4f} … {chi:.4f}]  x{cm / pm:5.3f}")
                del q, k, v, cache
                torch.cuda.empty_cache()
    emit(f"\n# tree / plain over the {len(ratios)} rows: {min(ratios):.3f} … {max(ratios):.3f}; above the plain call's spread + 5 % in "
         f"{len(misses)} rows" + "".join("\n#   " + m for m in misses))
    path = Path(args.log)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
