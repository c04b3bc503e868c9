#!/usr/bin/env python3
"""Split key walks of block-sparse prefill attention, measured.

    python tools/bench_block_attention_prefill_split.py [--rounds 3] [--iters 3] [--limit 240]
                                                        [--log profiles/r30_block_attention_prefill_split.log] [--append]
    python tools/bench_block_attention_prefill_split.py --case chunk:1:512:131072 --log …     (one case, in this process)

The protocol of tools/bench_block_attention_prefill.py: bfloat16, D = 128, Hq = 32 query heads over Hkv = 8 k / v heads, block 64,
the contiguous cache; the three layouts of that tool (a window of 16 blocks + 1 global block, random 10 % of the lower
triangle + the diagonal, fully kept).  Cases:
  chunk:B:T:K   a chunk of T tokens behind a prefix, k_len = K, batch B: block_sparse_attention_prefill with split ∈ SPLITS
                and the UNSPLIT call (split=None, the parent's code path) in the SAME interleaved rounds; at T = 64 also
                block_sparse_attention_decode (G = 4 is within its bound), the call the unsplit docstring used to point to.
  whole:K       a whole prompt, T = k_len = K, B = 1, fully kept, unsplit: the whole-prompt rate of this run.
Each figure is the median over the rounds of the mean of `iters` back-to-back calls between two events, with [min … max];
per row: the best split, best / unsplit, the matrix-core rate over the blocks computed (4 · 64 · 64 · D flop per block pair and
query head) and the workspace of every split.  Before a row is timed every split call — and the unsplit one — is checked
under the project's rule on the last tile of item 0, query heads 0 and Hq − 1: e_dev ≤ 8 · e_ref against dense masked
attention in float64, e_ref the error of the float32 evaluation narrowed to bfloat16; a row that misses ends the case.
Without --case every case runs as a fresh child process under its own time limit; the first child that fails or runs out of
time ends the run.
"""
import argparse
import statistics
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "matrix-multiplication_amd"))
sys.path.insert(0, str(REPO / "tools"))

D, BLOCK, HQ, HKV = 128, 64, 32, 8
SPLITS = (16, 32, 64, 128, 256, 512)
FACTOR = 8.0
CASES = ["whole:16384"] + [f"chunk:{B}:{T}:{K}" for B in (1, 4) for T in (64, 512, 2048) for K in (8192, 32768, 131072)]


def workspace_bytes(B, T, K, split):
    parts = -(-(K // BLOCK) // split)
    return 0 if parts <= 1 else B * HQ * (-(-T // BLOCK) + 1) * parts * BLOCK * (D + 2) * 4


def rule_check(torch, q, k, v, mask, T, K, outs):
    """{name: worst e_dev / e_ref} over the last tile of item 0, query heads 0 and Hq − 1; e_ref of the float32 evaluation."""
    n = min(T, BLOCK)
    pos = torch.arange(K - n, K, device=q.device)
    keys = torch.arange(K, device=q.device)
    seen = mask[pos // BLOCK][:, keys // BLOCK] & (keys[None, :] <= pos[:, None])
    worst = {name: 0.0 for name in outs}
    for h in (0, HQ - 1):
        kk, vv, qq = k[0, h // (HQ // HKV)], v[0, h // (HQ // HKV)], q[0, h, T - n:]
        res = {}
        for dt in (torch.float64, torch.float32):
            s = (qq.to(dt) @ kk.to(dt).T / D ** 0.5).masked_fill(~seen, -float("inf"))
            res[dt] = torch.softmax(s, -1) @ vv.to(dt)
        ref = res[torch.float64]
        scale = float(ref.abs().max())
        e_ref = float((res[torch.float32].bfloat16().double() - ref).abs().max()) / scale
        for name, out in outs.items():
            e_dev = float((out[0, h, T - n:].double() - ref).abs().max()) / scale
            worst[name] = max(worst[name], e_dev / e_ref)
    return worst


def run_case(case, rounds, iters, emit):
    import torch
    import matmuls
    from bench_block_attention import timed
    from bench_block_attention_prefill import block_mask
    kind, *nums = case.split(":")
    B, T, K = (1, int(nums[0]), int(nums[0])) if kind == "whole" else map(int, nums)
    dev = torch.device("cuda:0")
    emit(f"\n# {case} on {torch.cuda.get_device_name(0)}")
    nb = K // BLOCK
    g = torch.Generator(device=dev).manual_seed(30)
    q = torch.randn(B, HQ, T, D, device=dev, generator=g).bfloat16()
    k = torch.randn(B, HKV, K, D, device=dev, dtype=torch.bfloat16, generator=g)
    v = torch.randn(B, HKV, K, D, device=dev, dtype=torch.bfloat16, generator=g)
    lens = torch.full((B,), K, device=dev, dtype=torch.int32)
    for name in ("fully kept",) if kind == "whole" else ("window 16 + global", "random 10 %", "fully kept"):
        mask = block_mask(name, nb, dev, 27)
        layout = mask.float().to_sparse_csr()
        pairs = int(mask[(K - T) // BLOCK:].sum()) * B * HQ
        runs = {"unsplit": lambda: matmuls.block_sparse_attention_prefill(q, k, v, layout, lens)}
        if kind == "chunk":
            for s in SPLITS:
                if -(-nb // s) > 1:  # (one part is the unsplit launch)
                    runs[f"split {s}"] = lambda s=s: matmuls.block_sparse_attention_prefill(q, k, v, layout, lens, split=s)
            if T == 64:
                runs["decode call"] = lambda: matmuls.block_sparse_attention_decode(q, k, v, layout, lens)
        ratios = rule_check(torch, q, k, v, mask, T, K, {n: fn() for n, fn in runs.items()})
        emit(f"\n{case}, B = {B}, T = {T}, k_len = {K}, {name}: {pairs // (B * HQ)} block pairs per head; e_dev / e_ref: "
             + ", ".join(f"{n} {r:.2f}" for n, r in ratios.items()))
        bad = [n for n, r in ratios.items() if r > FACTOR]
        if bad:
            emit(f"  {bad} MISS the rule e_dev <= {FACTOR:g} · e_ref: the case ends here")
            return 1
        torch.cuda.synchronize()
        samples = {n: [] for n in runs}
        for _ in range(rounds):
            for n, fn in runs.items():
                samples[n].append(timed(fn, iters))
        res = {n: (statistics.median(xs), min(xs), max(xs)) for n, xs in samples.items()}
        base = res["unsplit"][0]
        for n, (med, lo, hi) in res.items():
            ws = workspace_bytes(B, T, K, int(n.split()[1])) if n.startswith("split") else 0
            emit(f"  {n:12s} {med:10.4f}  [{lo:.4f} … {hi:.4f}]  x{med / base:6.3f} of unsplit  "
                 f"{pairs * 4 * BLOCK * BLOCK * D / (med * 1e-3) / 1e12:7.1f} TFLOP/s  workspace {ws / 2 ** 20:9.1f} MiB")
        splits = {n: r for n, r in res.items() if n.startswith("split")}
        if splits:
            best = min(splits, key=lambda n: splits[n][0])
            emit(f"  best: {best}, {splits[best][0] / base:.3f} of unsplit (unsplit spread {res['unsplit'][1] / base:.3f} … "
                 f"{res['unsplit'][2] / base:.3f}), {pairs * 4 * BLOCK * BLOCK * D / (splits[best][0] * 1e-3) / 1e12:.1f} TFLOP/s")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default=None)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--log", default=str(REPO / "profiles" / "r30_block_attention_prefill_split.log"))
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    path = Path(args.log)
    path.parent.mkdir(parents=True, exist_ok=True)
    if args.case is None:  # (this process never opens the device: every case is a child of its own)
        with open(path, "a" if args.append else "w") as f:
            f.write(f"# tools/bench_block_attention_prefill_split.py --rounds {args.rounds} --iters {args.iters}: ms, median over the "
                    f"rounds [min … max]; bfloat16, D = {D}, Hq = {HQ}, Hkv = {HKV}, block {BLOCK}, the contiguous cache; ratio: to the "
                    f"unsplit call of the same rounds\n")
        for case in args.cases.split(","):
            try:  # a fresh child per case, under its own time limit; nothing more is started after a failure
                rc = subprocess.run([sys.executable, __file__, "--case", case, "--rounds", str(args.rounds), "--iters", str(args.iters),
                                     "--log", str(path)], timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                with open(path, "a") as f:
                    f.write(f"\n{case}: ended with status {rc}; the run stops here\n")
                sys.exit(rc)
        return
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    rc = run_case(args.case, args.rounds, args.iters, emit)
    with open(path, "a") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(rc)


if __name__ == "__main__":
    main()
