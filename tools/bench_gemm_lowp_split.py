"""The grid behind the split rule of the low-precision dense product (mi_gemm_lowp_split_count).

    python tools/bench_gemm_lowp_split.py [--log FILE] [--dtype bf16|fp16]

TN products (the FC weight gradient's form: A stored k × m, B stored k × n) for m, n ∈ {256, 768, 1536, 3072} and
k ∈ {2 K … 64 K}: every S ∈ {1, 2, 4, 8, 16, 32} timed through custom_mm.cublas_mmul_splitk(..., splits=S) — S = 1 is the
unsplit product — as interleaved medians in one process.  Per shape: the times, the best S, the rule's S and how far
the rule lies from the best (rule ms / best ms).
"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "matrix-multiplication_amd"))
sys.path.insert(0, str(ROOT / "tools"))
import custom_mm  # noqa: E402
from bench_hbm_regime import time_interleaved  # noqa: E402

SIZES = (256, 768, 1536, 3072)
KS = (2048, 4096, 8192, 16384, 32768, 65536)
SPLITS = (1, 2, 4, 8, 16, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log")
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp16"))
    args = ap.parse_args()
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16}[args.dtype]
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    lines, worst = [], 1.0
    for m in SIZES:
        for n in SIZES:
            for k in KS:
                a = (torch.rand(k, m, device=dev, generator=g) * 2 - 1).to(dt)
                b = (torch.rand(k, n, device=dev, generator=g) * 2 - 1).to(dt)
                c = torch.empty(m, n, device=dev, dtype=dt)
                ent = {S: (lambda S=S: custom_mm.cublas_mmul_splitk(a, b, c, True, False, None, S)) for S in SPLITS}
                t = time_interleaved(ent, rounds=3, budget_ms=20.0)
                best = min(t, key=t.get)
                rule = custom_mm.gemm_lowp_split_count(m, n, k)
                far = t[rule] / t[best]
                worst = max(worst, far)
                line = (f"{m:5d} x {n:5d} x {k:6d} | ms " + " ".join(f"S{S} {t[S]:.3f}" for S in SPLITS) +
                        f" | best S{best} rule S{rule} rule/best {far:.2f} rule/unsplit {t[rule] / t[1]:.2f}")
                print(line, flush=True)
                lines.append(line)
    lines.append(f"worst rule/best over the grid: {worst:.2f}")
    print(lines[-1])
    if args.log:
        Path(args.log).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
