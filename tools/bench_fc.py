"""Developer probe: the FC-layer modules (fc_layers.cublasLinear / cusparseLinear) vs torch.nn.Linear,
forward + backward, at BERT-base FFN shapes with ReLU-sparse activations.

    python tools/bench_fc.py                              the float32 rows
    python tools/bench_fc.py --dtype bf16 [--log FILE]    the low-precision rows, interleaved medians:
        the bias epilogue against the plain product and against product + torch add; the split weight gradient against
        the unsplit product; cublasLinear in T beside nn.Linear in T and our float32 layer; the fp32 sparse route of
        cusparseLinear against the T dense route at 99 % zeros
    python tools/bench_fc.py --dtype bf16 --profile       one forward + backward of the 3072 -> 768 layer (for kstats.sh)
"""
import argparse
import sys
from pathlib import Path
import torch
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "matrix-multiplication_amd"))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import custom_mm  # noqa: E402
import fc_layers  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--dtype", default="fp32", choices=("fp32", "bf16", "fp16"))
ap.add_argument("--log")
ap.add_argument("--profile", action="store_true")
ARGS = ap.parse_args()
dev = torch.device("cuda")


def lowp_rows(dt):
    from bench_hbm_regime import time_interleaved
    out = []

    def say(line):
        print(line, flush=True)
        out.append(line)

    def rand(shape, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        return torch.rand(shape, device=dev, generator=g) * 2 - 1

    for tokens, fin, fout in ((16384, 3072, 768), (16384, 768, 3072), (4096, 4096, 4096)):
        x32, w32, b32, dy32 = rand((tokens, fin), 1), rand((fout, fin), 2), rand((fout,), 3), rand((tokens, fout), 4)
        x, w, b, dy = (v.to(dt) for v in (x32, w32, b32, dy32))
        y, gw = torch.empty(tokens, fout, device=dev, dtype=dt), torch.empty(fout, fin, device=dev, dtype=dt)

        def composed():
            custom_mm.cublas_mmul(x, w, y, False, True)
            return y + b

        t = time_interleaved({"plain": lambda: custom_mm.cublas_mmul(x, w, y, False, True),
                              "bias": lambda: custom_mm.cublas_mmul_bias(x, w, b, y, False, True),
                              "plain+torch_add": composed})
        say(f"{tokens} x {fin} -> {fout} {ARGS.dtype} forward | ms plain {t['plain']:.3f} bias epilogue {t['bias']:.3f} "
            f"plain + torch add {t['plain+torch_add']:.3f} | bias/plain {t['bias'] / t['plain']:.3f} "
            f"bias/composed {t['bias'] / t['plain+torch_add']:.3f}")
        S = custom_mm.gemm_lowp_split_count(fout, fin, tokens)
        t = time_interleaved({"unsplit": lambda: custom_mm.cublas_mmul(dy, x, gw, True, False),
                              "split": lambda: custom_mm.cublas_mmul_splitk(dy, x, gw, True, False),
                              "torch": lambda: torch.matmul(dy.t(), x, out=gw)})
        say(f"{tokens} x {fin} -> {fout} {ARGS.dtype} weight gradient {fout} x {fin} x {tokens} | S {S} | ms unsplit "
            f"{t['unsplit']:.3f} split {t['split']:.3f} torch {t['torch']:.3f} | split/unsplit {t['split'] / t['unsplit']:.3f} "
            f"split/torch {t['split'] / t['torch']:.2f}")
        t = time_interleaved({"T": lambda: custom_mm.column_sums(dy), "fp32": lambda: custom_mm.column_sums(dy32),
                              "torch_T": lambda: dy.sum(0)})
        say(f"{tokens} x {fout} column sums | ms {ARGS.dtype} {t['T']:.3f} fp32 {t['fp32']:.3f} torch {ARGS.dtype} {t['torch_T']:.3f}")
        layers = {"ours_T": (fc_layers.cublasLinear(fin, fout).to(dev).to(dt), x, dy),
                  "torch_T": (torch.nn.Linear(fin, fout).to(dev).to(dt), x, dy),
                  "ours_fp32": (fc_layers.cublasLinear(fin, fout).to(dev), x32, dy32)}

        def fwd(name):
            layer, xi, _ = layers[name]

            def run():
                with torch.no_grad():
                    layer(xi)
            return run

        def step(name):
            layer, xi, g = layers[name]

            def run():
                xx = xi.detach().requires_grad_(True)
                layer.zero_grad(set_to_none=True)
                layer(xx).backward(g)
            return run

        tf = time_interleaved({k: fwd(k) for k in layers})
        ts = time_interleaved({k: step(k) for k in layers})
        say(f"{tokens} x {fin} -> {fout} layer | fwd ms ours-{ARGS.dtype} {tf['ours_T']:.3f} nn.Linear-{ARGS.dtype} {tf['torch_T']:.3f} "
            f"ours-fp32 {tf['ours_fp32']:.3f} | fwd+bwd ms ours-{ARGS.dtype} {ts['ours_T']:.3f} nn.Linear-{ARGS.dtype} "
            f"{ts['torch_T']:.3f} ours-fp32 {ts['ours_fp32']:.3f} | fwd+bwd ours-T/ours-fp32 {ts['ours_T'] / ts['ours_fp32']:.2f} "
            f"ours-T/torch-T {ts['ours_T'] / ts['torch_T']:.2f}")
    # the sparse route of the float32 cusparseLinear against the T dense route, 99 % zeros, 16384 x 3072 -> 768
    tokens, fin, fout = 16384, 3072, 768
    g = torch.Generator(device=dev).manual_seed(0)
    x32 = torch.rand(tokens, fin, device=dev, generator=g) * (torch.rand(tokens, fin, device=dev, generator=g) >= 0.99)
    sp32, spT = fc_layers.cusparseLinear(fin, fout).to(dev), fc_layers.cusparseLinear(fin, fout).to(dev).to(dt)
    xT = x32.to(dt)

    def f32():
        with torch.no_grad():
            sp32(x32)

    def fT():
        with torch.no_grad():
            spT(xT)

    t = time_interleaved({"fp32_sparse": f32, "T_dense": fT})
    say(f"cusparseLinear {tokens} x {fin} -> {fout}, 99 % zeros, forward | ms fp32 (sparse route) {t['fp32_sparse']:.3f} "
        f"{ARGS.dtype} (dense route) {t['T_dense']:.3f}")
    if ARGS.log:
        Path(ARGS.log).write_text("\n".join(out) + "\n")


if ARGS.dtype != "fp32":
    DT = {"bf16": torch.bfloat16, "fp16": torch.float16}[ARGS.dtype]
    if ARGS.profile:
        layer = fc_layers.cublasLinear(3072, 768).to(dev).to(DT)
        xp = torch.rand(16384, 3072, device=dev).to(DT).requires_grad_(True)
        for _ in range(3):
            layer.zero_grad(set_to_none=True)
            layer(xp).backward(torch.ones(16384, 768, device=dev, dtype=DT))
        torch.cuda.synchronize()
    else:
        lowp_rows(DT)
    sys.exit(0)


def timeit(fn, iters=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


SHAPES = [(32 * 512, 768, 3072), (32 * 512, 3072, 768), (4096, 4096, 4096), (32 * 512, 3072, 256)]
for (tokens, fin, fout, zero_frac) in [(t, i, o, z) for (t, i, o) in SHAPES for z in (0.5, 0.75, 0.9, 0.99)]:
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(tokens, fin, device=dev, generator=g)
    x = x * (torch.rand(tokens, fin, device=dev, generator=g) >= zero_frac)
    dy = torch.rand(tokens, fout, device=dev, generator=g)
    line = f"tokens={tokens} {fin}->{fout} zeros={zero_frac}:"
    for name, layer in [("nn.Linear", torch.nn.Linear(fin, fout).to(dev)), ("cublasLinear", fc_layers.cublasLinear(fin, fout).to(dev)),
                        ("cusparseLinear", fc_layers.cusparseLinear(fin, fout).to(dev))]:
        def step():
            xx = x.clone().requires_grad_(True)
            layer.zero_grad(set_to_none=True)
            layer(xx).backward(dy)
        def fwd():
            with torch.no_grad():
                layer(x)
        line += f"  {name} fwd {timeit(fwd):.3f} / fwd+bwd {timeit(step):.3f} ms"
    print(line, flush=True)

# components of the dense backward at tokens=16384, 768 -> 3072
tokens, fin, fout = 32 * 512, 768, 3072
g = torch.Generator(device=dev).manual_seed(1)
x = torch.rand(tokens, fin, device=dev, generator=g)
w = torch.rand(fout, fin, device=dev, generator=g)
dy = torch.rand(tokens, fout, device=dev, generator=g)
y = torch.empty(tokens, fout, device=dev)
gi = torch.empty(tokens, fin, device=dev)
gw = torch.empty(fout, fin, device=dev)
ones = torch.ones(1, tokens, device=dev)
gb = torch.empty(1, fout, device=dev)
print(f"fwd x.WT        {timeit(lambda: custom_mm.cublas_mmul(x, w, y, False, True)):.3f} ms (torch {timeit(lambda: torch.matmul(x, w.t(), out=y)):.3f})")
print(f"grad_inp dY.W   {timeit(lambda: custom_mm.cublas_mmul(dy, w, gi, False, False)):.3f} ms (torch {timeit(lambda: torch.matmul(dy, w, out=gi)):.3f})")
print(f"grad_w dYT.x    {timeit(lambda: custom_mm.cublas_mmul(dy, x, gw, True, False)):.3f} ms (torch {timeit(lambda: torch.matmul(dy.t(), x, out=gw)):.3f})")
print(f"grad_b colsums  {timeit(lambda: custom_mm.column_sums(dy)):.3f} ms (torch sum {timeit(lambda: dy.sum(0)):.3f}; as a 1 x tokens GEMM "
      f"{timeit(lambda: custom_mm.cublas_mmul(ones, dy, gb, False, False)):.3f})")
