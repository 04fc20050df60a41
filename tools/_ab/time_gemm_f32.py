"""A/B of the fp32 build's two GEMM kernels in one process: the exact one (v_mfma_f32_32x32x2_f32) and the split one (three bf16
MFMA products per fp32 product; ops.f32_split), alternated per round at the SiT-XL/2 shapes, all three layouts.

    python tools/_ab/time_gemm_f32.py [--mode both|exact|split] [--rounds 5] [--reps 10] [--out FILE]

Per shape: the median over rounds of the mean time of `reps` back-to-back launches (device events), in us and TFLOP/s (2 M N K, the
fp32 problem's flops for both kernels), the split kernel's speed-up, and the largest |difference| of the two outputs over the
largest |output| (the same seeded operands)."""
import argparse
import statistics
import sys

import torch

sys.path.insert(0, ".")
from reed_amd import ops  # noqa: E402

NK = ((1152, 1152), (4608, 1152), (1152, 4608), (3456, 1152))
MS = (8192, 65536)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["both", "exact", "split"], default="both")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    modes = {"both": (False, True), "exact": (False,), "split": (True,)}[a.mode]
    lines = [f"# tools/_ab/time_gemm_f32.py --mode {a.mode} --rounds {a.rounds} --reps {a.reps}: median of rounds, kernels alternated "
             f"per round; {torch.cuda.get_device_name(0)}",
             f"{'layout':6} {'M':>6} {'N':>5} {'K':>5} | {'exact us':>9} {'TFLOP/s':>8} | {'split us':>9} {'TFLOP/s':>8} | {'speed-up':>8} | max|diff|/max|C|"]
    print("\n".join(lines), flush=True)
    prev = ops.use("fp32")
    try:
        for lay, name in ((ops.NT, "NT"), (ops.NN, "NN"), (ops.TN, "TN")):
            for M in MS:
                for N, K in NK:
                    g = torch.Generator(device=dev).manual_seed(M + N + K)
                    P = torch.randn(M if lay != ops.TN else K, K if lay != ops.TN else M, device=dev, generator=g)
                    Q = torch.randn(N if lay == ops.NT else K, K if lay == ops.NT else N, device=dev, generator=g) / K ** 0.5
                    C = {m: torch.empty(M, N, device=dev) for m in modes}
                    times = {m: [] for m in modes}

                    def run(m):
                        ops.gemm(lay, ops.EPI_F32, P, Q, M, N, K, C[m], P.shape[1], Q.shape[1], N)

                    for m in modes:                       # warm up both kernels at this shape
                        with ops.f32_split_mode(m):
                            run(m)
                    torch.cuda.synchronize()
                    for _ in range(a.rounds):
                        for m in modes:
                            with ops.f32_split_mode(m):
                                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                                e0.record()
                                for _ in range(a.reps):
                                    run(m)
                                e1.record()
                                torch.cuda.synchronize()
                            times[m].append(e0.elapsed_time(e1) * 1e3 / a.reps)
                    us = {m: statistics.median(t) for m, t in times.items()}
                    tf = {m: 2.0 * M * N * K / u / 1e6 for m, u in us.items()}
                    cell = lambda m: f"{us[m]:9.1f} {tf[m]:8.1f}" if m in us else f"{'-':>9} {'-':>8}"  # noqa: E731
                    extra = f"{'-':>8} | -"
                    if len(modes) == 2:
                        diff = float((C[True] - C[False]).abs().max() / C[False].abs().max())
                        extra = f"{us[False] / us[True]:7.2f}x | {diff:.1e}"
                    line = f"{name:6} {M:6d} {N:5d} {K:5d} | {cell(False)} | {cell(True)} | {extra}"
                    lines.append(line)
                    print(line, flush=True)
    finally:
        ops.use(prev)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
