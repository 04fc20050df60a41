"""A/B in one process of a SiT-XL/2 block linear as the fp16 GEMM the planner picks today, as the MX-fp8 block GEMM alone
(operands pre-quantised) and as the MX-fp8 GEMM behind the row pass that quantises its A operand — alternated per round, at the four
block shapes with each layer's own epilogue, M = 16384 and 65536.

    python tools/time_gemm_mxfp8.py [--rounds 5] [--reps 10] [--ms 16384,65536] [--out FILE]

Per shape: the median over rounds of the mean time of `reps` back-to-back launches (device events), in us and TFLOP/s (2 M N K for
every arm), the speed-ups of the two fp8 arms over fp16, and the kernel the fp16 arm ran (ops.gemm_plan)."""
import argparse
import statistics
import sys

import torch

sys.path.insert(0, ".")
from reed_amd import ops  # noqa: E402

# (layer, epilogue, N, K) of SiT-XL/2 (D = 1152)
LAYERS = (("qkv", ops.EPI_BF16, 3456, 1152), ("proj", ops.EPI_GATE_RES, 1152, 1152), ("fc1", ops.EPI_GELU, 4608, 1152),
          ("fc2", ops.EPI_GATE_RES, 1152, 4608))
ARMS = ("fp16", "fp8", "fp8+quant")
T = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ms", default="16384,65536")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"# tools/time_gemm_mxfp8.py --rounds {a.rounds} --reps {a.reps}: median of rounds, arms alternated per round; "
             f"{torch.cuda.get_device_name(0)}",
             f"{'layer':5} {'M':>6} {'N':>5} {'K':>5} | {'fp16 us':>8} {'TF/s':>7} {'kernel':>7} | {'fp8 us':>8} {'TF/s':>7} {'x':>5} | "
             f"{'fp8+q us':>8} {'TF/s':>7} {'x':>5} | {'quant us':>8} {'GB/s':>6}"]
    print("\n".join(lines), flush=True)
    prev = ops.use("fp16")
    try:
        for M in (int(v) for v in a.ms.split(",")):
            for name, epi, N, K in LAYERS:
                g = torch.Generator(device=dev).manual_seed(M + N + K)
                A = torch.randn(M, K, device=dev, generator=g).half()
                W = (torch.randn(N, K, device=dev, generator=g) / K ** 0.5).half()
                bias = torch.randn(N, device=dev, generator=g).half()
                gate = torch.randn(M // T, N, device=dev, generator=g).half()
                R = torch.randn(M, N, device=dev, generator=g)
                gres = epi == ops.EPI_GATE_RES
                C = torch.empty(M, N, device=dev, dtype=torch.float32 if gres else torch.float16)
                kw = dict(bias=bias)
                if gres:
                    kw.update(R=R, ldr=N, gate=gate, ldgate=N, rows_per_gate=T)
                if epi == ops.EPI_GELU:
                    kw.update(C2=C, ldc2=N)
                Cm = None if epi == ops.EPI_GELU else C
                Aq, As = torch.empty(M, K, dtype=torch.uint8, device=dev), torch.empty(M, K // 32, dtype=torch.uint8, device=dev)
                Wq, Ws = torch.empty(N, K, dtype=torch.uint8, device=dev), torch.empty(N, K // 32, dtype=torch.uint8, device=dev)
                ops.mx_quantize(A, Aq, As, M, K)
                ops.mx_quantize(W, Wq, Ws, N, K)
                _, launches = ops.gemm_plan(ops.NT, epi, M, N, K, rows_per_gate=T if gres else 1, precision="fp16")
                kern = "+".join(l["kernel"] for l in launches)

                def run(arm):
                    if arm == "fp16":
                        ops.gemm(ops.NT, epi, A, W, M, N, K, Cm, K, K, N, **kw)
                    elif arm == "quant":
                        ops.mx_quantize(A, Aq, As, M, K)
                    else:
                        if arm == "fp8+quant":
                            ops.mx_quantize(A, Aq, As, M, K)
                        ops.gemm_mxfp8(epi, Aq, As, Wq, Ws, M, N, K, Cm, N, **kw)

                arms = ARMS + ("quant",)
                times = {m: [] for m in arms}
                for m in arms:
                    run(m)
                torch.cuda.synchronize()
                for _ in range(a.rounds):
                    for m in arms:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(a.reps):
                            run(m)
                        e1.record()
                        torch.cuda.synchronize()
                        times[m].append(e0.elapsed_time(e1) * 1e3 / a.reps)
                us = {m: statistics.median(t) for m, t in times.items()}
                tf = {m: 2.0 * M * N * K / us[m] / 1e6 for m in ARMS}
                line = (f"{name:5} {M:6d} {N:5d} {K:5d} | {us['fp16']:8.1f} {tf['fp16']:7.1f} {kern:>7} | {us['fp8']:8.1f} {tf['fp8']:7.1f} "
                        f"{us['fp16'] / us['fp8']:5.2f} | {us['fp8+quant']:8.1f} {tf['fp8+quant']:7.1f} {us['fp16'] / us['fp8+quant']:5.2f} | "
                        f"{us['quant']:8.1f} {M * K * (2 + 33 / 32) / us['quant'] / 1e3:6.0f}")
                lines.append(line)
                print(line, flush=True)
    finally:
        ops.use(prev)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
