"""Times the LoRA path on one MI355X, same process, interleaved with the paths it replaces; writes profiles/lora.txt.

    python tools/time_lora.py [--out profiles/lora.txt] [--batches 32 256] [--ranks 16 64]

SiT-XL/2 (D = 1152, T = 256 tokens per image) at the given local batches.  Per adapted linear: reed_lora_grads against the per-GEMM
weight gradient it replaces (ops.plan_wgrad + ops.linear_wgrad), a quarter of the block's grouped launch (ops.wgrad_group), and the
obvious alternative "full dW, then B^T dW and dW A^T" (two torch matmuls on the fp32 dW); the achieved TB/s against the bytes
csrc/lora.hip states; the per-step merge of all adapted weights; the adapters-only step and its peak memory against the fully
trainable step and against --train-only of the same four linears; the optimiser pass alone.  Medians of interleaved repetitions.
"""
import argparse
import copy
import gc
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from reed_amd import ops  # noqa: E402

D, HM, T = 1152, 4608, 256
LINEARS = (("attn.qkv", 3 * D, D), ("attn.proj", D, D), ("mlp.fc1", HM, D), ("mlp.fc2", D, HM))


def timed(fns, reps=7, inner=3):
    """{name: median ms per call}; the candidates take turns, `inner` calls per turn between two events."""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                f()
            e1.record()
            e1.synchronize()
            res[k].append(e0.elapsed_time(e1) / inner)
    return {k: statistics.median(v) for k, v in res.items()}


def kernel_table(b, R, dev, say):
    M = b * T
    hd = torch.bfloat16
    bufs = {}
    for name, N, K in LINEARS:
        g = torch.Generator(device=dev).manual_seed(N + K)
        bufs[name] = dict(x=torch.randn(M, K, device=dev, generator=g).to(hd), dy=(0.05 * torch.randn(M, N, device=dev, generator=g)).to(hd),
                          a=(torch.randn(R, K, device=dev, generator=g) / K ** 0.5).to(hd), b=(0.1 * torch.randn(N, R, device=dev, generator=g)).to(hd),
                          da=torch.empty(R, K, device=dev), db=torch.empty(N, R, device=dev), dw=torch.empty(N, K, device=dev),
                          dbias=torch.empty(N, device=dev))
    group = [(v["dy"], v["x"], v["dw"], v["dbias"], N, K) for (name, N, K), v in zip(LINEARS, bufs.values())]
    grouped = ops.wgrad_group_fits([(N, K) for _, N, K in LINEARS])
    tg = timed({"group": lambda: ops.wgrad_group(group, M)})["group"] if grouped else float("nan")
    say(f"-- local batch {b} (M = {M} tokens), R = {R}; the block's grouped weight-gradient launch: {tg:.3f} ms "
        f"({'four linears in one launch' if grouped else 'not taken at this size'})")
    say(f"{'linear':10s} {'lora_grads':>10s} {'per-GEMM dW':>11s} {'group / 4':>9s} {'dW + 2 mm':>9s} {'stated MB':>9s} {'TB/s':>6s}")
    total = 0.0
    for name, N, K in LINEARS:
        v = bufs[name]
        nws = ops.lora_grads_ws_floats(M, N, K, R)
        ws = torch.empty(nws, device=dev)
        lay, split = ops.plan_wgrad(M, N, K)
        wsw = torch.empty(split * (N * K + N), device=dev) if split > 1 else None
        a32, b32 = v["a"].float(), v["b"].float()

        def lora():
            ops.lora_grads(v["x"], v["dy"], v["a"], v["b"], 2.0, v["da"], v["db"], ws, M, N, K, R)

        def wgrad():
            ops.linear_wgrad(v["dy"], v["x"], v["dw"], dbias=v["dbias"], split_k=split, Mtok=M, N=N, K=K, ws=wsw, lay=lay)

        def full():
            wgrad()
            torch.matmul(v["dw"], a32.t(), out=v["db"])
            torch.matmul(b32.t(), v["dw"], out=v["da"])

        t = timed({"lora": lora, "wgrad": wgrad, "full": full})
        slabs = min(32, (M + 31) // 32)
        nbytes = 4 * M * (N + K) + 8 * M * R + 8 * slabs * R * (N + K)
        total += t["lora"]
        say(f"{name:10s} {t['lora']:10.3f} {t['wgrad']:11.3f} {tg / 4:9.3f} {t['full']:9.3f} {nbytes / 1e6:9.1f} {nbytes / t['lora'] / 1e9:6.2f}")
    say(f"{'block':10s} {total:10.3f} ms for the four reed_lora_grads calls of a block")


def make(dev, lora_rank=0, train_only=None):
    from reed_amd.models.sit import SiT_models
    from reed_amd.optim import FusedAdamWEMA
    from reed_amd.train import apply_freeze, apply_lora_freeze
    torch.manual_seed(0)
    kw = dict(lora_rank=lora_rank, lora_alpha=2 * lora_rank) if lora_rank else {}
    m = SiT_models["SiT-XL/2"](input_size=32, num_classes=1000, use_cfg=True, z_dims=[768], z_types=["i"], encoder_depth=8, **kw)
    with torch.no_grad():   # off the identity init: every block contributes
        for n, p in m.named_parameters():
            if "adaLN" in n or n.startswith("final_layer.linear") or n.endswith("lora_B"):
                p.normal_(0, 0.02)
    m = m.to(dev).train()
    if lora_rank:
        n_on = apply_lora_freeze(m)
    elif train_only:
        n_on = apply_freeze(m, None, train_only)
    else:
        n_on = sum(p.numel() for p in m.parameters() if p.requires_grad)
    ema = copy.deepcopy(m).requires_grad_(False).eval()
    return m, ema, FusedAdamWEMA(m, ema, lr=1e-4, overlap=True), n_on


def step_table(batches, ranks, dev, say):
    from reed_amd.loss import SILoss
    from reed_amd.trainer import TrainStep
    four = [f"blocks.*.{lin}.weight" for lin, _, _ in LINEARS] + [f"blocks.*.{lin}.bias" for lin, _, _ in LINEARS]
    configs = [("fully trainable", dict())] + [("--train-only the four linears", dict(train_only=four))] + \
              [(f"adapters only, R = {R}", dict(lora_rank=R)) for R in ranks]
    say(f"{'configuration':32s} {'trainable':>12s} " + " ".join(f"{'b=' + str(b) + ' ms':>10s} {'peak GB':>8s} {'opt ms':>7s}" for b in batches))
    for tag, kw in configs:
        m, ema, opt, n_on = make(dev, **kw)
        step = TrainStep(m, SILoss(enc_names=["dinov2"], loss_weights={"dinov2": 1.0}), opt, None, proj_coeff=0.5,
                         diffusion_warm_up_steps=0)
        cells = []
        for b in batches:
            g = torch.Generator(device=dev).manual_seed(b)
            x = torch.randn(b, 4, 32, 32, device=dev, generator=g)
            y = torch.randint(0, 1000, (b,), device=dev, generator=g)
            zs = [torch.randn(b, T, 768, device=dev, generator=g)]
            for _ in range(2):
                step(x, y, zs)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                step(x, y, zs)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            peak = torch.cuda.max_memory_allocated() / 2 ** 30
            to = []
            for _ in range(5):   # the optimiser pass alone, on the gradients of the last step (merge included where there are adapters)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                opt.step()
                opt.flush()
                torch.cuda.synchronize()
                to.append((time.perf_counter() - t0) * 1e3)
            cells.append(f"{statistics.median(ts):10.2f} {peak:8.2f} {statistics.median(to):7.2f}")
        say(f"{tag:32s} {n_on:12,d} " + " ".join(cells))
        if kw.get("lora_rank"):
            A = m._arena
            prev = ops.use("bf16")
            A.ensure_shadow("bf16")
            tm = timed({"merge": A.merge_lora})["merge"]
            ops.use(prev)
            n_el = sum(A.layout.numel(w) for _, w, _, _ in A.layout.lora)
            say(f"{'':32s} merge of {len(A.layout.lora)} adapted weights ({n_el / 1e6:.0f} M elements, 6 B each): {tm:.3f} ms = "
                f"{6 * n_el / tm / 1e9:.2f} TB/s")
        m._engine = ema._engine = None   # (model <-> engine reference cycle)
        del m, ema, opt, step
        gc.collect()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora.txt"))
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--ranks", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--no-steps", action="store_true", help="the kernel table only")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/time_lora.py on {torch.cuda.get_device_name(0)}: SiT-XL/2, bf16 build; medians of interleaved repetitions, ms")
    say("# reed_lora_grads (csrc/lora.hip) per adapted linear against what it replaces; stated bytes = 4 M (N + K) + 8 M R + 8 S R (N + K)")
    ops.use("bf16")
    for b in a.batches:
        for R in a.ranks:
            kernel_table(b, R, dev, say)
    if not a.no_steps:
        say("# one training step (TrainStep: loss + backward + fused optimiser with overlap; projector loss on), one GPU")
        try:
            step_table(a.batches, a.ranks, dev, say)
        except Exception as e:   # keep the kernel table
            say(f"# step table failed: {type(e).__name__}: {e}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
