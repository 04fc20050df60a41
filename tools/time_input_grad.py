#!/usr/bin/env python
"""Time the input-gradient path of SiT-XL/2 in bf16 at 8192 and 65536 tokens (b = 32 and 256 at 32 x 32 latents):
reed_patch_embed_bwd_x beside the patch-embed small-K weight gradient on the same dx (both read that array once), and the full
backward beside the frozen-weight backward.  Prints to stdout; --out appends the same lines to a file."""
import argparse, os, statistics, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import detfill
from reed_amd import ops
from reed_amd.models.sit import SiT_models

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--batches", type=int, nargs="+", default=[32, 256])
ap.add_argument("--iters", type=int, default=7)
args = ap.parse_args()
dev = torch.device("cuda")
D, T, K, PEAK = 1152, 256, 16, 8.0
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def kernel_us(fn, it=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):   # 5 windows of `it` launches: the median window
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(it):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / it)
    return statistics.median(ts), min(ts), max(ts)


def backward_ms(m, B, inputs_grad):
    """Median time of .backward() alone over args.iters steps (2 warm-up steps in front); the loss is a plain sum of the outputs."""
    y = torch.randint(0, 1000, (B,), device=dev)
    ts = []
    for i in range(2 + args.iters):
        x = torch.randn(B, 4, 32, 32, device=dev).requires_grad_(inputs_grad)
        t = torch.rand(B, device=dev).requires_grad_(inputs_grad)
        out, zs = m(x, t, y, inference=False)
        loss = out.sum() + sum(z.float().sum() for z in zs)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        loss.backward()
        e1.record()
        torch.cuda.synchronize()
        m.engine().zero_grad()
        if i >= 2:
            ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


say(f"input gradients, SiT-XL/2 bf16 on {torch.cuda.get_device_name(0)}: kernels = median (min .. max) of 5 windows of 20 launches; "
    f"backward = median (min .. max) of {args.iters} steps; TB/s = the {D} fp32 columns of dx read once, of {PEAK:g} TB/s peak")
ops.use("bf16")
for B in args.batches:
    M = B * T
    dx = torch.randn(M, D, device=dev)
    w = (0.1 * torch.randn(D, K, device=dev)).bfloat16()
    xb = torch.randn(M, K, device=dev).bfloat16()
    out = torch.empty(B, 4, 32, 32, device=dev)
    ws = torch.empty(ops.smallk_ws_floats(D, K), device=dev)
    gw, gb = torch.zeros(D * K, device=dev), torch.zeros(D, device=dev)
    ref = (dx.bfloat16().double() @ w.double())
    ops.patch_embed_bwd_x(dx, w, out, B, 4, 32, 2, D)
    got = out.view(B, 4, 16, 2, 16, 2).permute(0, 2, 4, 1, 3, 5).reshape(M, K).double()
    err = float((got - ref).abs().max() / ref.abs().max())
    a = kernel_us(lambda: ops.patch_embed_bwd_x(dx, w, out, B, 4, 32, 2, D))
    b = kernel_us(lambda: ops.smallk_wgrad(dx, True, xb, ws, gw, gb, None, M, D, K, 0, False))
    gbytes = M * D * 4 / 1e12
    for name, (med, lo, hi) in (("reed_patch_embed_bwd_x", a), ("reed_smallk_wgrad (2 launches)", b)):
        say(f"[{M:6d} tokens] {name:32s} {med:8.1f} us ({lo:.1f} .. {hi:.1f})  {gbytes / (med * 1e-6):5.2f} TB/s = "
            f"{100 * gbytes / (med * 1e-6) / PEAK:4.1f} % of peak")
    say(f"[{M:6d} tokens] ratio bwd_x / small-K wgrad {a[0] / b[0]:.2f}; bwd_x worst error vs fp64 {err:.1e} of max|dx|")
    del dx, xb, out, ws, ref, got

m = SiT_models["SiT-XL/2"]()
detfill.fill_state_dict(m.state_dict(), base_seed=0)
m = m.to(dev).train()
res = {}
for B in args.batches:
    res[B, "full"] = backward_ms(m, B, False)
    res[B, "full+inputs"] = backward_ms(m, B, True)
m.requires_grad_(False)
for B in args.batches:
    res[B, "frozen"] = backward_ms(m, B, True)
for B in args.batches:
    for mode, what in (("full", "full backward (parameters only, as before)"), ("full+inputs", "full backward + dL/dx + dL/dt"),
                       ("frozen", "frozen-weight backward (dL/dx + dL/dt only)")):
        med, lo, hi = res[B, mode]
        say(f"[{B * T:6d} tokens] {what:46s} {med:8.2f} ms ({lo:.2f} .. {hi:.2f})")
    say(f"[{B * T:6d} tokens] frozen / full {res[B, 'frozen'][0] / res[B, 'full'][0]:.3f}; the two input gradients cost "
        f"{res[B, 'full+inputs'][0] - res[B, 'full'][0]:+.2f} ms on top of the full backward")
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
