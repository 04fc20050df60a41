"""Times activation recomputation (reed_amd/recompute.py) on one MI355X; writes profiles/recompute.txt.

    python tools/time_recompute.py [--out profiles/recompute.txt] [--parent DIR] [--repeats 3] [--steps 10]

SiT-XL/2, bf16, one 768-d alignment projector, synthetic latents and features, random-init weights with non-zero adaLN (every block
does real work), TrainStep as train.py builds it (loss + backward + fused optimiser).  One process per row (this script starts itself
with --row): 3 warm-up + `steps` timed steps (wall clock between synchronisations, median), then `steps` event-timed backward()
calls of the same loss (forward outside the events, median), peak = torch.cuda.max_memory_allocated over the timed steps.

  * recompute in {0, 14, all} at 256^2 with local batch 32 and 256, and at 512^2 with local batch 32;
  * with --parent DIR (a checkout of the parent commit: its reed_amd/ and include/; its libraries, or this tree's where it has
    none built), the recompute = 0 rows against the parent, interleaved: parent, this, parent, this, ...;
  * at 512^2 the largest power-of-two local batch each of 0 and all can hold, found from Engine.saved_activation_bytes against the
    free memory and Engine.max_tokens — not by running out of memory;
  * LoRA at R = 16 with 0 and all.
A row whose process fails (a fault, an abort, out of memory, a time limit) ends the run: what is in hand is written, nothing more
is started on the GPU, the exit status is 1.  The file is this tool's alone (the tests' figures are in profiles/recompute_tests.txt).
"""
import argparse
import copy
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_OF = {256: 256, 512: 1024}


def row(spec):
    """One process: build the model from the tree spec["tree"], run spec["settings"] in turn; one JSON line on stdout."""
    sys.path.insert(0, spec["tree"])
    import torch
    import reed_amd
    assert os.path.dirname(os.path.abspath(reed_amd.__file__)) == os.path.join(os.path.abspath(spec["tree"]), "reed_amd")
    from reed_amd.loss import SILoss
    from reed_amd.models.sit import SiT_models
    from reed_amd.optim import FusedAdamWEMA
    from reed_amd.trainer import TrainStep
    dev = torch.device("cuda:0")
    res, steps, R = spec["resolution"], spec["steps"], spec.get("lora", 0)
    T = T_OF[res]
    torch.manual_seed(0)
    kw = dict(lora_rank=R, lora_alpha=2 * R) if R else {}
    m = SiT_models["SiT-XL/2"](input_size=res // 8, num_classes=1000, use_cfg=True, z_dims=[768], z_types=["i"], encoder_depth=8, **kw)
    with torch.no_grad():   # off the identity init: every block contributes
        for n, p in m.named_parameters():
            if "adaLN" in n or n.startswith("final_layer.linear") or n.endswith("lora_B"):
                p.normal_(0, 0.02)
    m = m.to(dev).train()
    if R:
        from reed_amd.train import apply_lora_freeze
        apply_lora_freeze(m)
    ema = copy.deepcopy(m).requires_grad_(False).eval()
    opt = FusedAdamWEMA(m, ema, lr=1e-4)
    loss_fn = SILoss(enc_names=["dinov2"], loss_weights={"dinov2": 1.0})
    step = TrainStep(m, loss_fn, opt, None, proj_coeff=0.5, diffusion_warm_up_steps=0)
    eng = m.engine()
    out = {"tree": spec["tag"], "resolution": res, "lora": R, "rows": []}
    for setting in spec["settings"]:
        if spec["tag"] != "parent":
            m.recompute = setting
        b = spec["batch"]
        note = ""
        if b == "max":   # the largest power of two whose tape, one block's live set and the backward's temporaries fit, by the closed form
            from reed_amd.recompute import block_bytes
            torch.cuda.synchronize()
            free, _total = torch.cuda.mem_get_info()
            free += torch.cuda.memory_reserved() - torch.cuda.memory_allocated()
            cap = eng.max_tokens() // T
            b, tried = 1, []
            while True:
                nb = 2 * b
                # beside the tape: the block in flight (a rebuilt set or the newest saved one's gradients) — budgeted as three blocks'
                # worth of arrays, the backward's dy / da / dqkv / dx chain and the attention workspace among them — and 4 GiB
                need = eng.saved_activation_bytes(nb, recompute=setting) + 3 * block_bytes(nb * T, eng.D, eng.Hm, eng.H, 2) + (4 << 30)
                tried.append((nb, round(need / 2 ** 30, 1)))
                if nb > cap or need > free:
                    break
                b = nb
            note = (f"free {free / 2 ** 30:.1f} GiB; tape + 3 blocks + 4 GiB by the closed form (batch, GiB): {tried}; "
                    f"Engine.max_tokens {eng.max_tokens()} = {cap} images")
        g = torch.Generator(device=dev).manual_seed(b)
        x = torch.randn(b, 4, res // 8, res // 8, device=dev, generator=g)
        y = torch.randint(0, 1000, (b,), device=dev, generator=g)
        zs = [torch.randn(b, T, 768, device=dev, generator=g)]
        for _ in range(3):
            r = step(x, y, zs)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ts = []
        for _ in range(steps):
            t0 = time.perf_counter()
            r = step(x, y, zs)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        peak = torch.cuda.max_memory_allocated()
        loss = float(r["loss"])
        tb = []
        for _ in range(steps):
            o = loss_fn(m, x, dict(y=y), zs=zs)
            total = o["denoising_loss"].mean() + 0.5 * o["proj_loss"].mean()
            eng.zero_grad()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            total.backward()
            e1.record()
            e1.synchronize()
            tb.append(e0.elapsed_time(e1))
        opt.zero_grad()
        out["rows"].append(dict(setting=setting, batch=b, ms_step=statistics.median(ts), ms_bwd=statistics.median(tb), peak=peak,
                                loss=loss, recomputed=getattr(eng, "recomputed", 0), note=note,
                                saved=eng.saved_activation_bytes(b, recompute=setting) if hasattr(eng, "saved_activation_bytes") else None))
        del x, y, zs, r, o, total
        torch.cuda.empty_cache()
    print("ROW " + json.dumps(out), flush=True)


def spawn(spec, say):
    env = dict(os.environ)
    if spec["tag"] == "parent" and not os.path.exists(os.path.join(spec["tree"], "reed_amd", "libreed_hip.so")):
        env["REED_HIP_LIB"] = os.path.join(ROOT, "reed_amd", "libreed_hip.so")    # the parent's sources on this tree's build
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--row", json.dumps(spec)], env=env, capture_output=True,
                           text=True, timeout=600)
    except subprocess.TimeoutExpired:
        raise RowFailed(f"# row {spec['tag']} {spec['resolution']} b={spec['batch']} {spec['settings']} did not finish in 600 s; "
                        f"nothing more is started on the GPU") from None
    line = [l for l in p.stdout.splitlines() if l.startswith("ROW ")]
    if p.returncode != 0 or not line:
        raise RowFailed(f"# row {spec['tag']} {spec['resolution']} b={spec['batch']} {spec['settings']} failed (exit {p.returncode}): "
                        f"{(p.stderr.strip().splitlines() or ['?'])[-1]}; nothing more is started on the GPU")
    return json.loads(line[0][4:])


class RowFailed(RuntimeError):
    """A row's process ended badly (a fault, an abort, out of memory, a time limit): the whole run ends there."""


def fmt(r, base=None):
    rel = f" ({r['ms_step'] / base['ms_step']:.3f} x)" if base else ""
    relb = f" ({r['ms_bwd'] / base['ms_bwd']:.3f} x)" if base else ""
    saved = f"{r['saved'] / 2 ** 30:8.2f}" if r.get("saved") else "       -"
    return (f"{str(r['setting']):>5s} {r['batch']:6d} {r['ms_step']:9.2f}{rel:10s} {r['ms_bwd']:9.2f}{relb:10s} {r['peak'] / 2 ** 30:8.2f} "
            f"{saved} {r['recomputed']:4d}  {r['loss']:.5f}")


HEAD = f"{'rc':>5s} {'batch':>6s} {'ms/step':>9s}{'':10s} {'ms bwd':>9s}{'':10s} {'peak GiB':>8s} {'tape GiB':>8s} {'rbld':>4s}  loss"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recompute.txt"))
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, for the interleaved recompute = 0 rows")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--cases", nargs="+", default=["256:32", "256:256", "512:32"], help="resolution:batch")
    ap.add_argument("--no-max", action="store_true")
    ap.add_argument("--no-lora", action="store_true")
    ap.add_argument("--row", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.row:
        return row(json.loads(a.row))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    try:
        measure(a, say, flush)
    except RowFailed as e:   # after a row that failed nothing else runs: what is in hand is written, the exit status says so
        say(str(e))
        flush()
        sys.exit(1)
    flush()


def measure(a, say, flush):
    say("# tools/time_recompute.py: SiT-XL/2 on one MI355X, bf16, one process per row; ms/step = median wall clock of "
        f"{a.steps} steps after 3, ms bwd = median of {a.steps} event-timed backward() calls; rbld = blocks the last backward rebuilt; "
        "tape GiB = Engine.saved_activation_bytes")
    for case in a.cases:
        res, b = (int(v) for v in case.split(":"))
        say(f"\n== {res}^2 (T = {T_OF[res]}), local batch {b}")
        mine = dict(tree=ROOT, tag="this", resolution=res, batch=b, steps=a.steps)
        zero = []
        if a.parent:
            theirs = dict(mine, tree=os.path.abspath(a.parent), tag="parent", settings=[0])
            par = []
            for _ in range(a.repeats):
                for spec, acc in ((theirs, par), (dict(mine, settings=[0]), zero)):
                    r = spawn(spec, say)
                    if r:
                        acc.append(r["rows"][0])
            say("recompute = 0 against the parent commit, interleaved (parent, this, parent, this, ...)")
            for tag, acc in (("parent", par), ("this", zero)):
                say(f"  {tag:7s} ms/step " + " ".join(f"{r['ms_step']:8.3f}" for r in acc) + "   ms bwd " +
                    " ".join(f"{r['ms_bwd']:8.3f}" for r in acc) + "   peak GiB " + " ".join(f"{r['peak'] / 2 ** 30:.3f}" for r in acc) +
                    "   loss " + " ".join(f"{r['loss']:.5f}" for r in acc))
            if par and zero:
                ms = [statistics.mean(r["ms_step"] for r in acc) for acc in (par, zero)]
                sp = [max(r["ms_step"] for r in acc) / min(r["ms_step"] for r in acc) - 1 for acc in (par, zero)]
                say(f"  mean ms/step {ms[0]:.3f} -> {ms[1]:.3f} ({(ms[1] / ms[0] - 1) * 100:+.2f} %); run-to-run spread (max / min - 1) "
                    f"parent {sp[0] * 100:.2f} %, this {sp[1] * 100:.2f} %")
            flush()
        r = spawn(dict(mine, settings=[0, 14, "all"]), say)
        if r:
            say(HEAD)
            for k, rr in enumerate(r["rows"]):
                say(fmt(rr, r["rows"][0] if k else None))
        flush()
    if not a.no_lora:
        say("\n== LoRA, R = 16 on the four block linears, adapters only (256^2)")
        say(HEAD)
        for b in (32, 256):
            r = spawn(dict(tree=ROOT, tag="this", resolution=256, batch=b, steps=a.steps, settings=[0, "all"], lora=16), say)
            if r:
                for k, rr in enumerate(r["rows"]):
                    say(fmt(rr, r["rows"][0] if k else None))
            flush()
    if not a.no_max:
        say("\n== 512^2 (T = 1024): the largest power-of-two local batch by the closed form")
        say(HEAD)
        for setting in (0, "all"):
            r = spawn(dict(tree=ROOT, tag="this", resolution=512, batch="max", steps=max(3, a.steps // 2), settings=[setting]), say)
            if r:
                say(fmt(r["rows"][0]))
                say(f"      {r['rows'][0]['note']}")
            flush()


if __name__ == "__main__":
    main()
