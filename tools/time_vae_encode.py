"""SD-VAE encode rate (`python -m reed_amd.dataset encode`): the HIP path of reed_amd/vae.py:SDVAEEncoder.encode per operand type
against the same module on torch's operators (MIOpen convolutions, fp32), published sd-vae-ft configuration, random weights, uint8
images at 256^2 (-> [8, 32, 32]) and 512^2 (-> [8, 64, 64], T = 4096 in the mid-block attention).  Device events around `reps`
calls after one warm-up call per form.  FLOP per image: the unpadded contractions (every convolution and Linear, the two attention
products), counted from the module's shapes.
usage (GPU box): python tools/time_vae_encode.py [--batch 8] [--reps 3] [--resolutions 256,512]"""
import argparse
import sys

import torch
import torch.nn as nn

sys.path.insert(0, ".")
from reed_amd import vae as rvae  # noqa: E402


def flop_per_image(enc, res):
    """2 * MACs of every Conv2d / Linear on a meta-device forward, plus the attention's Q K^T and P V"""
    meta = rvae.SDVAEEncoder().to("meta")
    total = [0]

    def hook(m, inp, out):
        if isinstance(m, nn.Conv2d):
            total[0] += 2 * out.numel() * m.in_channels * m.kernel_size[0] * m.kernel_size[1]
        else:
            total[0] += 2 * out.numel() * m.in_features

    for m in meta.modules():
        if isinstance(m, (nn.Conv2d, nn.Linear)):
            m.register_forward_hook(hook)
    meta.encode_torch(torch.empty(1, 3, res, res, device="meta"))
    c = enc.encoder.mid_block.attentions[0].to_q.in_features
    T = (res // 8) ** 2
    return total[0] + 2 * 2 * T * T * c


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--resolutions", default="256,512")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    enc = rvae.SDVAEEncoder()
    for p in enc.parameters():
        p.data.normal_(0, 0.02)
    enc = enc.to(dev)
    print(f"{torch.cuda.get_device_name(0)}, batch {a.batch}, {a.reps} timed calls per form")
    for res in [int(r) for r in a.resolutions.split(",")]:
        flop = flop_per_image(enc, res)
        raw = torch.randint(0, 256, (a.batch, 3, res, res), dtype=torch.uint8, device=dev)
        print(f"{res}^2 -> [8, {res // 8}, {res // 8}]: {flop / 1e9:.1f} GFLOP per image (unpadded contractions)")
        for prec in ("fp32", "tf32", "fp16", "bf16"):
            t = timed(lambda: enc.encode(raw, precision=prec), a.reps)
            print(f"  HIP {prec}: {t * 1e3 / a.batch:8.2f} ms / image, {a.batch / t:8.1f} images/s, {flop * a.batch / t / 1e12:7.1f} TFLOP/s")
        x = raw.float() / 127.5 - 1
        with torch.no_grad():
            t = timed(lambda: enc.encode_torch(x), a.reps)
        print(f"  torch operators (MIOpen), fp32: {t * 1e3 / a.batch:8.2f} ms / image, {a.batch / t:8.1f} images/s")


if __name__ == "__main__":
    main()
