"""Shared by tools/gen_golden.py (g_dinov2_g) and the SwiGLU tests: the deterministic fill of a DINOv2 tower whose feed-forward is
the hub's SwiGLUFFNFused (blocks.{i}.mlp.w12 / mlp.w3 in place of fc1 / fc2), under the hub's parameter names, and the epilogue's
arithmetic restated in torch with its three bf16 roundings written out."""
import torch

from oracle import detfill
from oracle import vit_towers as ot

SEED_W12, SEED_B12, SEED_W3, SEED_B3 = 7101, 7102, 7103, 7104


def swiglu_hidden(embed):
    """dinov2/layers/swiglu_ffn.py SwiGLUFFNFused with mlp_ratio 4: (int(4 E * 2 / 3) + 7) // 8 * 8."""
    return (int(int(4 * embed) * 2 / 3) + 7) // 8 * 8


def swiglu_fill(embed, block, hidden=None):
    """The four SwiGLU tensors of block `block`: N(0, 1) * fan_in ** -0.5 weights, N(0, 1) * 0.02 biases, fixed seeds."""
    Hd = hidden or swiglu_hidden(embed)
    b = f"blocks.{block}.mlp."
    s = 16 * block
    return {b + "w12.weight": detfill.normal((2 * Hd, embed), SEED_W12 + s) * embed ** -0.5,
            b + "w12.bias": detfill.normal((2 * Hd,), SEED_B12 + s) * 0.02,
            b + "w3.weight": detfill.normal((embed, Hd), SEED_W3 + s) * Hd ** -0.5,
            b + "w3.bias": detfill.normal((embed,), SEED_B3 + s) * 0.02}


def hub_params(embed, depth, heads, image, reg, base_seed=21):
    """Hub-named state dict of a SwiGLU DINOv2 tower: everything but the feed-forward from oracle.vit_towers.fill_params."""
    P = ot.fill_params(ot.make_config(embed, depth, heads, 14, image, True, True, "learned", ls=True, reg=reg), base_seed=base_seed)
    P = {k: v for k, v in P.items() if ".mlp.fc" not in k}
    for i in range(depth):
        P.update(swiglu_fill(embed, i))
    return P


def swiglu_epilogue_ref(x, w12, b12):
    """x bf16 [M, K], w12 bf16 [2 Hd, K] (UNPACKED: rows [0, Hd) = x1), b12 bf16 [2 Hd] or None -> bf16 [M, Hd]: eager bf16-autocast
    arithmetic with fp32 accumulation: x12 = bf16(acc + bias); h = bf16(float(bf16(silu(float(x1)))) * float(x2))."""
    acc = x.float() @ w12.float().t()
    if b12 is not None:
        acc = acc + b12.float()
    x12 = acc.to(torch.bfloat16)
    Hd = w12.shape[0] // 2
    x1, x2 = x12[:, :Hd].float(), x12[:, Hd:].float()
    s = (x1 * torch.sigmoid(x1)).to(torch.bfloat16)
    return (s.float() * x2).to(torch.bfloat16)
