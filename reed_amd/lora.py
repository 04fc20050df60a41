"""LoRA fine-tuning of reed_amd.SiT: low-rank adapters on the four linears of every block.

    SiT(..., lora_rank=R, lora_alpha=ALPHA, lora_targets=("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2"))

Each adapted linear blocks.{i}.{lin} gains lora_A [R, k_in] and lora_B [n_out, R] in the parameter arena, right behind its bias;
its effective weight is W' = W + (ALPHA / R) B A.  The model has no nn.Linear to wrap and its GEMMs are hand-written, so the
adapters are MERGED into the operand copies the kernels read: wherever the arena refreshes its 16-bit (or fp32) shadow, the shadow
of an adapted weight becomes r(W') (arena.ParamArena.merge_lora -> csrc/lora.hip: reed_lora_merge, from the fp32 masters), and
the transposed and MX-fp8 copies follow by their own mechanism.  The forward, the input gradients, the samplers, fp8 sampling and
the EMA copy therefore run the kernels they always ran: inference costs nothing extra.  (A merged forward cannot carry LoRA
dropout; none is offered.)  The backward takes the adapters' gradients from the (dy, x) pair of the linear
(Engine._lin_grads -> Engine._lora_grads -> reed_lora_grads), beside the base weight's gradient or — the usual case, the base frozen — instead of it.

This module: the configuration check, the adapter file, the merged export, and

    python -m reed_amd.lora merge CKPT OUT      a checkpoint {"model", "ema", "args", "steps"} with W' in place of W, no adapter
                                                keys and no lora_* args: generate.py --ckpt OUT and the reference load it unchanged
    python -m reed_amd.lora extract CKPT OUT    the adapters alone (a few MB): load_adapter() puts them on a base model
"""
import argparse
import copy
import sys

import torch

TARGETS = ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2")
RANKS = (8, 16, 32, 64)
SUFFIXES = (".lora_A", ".lora_B")


def check_config(rank, alpha=None, targets=None):
    """(rank, alpha, targets) as the model keeps them; rank None / 0 = no adapters: (0, None, ())."""
    if not rank:
        if alpha is not None or targets:
            raise ValueError("lora_alpha / lora_targets without lora_rank")
        return 0, None, ()
    rank = int(rank)
    if rank not in RANKS:
        raise ValueError(f"lora_rank={rank}: one of {RANKS}")
    alpha = float(rank if alpha is None else alpha)
    targets = tuple(TARGETS if targets is None else targets)
    bad = [t for t in targets if t not in TARGETS]
    if bad or not targets or len(set(targets)) != len(targets):
        raise ValueError(f"lora_targets={list(targets)}: a non-empty subset of {TARGETS}")
    return rank, alpha, tuple(t for t in TARGETS if t in targets)


def is_adapter_key(name):
    return name.endswith(SUFFIXES)


def adapter_state_dict(model):
    """{name: tensor} of the adapters alone (clones, on the model's device)."""
    if not getattr(model, "lora_rank", 0):
        raise ValueError("the model has no adapters (lora_rank unset)")
    return {k: v.detach().clone() for k, v in model.state_dict().items() if is_adapter_key(k)}


@torch.no_grad()
def load_adapter(model, sd):
    """Copy the adapters of `sd` (adapter_state_dict's layout) into the model: exactly the model's adapter keys, same shapes."""
    own = {k: v for k, v in model.named_parameters() if is_adapter_key(k)}
    if not own:
        raise ValueError("the model has no adapters (lora_rank unset)")
    missing, extra = sorted(set(own) - set(sd)), sorted(set(sd) - set(own))
    if missing or extra:
        raise KeyError(f"load_adapter: missing {missing[:3]}{'...' if len(missing) > 3 else ''}, "
                       f"unexpected {extra[:3]}{'...' if len(extra) > 3 else ''}")
    model._arena.wait_all()
    for k, p in own.items():
        if tuple(sd[k].shape) != tuple(p.shape):
            raise ValueError(f"load_adapter: {k} has shape {tuple(sd[k].shape)}, the model's is {tuple(p.shape)}")
        p.copy_(sd[k])
    model._arena.shadow_version = -1   # merged again at the next forward


@torch.no_grad()
def merge_state_dict(sd, scale, device=None):
    """A state dict with adapter keys -> the reference-layout keys only, every adapted weight as W' = W + scale B A in fp32,
    formed on the GPU by the merge kernel's fp32 output (the very arithmetic behind the shadows the model computes with)."""
    from . import ops
    out = {}
    for k, v in sd.items():
        if is_adapter_key(k):
            continue
        base = k[:-len(".weight")] if k.endswith(".weight") else None
        if base is None or base + ".lora_A" not in sd:
            out[k] = v.detach().clone()
            continue
        dev = torch.device(device) if device is not None else v.device
        if dev.type != "cuda":
            raise RuntimeError("reed_amd.lora: the merge runs on the GPU (reed_lora_merge); pass device='cuda'")
        w = v.detach().to(dev, torch.float32).contiguous()
        a = sd[base + ".lora_A"].detach().to(dev, torch.float32).contiguous()
        b = sd[base + ".lora_B"].detach().to(dev, torch.float32).contiguous()
        w32 = torch.empty_like(w)
        with torch.cuda.device(dev):
            ops.lora_merge(w, a, b, scale, None, w32, w.shape[0], w.shape[1], a.shape[0])
        out[k] = w32.to(v.device)
    return out


def merged_state_dict(model):
    """The model as a plain SiT's state dict: reference-layout keys only, W' in fp32."""
    if not getattr(model, "lora_rank", 0):
        raise ValueError("the model has no adapters (lora_rank unset)")
    return merge_state_dict(model.state_dict(), model.lora_alpha / model.lora_rank)


def _scale_of(args):
    rank = getattr(args, "lora_rank", 0)
    if not rank:
        raise ValueError("the checkpoint was not trained with --lora-rank (no lora_rank in its args)")
    alpha = getattr(args, "lora_alpha", None)
    return (float(alpha) if alpha is not None else float(rank)) / rank


def merge_checkpoint(src, dst, device="cuda"):
    ckpt = torch.load(src, map_location="cpu", weights_only=False)
    scale = _scale_of(ckpt["args"])
    args = copy.copy(ckpt["args"])
    for k in [k for k in vars(args) if k.startswith("lora_")]:
        delattr(args, k)
    out = {"model": merge_state_dict(ckpt["model"], scale, device), "ema": merge_state_dict(ckpt["ema"], scale, device),
           "args": args, "steps": ckpt.get("steps", 0)}
    torch.save(out, dst)
    return out


def extract_checkpoint(src, dst):
    ckpt = torch.load(src, map_location="cpu", weights_only=False)
    a = ckpt["args"]
    _scale_of(a)
    out = {"adapter": {k: v for k, v in ckpt["model"].items() if is_adapter_key(k)},
           "ema_adapter": {k: v for k, v in ckpt["ema"].items() if is_adapter_key(k)},
           "lora_rank": a.lora_rank, "lora_alpha": getattr(a, "lora_alpha", None) or float(a.lora_rank),
           "lora_targets": list(getattr(a, "lora_targets", None) or TARGETS), "steps": ckpt.get("steps", 0)}
    torch.save(out, dst)
    return out


def main(argv=None):
    p = argparse.ArgumentParser(prog="python -m reed_amd.lora", description=__doc__.split("\n")[0])
    sub = p.add_subparsers(dest="cmd", required=True)
    for name, text in (("merge", "write a checkpoint with the adapters merged into the weights"),
                       ("extract", "write the adapters alone")):
        s = sub.add_parser(name, help=text)
        s.add_argument("ckpt")
        s.add_argument("out")
    a = p.parse_args(argv)
    if a.cmd == "merge":
        out = merge_checkpoint(a.ckpt, a.out)
        print(f"[reed_amd.lora] merged {a.ckpt} -> {a.out}: {len(out['model'])} keys, step {out['steps']}")
    else:
        out = extract_checkpoint(a.ckpt, a.out)
        n = sum(v.numel() for v in out["adapter"].values())
        print(f"[reed_amd.lora] adapters of {a.ckpt} -> {a.out}: {len(out['adapter'])} tensors, {n:,} elements")
    return 0


if __name__ == "__main__":
    sys.exit(main())
