"""Shared by the tower-precision tests: the frozen towers' forward restated once more with the autocast dtype as a parameter.
oracle.vit_towers.forward and oracle.clip_vit.forward know `autocast_bf16` only; the reference runs its encoders under
accelerator.autocast() with fp16 (its default), bf16 or nothing (image/train.py:351-357), so the fp16 and fp64 references the
precision tests need come from here.  The code is the oracles' line for line (test_tower_precision_cpu.py pins it to them bit for
bit with autocast=torch.bfloat16 and None) plus DINOv2 ViT-g's SwiGLU feed-forward (blocks.{i}.mlp.w12 / w3, as
tests/test_swiglu_gpu.py restates it).  With the parameters and the input cast to double it runs in float64."""
import torch
import torch.nn.functional as F


def to_double(P):
    return {k: (v.double() if torch.is_floating_point(v) else v) for k, v in P.items()}


def _vit(P, cfg, x):
    E, H = cfg["embed"], cfg["heads"]
    hd = E // H
    x = F.conv2d(x, P["patch_embed.proj.weight"], P["patch_embed.proj.bias"], stride=cfg["patch"])
    x = x.flatten(2).transpose(1, 2)
    if cfg["cls"]:
        x = torch.cat((P["cls_token"].expand(x.shape[0], -1, -1), x), dim=1)
    x = x + P["pos_embed"]
    if cfg.get("reg"):   # registers go in behind the class token AFTER the position embedding was added
        x = torch.cat((x[:, :1], P["register_tokens"].expand(x.shape[0], -1, -1), x[:, 1:]), dim=1)
    g = (lambda k: P[k]) if cfg.get("ls") else (lambda k: 1.0)
    for i in range(cfg["depth"]):
        b = f"blocks.{i}."
        h = F.layer_norm(x, (E,), P[b + "norm1.weight"], P[b + "norm1.bias"], 1e-6)
        B, N, _ = h.shape
        qkv = F.linear(h, P[b + "attn.qkv.weight"], P[b + "attn.qkv.bias"]).reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        a = ((q @ k.transpose(-2, -1)) * hd ** -0.5).softmax(dim=-1)
        a = (a @ v).transpose(1, 2).reshape(B, N, E)
        x = x + F.linear(a, P[b + "attn.proj.weight"], P[b + "attn.proj.bias"]) * g(b + "ls1.gamma")
        h = F.layer_norm(x, (E,), P[b + "norm2.weight"], P[b + "norm2.bias"], 1e-6)
        if b + "mlp.w12.weight" in P:   # SwiGLUFFNFused (DINOv2 ViT-g)
            x1, x2 = F.linear(h, P[b + "mlp.w12.weight"], P[b + "mlp.w12.bias"]).chunk(2, dim=-1)
            u = F.silu(x1) * x2
            x = x + F.linear(u, P[b + "mlp.w3.weight"], P[b + "mlp.w3.bias"]) * g(b + "ls2.gamma")
        else:
            u = F.gelu(F.linear(h, P[b + "mlp.fc1.weight"], P[b + "mlp.fc1.bias"]))
            x = x + F.linear(u, P[b + "mlp.fc2.weight"], P[b + "mlp.fc2.bias"]) * g(b + "ls2.gamma")
    if cfg["final_norm"]:
        x = F.layer_norm(x, (E,), P["norm.weight"], P["norm.bias"], 1e-6)
    npre = (1 if cfg["cls"] else 0) + cfg.get("reg", 0)
    return x[:, npre:] if npre else x


def _ln(x, w, b):   # clip_vit.py:159-165: computed in fp32 (fp64 in the double run), returned in the input's dtype
    wide = torch.float64 if x.dtype == torch.float64 else torch.float32
    return F.layer_norm(x.type(wide), (x.shape[-1],), w, b, 1e-5).type(x.dtype)


def _clip(P, cfg, x):
    W, H = cfg["width"], cfg["heads"]
    x = F.conv2d(x, P["conv1.weight"], stride=cfg["patch"])
    x = x.reshape(x.shape[0], x.shape[1], -1).permute(0, 2, 1)
    cls = P["class_embedding"].to(x.dtype) + torch.zeros(x.shape[0], 1, x.shape[-1], dtype=x.dtype)
    x = torch.cat([cls, x], dim=1)
    x = x + P["positional_embedding"].to(x.dtype)
    x = _ln(x, P["ln_pre.weight"], P["ln_pre.bias"])
    x = x.permute(1, 0, 2)
    for i in range(cfg["layers"]):
        b = f"transformer.resblocks.{i}."
        h = _ln(x, P[b + "ln_1.weight"], P[b + "ln_1.bias"])
        a = F.multi_head_attention_forward(
            h, h, h, W, H, P[b + "attn.in_proj_weight"], P[b + "attn.in_proj_bias"], None, None, False, 0.0,
            P[b + "attn.out_proj.weight"], P[b + "attn.out_proj.bias"], training=False, need_weights=False)[0]
        x = x + a
        h = _ln(x, P[b + "ln_2.weight"], P[b + "ln_2.bias"])
        u = F.linear(h, P[b + "mlp.c_fc.weight"], P[b + "mlp.c_fc.bias"])
        u = u * torch.sigmoid(1.702 * u)
        x = x + F.linear(u, P[b + "mlp.c_proj.weight"], P[b + "mlp.c_proj.bias"])
    return x.permute(1, 0, 2)[:, 1:]


@torch.no_grad()
def forward(P, cfg, x, autocast=None):
    """P, cfg as oracle.vit_towers (cfg has 'embed') or oracle.clip_vit (cfg has 'width'); x f32 (or f64 with to_double(P))
    [B,3,S,S]; autocast None | torch.bfloat16 | torch.float16 -> patch tokens without the prefix tokens."""
    if autocast not in (None, torch.bfloat16, torch.float16):
        raise ValueError(f"autocast={autocast!r}")
    with torch.autocast("cpu", dtype=autocast or torch.bfloat16, enabled=autocast is not None):
        return (_clip if "width" in cfg else _vit)(P, cfg, x)


def forward64(P, cfg, x):
    return forward(to_double(P), cfg, x.double(), None)


def gap(a, b, scale):
    """max|a - b| / scale in float64."""
    return (a.double() - b.double()).abs().max().item() / scale


# ---- the small tower cases of the existing encoder tests, with their goldens and the references derived here ------------------
def _vit_kwargs(cfg, ffn="mlp"):
    return dict(embed=cfg["embed"], depth=cfg["depth"], heads=cfg["heads"], patch=cfg["patch"], image=cfg["image"], cls=cfg["cls"],
                final_norm=cfg["final_norm"], layerscale=bool(cfg.get("ls")), registers=cfg.get("reg", 0), ffn=ffn)


def _build_cases():
    from oracle import clip_vit as oclip
    from oracle import detfill
    from oracle import vit_towers as ot
    from tests import swiglu_ref
    from tests.test_encoder_gpu import TOWER_CASES
    c = {}
    for tag, (kw, pos, B) in TOWER_CASES.items():     # test_vit_tower_vs_reference
        cfg = ot.make_config(pos=pos, **kw)
        c[tag] = dict(kind="vit", golden=("towers", tag), cfg=cfg, enc=_vit_kwargs(cfg),
                      params=lambda cfg=cfg: ot.fill_params(cfg, base_seed=9), x=((B, 3, kw["image"], kw["image"]), 55))
    for tag, E, H, depth, image, reg, B in (("plain", 128, 2, 2, 56, 0, 3), ("reg4", 256, 4, 3, 28, 4, 2)):   # test_dinov2_tower_vs_hf_port
        cfg = ot.make_config(E, depth, H, 14, image, True, True, "learned", ls=True, reg=reg)
        c["dinov2." + tag] = dict(kind="vit", golden=("dinov2", tag), cfg=cfg, enc=_vit_kwargs(cfg),
                                  params=lambda cfg=cfg: ot.fill_params(cfg, base_seed=21), x=((B, 3, image, image), 56))
    for tag, cfg, B in (("t2", oclip.make_config(width=128, layers=2, heads=2, patch=14, image=56), 3),    # test_tower_vs_oracle_and_reference
                        ("t3", oclip.make_config(width=256, layers=3, heads=4, patch=14, image=28), 2)):
        c["clip." + tag] = dict(kind="clip", golden=("clip", tag), cfg=cfg, enc=dict(cfg),
                                params=lambda cfg=cfg: oclip.fill_params(cfg, base_seed=5), x=((B, 3, cfg["image"], cfg["image"]), 77))
    for tag, depth, image, reg, B in (("plain", 2, 56, 0, 3), ("reg4", 2, 28, 4, 2)):                       # test_dinov2_g_tower_vs_hf_port
        cfg = ot.make_config(384, depth, 6, 14, image, True, True, "learned", ls=True, reg=reg)
        c["dinov2_g." + tag] = dict(kind="vit", golden=("dinov2_g", tag), cfg=cfg, enc=_vit_kwargs(cfg, "swiglu"),
                                    params=lambda depth=depth, image=image, reg=reg: swiglu_ref.hub_params(384, depth, 6, image, reg),
                                    x=((B, 3, image, image), 64))
    return c


CASE_NAMES = ("jepa80", "jepa64", "mae", "moco", "dinov2.plain", "dinov2.reg4", "clip.t2", "clip.t3", "dinov2_g.plain",
              "dinov2_g.reg4")
_cases, _refs = None, {}


def case(name):
    global _cases
    if _cases is None:
        _cases = _build_cases()
        assert tuple(_cases) == CASE_NAMES
    return _cases[name]


def case_inputs(name):
    from oracle import detfill
    c = case(name)
    return c["params"](), detfill.normal(*c["x"])


def reference(name):
    """Computed once per process and left unchanged: the golden fp32 / bf16 outputs, their gap, and from this file's forward the
    fp16-autocast output's gap to the golden fp32 (g16), the float64 output (o64) and the fp32 output's gap to it (g32).  Every gap
    is a fraction of max|golden fp32|."""
    if name not in _refs:
        from tests.test_oracle_golden import load
        c = case(name)
        P, x = case_inputs(name)
        g = load(c["golden"][0])
        r32, r16 = torch.from_numpy(g[c["golden"][1] + ".fp32"]), torch.from_numpy(g[c["golden"][1] + ".bf16"]).float()
        sc = r32.abs().max().item()
        o64 = forward64(P, c["cfg"], x)
        _refs[name] = dict(golden32=r32, scale=sc, gbf16=gap(r16, r32, sc), g16=gap(forward(P, c["cfg"], x, torch.float16), r32, sc),
                           o64=o64, g32=gap(forward(P, c["cfg"], x), o64, sc))
    return _refs[name]
