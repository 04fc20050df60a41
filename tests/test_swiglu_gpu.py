"""DINOv2 ViT-g on the GPU: reed_gemm's SwiGLU epilogue (17) against torch on every kernel the tower's shapes reach, its argument
checks, the tower against transformers' port of the model (tests/golden/dinov2_g.npz) and against an fp32 restatement at the
real width, and train.py with the tower running every step at 256 and 512."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import detfill
from tests import swiglu_ref

pytestmark = pytest.mark.gpu

NAN = float("nan")
# (M, Hd, K); the GEMM is [M, 2 Hd] wide.  (300, 192, 128): ragged rows over a 128 and a 256 tile, one and a half 256-column tiles;
# (771, 1024, 384): the fixture tower's shape, 3 x 257 rows; (16, 64, 64): one strip (the skinny kernel's unit); (4112, 4096, 1536):
# ViT-g's width, 16 x 257 rows: the ragged-M split (tail rows on the skinny kernel) and the persistent form of the four-wave kernel
SHAPES = [(300, 192, 128), (771, 1024, 384), (16, 64, 64), (4112, 4096, 1536)]
_cases = {}


def _case(dev, M, Hd, K):
    """Inputs and the torch reference (from the UNPACKED weight) of one shape, computed once: x ~ N(0, 1), w ~ N(0, 1 / K),
    b ~ N(0, 1), so the outputs are O(1)."""
    from reed_amd import ops
    key = (M, Hd, K)
    if key not in _cases:
        g = torch.Generator().manual_seed(M + Hd + K)
        x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
        w12 = (torch.randn(2 * Hd, K, generator=g) / K ** 0.5).to(torch.bfloat16).to(dev)
        b12 = torch.randn(2 * Hd, generator=g).to(torch.bfloat16).to(dev)
        pw, pb = ops.swiglu_pack(w12, b12)
        _cases[key] = dict(x=x, pw=pw, pb=pb, ref={True: swiglu_ref.swiglu_epilogue_ref(x, w12, b12).float(),
                                                   False: swiglu_ref.swiglu_epilogue_ref(x, w12, None).float()})
    return _cases[key]


def _run(c, M, Hd, K, bias, tile=0, out=None):
    from reed_amd import ops
    if out is None:
        out = torch.full((M, Hd), NAN, dtype=torch.bfloat16, device=c["x"].device)
    with ops.forced_tile(tile):
        ops.gemm(ops.NT, ops.EPI_SWIGLU, c["x"], c["pw"], M, 2 * Hd, K, out, K, K, out.stride(0), bias=c["pb"] if bias else None)
        torch.cuda.synchronize()
    return out


def _check(out, ref, what, atol=2e-2):
    """Element bar: the two-rounding activation epilogues' (test_quickgelu_and_residual_epilogues) — a bf16 rounding of x1 or x2
    flipped by the accumulation order moves the product by at most ~3 bf16 ulps.  Mean bar (the LayerScale test's): a systematic
    mispairing of O(1) values cannot hide under it."""
    o = out.float()
    err, mean = (o - ref).abs().max().item(), (o - ref).abs().mean().item()
    print(f"swiglu {what}: max|HIP - torch| {err:.3e}, mean {mean:.3e}, max|ref| {ref.abs().max().item():.2f}")
    torch.testing.assert_close(o, ref, atol=atol, rtol=2e-2)
    assert mean < 2e-3, mean


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("M,Hd,K", SHAPES)
def test_swiglu_epilogue_vs_torch(dev, M, Hd, K, bias):
    c = _case(dev, M, Hd, K)
    _check(_run(c, M, Hd, K, bias), c["ref"][bias], f"{(M, Hd, K)} bias={bias}")


@pytest.mark.parametrize("M,Hd,K,tiles", [(*SHAPES[0], (0, 128, 256, 257, 258)), (*SHAPES[1], (0, 128, 256, 257, 258)),
                                          (*SHAPES[3], (0, 257, 258))])
def test_swiglu_tile_choice_is_invisible(dev, M, Hd, K, tiles):
    """The 128^2 kernel, the eight-wave and the four-wave 256^2 kernel (one-shot and persistent) and the dispatcher's own choice
    form every element from the same products in the same order: bit-identical outputs.  The skinny one-wave kernel (tile 64) is
    held to the reference at the bar the ragged-M split's test holds the exact-GELU epilogue to."""
    c = _case(dev, M, Hd, K)
    outs = {t: _run(c, M, Hd, K, True, tile=t) for t in tiles}
    for t in tiles:
        _check(outs[t], c["ref"][True], f"{(M, Hd, K)} tile {t}")
    for t in tiles[1:]:
        ne = outs[t] != outs[tiles[0]]
        assert not ne.any(), (t, int(ne.sum()), ne.nonzero()[:4].tolist())
    if M <= 1024:
        _check(_run(c, M, Hd, K, True, tile=64), c["ref"][True], f"{(M, Hd, K)} tile 64", atol=4e-2)


@pytest.mark.parametrize("tile", [0, 128, 256, 257, 64])
@pytest.mark.parametrize("M,Hd,K", SHAPES[:3])
def test_swiglu_writes_only_its_half_width_output(dev, M, Hd, K, tile):
    """C has N / 2 columns at row stride ldc = Hd + 64, in a NaN-filled buffer with 8 spare rows: nothing lands past row M - 1 or
    past column Hd - 1."""
    c = _case(dev, M, Hd, K)
    buf = torch.full((M + 8, Hd + 64), NAN, dtype=torch.bfloat16, device=dev)
    _run(c, M, Hd, K, True, tile=tile, out=buf)
    assert torch.isnan(buf[M:].float()).all() and torch.isnan(buf[:, Hd:].float()).all()
    _check(buf[:M, :Hd], c["ref"][True], f"{(M, Hd, K)} ldc {Hd + 64} tile {tile}", atol=4e-2 if tile == 64 else 2e-2)


def test_swiglu_argument_checks(dev):
    """Each refused call raises with the library's message and launches nothing (the NaN-filled output stays as it was)."""
    from reed_amd import ops
    M, Hd, K = 64, 128, 128
    x = torch.randn(M, K, device=dev).to(torch.bfloat16)
    w = torch.randn(2 * Hd, K, device=dev).to(torch.bfloat16)
    out = torch.full((M, 2 * Hd), NAN, dtype=torch.bfloat16, device=dev)
    bad = {"NN layout": lambda: ops.gemm(ops.NN, ops.EPI_SWIGLU, x, w, M, 2 * Hd, K, out, K, 2 * Hd, Hd),
           "split_k = 2": lambda: ops.gemm(ops.NT, ops.EPI_SWIGLU, x, w, M, 2 * Hd, K, out, K, K, Hd, split_k=2),
           "ldc < Hd": lambda: ops.gemm(ops.NT, ops.EPI_SWIGLU, x, w, M, 2 * Hd, K, out, K, K, Hd - 8),
           "N = 192": lambda: ops.gemm(ops.NT, ops.EPI_SWIGLU, x, w, M, 192, K, out, K, K, 96)}
    for what, call in bad.items():
        with pytest.raises(RuntimeError, match="SwiGLU epilogue"):
            call()
        torch.cuda.synchronize()
        assert torch.isnan(out.float()).all(), what
    # the fp32-operand build does not carry the epilogue (the towers run on the bf16 library)
    x32, w32, o32 = x.float(), w.float(), torch.full((M, Hd), NAN, device=dev)
    prev = ops.use("fp32")
    try:
        with pytest.raises(RuntimeError, match="fp32-operand build"):
            ops.gemm(ops.NT, ops.EPI_SWIGLU, x32, w32, M, 2 * Hd, K, o32, K, K, Hd)
    finally:
        ops.use(prev)
    torch.cuda.synchronize()
    assert torch.isnan(o32).all()
    # and the accepted call runs
    ops.gemm(ops.NT, ops.EPI_SWIGLU, x, w, M, 2 * Hd, K, out, K, K, 2 * Hd)
    torch.cuda.synchronize()
    assert torch.isfinite(out[:, :Hd].float()).all() and torch.isnan(out[:, Hd:].float()).all()


def test_swiglu_fp16_build(dev):
    """The IEEE-half build compiles the same sources and carries the epilogue."""
    from reed_amd import ops
    M, Hd, K = 300, 192, 128
    g = torch.Generator().manual_seed(9)
    x = torch.randn(M, K, generator=g).half().to(dev)
    w12 = (torch.randn(2 * Hd, K, generator=g) / K ** 0.5).half().to(dev)
    b12 = torch.randn(2 * Hd, generator=g).half().to(dev)
    pw, pb = ops.swiglu_pack(w12, b12)
    out = torch.full((M, Hd), NAN, dtype=torch.float16, device=dev)
    prev = ops.use("fp16")
    try:
        ops.gemm(ops.NT, ops.EPI_SWIGLU, x, pw, M, 2 * Hd, K, out, K, K, Hd, bias=pb)
        torch.cuda.synchronize()
    finally:
        ops.use(prev)
    x12 = (x.float() @ w12.float().t() + b12.float()).half().float()
    ref = ((x12[:, :Hd] * torch.sigmoid(x12[:, :Hd])).half().float() * x12[:, Hd:]).half().float()
    torch.testing.assert_close(out.float(), ref, atol=4e-3, rtol=4e-3)   # ~3 ulps of half (2^-11) of an O(1) product


# ---- the tower --------------------------------------------------------------------------------------------------------------
def _bar(out, ref32, ref16, what):
    """The existing DINOv2 bar (test_dinov2_tower_vs_hf_port)."""
    assert out.shape == ref32.shape, (out.shape, ref32.shape)
    sc = ref32.abs().max().item()
    e32, eref = (out - ref32).abs().max().item() / sc, (ref16 - ref32).abs().max().item() / sc
    c32 = F.cosine_similarity(out.flatten(), ref32.flatten(), dim=0).item()
    print(f"dinov2-g {what}: max|HIP - fp32| {e32:.2e} (the reference's own bf16-vs-fp32 {eref:.2e}) of the output range; cosine {c32:.6f}")
    assert e32 <= 2.0 * eref + 2e-3 and c32 > 0.9998


@pytest.mark.parametrize("tag,depth,image,reg,B", [("plain", 2, 56, 0, 3), ("reg4", 2, 28, 4, 2)])
def test_dinov2_g_tower_vs_hf_port(dev, tag, depth, image, reg, B):
    """Width 384 (Hd 1024) with the SwiGLU feed-forward, hub parameter names, against transformers' Dinov2Model /
    Dinov2WithRegistersModel built with use_swiglu_ffn=True (tools/gen_golden.py: g_dinov2_g)."""
    from reed_amd.encoders import VitEncoder
    from tests.test_oracle_golden import load
    g = load("dinov2_g")
    P = swiglu_ref.hub_params(384, depth, 6, image, reg)
    P["mask_token"] = torch.zeros(1, 384)
    enc = VitEncoder(embed=384, depth=depth, heads=6, patch=14, image=image, cls=True, final_norm=True, layerscale=True,
                     registers=reg, ffn="swiglu")
    missing, unexpected = enc.load_state_dict(P)
    assert not missing and not unexpected
    enc = enc.to(dev).eval()
    out = enc(detfill.normal((B, 3, image, image), 64).to(dev)).float().cpu()
    _bar(out, torch.from_numpy(g[tag + ".fp32"]), torch.from_numpy(g[tag + ".bf16"]), tag)


def test_dinov2_g_tower_448_vs_hf_port(dev, tmp_path, monkeypatch):
    """The --resolution 512 path: load_vit_encoder(resolution=512) builds the 448-pixel tower (T = 1029) from a hub-layout
    checkpoint, resampling its 37 x 37 table."""
    from reed_amd import encoders
    from tests.test_oracle_golden import load
    g = load("dinov2_g")
    key = "dinov2reg-vit-g"
    monkeypatch.setitem(encoders.VIT_TOWERS, key, dict(encoders.VIT_TOWERS[key], embed=384, heads=6, depth=1))
    P = swiglu_ref.hub_params(384, 1, 6, 448, 4)
    P["pos_embed"] = detfill.normal((1, 1 + 37 * 37, 384), 63) * 0.5
    P["mask_token"] = torch.zeros(1, 384)
    path = str(tmp_path / "hub.pth")
    torch.save(P, path)
    enc = encoders.load_vit_encoder(key, path, dev, resolution=512)      # raises on a missing key
    assert set(enc.state_dict()) == set(P) - {"mask_token"}              # nothing unexpected
    assert enc.image == 448 and enc.tokens == 1029 and enc.ffn_hidden == 1024
    out = enc(detfill.normal((1, 3, 448, 448), 64).to(dev)).float().cpu()[:, ::8]
    _bar(out, torch.from_numpy(g["p448.fp32"]), torch.from_numpy(g["p448.bf16"]), "p448")


def _tower_ref(P, x, heads, reg, depth, autocast):
    """The published model restated in torch (DinoVisionTransformer.forward_features with SwiGLUFFNFused blocks) -> patch tokens."""
    E = P["cls_token"].shape[-1]
    hd = E // heads
    with torch.autocast(x.device.type, dtype=torch.bfloat16, enabled=autocast):
        x = F.conv2d(x, P["patch_embed.proj.weight"], P["patch_embed.proj.bias"], stride=14).flatten(2).transpose(1, 2)
        x = torch.cat((P["cls_token"].expand(x.shape[0], -1, -1), x), dim=1) + P["pos_embed"]
        if reg:
            x = torch.cat((x[:, :1], P["register_tokens"].expand(x.shape[0], -1, -1), x[:, 1:]), dim=1)
        for i in range(depth):
            b = f"blocks.{i}."
            h = F.layer_norm(x, (E,), P[b + "norm1.weight"], P[b + "norm1.bias"], 1e-6)
            B, N, _ = h.shape
            qkv = F.linear(h, P[b + "attn.qkv.weight"], P[b + "attn.qkv.bias"]).reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
            a = ((qkv[0] @ qkv[1].transpose(-2, -1)) * hd ** -0.5).softmax(dim=-1)
            a = (a @ qkv[2]).transpose(1, 2).reshape(B, N, E)
            x = x + F.linear(a, P[b + "attn.proj.weight"], P[b + "attn.proj.bias"]) * P[b + "ls1.gamma"]
            h = F.layer_norm(x, (E,), P[b + "norm2.weight"], P[b + "norm2.bias"], 1e-6)
            x1, x2 = F.linear(h, P[b + "mlp.w12.weight"], P[b + "mlp.w12.bias"]).chunk(2, dim=-1)
            x = x + F.linear(F.silu(x1) * x2, P[b + "mlp.w3.weight"], P[b + "mlp.w3.bias"]) * P[b + "ls2.gamma"]
        x = F.layer_norm(x, (E,), P["norm.weight"], P["norm.bias"], 1e-6)
        return x[:, 1 + reg:].float()


@pytest.fixture(scope="module")
def vitg_block():
    """One block of the true ViT-g configuration under the hub's names (37 x 37 pos_embed, mask_token, 4 register tokens)."""
    from reed_amd.encoders import VIT_TOWERS, VitEncoder
    shapes = {k: v.shape for k, v in VitEncoder(**dict(VIT_TOWERS["dinov2reg-vit-g"], depth=1)).state_dict().items()}
    g = torch.Generator().manual_seed(11)
    P = {}
    for k, s in shapes.items():
        if k.endswith("gamma"):
            P[k] = 0.1 + torch.rand(s, generator=g)
        elif "norm" in k and k.endswith("weight"):
            P[k] = 1.0 + 0.1 * torch.randn(s, generator=g)
        elif k.endswith("weight"):
            P[k] = torch.randn(s, generator=g) * (s.numel() // s[0]) ** -0.5
        else:
            P[k] = torch.randn(s, generator=g) * 0.02
    P["pos_embed"] = torch.randn(1, 1 + 37 * 37, 1536, generator=g) * 0.02
    P["mask_token"] = torch.zeros(1, 1536)
    return P


def _save(P, path, reg):
    torch.save({k: v for k, v in P.items() if reg or k != "register_tokens"}, path)
    return path


def test_vit_g_block_at_the_real_width(dev, tmp_path, monkeypatch, vitg_block):
    """E 1536, 24 heads, Hd 4096, T 257, B 2 through the loader (16 x 16 table resampled from the hub's) against the fp32
    restatement; eref = the restatement's own gap under torch.autocast."""
    from reed_amd import encoders
    key = "dinov2-vit-g"
    monkeypatch.setitem(encoders.VIT_TOWERS, key, dict(encoders.VIT_TOWERS[key], depth=1))
    enc = encoders.load_vit_encoder(key, _save(vitg_block, str(tmp_path / "g.pth"), False), dev)
    assert enc.embed == 1536 and enc.heads == 24 and enc.ffn_hidden == 4096 and enc.tokens == 257 and enc.depth == 1
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(12)).to(dev)
    out = enc(x).float()
    assert out.shape == (2, 256, 1536)
    P = {k: v.to(dev) for k, v in vitg_block.items()}
    P["pos_embed"] = enc.pos_embed.detach().float()
    ref32, ref16 = _tower_ref(P, x, 24, 0, 1, False), _tower_ref(P, x, 24, 0, 1, True)
    _bar(out.cpu(), ref32.cpu(), ref16.cpu(), "real width")


def _folder_dataset(root, res, n=4):
    import PIL.Image
    (root / "images" / "00000").mkdir(parents=True)
    (root / "vae-sd" / "00000").mkdir(parents=True)
    rng = np.random.default_rng(1)
    labels = []
    for i in range(n):
        PIL.Image.fromarray(rng.integers(0, 256, (res, res, 3), dtype=np.uint8)).save(root / "images" / "00000" / f"img{i:08d}.png")
        mom = np.concatenate([rng.standard_normal((4, res // 8, res // 8)) * 5.0, np.full((4, res // 8, res // 8), 0.5)])
        np.save(root / "vae-sd" / "00000" / f"img-mean-std-{i:08d}.npy", mom.astype(np.float32))
        labels.append([f"00000/img-mean-std-{i:08d}.npy", int(i % 3)])
    json.dump({"labels": labels}, open(root / "vae-sd" / "dataset.json", "w"))


@pytest.mark.parametrize("res,key", [(256, "dinov2-vit-g"), (512, "dinov2reg-vit-g")])
def test_train_cli_with_on_device_vit_g(dev, tmp_path, monkeypatch, vitg_block, res, key):
    """train.py --enc-type dinov2[reg]-vit-g --encoder-ckpts <hub checkpoint>: one block of the real width runs every step on the
    raw images (224 px at --resolution 256, 448 px / T = 1029 at 512) and the SiT projector aligns to its 1536-wide tokens."""
    from reed_amd import encoders, train
    data = tmp_path / "data"
    _folder_dataset(data, res)
    monkeypatch.setitem(encoders.VIT_TOWERS, key, dict(encoders.VIT_TOWERS[key], depth=1))
    ck = _save(vitg_block, str(tmp_path / "dinov2_vitg14.pth"), key.startswith("dinov2reg"))
    a = train.parse_args(["--exp-name", "g", "--model", "SiT-S/2", "--resolution", str(res), "--output-dir", str(tmp_path / "exps"),
                          "--data-dir", str(data), "--enc-type", key, "--encoder-ckpts", ck, "--mixed-precision", "bf16",
                          "--batch-size", "4", "--num-workers", "0", "--diffusion-warm-up-steps", "0", "--report-to", "none",
                          "--max-train-steps", "2", "--num-classes", "3", "--checkpointing-steps", "2"])
    try:
        d = train.main(a)
    finally:
        torch.set_grad_enabled(True)
    logs = [json.loads(l) for l in open(os.path.join(d, "metrics.jsonl"))]
    assert len(logs) == 2 and all(np.isfinite(r["proj_loss"]) and np.isfinite(r["training_denoising_loss"]) for r in logs)
    assert logs[0]["img_proj_loss"] != 0.0
    sd = torch.load(os.path.join(d, "checkpoints", "0000002.pt"), map_location="cpu", weights_only=False)["model"]
    last = max(int(k.split(".")[2]) for k in sd if k.startswith("projectors.0.") and k.endswith(".weight"))
    assert sd[f"projectors.0.{last}.weight"].shape[0] == 1536
