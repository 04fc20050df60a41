"""The DINOv2 towers at --resolution 512 on the GPU: the attention forward past 512 keys with a <= 16-row query tail
(attn_fwd_kernel<64, true>: T = 1025 / 1029 at 448 px), the 448-pixel towers against transformers' port of the hub model
(tests/golden/dinov2_512.npz), and train.py at 512 with the DINOv2 tower running every step."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import detfill

pytestmark = pytest.mark.gpu


# 1025 / 1029: the DINOv2 towers at 448 px; 513: the first length past the row kernel's 512 keys; 1040: a 16-row tail; 2049,
# 4112: more key tiles, and a tail at the upper end; (32, 1025, 16): more (batch, head) items than CUs
@pytest.mark.parametrize("B,T,H", [(2, 513, 3), (2, 1025, 4), (3, 1029, 2), (2, 1040, 3), (1, 2049, 2), (1, 4112, 2),
                                   (32, 1025, 16)])
def test_attention_fwd_tail_past_512(dev, B, T, H):
    from reed_amd import ops
    from tests.test_attention_gpu import _ref
    hd = 64
    g = torch.Generator().manual_seed(B * T + H)
    qkv = (torch.randn(B, T, 3, H, hd, generator=g) * 1.5).to(torch.bfloat16).to(dev)
    o = torch.full((B, T, H * hd), float("nan"), dtype=torch.bfloat16, device=dev)
    lse = torch.full((B, H, T), float("nan"), device=dev)
    ops.attention_fwd(qkv, o, lse, B, T, H, hd)
    ro, rl = _ref(qkv, B, T, H, hd)
    torch.testing.assert_close(lse, rl, atol=2e-3, rtol=1e-4)
    torch.testing.assert_close(o.float(), ro, atol=2e-2, rtol=2e-2)
    tail = T % 256
    torch.testing.assert_close(o[:, T - tail:].float(), ro[:, T - tail:], atol=2e-2, rtol=2e-2)
    o2 = torch.full_like(o, float("nan"))
    lse2 = torch.full_like(lse, float("nan"))
    ops.attention_fwd(qkv, o2, lse2, B, T, H, hd)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    o3 = torch.full_like(o, float("nan"))
    ops.attention_fwd(qkv, o3, None, B, T, H, hd)
    assert torch.equal(o, o3)


def _hub_tower(E, H, depth, reg, seed_pos):
    """oracle parameters under the hub's names with the hub's 37 x 37 pos_embed (the fixture's table, before resampling)."""
    from oracle import vit_towers as ot
    P = ot.fill_params(ot.make_config(E, depth, H, 14, 448, True, True, "learned", ls=True, reg=reg), base_seed=21)
    P["pos_embed"] = detfill.normal((1, 1 + 37 * 37, E), seed_pos) * 0.5
    P["mask_token"] = torch.zeros(1, E)
    return P


@pytest.mark.parametrize("tag,E,H,reg,step", [("plain", 128, 2, 0, 8), ("reg4", 256, 4, 4, 16)])
def test_dinov2_tower_448_vs_hf_port(dev, tmp_path, monkeypatch, tag, E, H, reg, step):
    """VitEncoder(image=448) built by load_vit_encoder(resolution=512) from a hub-layout checkpoint (the 37 x 37 table resampled
    at load) against transformers' Dinov2Model / Dinov2WithRegistersModel at image_size 448, with the bars of
    test_dinov2_tower_vs_hf_port."""
    from reed_amd import encoders
    from tests.test_oracle_golden import load
    g = load("dinov2_512")
    key = "dinov2reg-vit-b" if reg else "dinov2-vit-b"
    monkeypatch.setitem(encoders.VIT_TOWERS, key, dict(encoders.VIT_TOWERS[key], embed=E, heads=H, depth=2))
    path = str(tmp_path / "hub.pth")
    torch.save(_hub_tower(E, H, 2, reg, 58 + reg), path)
    enc = encoders.load_vit_encoder(key, path, dev, resolution=512)
    assert enc.image == 448 and enc.tokens == 1025 + reg
    x = detfill.normal((2, 3, 448, 448), 59)
    out = enc(x.to(dev)).float().cpu()[:, ::step]
    ref32, ref16 = torch.from_numpy(g[tag + ".fp32"]), torch.from_numpy(g[tag + ".bf16"])
    assert out.shape == ref32.shape
    sc = ref32.abs().max().item()
    e32, eref = (out - ref32).abs().max().item() / sc, (ref16 - ref32).abs().max().item() / sc
    c32 = torch.nn.functional.cosine_similarity(out.flatten(), ref32.flatten(), dim=0).item()
    print(f"dinov2 448 {tag}: max|HIP - fp32| {e32:.2e} (the port's own bf16-vs-fp32 {eref:.2e}) of the output range; cosine {c32:.6f}")
    assert e32 <= 2.0 * eref + 2e-3 and c32 > 0.9998


def test_dinov2_448_end_to_end_from_raw_512(dev, tmp_path, monkeypatch):
    """preprocess_raw_image(uint8 512^2, 'dinov2') in front of the 448-pixel tower against oracle.vit_towers.preprocess feeding the
    same tower: the preprocessing's deviation does not move the tokens past bf16 noise."""
    from oracle import vit_towers as ot
    from reed_amd import encoders
    key = "dinov2reg-vit-b"
    monkeypatch.setitem(encoders.VIT_TOWERS, key, dict(encoders.VIT_TOWERS[key], embed=256, heads=4, depth=2))
    path = str(tmp_path / "hub.pth")
    torch.save(_hub_tower(256, 4, 2, 4, 62), path)
    enc = encoders.load_vit_encoder(key, path, dev, resolution=512)
    raw = torch.randint(0, 256, (2, 3, 512, 512), generator=torch.Generator().manual_seed(6), dtype=torch.uint8)
    pre = ot.preprocess(raw, "dinov2")
    assert pre.shape == (2, 3, 448, 448)
    got = enc.encode_raw(raw.to(dev)).float().cpu()
    want = enc(pre.to(dev)).float().cpu()
    assert got.shape == (2, 1024, 256) and bool(torch.isfinite(got).all())
    cos = torch.nn.functional.cosine_similarity(got.flatten(), want.flatten(), dim=0).item()
    assert cos > 0.9999, cos


def test_train_512_with_on_device_dinov2_tower(dev, tmp_path, monkeypatch):
    """train.py --resolution 512 --enc-type dinov2reg-vit-b --encoder-ckpts <hub checkpoint>: the 448-pixel tower (1 block of
    ViT-B width) runs every step on the raw 512^2 images, through --data-dir and through --packed-dir; the first steps agree."""
    import PIL.Image
    from oracle import vit_towers as ot
    from reed_amd import encoders, train
    from reed_amd.dataset import pack_dataset
    data = tmp_path / "data"
    (data / "images" / "00000").mkdir(parents=True)
    (data / "vae-sd" / "00000").mkdir(parents=True)
    rng = np.random.default_rng(1)
    labels = []
    for i in range(8):
        PIL.Image.fromarray(rng.integers(0, 256, (512, 512, 3), dtype=np.uint8)).save(data / "images" / "00000" / f"img{i:08d}.png")
        mom = np.concatenate([rng.standard_normal((4, 64, 64)) * 5.0, np.full((4, 64, 64), 0.5)]).astype(np.float32)
        np.save(data / "vae-sd" / "00000" / f"img-mean-std-{i:08d}.npy", mom)
        labels.append([f"00000/img-mean-std-{i:08d}.npy", int(i % 5)])
    json.dump({"labels": labels}, open(data / "vae-sd" / "dataset.json", "w"))
    packed = tmp_path / "packed"
    pack_dataset(str(data), str(packed), with_images=True)
    kw = dict(encoders.VIT_TOWERS["dinov2reg-vit-b"], depth=1)
    monkeypatch.setitem(encoders.VIT_TOWERS, "dinov2reg-vit-b", kw)
    P = ot.fill_params(ot.make_config(768, 1, 12, 14, 224, True, True, "learned", ls=True, reg=4), base_seed=2)
    P["pos_embed"] = torch.randn(1, 1 + 37 * 37, 768, generator=torch.Generator().manual_seed(1)) * 0.02
    P["mask_token"] = torch.zeros(1, 768)
    ck = str(tmp_path / "dinov2_vitb14_reg4_pretrain.pth")
    torch.save(P, ck)
    firsts = []
    for name, src in (("dir", ["--data-dir", str(data)]), ("packed", ["--packed-dir", str(packed)])):
        a = train.parse_args(["--exp-name", name, "--model", "SiT-S/2", "--resolution", "512", "--output-dir", str(tmp_path / "exps"),
                              *src, "--enc-type", "dinov2reg-vit-b", "--encoder-ckpts", ck, "--mixed-precision", "bf16",
                              "--batch-size", "4", "--num-workers", "0", "--diffusion-warm-up-steps", "0", "--report-to", "none",
                              "--max-train-steps", "2", "--num-classes", "5", "--checkpointing-steps", "100"])
        d = train.main(a)
        logs = [json.loads(l) for l in open(os.path.join(d, "metrics.jsonl"))]
        assert len(logs) == 2 and all(np.isfinite(r["proj_loss"]) and np.isfinite(r["training_denoising_loss"]) for r in logs)
        assert logs[0]["img_proj_loss"] != 0.0
        firsts.append((logs[0]["training_denoising_loss"], logs[0]["proj_loss"]))
    torch.set_grad_enabled(True)
    assert firsts[0] == firsts[1], firsts
