"""DINOv2 ViT-g on the host side (no GPU): the packed weight layout of the SwiGLU GEMM epilogue, the tower's hub-named
parameters and its loader, and the fixture of the GPU tests."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("Hd,K", [(8, 3), (64, 16), (1024, 8)])
def test_swiglu_pack_layout_and_round_trip(Hd, K):
    from reed_amd import ops
    g = ops.SWIGLU_GROUP
    assert ops.EPI_SWIGLU == 17 and g == 8
    gen = torch.Generator().manual_seed(Hd)
    w12, b12 = torch.randn(2 * Hd, K, generator=gen), torch.randn(2 * Hd, generator=gen)
    pw, pb = ops.swiglu_pack(w12, b12)
    assert pw.shape == w12.shape and pb.shape == b12.shape and pw.is_contiguous()
    for k in range(Hd // g):
        for j in range(g):
            assert torch.equal(pw[2 * g * k + j], w12[g * k + j]) and pb[2 * g * k + j] == b12[g * k + j]
            assert torch.equal(pw[2 * g * k + g + j], w12[Hd + g * k + j]) and pb[2 * g * k + g + j] == b12[Hd + g * k + j]
    uw, ub = ops.swiglu_unpack(pw, pb)
    assert torch.equal(uw, w12) and torch.equal(ub, b12)
    pw2, none = ops.swiglu_pack(w12)
    assert none is None and torch.equal(pw2, pw)
    uw2, none = ops.swiglu_unpack(pw2)
    assert none is None and torch.equal(uw2, w12)
    # the pairing in the unpacked order: output column c is silu(x1[c]) * x2[c]
    x = torch.randn(5, K, generator=gen)
    y = (x @ pw.t() + pb).view(5, Hd // g, 2, g)
    want = x @ w12.t() + b12
    assert torch.equal(y[:, :, 0].reshape(5, Hd), want[:, :Hd]) and torch.equal(y[:, :, 1].reshape(5, Hd), want[:, Hd:])


def test_swiglu_pack_refuses_a_ragged_group():
    from reed_amd import ops
    with pytest.raises(ValueError, match="SWIGLU_GROUP"):
        ops.swiglu_pack(torch.zeros(2 * 12, 4))


def test_vit_towers_hold_vit_g():
    from reed_amd.encoders import VIT_TOWERS
    for key, reg in (("dinov2-vit-g", 0), ("dinov2reg-vit-g", 4)):
        c = VIT_TOWERS[key]
        assert (c["embed"], c["depth"], c["heads"], c["patch"], c["image"]) == (1536, 40, 24, 14, 224)
        assert c["cls"] and c["final_norm"] and c["layerscale"] and c["ffn"] == "swiglu" and c.get("registers", 0) == reg


def _hub_state_dict(enc, reg):
    """Hub-named tensors of the shapes `enc` holds, with the hub's 37 x 37 pos_embed and its mask_token."""
    gen = torch.Generator().manual_seed(5)
    sd = {k: torch.randn(v.shape, generator=gen) * 0.02 for k, v in enc.state_dict().items()}
    sd["pos_embed"] = torch.randn(1, 1 + 37 * 37, enc.embed, generator=gen) * 0.02
    sd["mask_token"] = torch.zeros(1, enc.embed)
    return sd


@pytest.mark.parametrize("key,reg", [("dinov2-vit-g", 0), ("dinov2reg-vit-g", 4)])
def test_vit_g_parameters_and_loader(tmp_path, monkeypatch, key, reg):
    from reed_amd import encoders
    monkeypatch.setitem(encoders.VIT_TOWERS, key, dict(encoders.VIT_TOWERS[key], depth=1))
    enc = encoders.VitEncoder(**encoders.VIT_TOWERS[key])
    sd = enc.state_dict()
    assert enc.ffn == "swiglu" and enc.ffn_hidden == 4096 and enc.hd == 64 and enc.tokens == 257 + reg
    assert sd["blocks.0.mlp.w12.weight"].shape == (8192, 1536) and sd["blocks.0.mlp.w12.bias"].shape == (8192,)
    assert sd["blocks.0.mlp.w3.weight"].shape == (1536, 4096) and sd["blocks.0.mlp.w3.bias"].shape == (1536,)
    assert not [k for k in sd if "fc1" in k or "fc2" in k]
    assert ("register_tokens" in sd) == bool(reg)
    hub = _hub_state_dict(enc, reg)
    path = str(tmp_path / "hub.pth")
    torch.save(hub, path)
    got = encoders.load_vit_encoder(key, path, "cpu")          # raises on a missing key
    assert set(got.state_dict()) == set(hub) - {"mask_token"}  # nothing unexpected but the mask token
    assert got.pos_embed.shape == (1, 257, 1536) and got.image == 224
    assert torch.equal(got.pos_embed.detach(), encoders.resample_abs_pos_embed(hub["pos_embed"], (16, 16), 1))
    assert torch.equal(got.blocks[0].mlp.w12.weight, hub["blocks.0.mlp.w12.weight"])
    assert torch.equal(got.blocks[0].mlp.w3.bias, hub["blocks.0.mlp.w3.bias"])
    missing, unexpected = encoders.VitEncoder(**encoders.VIT_TOWERS[key]).load_state_dict(
        {k: v for k, v in hub.items() if k != "pos_embed"})
    assert missing == ["pos_embed"] and not unexpected
    # --resolution 512: the 448-pixel tower, the table resampled to 32 x 32
    assert encoders.vit_resolution_error(key, 512) is None
    big = encoders.load_vit_encoder(key, path, "cpu", resolution=512)
    assert big.image == 448 and big.tokens == 1025 + reg and big.pos_embed.shape == (1, 1025, 1536)


def test_default_ffn_is_the_mlp():
    from reed_amd.encoders import VitEncoder
    enc = VitEncoder(embed=128, depth=1, heads=2, patch=14, image=28)
    assert enc.ffn == "mlp" and enc.ffn_hidden == 512
    sd = enc.state_dict()
    assert sd["blocks.0.mlp.fc1.weight"].shape == (512, 128) and sd["blocks.0.mlp.fc2.weight"].shape == (128, 512)
    assert not [k for k in sd if "w12" in k or "w3" in k]


def test_swiglu_hidden_width_must_be_a_multiple_of_64():
    from reed_amd.encoders import VitEncoder, swiglu_hidden
    assert swiglu_hidden(1536) == 4096 and swiglu_hidden(384) == 1024 and swiglu_hidden(128) == 344
    with pytest.raises(ValueError, match="multiple of 64"):
        VitEncoder(embed=128, depth=1, heads=2, patch=14, image=28, ffn="swiglu")     # Hd = 344
    with pytest.raises(ValueError, match="ffn"):
        VitEncoder(embed=128, depth=1, heads=2, patch=14, image=28, ffn="glu")


def test_cli_accepts_vit_g_at_256_and_512():
    from reed_amd import train
    for res, enc in (("256", "dinov2-vit-g"), ("512", "dinov2reg-vit-g")):
        a = train.parse_args(["--exp-name", "x", "--model", "SiT-S/2", "--resolution", res, "--enc-type", enc,
                              "--encoder-ckpts", "g.pth"])
        assert a.encoder_ckpts == ["g.pth"]
        assert train.encoder_specs(enc) == ([enc.split("-")[0]], [1536])


def test_swiglu_ref_fill_and_fixture():
    from tests import swiglu_ref
    assert swiglu_ref.swiglu_hidden(384) == 1024
    P = swiglu_ref.hub_params(384, 2, 6, 56, 0)
    assert P["blocks.1.mlp.w12.weight"].shape == (2048, 384) and P["blocks.1.mlp.w3.weight"].shape == (384, 1024)
    assert not [k for k in P if ".mlp.fc" in k]
    assert not torch.equal(P["blocks.0.mlp.w12.weight"], P["blocks.1.mlp.w12.weight"])
    assert abs(P["blocks.0.mlp.w12.weight"].std().item() * 384 ** 0.5 - 1.0) < 0.02
    assert abs(P["blocks.0.mlp.w3.bias"].std().item() / 0.02 - 1.0) < 0.15
    path = os.path.join(ROOT, "tests", "golden", "dinov2_g.npz")
    g = np.load(path)
    assert g["plain.fp32"].shape == (3, 16, 384) and g["reg4.fp32"].shape == (2, 4, 384)
    assert g["p448.fp32"].shape == (1, 128, 384)                     # 1024 patches [::8]
    for k in ("plain", "reg4", "p448"):
        a, b = g[k + ".fp32"], g[k + ".bf16"]
        assert a.shape == b.shape and np.isfinite(a).all() and np.isfinite(b).all()
        assert 0 < np.abs(a - b).max() / np.abs(a).max() < 2e-2      # the port's own bf16-vs-fp32 gap
    assert os.path.getsize(path) < 1024 * 1024
    # the epilogue's restatement pairs column c of x1 with column c of x2
    x = torch.randn(4, 16, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)
    w = torch.randn(32, 16, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    h = swiglu_ref.swiglu_epilogue_ref(x, w, None).float()
    x12 = (x.float() @ w.float().t()).to(torch.bfloat16).float()
    want = torch.nn.functional.silu(x12[:, :16]) * x12[:, 16:]
    torch.testing.assert_close(h, want, atol=2e-2, rtol=2e-2)
