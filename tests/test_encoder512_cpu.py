"""The DINOv2 towers at --resolution 512 on the host side (no GPU): the CLI accepts them with --encoder-ckpts and keeps refusing
the families the reference cannot run at 448 / 512 pixels, the loader builds the 448-pixel tower with the hub's 37 x 37 pos_embed
resampled to 32 x 32, and the reference fixture of the GPU tests."""
import os

import numpy as np
import pytest
import torch

from oracle import detfill

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--exp-name", "x", "--model", "SiT-S/2", "--resolution", "512"]


@pytest.mark.parametrize("enc", ["dinov2-vit-b", "dinov2reg-vit-l", "dinov2-vit-s,dinov2reg-vit-b"])
def test_parse_args_accepts_dinov2_encoder_ckpts_at_512(enc):
    from reed_amd import train
    n = len(enc.split(","))
    a = train.parse_args(BASE + ["--enc-type", enc, "--encoder-ckpts", *[f"e{i}.pth" for i in range(n)]])
    assert a.resolution == 512 and a.encoder_ckpts == [f"e{i}.pth" for i in range(n)]


@pytest.mark.parametrize("enc,why", [("clip-vit-L", "positional_embedding"), ("mae-vit-l", "img_size=256"),
                                     ("mocov3-vit-b", "mocov3_vit.py:142"), ("jepa-vit-h", "class token"),
                                     ("dinov2-vit-b,clip-vit-L", "positional_embedding")])
def test_parse_args_refuses_other_towers_at_512(capsys, enc, why):
    from reed_amd import train
    n = len(enc.split(","))
    with pytest.raises(SystemExit):
        train.parse_args(BASE + ["--enc-type", enc, "--encoder-ckpts", *[f"e{i}.pth" for i in range(n)]])
    err = capsys.readouterr().err
    assert "--encoder-ckpts is built for --resolution 256 only" in err and why in err


def test_load_vit_encoder_refuses_other_towers_at_512(tmp_path):
    from reed_amd.encoders import load_vit_encoder
    for key in ("jepa-vit-h", "mae-vit-l", "mocov3-vit-b"):
        with pytest.raises(ValueError, match="resolution 512"):
            load_vit_encoder(key, str(tmp_path / "missing.pth"), "cpu", resolution=512)


def _hub_checkpoint(path, E, heads, reg):
    """A 1-block DINOv2 state dict in the torch.hub layout: 37 x 37 pos_embed, mask_token, register_tokens, ls{1,2}.gamma."""
    from oracle import vit_towers as ot
    P = ot.fill_params(ot.make_config(E, 1, heads, 14, 224, True, True, "learned", ls=True, reg=reg), base_seed=2)
    pe = detfill.normal((1, 1 + 37 * 37, E), 60)
    P["pos_embed"] = pe
    P["mask_token"] = torch.zeros(1, E)
    torch.save(P, path)
    return pe


@pytest.mark.parametrize("key,E,heads,reg,tokens", [("dinov2-vit-b", 768, 12, 0, 1025), ("dinov2reg-vit-l", 1024, 16, 4, 1029)])
def test_load_vit_encoder_dinov2_at_512(tmp_path, monkeypatch, key, E, heads, reg, tokens):
    from reed_amd import encoders
    monkeypatch.setitem(encoders.VIT_TOWERS, key, dict(encoders.VIT_TOWERS[key], depth=1))
    path = str(tmp_path / "hub.pth")
    pe = _hub_checkpoint(path, E, heads, reg)
    enc = encoders.load_vit_encoder(key, path, "cpu", resolution=512)
    assert enc.image == 448 and enc.npatch == 1024 and enc.tokens == tokens and enc.pos_embed.shape == (1, 1025, E)
    assert torch.equal(enc.pos_embed[:, :1], pe[:, :1])
    # the fixture's geometry (37 x 37 -> 32 x 32, bicubic, antialias) on its narrow table, through the loader's resampler
    g = np.load(os.path.join(ROOT, "tests", "golden", "dinov2_512.npz"))
    got = encoders.resample_abs_pos_embed(detfill.normal((1, 1 + 37 * 37, 16), 60), (32, 32), 1)
    np.testing.assert_allclose(got.numpy(), g["pos_resample32"], rtol=0, atol=1e-6)
    want = encoders.resample_abs_pos_embed(pe, (32, 32), 1)
    assert torch.equal(enc.pos_embed.detach(), want)
    # the default stays the 224-pixel tower
    enc256 = encoders.load_vit_encoder(key, path, "cpu")
    assert enc256.image == 224 and enc256.tokens == 257 + reg and enc256.pos_embed.shape == (1, 257, E)


def test_dinov2_512_fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "dinov2_512.npz"))
    assert g["plain.fp32"].shape == (2, 128, 128) and g["plain.bf16"].shape == (2, 128, 128)   # 1024 patches [::8]
    assert g["reg4.fp32"].shape == (2, 64, 256) and g["reg4.bf16"].shape == (2, 64, 256)       # 1024 patches [::16]
    assert g["pos_resample32"].shape == (1, 1025, 16)
    for k in g.files:
        assert np.isfinite(g[k]).all(), k
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "dinov2_512.npz")) <= 600 * 1024
