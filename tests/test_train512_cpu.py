"""512^2 training on the host side (no GPU): the CLI's resolution choices and refusals, synthetic latents at T = 1024, and the
reference fixture of the 512^2 GPU tests."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--exp-name", "x", "--model", "SiT-S/2", "--synthetic", "8", "--batch-size", "4"]


def test_parse_args_resolution_choices():
    from reed_amd import train
    assert train.parse_args(BASE).resolution == 256
    assert train.parse_args(BASE + ["--resolution", "512"]).resolution == 512
    with pytest.raises(SystemExit):
        train.parse_args(BASE + ["--resolution", "384"])


def test_encoder_ckpts_refused_at_512(capsys):
    from reed_amd import train
    with pytest.raises(SystemExit):
        train.parse_args(["--exp-name", "x", "--model", "SiT-S/2", "--resolution", "512", "--enc-type", "clip-vit-L",
                          "--encoder-ckpts", "clip.pt"])
    assert "--encoder-ckpts is built for --resolution 256 only" in capsys.readouterr().err
    a = train.parse_args(["--exp-name", "x", "--model", "SiT-S/2", "--enc-type", "clip-vit-L", "--encoder-ckpts", "clip.pt"])
    assert a.encoder_ckpts == ["clip.pt"] and a.resolution == 256


def test_synthetic_latents_at_512():
    from reed_amd.dataset import SyntheticLatents
    ds = SyntheticLatents(4, [768, 16], ["i", "t"], num_classes=10, seed=1, latent=64)
    item = ds[2]
    assert item[1].shape == (8, 64, 64)
    assert item[4].shape == (1024, 768) and item[5].shape == (16,)


def test_tiny512_fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "tiny512.npz"))
    for name, D, heads in (("hd64", 128, 2), ("xl3", 1152, 16)):
        assert g[f"{name}.denoising_loss"].shape == (2,)
        assert np.isfinite(float(g[f"{name}.total"]))
        assert g[f"{name}.grad.x_embedder.proj.weight"].shape == (D, 4, 2, 2)
        assert g[f"{name}.grad.blocks.0.attn.qkv.bias"].shape == (3 * D,)
        assert g[f"{name}.grad.final_layer.linear.weight"].shape == (2 * 2 * 4, D)
        # pos_embed is a fixed table (no gradient); every other parameter has its gradient norm
        assert f"{name}.gnorm.blocks.2.mlp.fc2.weight" in g and f"{name}.gnorm.pos_embed" not in g
