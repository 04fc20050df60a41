"""SD-VAE encoder (`python -m reed_amd.dataset encode`, the reference's image/preprocessing/dataset_tools.py encode through
diffusers' AutoencoderKL.encode) on the host: reed_amd/vae.py:SDVAEEncoder.encode_torch against an independent numpy fp64
restatement that walks the checkpoint keys (explicit im2col, the downsamplers' explicit (0, 1, 0, 1) pad), the published
configuration's key and parameter surface, one AutoencoderKL-style checkpoint with legacy attention names loading into both
halves, and the folder listing / labelling rules of `encode`.  PARITY UNPINNED against diffusers itself (no package and no
checkpoint offline): the two restatements and the published surface pin the architecture."""
import json
import os

import numpy as np
import pytest
import torch


# ---------------- numpy fp64 restatement ----------------
def _conv(x, w, b, stride=1, pad=(1, 1, 1, 1)):
    """x [B, C, H, W], w [O, C, kh, kw]; pad = (left, right, top, bottom) zeros; explicit im2col in (c, ky, kx) order."""
    x = np.pad(x, ((0, 0), (0, 0), (pad[2], pad[3]), (pad[0], pad[1])))
    B, C, H, W = x.shape
    O, _, kh, kw = w.shape
    Ho, Wo = (H - kh) // stride + 1, (W - kw) // stride + 1
    cols = np.empty((B, Ho, Wo, C, kh, kw))
    for ky in range(kh):
        for kx in range(kw):
            cols[..., ky, kx] = x[:, :, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride].transpose(0, 2, 3, 1)
    y = cols.reshape(B * Ho * Wo, C * kh * kw) @ w.reshape(O, -1).T + b
    return y.reshape(B, Ho, Wo, O).transpose(0, 3, 1, 2)


def _gn(x, g, b, G):
    B, C, H, W = x.shape
    xg = x.reshape(B, G, -1)
    m, v = xg.mean(-1, keepdims=True), xg.var(-1, keepdims=True)
    return ((xg - m) / np.sqrt(v + 1e-6)).reshape(B, C, H, W) * g[None, :, None, None] + b[None, :, None, None]


def _silu(x):
    return x / (1 + np.exp(-x))


class NumpyEncoder:
    def __init__(self, P, groups):
        self.P, self.G = P, groups

    def _resnet(self, x, p):
        P = self.P
        h = _conv(_silu(_gn(x, P[p + "norm1.weight"], P[p + "norm1.bias"], self.G)), P[p + "conv1.weight"], P[p + "conv1.bias"])
        h = _conv(_silu(_gn(h, P[p + "norm2.weight"], P[p + "norm2.bias"], self.G)), P[p + "conv2.weight"], P[p + "conv2.bias"])
        if p + "conv_shortcut.weight" in P:
            x = _conv(x, P[p + "conv_shortcut.weight"], P[p + "conv_shortcut.bias"], pad=(0, 0, 0, 0))
        return x + h

    def _attn(self, x, p):
        P = self.P
        B, C, H, W = x.shape
        t = _gn(x, P[p + "group_norm.weight"], P[p + "group_norm.bias"], self.G).reshape(B, C, H * W).transpose(0, 2, 1)
        lin = lambda n, v: v @ P[p + n + ".weight"].T + P[p + n + ".bias"]   # noqa: E731
        q, k, v = lin("to_q", t), lin("to_k", t), lin("to_v", t)
        s = q @ k.transpose(0, 2, 1) / np.sqrt(C)
        s = np.exp(s - s.max(-1, keepdims=True))
        o = lin("to_out.0", (s / s.sum(-1, keepdims=True)) @ v)
        return x + o.transpose(0, 2, 1).reshape(B, C, H, W)

    def encode(self, x):
        P = self.P
        x = _conv(x, P["encoder.conv_in.weight"], P["encoder.conv_in.bias"])
        i = 0
        while f"encoder.down_blocks.{i}.resnets.0.conv1.weight" in P:
            j = 0
            while f"encoder.down_blocks.{i}.resnets.{j}.conv1.weight" in P:
                x = self._resnet(x, f"encoder.down_blocks.{i}.resnets.{j}.")
                j += 1
            d = f"encoder.down_blocks.{i}.downsamplers.0.conv."
            if d + "weight" in P:
                x = _conv(x, P[d + "weight"], P[d + "bias"], stride=2, pad=(0, 1, 0, 1))
            i += 1
        x = self._resnet(x, "encoder.mid_block.resnets.0.")
        x = self._attn(x, "encoder.mid_block.attentions.0.")
        x = self._resnet(x, "encoder.mid_block.resnets.1.")
        x = _silu(_gn(x, P["encoder.conv_norm_out.weight"], P["encoder.conv_norm_out.bias"], self.G))
        x = _conv(x, P["encoder.conv_out.weight"], P["encoder.conv_out.bias"])
        z = _conv(x, P["quant_conv.weight"], P["quant_conv.bias"], pad=(0, 0, 0, 0))
        mean, logvar = np.split(z, 2, axis=1)
        return np.concatenate([mean, np.exp(0.5 * np.clip(logvar, -30.0, 20.0))], axis=1)


def _random_encoder(cfg, seed, std, dtype=torch.float64):
    from reed_amd import vae as rvae
    torch.manual_seed(seed)
    enc = rvae.SDVAEEncoder(**cfg).to(dtype)
    for p in enc.parameters():
        p.data.normal_(0, std)
    return enc


@pytest.mark.parametrize("cfg,shape", [(dict(block_out_channels=(16, 32, 32), layers_per_block=1, norm_num_groups=8), (2, 3, 13, 11)),
                                       (dict(block_out_channels=(8, 16), layers_per_block=2, norm_num_groups=4), (1, 3, 9, 7)),
                                       (dict(block_out_channels=(8, 16, 16, 16), layers_per_block=1, norm_num_groups=4), (2, 3, 17, 16))])
def test_encoder_two_restatements_agree(cfg, shape):
    """encode_torch (torch modules, F.pad + stride-2 conv) against the numpy walk over the keys, odd spatial sizes, to 1e-9;
    quant_conv's bias pushes some logvars below -30 and some above 20 so that both clamps are exercised."""
    enc = _random_encoder(cfg, 3, 0.2)
    with torch.no_grad():
        enc.quant_conv.bias[4:] = torch.tensor([-60.0, 60.0, 0.0, 0.0], dtype=torch.float64)
    x = torch.rand(*shape, dtype=torch.float64) * 2 - 1
    got = enc.encode_torch(x).numpy()
    want = NumpyEncoder({k: v.numpy() for k, v in enc.state_dict().items()}, cfg["norm_num_groups"]).encode(x.numpy())
    f = 2 ** (len(cfg["block_out_channels"]) - 1)
    h, w = shape[2], shape[3]
    for _ in range(len(cfg["block_out_channels"]) - 1):
        h, w = h // 2, w // 2
    assert got.shape == (shape[0], 8, h, w) and f > 1
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9 * np.abs(want).max())
    assert np.all(got[:, 4] == np.exp(-15.0)) and np.all(got[:, 5] == np.exp(10.0))     # the two clamp edges
    assert np.all(got[:, 6:] > 0) and not np.all(got[:, 6] == got[:, 6].flat[0])


def test_published_encoder_surface():
    """sd-vae-ft-{ema,mse}: 34,163,592 encoder parameters + 72 of quant_conv, downsamplers in blocks 0-2 only, double_z."""
    from reed_amd import vae as rvae
    sd = rvae.SDVAEEncoder().state_dict()
    assert sum(v.numel() for k, v in sd.items() if k.startswith("encoder.")) == 34_163_592
    assert sum(v.numel() for k, v in sd.items() if k.startswith("quant_conv.")) == 72
    assert set(sd) == {k for k in sd if k.startswith(("encoder.", "quant_conv."))}
    for i in range(3):
        assert sd[f"encoder.down_blocks.{i}.downsamplers.0.conv.weight"].shape == ((128, 256, 512)[i],) * 2 + (3, 3)
    assert not any(k.startswith("encoder.down_blocks.3.downsamplers") for k in sd)
    assert sd["encoder.conv_in.weight"].shape == (128, 3, 3, 3)
    assert sd["encoder.down_blocks.1.resnets.0.conv_shortcut.weight"].shape == (256, 128, 1, 1)
    assert sd["encoder.down_blocks.2.resnets.0.conv_shortcut.weight"].shape == (512, 256, 1, 1)
    assert "encoder.down_blocks.3.resnets.0.conv_shortcut.weight" not in sd
    assert sd["encoder.mid_block.attentions.0.to_q.weight"].shape == (512, 512)
    assert sd["encoder.conv_out.weight"].shape == (8, 512, 3, 3) and sd["quant_conv.weight"].shape == (8, 8, 1, 1)


@pytest.mark.parametrize("fmt", ["bin", "safetensors"])
def test_one_autoencoderkl_checkpoint_loads_into_both_halves(tmp_path, fmt):
    """A full AutoencoderKL-style state dict (encoder.*, quant_conv.*, post_quant_conv.*, decoder.*) with the legacy attention
    names and conv-shaped attention weights: load_sd_vae_encoder and load_sd_vae_decoder each take their half, strictly."""
    from reed_amd import vae as rvae
    cfg = dict(block_out_channels=(16, 32, 32), layers_per_block=1, norm_num_groups=8)
    enc = _random_encoder(cfg, 4, 0.15, torch.float32)
    torch.manual_seed(5)
    dec = rvae.SDVAEDecoder(**cfg)
    ren = {"to_q": "query", "to_k": "key", "to_v": "value", "to_out.0": "proj_attn"}
    full = {}
    for k, v in list(enc.state_dict().items()) + list(dec.state_dict().items()):
        for new, old in ren.items():
            if f".attentions.0.{new}." in k:
                k = k.replace(f".{new}.", f".{old}.")
                if k.endswith("weight"):
                    v = v[:, :, None, None]
        full[k] = v.clone().contiguous()
    assert len(full) == len(enc.state_dict()) + len(dec.state_dict())
    if fmt == "bin":
        torch.save(full, str(tmp_path / "diffusion_pytorch_model.bin"))
    else:
        from safetensors.torch import save_file
        save_file(full, str(tmp_path / "diffusion_pytorch_model.safetensors"))
    e2 = rvae.load_sd_vae_encoder(str(tmp_path), **cfg)
    d2 = rvae.load_sd_vae_decoder(str(tmp_path), **cfg)
    for a, b in ((enc, e2), (dec, d2)):
        sa, sb = a.state_dict(), b.state_dict()
        assert set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    x = torch.rand(1, 3, 12, 12) * 2 - 1
    assert torch.equal(e2.encode_torch(x), enc.encode_torch(x))


# ---------------- listing and labelling rules of `encode` ----------------
def _png(path, size=(8, 8), value=0):
    import PIL.Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    PIL.Image.fromarray(np.full(size + (3,), value, dtype=np.uint8)).save(path)


def test_listing_with_dataset_json(tmp_path):
    from reed_amd import dataset
    src = tmp_path / "images"
    names = ["00000/img00000002.png", "00000/img00000000.png", "00000/img00000001.png", "00001/img00001000.png"]
    for i, n in enumerate(names):
        _png(str(src / n), value=i)
    (src / "00000" / "notes.txt").write_text("not an image")
    json.dump({"labels": [[n, 7 + i] for i, n in enumerate(names)]}, open(src / "dataset.json", "w"))
    items = dataset.list_image_folder(str(src))
    assert [os.path.relpath(p, src) for p, _ in items] == sorted(names)         # sorted path order, non-images skipped
    assert [lab for _, lab in items] == [8, 9, 7, 10]
    assert dataset.moments_metadata(items) == {"labels": [["00000/img-mean-std-00000000.npy", 8], ["00000/img-mean-std-00000001.npy", 9],
                                                          ["00000/img-mean-std-00000002.npy", 7], ["00000/img-mean-std-00000003.npy", 10]]}
    assert dataset.moments_fname(123456) == "00123/img-mean-std-00123456.npy"
    two = dataset.list_image_folder(str(src), max_images=2)                     # --max-images: the first N in that order
    assert two == items[:2]
    # a dataset.json that misses one image: that label is None and the written labels become null
    json.dump({"labels": [[n, 1] for n in names[1:]]}, open(src / "dataset.json", "w"))
    items = dataset.list_image_folder(str(src))
    assert [lab for _, lab in items] == [1, 1, None, 1]
    assert dataset.moments_metadata(items) == {"labels": None}


def test_listing_labels_from_directory_names(tmp_path):
    from reed_amd import dataset
    src = tmp_path / "src"
    for n in ["dog/b.png", "cat/a.png", "cat/z/c.png", "dog/a.jpg"]:
        _png(str(src / n))
    json.dump({"labels": None}, open(src / "dataset.json", "w"))               # null labels: fall back to directory names
    items = dataset.list_image_folder(str(src))
    assert [(os.path.relpath(p, src), lab) for p, lab in items] == [("cat/a.png", 0), ("cat/z/c.png", 0), ("dog/a.jpg", 1), ("dog/b.png", 1)]
    assert dataset.moments_metadata(items)["labels"][2] == ["00000/img-mean-std-00000002.npy", 1]
    # one top-level name only (files at the root count as the name ""): no labels
    flat = tmp_path / "flat"
    for n in ["a.png", "b.png"]:
        _png(str(flat / n))
    items = dataset.list_image_folder(str(flat))
    assert [lab for _, lab in items] == [None, None] and dataset.moments_metadata(items) == {"labels": None}
    _png(str(flat / "sub" / "c.png"))                                          # "" and "sub": two names -> labels 0 and 1
    assert [lab for _, lab in dataset.list_image_folder(str(flat))] == [0, 0, 1]


def test_encode_refuses_a_non_empty_destination_and_zip(tmp_path):
    from reed_amd import dataset
    src = tmp_path / "images"
    _png(str(src / "a.png"))
    dest = tmp_path / "vae-sd"
    dest.mkdir()
    (dest / "old.npy").write_bytes(b"x")
    with pytest.raises(ValueError, match="must be empty"):
        dataset.encode_image_folder(str(src), str(dest), vae_ckpt=str(tmp_path / "missing"))
    with pytest.raises(ValueError, match="zip"):
        dataset.encode_image_folder(str(src), str(tmp_path / "out.zip"), vae_ckpt=str(tmp_path / "missing"))
    with pytest.raises(ValueError, match="zip"):
        dataset.encode_image_folder(str(tmp_path / "images.zip"), str(tmp_path / "new"), vae_ckpt=str(tmp_path / "missing"))
    assert os.listdir(dest) == ["old.npy"]
    with pytest.raises(SystemExit):
        dataset.main(["encode", str(src), str(dest), "--vae-ckpt", "x", "--num-workers", "17"])
