"""SD-VAE encoder on the device (`python -m reed_amd.dataset encode`): `reed_amd/vae.py:SDVAEEncoder.encode` = HIP kernels only
(reed_vae_image_rows, reed_conv3x3_down, reed_vae_moments and the decoder's passes; no torch / MIOpen operator) against the
torch-operator form of the same module.  PARITY UNPINNED against diffusers itself (neither the package nor a checkpoint is
available offline).  Kernel level: the stride-2 convolution in all three builds, conv_in's pixel rows, the moments pass with both
clamps; path level: reduced configurations in fp32, the published configuration at 256^2 in all three operand types and at 512^2
(T = 4096 in the mid block); the CLI end to end into a two-step training run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("prec", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("B,Hi,Wi,C,N,acc", [(2, 8, 6, 64, 128, False), (1, 7, 9, 128, 256, True), (3, 16, 16, 192, 128, True),
                                             (1, 33, 31, 128, 128, False), (2, 64, 64, 256, 256, False),
                                             (2, 5, 7, 4, 36, False), (1, 9, 4, 20, 12, True)])
def test_conv3x3_down(dev, prec, B, Hi, Wi, C, N, acc):
    """reed_conv3x3_down against F.conv2d(F.pad(x, (0, 1, 0, 1)), stride=2) in fp64 on the same rounded operands: even and odd
    sizes (the bottom / right zero row and column), ragged last row tile, in-place residual; the last two shapes are fp32-only."""
    if prec != "fp32" and (C % 64 or N % 128):
        pytest.skip("the 16-bit kernel takes C % 64 == 0, N % 128 == 0")
    from reed_amd import ops
    g = torch.Generator().manual_seed(B * Hi + Wi + C)
    hd = ops.half_dtype(prec)
    a = torch.randn(B, Hi, Wi, C, generator=g).to(hd)
    w = (torch.randn(N, C, 3, 3, generator=g) / (9 * C) ** 0.5).to(hd)
    bias = torch.randn(N, generator=g)
    want = F.conv2d(F.pad(a.double().permute(0, 3, 1, 2), (0, 1, 0, 1)), w.double(), bias.double(), stride=2).permute(0, 2, 3, 1)
    Ho, Wo = want.shape[1:3]
    assert (Ho, Wo) == (Hi // 2, Wi // 2)
    res = torch.randn(B, Ho, Wo, N, generator=g)
    out = res.clone().to(dev) if acc else torch.full((B, Ho, Wo, N), float("nan"), device=dev)
    prev = ops.use(prec)
    try:
        ops.conv3x3_down(a.to(dev), w.permute(0, 2, 3, 1).reshape(N, 9 * C).contiguous().to(dev), bias.to(dev), out, N, B, Hi, Wi, C,
                         N, accumulate=acc)
    finally:
        ops.use(prev)
    ref = want + res.double() if acc else want
    torch.testing.assert_close(out.cpu().double(), ref, rtol=2e-5, atol=2e-5 * float(ref.abs().max()))


@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
def test_vae_image_rows(dev, prec):
    """conv_in's rows from uint8 pixels against F.unfold(raw / 127.5 - 1, padding=1): the padding is 0 in the normalised domain,
    columns 27.. are zero, nothing beyond ldo is written, two row chunks."""
    from reed_amd import ops
    B, H, W = 2, 5, 7
    raw = torch.randint(0, 256, (B, 3, H, W), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    raw[0, :, 0, 0] = 0                                 # a black corner: its padded neighbours must be 0, not -1
    x = raw.float() / 127.5 - 1
    cols = F.unfold(x, 3, padding=1).view(B, 3, 9, H * W).permute(0, 3, 2, 1).reshape(B * H * W, 27)   # (tap, c) order
    hd = ops.half_dtype(prec)
    kcols = 28 if prec == "fp32" else 64
    ldo = kcols + 4
    M = B * H * W
    out = torch.full((M, ldo), 7.0, dtype=hd, device=dev)
    prev = ops.use(prec)
    try:
        half = M // 2 + 1
        for r0, n in ((0, half), (half, M - half)):
            ops.vae_image_rows(raw.to(dev), out.data_ptr() + r0 * ldo * out.element_size(), B, H, W, r0, n, kcols, ldo)
    finally:
        ops.use(prev)
    got = out.cpu()
    assert torch.equal(got[:, :27], cols.to(hd))
    assert torch.all(got[:, 27:kcols] == 0) and torch.all(got[:, kcols:] == 7.0)
    assert torch.all(got[0, :4 * 3] == 0) and float(cols[0, 12]) == -1.0    # outside: 0; the black pixel itself: -1


def test_vae_moments(dev):
    """quant_conv + (mean, std) against fp64 torch, NCHW output, ldc > 8, both logvar clamps."""
    from reed_amd import ops
    B, h, w, ldc = 3, 5, 7, 12
    g = torch.Generator().manual_seed(2)
    y = torch.randn(B * h * w, ldc, generator=g) * 3
    qw = torch.randn(8, 8, generator=g) * 0.5
    qb = torch.randn(8, generator=g)
    qb[4], qb[5] = -100.0, 100.0
    out = torch.full((B, 8, h, w), float("nan"), device=dev)
    prev = ops.use("fp32")
    try:
        ops.vae_moments(y.to(dev), ldc, B, h, w, qw.to(dev), qb.to(dev), out)
    finally:
        ops.use(prev)
    z = (y[:, :8].double() @ qw.double().T + qb.double()).view(B, h, w, 8).permute(0, 3, 1, 2)
    mean, logvar = z.chunk(2, dim=1)
    want = torch.cat([mean, torch.exp(0.5 * logvar.clamp(-30, 20))], 1)
    got = out.cpu().double()
    torch.testing.assert_close(got[:, :4], want[:, :4], rtol=1e-5, atol=1e-5 * float(want[:, :4].abs().max()))
    torch.testing.assert_close(got[:, 4:], want[:, 4:], rtol=2e-5, atol=0)
    for c, v in ((4, np.exp(-15.0)), (5, np.exp(10.0))):      # every logvar of these channels clamped: one value each
        assert torch.all(out[:, c] == out[0, c, 0, 0]) and abs(float(out[0, c, 0, 0]) / v - 1) < 1e-6


def _random_encoder(cfg, seed, std):
    from reed_amd import vae as rvae
    torch.manual_seed(seed)
    enc = rvae.SDVAEEncoder(**cfg)
    for p in enc.parameters():
        p.data.normal_(0, std)
    return enc


def _raw(shape, seed):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _err(got, want):
    """max abs error of the mean half and of the std half, each over its own scale"""
    out = []
    for sl in (slice(0, 4), slice(4, 8)):
        w = want[:, sl]
        out.append((float((got[:, sl].double() - w).abs().max()), float(w.abs().max())))
    return out


@pytest.mark.parametrize("cfg,shape", [(dict(block_out_channels=(16, 32, 32), layers_per_block=1, norm_num_groups=8), (2, 3, 33, 31)),
                                       (dict(block_out_channels=(32, 64, 64, 64), layers_per_block=2, norm_num_groups=16), (1, 3, 24, 20)),
                                       (dict(block_out_channels=(8, 16), layers_per_block=1, norm_num_groups=4), (3, 3, 9, 7))])
def test_encoder_hip_fp32_vs_torch_fp64(dev, cfg, shape):
    """Reduced configurations end to end on the fp32-operand kernels against the module on torch operators in fp64: odd sizes,
    shortcut convolutions, the attention block; cutting the workspace to 64 KiB (many row chunks) gives the same bits."""
    enc = _random_encoder(cfg, 1, 0.15)
    raw = _raw(shape, 3)
    want = enc.double().encode_torch(raw.double() / 127.5 - 1)
    enc = enc.float().to(dev)
    got = enc.encode(raw.to(dev)).cpu()
    assert got.dtype == torch.float32 and got.shape == want.shape
    for e, s in _err(got, want):
        print(f"reduced encoder fp32 vs fp64: max abs {e:.3e} of scale {s:.3f}")
        assert e <= 2e-5 * s
    enc._hip.WS_BYTES = 1 << 16
    assert torch.equal(enc.encode(raw.to(dev)).cpu(), got)


def test_encoder_published_config_256(dev):
    """The published sd-vae-ft configuration at 256^2 -> [8, 32, 32]: fp32 operands against the torch-operator form in fp64 on
    the GPU at the decoder's bar, then the fp16 and bf16 MFMA kernels against the same reference."""
    from reed_amd import ops
    enc = _random_encoder({}, 2, 0.02).to(dev)
    raw = _raw((2, 3, 256, 256), 5).to(dev)
    want = enc.double().encode_torch(raw.double() / 127.5 - 1)
    enc.float()
    got = enc.encode(raw)
    assert got.shape == (2, 8, 32, 32)
    assert ops._PRECISION == "bf16"                     # encode restores the selection
    for (e, s), half in zip(_err(got, want), ("mean", "std")):
        print(f"sd-vae-ft encoder 256^2, fp32 operands vs fp64 torch operators ({half}): max abs {e:.3e} of scale {s:.3f}")
        assert e <= 5e-5 * s
    for prec, bar in (("fp16", 3e-3), ("bf16", 3e-2)):
        for (e, s), half in zip(_err(enc.encode(raw, precision=prec), want), ("mean", "std")):
            print(f"  {prec} operands ({half}): max abs {e:.3e} ({e / s:.2e} of scale)")
            assert e <= bar * s
    assert ops.gemm_forced_tile() == 0                  # the pinned GEMM form is restored


def test_encoder_published_config_512(dev):
    """512^2 -> [8, 64, 64], T = 4096 in the mid-block attention: the 16-bit results against the HIP fp32 result."""
    enc = _random_encoder({}, 3, 0.02).to(dev)
    raw = _raw((1, 3, 512, 512), 6).to(dev)
    ref = enc.encode(raw).double()
    assert ref.shape == (1, 8, 64, 64) and torch.isfinite(ref).all()
    for prec, bar in (("fp16", 3e-3), ("bf16", 3e-2)):
        for (e, s), half in zip(_err(enc.encode(raw, precision=prec), ref), ("mean", "std")):
            print(f"sd-vae-ft encoder 512^2, {prec} vs fp32 operands ({half}): max abs {e:.3e} ({e / s:.2e} of scale)")
            assert e <= bar * s


def _run(args, timeout):
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def test_dataset_encode_cli_into_training(dev, tmp_path):
    """`python -m reed_amd.dataset encode` on a convert-style folder (five 256^2 PNGs + dataset.json) with a random-weight
    checkpoint in diffusers layout: file names, dataset.json, dtype / shape, values equal to SDVAEEncoder.encode of the same
    pixels, the same bits at --batch-size 1 and 3, CustomDataset alignment, and two training steps on the result."""
    import PIL.Image
    from safetensors.torch import save_file
    from reed_amd import vae as rvae
    from reed_amd.dataset import CustomDataset
    rng = np.random.default_rng(0)
    names = [f"00000/img{i:08d}.png" for i in range(5)]
    imgs = [rng.integers(0, 256, (256, 256, 3), dtype=np.uint8) for _ in names]
    for n, img in zip(names, imgs):
        os.makedirs(tmp_path / "images" / os.path.dirname(n), exist_ok=True)
        PIL.Image.fromarray(img).save(tmp_path / "images" / n)
    labels = [3, 1, 4, 1, 0]
    json.dump({"labels": [[n, lab] for n, lab in zip(names, labels)]}, open(tmp_path / "images" / "dataset.json", "w"))
    enc = _random_encoder({}, 7, 0.02)
    ck = tmp_path / "sd-vae"
    ck.mkdir()
    save_file({k: v.contiguous() for k, v in enc.state_dict().items()}, str(ck / "diffusion_pytorch_model.safetensors"))
    outs = {}
    for bs in (1, 3):
        dest = tmp_path / ("vae-sd" if bs == 1 else f"vae-sd-b{bs}")
        _run(["-m", "reed_amd.dataset", "encode", str(tmp_path / "images"), str(dest), "--vae-ckpt", str(ck), "--batch-size", str(bs),
              "--num-workers", "2"], timeout=600)
        files = sorted(os.path.relpath(os.path.join(r, f), dest) for r, _, fs in os.walk(dest) for f in fs)
        assert files == ["00000/img-mean-std-%08d.npy" % i for i in range(5)] + ["dataset.json"]
        assert json.load(open(dest / "dataset.json")) == {"labels": [["00000/img-mean-std-%08d.npy" % i, lab] for i, lab in enumerate(labels)]}
        outs[bs] = np.stack([np.load(dest / ("00000/img-mean-std-%08d.npy" % i)) for i in range(5)])
        assert outs[bs].dtype == np.float32 and outs[bs].shape == (5, 8, 32, 32)
    assert np.array_equal(outs[1], outs[3])
    raw = torch.from_numpy(np.stack(imgs)).permute(0, 3, 1, 2).contiguous().to(dev)
    want = rvae.load_sd_vae_encoder(str(ck), device=dev).encode(raw).cpu().numpy()
    assert np.array_equal(outs[1], want)
    ds = CustomDataset(str(tmp_path))
    assert len(ds) == 5
    for i in range(5):
        image, moments, label, _ = ds[i]
        assert torch.equal(image, torch.from_numpy(imgs[i]).permute(2, 0, 1)) and np.array_equal(moments.numpy(), want[i])
        assert int(label) == labels[i]
    # a second encode into the non-empty destination is refused
    r = subprocess.run([sys.executable, "-m", "reed_amd.dataset", "encode", str(tmp_path / "images"), str(tmp_path / "vae-sd"),
                        "--vae-ckpt", str(ck)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "must be empty" in r.stderr
    exps = tmp_path / "exps"
    _run(["-m", "reed_amd.train", "--data-dir", str(tmp_path), "--model", "SiT-S/2", "--enc-type", "None", "--exp-name", "enc",
          "--output-dir", str(exps), "--batch-size", "4", "--num-workers", "0", "--max-train-steps", "2", "--mixed-precision", "bf16",
          "--diffusion-warm-up-steps", "0", "--report-to", "none", "--checkpointing-steps", "100"], timeout=600)
    logs = [json.loads(line) for p in exps.rglob("metrics.jsonl") for line in open(p)]
    assert len(logs) == 2 and all(np.isfinite(r["training_denoising_loss"]) for r in logs)
