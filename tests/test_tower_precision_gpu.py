"""The frozen towers in fp16 and fp32 on the GPU (encoders.py: precision=...; train.py: --encoder-precision): every small tower case of
the existing encoder tests against the reference's fp32 golden (fp16) and against a float64 restatement (fp32), the 448-pixel tower,
the default path bit for bit, the selection of the library build, and the two pieces the fp32 library gained for it — the head_dim-80
attention forward and reed_swiglu_rows.  Notation: e(x) = max|HIP - x| / max|golden fp32|; g16, g32, gbf16 from tests/tower_prec_ref.py."""
import json
import logging
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import tower_prec_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _tower(name, dev, **kw):
    from reed_amd.encoders import ClipVisionEncoder, VitEncoder
    c = R.case(name)
    P, x = R.case_inputs(name)
    if c["kind"] == "clip":
        enc = ClipVisionEncoder(**c["enc"], **kw)
        enc.load_state_dict(P, strict=True)
    else:
        enc = VitEncoder(**c["enc"], **kw)
        missing, unexpected = enc.load_state_dict(P)
        assert not missing and not unexpected
    return enc.to(dev).eval(), x.to(dev)


def _bars_fp16(out, r, what):
    """1. within twice the reference's own fp16 gap (the factor the bf16 tests give the HIP tower over the reference's bf16 gap; their
    additive 2e-3 is larger than the whole fp16 gap and is dropped); 2. a third of the golden's bf16 gap at the most: a tower that is
    still bf16 sits at about 1, the fp16 oracle at 1/6.4 to 1/8.4; 3. cosine."""
    assert out.shape == r["golden32"].shape, (out.shape, r["golden32"].shape)
    e = R.gap(out, r["golden32"], r["scale"])
    cs = F.cosine_similarity(out.double().flatten(), r["golden32"].double().flatten(), dim=0).item()
    print(f"fp16 {what}: e(golden.fp32) {e:.3e}  g16 {r['g16']:.3e}  e/g16 {e / r['g16']:.2f}  gbf16 {r['gbf16']:.3e}  "
          f"gbf16/e {r['gbf16'] / e:.1f}  cosine {cs:.7f}")
    assert e <= 2 * r["g16"]
    assert e <= r["gbf16"] / 3
    assert cs > 0.99999


def _bars_fp32(out, r, what):
    """against float64 within 8 x the restatement's own fp32-vs-fp64 gap: the margin for the MFMA's K order, the row reductions, the
    device expf and the erf form of gelu_erf_f."""
    assert out.shape == r["o64"].shape, (out.shape, r["o64"].shape)
    e = R.gap(out, r["o64"], r["scale"])
    print(f"fp32 {what}: e(o64) {e:.3e}  g32 {r['g32']:.3e}  e/g32 {e / r['g32']:.2f}")
    assert e <= 8 * r["g32"]


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_fp16_tower(dev, name):
    enc, x = _tower(name, dev, precision="fp16")
    out = enc(x)
    assert out.dtype == (torch.float16 if R.case(name)["kind"] == "clip" else torch.float32)
    _bars_fp16(out.float().cpu(), R.reference(name), name)


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_fp32_tower(dev, name):
    enc, x = _tower(name, dev, precision="fp32")
    out = enc(x)
    assert out.dtype == torch.float32
    _bars_fp32(out.cpu(), R.reference(name), name)


# ---- T = 1025: the 448-pixel DINOv2 tower of --resolution 512 -----------------------------------------------------------------------
_ref448 = {}


def _case448():
    """The `plain` case of tests/golden/dinov2_512.npz (test_dinov2_tower_448_vs_hf_port): E 128, 2 heads, 2 blocks, every 8th token."""
    if not _ref448:
        from oracle import detfill
        from oracle import vit_towers as ot
        from tests.test_encoder512_gpu import _hub_tower
        from tests.test_oracle_golden import load
        P = _hub_tower(128, 2, 2, 0, 58)
        cfg = ot.make_config(128, 2, 2, 14, 448, True, True, "learned", ls=True, reg=0)
        Q = dict(P, pos_embed=ot.resample_abs_pos_embed(P["pos_embed"], (32, 32), 1))
        x = detfill.normal((2, 3, 448, 448), 59)
        g = load("dinov2_512")
        r32, r16 = torch.from_numpy(g["plain.fp32"]), torch.from_numpy(g["plain.bf16"]).float()
        sc = r32.abs().max().item()
        o64 = R.forward64(Q, cfg, x)[:, ::8]
        _ref448.update(P=P, x=x, ref=dict(golden32=r32, scale=sc, gbf16=R.gap(r16, r32, sc), o64=o64,
                                          g16=R.gap(R.forward(Q, cfg, x, torch.float16)[:, ::8], r32, sc),
                                          g32=R.gap(R.forward(Q, cfg, x)[:, ::8], o64, sc)))
    return _ref448


@pytest.mark.parametrize("precision", ["fp16", "fp32"])
def test_tower_448_t1025(dev, tmp_path, monkeypatch, precision):
    from reed_amd import encoders
    c = _case448()
    key = "dinov2-vit-b"
    monkeypatch.setitem(encoders.VIT_TOWERS, key, dict(encoders.VIT_TOWERS[key], embed=128, heads=2, depth=2))
    path = str(tmp_path / "hub.pth")
    torch.save(c["P"], path)
    enc = encoders.load_vit_encoder(key, path, dev, resolution=512, precision=precision)
    assert enc.image == 448 and enc.tokens == 1025 and enc.precision == precision
    out = enc(c["x"].to(dev)).float().cpu()[:, ::8]
    (_bars_fp16 if precision == "fp16" else _bars_fp32)(out, c["ref"], "dinov2 448 plain")


# ---- the default path, and which library a forward runs on ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dinov2.reg4", "clip.t3"])
def test_explicit_bf16_is_the_default_bit_for_bit(dev, name):
    enc0, x = _tower(name, dev)
    enc1, _ = _tower(name, dev, precision="bf16")
    assert enc0.precision == "bf16"
    a, b = enc0(x), enc1(x)
    assert a.dtype == b.dtype and torch.equal(a, b)


@pytest.mark.parametrize("name", ["dinov2.reg4", "clip.t3"])
def test_build_isolation(dev, name):
    """One tower at bf16, fp16, bf16: the operand cache follows the precision and the first and third outputs are the same bits; a
    forward that raises leaves the library selection where it was."""
    from reed_amd import ops
    enc, x = _tower(name, dev)
    a = enc(x).clone()
    enc.precision = "fp16"
    mid = enc(x).clone()
    enc.precision = "bf16"
    c = enc(x)
    assert torch.equal(a, c)
    assert not torch.equal(a.float(), mid.float())
    assert ops._PRECISION == "bf16"
    prev = ops.use("fp16")
    try:
        enc.precision = "fp32"
        with pytest.raises(ValueError, match="input"):
            enc(torch.zeros(1, 3, 17, 17, device=dev))
        assert ops._PRECISION == "fp16"
        assert enc(x).dtype == torch.float32 and ops._PRECISION == "fp16"
    finally:
        ops.use(prev)


# ---- fp32 library: attention forward at head_dim 80 -----------------------------------------------------------------------------------
# (2, 77, 3): a ragged 32-row stage (77 = 2 x 32 + 13) whose last 8-key chunk is ragged too; (1, 261, 2): a second query block of 5 rows
@pytest.mark.parametrize("B,T,H", [(2, 77, 3), (1, 261, 2)])
def test_fp32_attention_fwd_head_dim_80(dev, B, T, H):
    from reed_amd import ops
    hd = 80
    qkv = torch.randn(B, T, 3, H, hd, generator=torch.Generator().manual_seed(T)) * 1.2
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3).double() for i in range(3))
    s = q @ k.transpose(-1, -2) * hd ** -0.5
    ro = (s.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(B, T, H * hd)
    rl = torch.logsumexp(s, -1)
    d = qkv.to(dev)
    o = torch.full((B, T, H * hd), NAN, device=dev)
    lse = torch.full((B, H, T), NAN, device=dev)
    o2 = torch.full_like(o, NAN)
    prev = ops.use("fp32")
    try:
        ops.attention_fwd(d, o, lse, B, T, H, hd)
        ops.attention_fwd(d, o2, None, B, T, H, hd)
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match="head_dim 80"):
            ops.attention_bwd(d, o, o, lse, torch.empty_like(d), B, T, H, hd)
    finally:
        ops.use(prev)
    atol = 1e-5 * ro.abs().max().item()
    print(f"fp32 attention hd 80 {(B, T, H)}: max|o - o64| {(o.cpu().double() - ro).abs().max().item():.2e}, "
          f"max|lse - lse64| {(lse.cpu().double() - rl).abs().max().item():.2e}, max|o| {ro.abs().max().item():.2f}")
    torch.testing.assert_close(o.cpu().double(), ro, rtol=1e-5, atol=atol)
    torch.testing.assert_close(lse.cpu().double(), rl, rtol=1e-5, atol=atol)
    assert torch.equal(o, o2)


# ---- reed_swiglu_rows ---------------------------------------------------------------------------------------------------------------
def _ulp32(v):
    """Spacing of fp32 at |v| (v float64)."""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(v), e - 24)


# (300, 4096): more rows than the launch has row blocks — the kernel's row loop; the last case: ld > 2 Hd and ldu > Hd
@pytest.mark.parametrize("M,Hd,ld,ldu", [(5, 8, 16, 8), (33, 72, 144, 72), (300, 4096, 8192, 4096), (33, 72, 160, 80)])
def test_swiglu_rows_fp32_vs_float64(dev, M, Hd, ld, ldu):
    from reed_amd import ops
    g = torch.Generator().manual_seed(M + Hd + ld)
    x12 = torch.full((M, ld), NAN)
    x12[:, :2 * Hd] = torch.randn(M, 2 * Hd, generator=g) * 1.5
    buf = torch.full((M * ldu + 64,), NAN, device=dev)        # 64 floats of canary behind u
    prev = ops.use("fp32")
    try:
        ops.swiglu_rows(x12.to(dev), buf, M, Hd, ld=ld, ldu=ldu)
        torch.cuda.synchronize()
    finally:
        ops.use(prev)
    assert torch.isnan(buf[M * ldu:]).all()
    u = buf[:M * ldu].view(M, ldu).cpu()
    assert torch.isnan(u[:, Hd:]).all()
    x1, x2 = x12[:, :Hd].double(), x12[:, Hd:2 * Hd].double()
    ref = x1 * torch.sigmoid(x1) * x2
    err = ((u[:, :Hd].double() - ref).abs() / _ulp32(ref)).max().item()
    print(f"swiglu_rows fp32 {(M, Hd, ld, ldu)}: max error {err:.2f} ulp")
    assert err <= 4.0


# (33, 128): the issue's shape; (1100, 64): more rows than row blocks in the 16-bit builds too
@pytest.mark.parametrize("M,Hd", [(33, 128), (1100, 64)])
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_swiglu_rows_equals_the_fused_epilogue(dev, precision, M, Hd):
    """16-bit builds: gemm(EPI_BF16) on the unpacked w12 into [M, 2 Hd], then swiglu_rows = gemm(EPI_SWIGLU) on the packed weight."""
    from reed_amd import ops
    K = 64
    half = ops.half_dtype(precision)
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, K, generator=g).to(half).to(dev)
    w12 = (torch.randn(2 * Hd, K, generator=g) / K ** 0.5).to(half).to(dev)
    b12 = torch.randn(2 * Hd, generator=g).to(half).to(dev)
    pw, pb = ops.swiglu_pack(w12, b12)
    x12 = torch.full((M, 2 * Hd), NAN, dtype=half, device=dev)
    buf = torch.full((M * Hd + 64,), NAN, dtype=half, device=dev)
    fused = torch.full((M, Hd), NAN, dtype=half, device=dev)
    prev = ops.use(precision)
    try:
        ops.gemm(ops.NT, ops.EPI_BF16, x, w12, M, 2 * Hd, K, x12, K, K, 2 * Hd, bias=b12)
        ops.swiglu_rows(x12, buf, M, Hd)
        ops.gemm(ops.NT, ops.EPI_SWIGLU, x, pw, M, 2 * Hd, K, fused, K, K, Hd, bias=pb)
        torch.cuda.synchronize()
    finally:
        ops.use(prev)
    assert torch.isnan(buf[M * Hd:].float()).all()
    two = buf[:M * Hd].view(M, Hd)
    assert torch.isfinite(two.float()).all()
    ne = two != fused
    assert not ne.any(), (int(ne.sum()), ne.nonzero()[:4].tolist())


@pytest.mark.parametrize("precision", ["bf16", "fp16", "fp32"])
def test_swiglu_rows_argument_checks(dev, precision):
    from reed_amd import ops
    half = ops.half_dtype(precision)
    x12 = torch.zeros(8, 32, dtype=half, device=dev)
    u = torch.full((8, 16), NAN, dtype=half, device=dev)
    bad = {"null x12": lambda: ops.swiglu_rows(None, u, 8, 16), "null u": lambda: ops.swiglu_rows(x12, None, 8, 16),
           "M = 0": lambda: ops.swiglu_rows(x12, u, 0, 16), "Hd = 12": lambda: ops.swiglu_rows(x12, u, 8, 12),
           "ld < 2 Hd": lambda: ops.swiglu_rows(x12, u, 8, 16, ld=24), "ldu < Hd": lambda: ops.swiglu_rows(x12, u, 8, 16, ldu=8)}
    prev = ops.use(precision)
    try:
        for what, call in bad.items():
            with pytest.raises(RuntimeError, match="swiglu_rows"):
                call()
            torch.cuda.synchronize()
            assert torch.isnan(u.float()).all(), what
        ops.swiglu_rows(x12, u, 8, 16)
        torch.cuda.synchronize()
    finally:
        ops.use(prev)
    assert (u.float() == 0).all()


# ---- train.py -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixed,want", [("fp16", "fp16"), ("no", "fp32")])
def test_train_encoder_precision_match(dev, tmp_path, monkeypatch, caplog, mixed, want):
    """Two optimiser steps of SiT-S/2 at 256 with a one-block dinov2-vit-b running every step at --encoder-precision match: finite
    losses, the resolved precision in the log and in args.json, and the features the loss gets are those of a direct encode_raw call
    of a tower loaded at that precision."""
    import PIL.Image
    from oracle import vit_towers as ot
    from reed_amd import encoders, train, trainer
    data = tmp_path / "data"
    (data / "images" / "00000").mkdir(parents=True)
    (data / "vae-sd" / "00000").mkdir(parents=True)
    rng = np.random.default_rng(1)
    labels = []
    for i in range(4):
        PIL.Image.fromarray(rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)).save(data / "images" / "00000" / f"img{i:08d}.png")
        mom = np.concatenate([rng.standard_normal((4, 32, 32)) * 5.0, np.full((4, 32, 32), 0.5)]).astype(np.float32)
        np.save(data / "vae-sd" / "00000" / f"img-mean-std-{i:08d}.npy", mom)
        labels.append([f"00000/img-mean-std-{i:08d}.npy", int(i % 3)])
    json.dump({"labels": labels}, open(data / "vae-sd" / "dataset.json", "w"))
    key = "dinov2-vit-b"
    monkeypatch.setitem(encoders.VIT_TOWERS, key, dict(encoders.VIT_TOWERS[key], depth=1))
    P = ot.fill_params(ot.make_config(768, 1, 12, 14, 224, True, True, "learned", ls=True), base_seed=2)
    P["pos_embed"] = torch.randn(1, 1 + 37 * 37, 768, generator=torch.Generator().manual_seed(1)) * 0.02
    P["mask_token"] = torch.zeros(1, 768)
    ck = str(tmp_path / "dinov2_vitb14_pretrain.pth")
    torch.save(P, ck)

    seen, handed = [], []
    load = encoders.load_vit_encoder

    def loading(*a, **kw):
        enc = load(*a, **kw)
        direct = enc.encode_raw

        def encode_raw(raw):
            out = direct(raw)
            seen.append((raw.clone(), out.clone()))
            return out
        enc.encode_raw = encode_raw
        return enc

    call = trainer.TrainStep.__call__

    def stepping(self, x, labels, zs, **kw):
        handed.append(zs[0].clone())
        return call(self, x, labels, zs, **kw)

    monkeypatch.setattr(encoders, "load_vit_encoder", loading)
    monkeypatch.setattr(trainer.TrainStep, "__call__", stepping)
    a = train.parse_args(["--exp-name", "prec", "--model", "SiT-S/2", "--output-dir", str(tmp_path / "exps"), "--data-dir", str(data),
                          "--enc-type", key, "--encoder-ckpts", ck, "--mixed-precision", mixed, "--encoder-precision", "match",
                          "--batch-size", "4", "--num-workers", "0", "--diffusion-warm-up-steps", "0", "--report-to", "none",
                          "--max-train-steps", "2", "--num-classes", "3", "--checkpointing-steps", "100"])
    assert a.encoder_precision == want
    caplog.set_level(logging.INFO, logger="reed_amd.train")
    try:
        d = train.main(a)
    finally:
        torch.set_grad_enabled(True)
    logs = [json.loads(l) for l in open(os.path.join(d, "metrics.jsonl"))]
    assert len(logs) == 2 and all(np.isfinite(r["proj_loss"]) and np.isfinite(r["training_denoising_loss"]) for r in logs)
    assert logs[0]["img_proj_loss"] != 0.0
    assert f"frozen encoders: {key} at {want}" in caplog.text
    assert json.load(open(os.path.join(d, "args.json")))["encoder_precision"] == want
    assert len(seen) == 2 and len(handed) == 2
    fresh = load(key, ck, dev, precision=want)
    assert fresh.precision == want
    for (raw, out), z in zip(seen, handed):
        assert out.dtype == torch.float32 and out.shape == (4, 256, 768) and torch.isfinite(out).all()
        assert torch.equal(z, out)
        assert torch.equal(fresh.encode_raw(raw), out)
