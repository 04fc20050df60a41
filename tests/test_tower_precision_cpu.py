"""The frozen towers' precision argument on the host: the dtype-parameterised restatement (tests/tower_prec_ref.py) is the oracle
bit for bit where the oracle has a say, its fp16-autocast and fp32 outputs sit where the precision tests on the GPU need them, and
--encoder-precision / the constructors / the loaders take and refuse what they should."""
import pytest
import torch

from tests import tower_prec_ref as R

VIT_NAMES = R.CASE_NAMES[:6]   # the four TOWER_CASES and the two DINOv2 cases of dinov2.npz


@pytest.mark.parametrize("name", R.CASE_NAMES[:4])
def test_helper_is_the_oracle_bit_for_bit(name):
    from oracle import vit_towers as ot
    P, x = R.case_inputs(name)
    cfg = R.case(name)["cfg"]
    with torch.no_grad():
        assert torch.equal(R.forward(P, cfg, x, torch.bfloat16), ot.forward(P, cfg, x, autocast_bf16=True))
        assert torch.equal(R.forward(P, cfg, x, None), ot.forward(P, cfg, x))


@pytest.mark.parametrize("name", ["clip.t2", "clip.t3"])
def test_clip_helper_is_the_oracle_bit_for_bit(name):
    from oracle import clip_vit as oclip
    P, x = R.case_inputs(name)
    cfg = R.case(name)["cfg"]
    with torch.no_grad():
        assert torch.equal(R.forward(P, cfg, x, torch.bfloat16), oclip.forward(P, cfg, x, autocast_bf16=True))
        assert torch.equal(R.forward(P, cfg, x, None), oclip.forward(P, cfg, x))


@pytest.mark.parametrize("name", VIT_NAMES)
def test_fp16_and_fp32_gaps(name):
    """fp16 autocast sits at most a third of the golden's own bf16 gap from the golden fp32 (three more mantissa bits: 1/8 nominally;
    measured 1/6.4 to 1/8.4), and fp32 sits below 2e-6 of the output range from float64 (measured 6.6e-7 to 9.9e-7)."""
    r = R.reference(name)
    print(f"{name}: fp16 gap {r['g16']:.2e}, golden bf16 gap {r['gbf16']:.2e} (ratio {r['gbf16'] / r['g16']:.1f}), fp32-vs-fp64 {r['g32']:.2e}")
    assert r["g16"] <= r["gbf16"] / 3
    assert r["g32"] < 2e-6


BASE = ["--exp-name", "x", "--model", "SiT-S/2"]


def test_cli_encoder_precision():
    from reed_amd import train
    assert train.parse_args(BASE).encoder_precision == "bf16"
    assert train.parse_args(BASE + ["--mixed-precision", "no"]).encoder_precision == "bf16"      # the default does not follow
    for mp, want in (("fp16", "fp16"), ("bf16", "bf16"), ("no", "fp32")):
        assert train.parse_args(BASE + ["--mixed-precision", mp, "--encoder-precision", "match"]).encoder_precision == want
    for p in ("bf16", "fp16", "fp32"):
        assert train.parse_args(BASE + ["--mixed-precision", "bf16", "--encoder-precision", p]).encoder_precision == p
    with pytest.raises(SystemExit):
        train.parse_args(BASE + ["--encoder-precision", "int8"])


def test_constructors_refuse_unknown_precision():
    from reed_amd.encoders import ClipVisionEncoder, VitEncoder
    tiny = dict(embed=128, depth=1, heads=2, patch=16, image=32)
    with pytest.raises(ValueError, match="precision"):
        VitEncoder(**tiny, precision="int8")
    with pytest.raises(ValueError, match="precision"):
        ClipVisionEncoder(width=128, layers=1, heads=2, patch=14, image=28, precision="int8")
    for p in ("bf16", "fp16", "fp32"):
        assert VitEncoder(**tiny, precision=p).precision == p
        assert ClipVisionEncoder(width=128, layers=1, heads=2, patch=14, image=28, precision=p).precision == p
    assert VitEncoder(**tiny).precision == "bf16" and ClipVisionEncoder(width=128, layers=1, heads=2, patch=14, image=28).precision == "bf16"


def test_loaders_pass_the_precision_on(tmp_path, monkeypatch):
    from oracle import clip_vit as oclip
    from reed_amd import encoders
    tiny = dict(embed=128, depth=2, heads=2, patch=16, image=64, cls=True, final_norm=True)
    monkeypatch.setitem(encoders.VIT_TOWERS, "mocov3-vit-l", tiny)
    path = str(tmp_path / "tower.pth")
    torch.save(encoders.VitEncoder(**tiny).state_dict(), path)
    enc = encoders.load_vit_encoder("mocov3-vit-l", path, "cpu", precision="fp16")
    assert enc.precision == "fp16"
    assert encoders.load_vit_encoder("mocov3-vit-l", path, "cpu").precision == "bf16"
    with pytest.raises(ValueError, match="precision"):
        encoders.load_vit_encoder("mocov3-vit-l", path, "cpu", precision="tf32")
    cfg = oclip.make_config(width=128, layers=1, heads=2, patch=14, image=28)
    monkeypatch.setitem(encoders.CLIP_CONFIGS, "B", cfg)
    cpath = str(tmp_path / "clip.pth")
    torch.save(oclip.fill_params(cfg, base_seed=1), cpath)
    assert encoders.load_clip_encoder("B", cpath, "cpu", precision="fp32").precision == "fp32"
    assert encoders.load_clip_encoder("B", cpath, "cpu").precision == "bf16"
