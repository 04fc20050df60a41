"""The fp8 sampling path (SiT.fp8: the blocks' four linears as MX-fp8 block GEMMs, csrc/gemm_mxfp8.hip) against the oracle, in both
16-bit builds.  The bounds come from the oracle alone, computed here on the CPU (relative L2 from the fp64 oracle):
  d_mx = the MX-emulating oracle's distance (tests/mxfp8_ref.py: mx_emulation), d_16 = the 16-bit-autocast oracle's;
  the HIP fp8 model must stay within 1.15 sqrt(d_mx^2 + d_16^2) (the two error sources add in quadrature; the kernels round at
  other places than autocast does) and must be CLOSER to the emulated oracle than d_mx (it implements this format, not another).
Then the properties of the switch, SiT-XL/2 on the committed fixtures, and a 25-step Heun + CFG trajectory."""
import copy

import numpy as np
import pytest
import torch

from oracle import detfill
from oracle import sit as osit
from tests import mxfp8_ref as R
from tests.test_model_gpu import build_hip_model
from tests.test_oracle_golden import TINY_CASES, inputs, load

pytestmark = pytest.mark.gpu

KINDS = ("bf16", "fp16")
TINY = ("hd64", "qknorm", "patch4", "xl3")
_REF = {}


def _tiny_inputs(cfg):
    xi, _, ti, yi, _, _ = inputs(4, 4, cfg["input_size"], 11, [], 0, 10)
    return xi, ti, yi


def _oracle_refs(name):
    """fp64 oracle, MX-emulating fp64 oracle and the two autocast oracles of one tiny case: once, shared, never modified."""
    if name not in _REF:
        cfg = TINY_CASES[name]["cfg"]
        xi, ti, yi = _tiny_inputs(cfg)
        P = detfill.fill_state_dict(osit.init_params(cfg), base_seed=11)
        P64 = {k: v.double() for k, v in P.items()}
        with torch.no_grad():
            exact = osit.OracleModel(P64, cfg)(xi.double(), ti.double(), yi)[0]
            with R.mx_emulation(P64, cfg["depth"]) as count:
                mx = osit.OracleModel(P64, cfg)(xi.double(), ti.double(), yi)[0]
            assert count[0] == 4 * cfg["depth"]
            auto = {k: osit.OracleModel(P, cfg, autocast_dtype=dt)(xi, ti, yi)[0]
                    for k, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16))}
        _REF[name] = dict(exact=exact, mx=mx, d_mx=R.rel_l2(mx, exact), d_16={k: R.rel_l2(v, exact) for k, v in auto.items()})
    return _REF[name]


def _hip(m, xi, ti, yi, dev):
    with torch.no_grad():
        o, z = m(xi.to(dev), ti.to(dev), yi.to(dev))
    assert z is None
    return o.cpu()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", TINY)
def test_tiny_fp8_forward_within_the_oracles_distances(dev, name, kind):
    cfg = TINY_CASES[name]["cfg"]
    ref = _oracle_refs(name)
    m = build_hip_model(cfg, dev, 11).eval()
    m.precision, m.fp8 = kind, True
    assert all(m.engine().fp8_layers(4 * m.num_patches).values())
    o = _hip(m, *_tiny_inputs(cfg), dev)
    d_hip, d_emu = R.rel_l2(o, ref["exact"]), R.rel_l2(o, ref["mx"])
    d_mx, d_16 = ref["d_mx"], ref["d_16"][kind]
    root = (d_mx ** 2 + d_16 ** 2) ** 0.5
    print(f"[fp8 {name} {kind}] rel L2 from the fp64 oracle: HIP fp8 {d_hip:.3e}, MX-emulating oracle {d_mx:.3e}, {kind}-autocast oracle "
          f"{d_16:.3e} (root {root:.3e}: ratio {d_hip / root:.3f}); HIP fp8 from the emulating oracle {d_emu:.3e} ({d_emu / d_mx:.3f} of d_mx)")
    assert d_hip <= 1.15 * root
    assert d_emu < d_mx


@pytest.mark.parametrize("kind", KINDS)
def test_fp8_switch_properties(dev, kind):
    cfg = TINY_CASES["hd64"]["cfg"]
    xi, ti, yi = _tiny_inputs(cfg)
    plain = build_hip_model(cfg, dev, 11).eval()       # never had the attribute touched
    plain.precision = kind
    base = _hip(plain, xi, ti, yi, dev)
    m = build_hip_model(cfg, dev, 11).eval()
    m.precision, m.fp8 = kind, False
    assert torch.equal(_hip(m, xi, ti, yi, dev), base)
    m.fp8 = True
    a = _hip(m, xi, ti, yi, dev)
    assert not torch.equal(a, base), "SiT.fp8 is ignored: the fp8 forward returned the 16-bit forward's bits"
    assert torch.equal(_hip(m, xi, ti, yi, dev), a)    # two runs, the same bits
    assert set(m._arena.mx_seg) == set(m._arena.t_names())
    m.fp8 = False
    assert torch.equal(_hip(m, xi, ti, yi, dev), base)
    # the quantised weights follow load_state_dict
    m.fp8 = True
    other = build_hip_model(cfg, dev, 12).eval()
    other.precision, other.fp8 = kind, True
    b = _hip(other, xi, ti, yi, dev)
    assert not torch.equal(a, b)
    m.load_state_dict(other.state_dict())
    assert torch.equal(_hip(m, xi, ti, yi, dev), b)
    # an inf in x is seen: non-finite output, never a clamped finite value
    xbad = xi.clone()
    xbad[1, 2, 3, 3] = float("inf")
    assert not bool(torch.isfinite(_hip(m, xbad, ti, yi, dev)[1]).all())
    # a forward that builds a graph raises while fp8 is set
    m.train()
    with pytest.raises(RuntimeError, match="fp8"):
        m(xi.to(dev), ti.to(dev), yi.to(dev))
    xg = xi.to(dev).requires_grad_(True)
    m.eval().requires_grad_(False)
    with pytest.raises(RuntimeError, match="fp8"):
        m(xg, ti.to(dev), yi.to(dev))


def test_fp8_weights_follow_an_optimizer_step(dev):
    from reed_amd.loss import SILoss
    from reed_amd.optim import FusedAdamWEMA
    from reed_amd.trainer import TrainStep
    c = TINY_CASES["hd64"]
    cfg = c["cfg"]
    T = (cfg["input_size"] // cfg["patch_size"]) ** 2
    x, noise, t, y, drop_u, zs = inputs(8, 4, cfg["input_size"], 31, c["zspec"], T, cfg["num_classes"])
    xi, ti, yi = _tiny_inputs(cfg)
    m = build_hip_model(cfg, dev, 31)
    m.eval().fp8 = True
    before = _hip(m, xi, ti, yi, dev)                  # builds the quantised copy
    m.fp8 = False
    m.train()
    ema = copy.deepcopy(m).requires_grad_(False).eval()
    opt = FusedAdamWEMA(m, ema, lr=1e-2)
    step = TrainStep(m, SILoss(enc_names=c["enc"], loss_weights=dict(zip(c["enc"], c["co"]))), opt, None, proj_coeff=0.5,
                     diffusion_warm_up_steps=0)
    m.force_drop_mask = drop_u < cfg["class_dropout_prob"]
    step(x.to(dev), y.to(dev), [z.to(dev) for z in zs], time_input=t, noises=noise)
    m.force_drop_mask = None
    m.eval().fp8 = True
    after = _hip(m, xi, ti, yi, dev)
    fresh = build_hip_model(cfg, dev, 0).eval()
    fresh.load_state_dict(m.state_dict())
    fresh.fp8 = True
    assert not torch.equal(after, before)
    assert torch.equal(after, _hip(fresh, xi, ti, yi, dev)), "the quantised weights were not rebuilt after the optimiser step"


def test_no_layer_is_eligible_at_width_144(dev):
    """Tiny hd72 (D = 144): no block linear has N and K in multiples of 128, fp8_layers() says so, and the forward keeps its bits.
    The 16-bit builds refuse this width for every GEMM (Engine._check_dims), so the forward runs on the fp32-operand build, where
    the attribute has no meaning either."""
    cfg = TINY_CASES["hd72"]["cfg"]
    xi, ti, yi = _tiny_inputs(cfg)
    m = build_hip_model(cfg, dev, 11).eval()
    for kind in KINDS:
        assert not any(m.engine().fp8_layers(4 * m.num_patches, kind).values())
    m.precision = "fp32"
    base = _hip(m, xi, ti, yi, dev)
    m.fp8 = True
    assert not any(m.engine().fp8_layers().values())
    assert torch.equal(_hip(m, xi, ti, yi, dev), base)


def _xl2(dev):
    from reed_amd.models.sit import SiT_models
    m = SiT_models["SiT-XL/2"](z_dims=[1024], z_types=["i"], encoder_depth=8, use_cfg=True)
    detfill.fill_state_dict(m.state_dict(), base_seed=0)
    return m.to(dev).eval()


@pytest.mark.parametrize("kind", KINDS)
def test_xl2_fp8_evaluation_on_the_fixtures(dev, kind):
    """test_model_gpu.py's XL/2 evaluation (xl2_infer.npz: [x; x], labels [y; 1000], t = 0.9 and 0.35) with fp8: distances from the
    fixture's fp32 array; d_mx from xl2_infer_mxfp8.npz (tools/gen_mxfp8_golden.py), d_16 from the fixture's bf16 array."""
    g, gm = load("xl2_infer"), load("xl2_infer_mxfp8")
    m = _xl2(dev)
    m.precision, m.fp8 = kind, True
    x, _, _, y, _, _ = inputs(2, 4, 32, 77, [], 256, 1000)
    xx, yy = torch.cat([x, x]), torch.cat([y, torch.tensor([1000, 1000])])
    for tv in (0.9, 0.35):
        o = _hip(m, xx, torch.full((4,), tv), yy, dev)
        rf, rb, rm = (torch.from_numpy(a) for a in (g[f"fp32.t{tv}"], g[f"bf16.t{tv}"], gm[f"mx.t{tv}"]))
        d_hip, d_emu, d_mx, d_16 = R.rel_l2(o, rf), R.rel_l2(o, rm), R.rel_l2(rm, rf), R.rel_l2(rb, rf)
        root = (d_mx ** 2 + d_16 ** 2) ** 0.5
        cs = torch.nn.functional.cosine_similarity(o.flatten().double(), rf.flatten().double(), dim=0).item()
        print(f"[fp8 XL/2 {kind} t={tv}] rel L2 from fp32: HIP fp8 {d_hip:.3e} (1 - cos {1 - cs:.2e}), MX-emulating oracle {d_mx:.3e}, bf16 "
              f"fixture {d_16:.3e} (root {root:.3e}: ratio {d_hip / root:.3f}); HIP fp8 from the emulating oracle {d_emu:.3e} "
              f"({d_emu / d_mx:.3f} of d_mx)")
        assert d_hip <= 1.15 * root
        assert d_emu < d_mx


def test_xl2_fp8_long_horizon_drift(dev):
    """25-step Heun + CFG 1.5 on samplers_long_xl.npz (49 evaluations at batch 4): the fp8 sampler (fp16 build + fp8, what
    generate.py --sample-precision fp8 runs) ends finite and within 10 x the bf16 build's end-point drift, measured here in the same
    run (one evaluation is 4.4 x as far from fp32 as bf16; doubled because trajectories compound errors differently).  A ceiling
    against nonsense; the measured ratio is printed."""
    from reed_amd.samplers import euler_sampler
    g = load("samplers_long_xl")
    m = _xl2(dev)
    z = detfill.normal((2, 4, 32, 32), 191).to(dev)
    y = torch.tensor([207, 980], device=dev)
    ref = torch.from_numpy(g["final"])
    end = {}
    for tag, prec, fp8 in (("bf16", "bf16", False), ("fp8", "fp16", True)):
        m.precision, m.fp8 = prec, fp8
        with torch.no_grad():
            out = euler_sampler(m, z, y, num_steps=25, heun=True, cfg_scale=1.5).cpu()
        assert bool(torch.isfinite(out).all())
        end[tag] = ((out - ref).abs().max().item(), (out - ref).pow(2).mean().sqrt().item())
    scale = ref.abs().max().item()
    print(f"[fp8 XL/2 25-step Heun + CFG] end-point drift from the fp32 reference, max abs (rms): bf16 {end['bf16'][0]:.3e} "
          f"({end['bf16'][1]:.3e}), fp8 {end['fp8'][0]:.3e} ({end['fp8'][1]:.3e}): ratio {end['fp8'][0] / end['bf16'][0]:.2f}; latent scale {scale:.2f}")
    assert end["fp8"][0] <= 10 * end["bf16"][0]
