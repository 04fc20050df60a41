"""dL/dx and dL/dt through reed_amd.SiT, and the frozen-weight backward, against the oracle (oracle/sit.py) on the CPU.

References: the oracle at fp64 (init_params(cfg, dtype=torch.float64): the same fp32 weight values, held in fp64) and the oracle
under bf16 autocast, on the inputs of the tiny tests (inputs(4, 4, input_size, 11, ...), fill seed 11, the drop mask from drop_u).
Functional: L = sum(out G) + sum_j sum(z_j G_j) / sqrt(z_dim_j), G = detfill.normal(shape, 777), G_j = detfill.normal(shape, 800 + j).

Bars (set by the issue that asked for the feature, from the reference measured against itself with this functional: fp32 oracle vs
fp64 dx cosine 1.0000000, norm gap <= 3.2e-8, dt <= 2.3e-5 relative; bf16-autocast oracle vs fp64 dx cosine >= 0.9999875, norm gap
<= 4.5e-4, dt up to 9e-3 absolute = 1.2e-2 of max|dt|, and 0.31 relative on the smallest elements of dt, which range from 0.0056 to
0.8 — hence an absolute bound on dt):
  fp32 build   dx: cosine > 1 - 1e-6, |norm ratio - 1| < 1e-4 (the bars of test_tiny_fp32_vs_reference); |dt - dt64| <= 1e-4 max|dt64|
  16-bit       dx: cosine >= 0.9999, |norm ratio - 1| <= 0.004 (GRAD_BAR); |dt - dt64| <= 3 x the worst |dt(bf16-autocast
               oracle) - dt64| of the same case, computed here reference against reference (3: the kernels round at other places
               than autocast does)
Both gaps are printed; profiles/input_grad_tests.txt records them.
"""
import pytest
import torch

from oracle import detfill
from oracle import sit as osit
from tests.rowpass_ref import KINDS, bits
from tests.test_model_gpu import GRAD_BAR, build_hip_model, cos
from tests.test_oracle_golden import TINY_CASES, inputs

pytestmark = pytest.mark.gpu
CASES_16 = ("hd64", "patch4", "two_split", "qknorm")
_REF = {}


def _case(name):
    c = TINY_CASES[name]
    cfg = c["cfg"]
    T = (cfg["input_size"] // cfg["patch_size"]) ** 2
    x, _, t, y, drop_u, _ = inputs(4, 4, cfg["input_size"], 11, c["zspec"], T, cfg["num_classes"])
    return cfg, x, t, y, drop_u < cfg["class_dropout_prob"]


def functional(out, zs):
    L = (out.double() * detfill.normal(tuple(out.shape), 777).to(out.device)).sum()
    for j, z in enumerate(zs or []):
        L = L + (z.double() * detfill.normal(tuple(z.shape), 800 + j).to(z.device)).sum() / z.shape[-1] ** 0.5
    return L


def oracle_grads(name, inference):
    """{"f64": (dx, dt), "bf16": (dx, dt)} of the oracle on the CPU: computed once per case, shared, never modified."""
    key = (name, inference)
    if key not in _REF:
        cfg, x, t, y, drop = _case(name)
        res = {}
        for tag, dt_, auto in (("f64", torch.float64, False), ("bf16", torch.float32, True)):
            P = detfill.fill_state_dict(osit.init_params(cfg, dtype=dt_), base_seed=11)
            om = osit.OracleModel(P, cfg, autocast_bf16=auto, training=True)
            om.drop_mask = drop
            xr, tr = x.to(dt_).requires_grad_(True), t.to(dt_).requires_grad_(True)
            out, zs = om(xr, tr, y, inference)
            functional(out, zs).backward()
            res[tag] = (xr.grad.double(), tr.grad.double())
        _REF[key] = res
    return _REF[key]


def hip_grads(m, dev, name, inference, x_grad=True, t_grad=True, x_dtype=torch.float32, t_dtype=torch.float32):
    """One forward and backward of the functional through the HIP model; (x.grad, t.grad) as autograd leaves them."""
    cfg, x, t, y, drop = _case(name)
    m.train()
    m.force_drop_mask = drop
    xr = x.to(dev, x_dtype).requires_grad_(x_grad)
    tr = t.to(dev, t_dtype).requires_grad_(t_grad)
    out, zs = m(xr, tr, y.to(dev), inference=inference)
    functional(out, zs).backward()
    torch.cuda.synchronize()
    return xr.grad, tr.grad


def _drop_grads(m):
    for p in m.parameters():
        p.grad = None


@pytest.mark.parametrize("inference", [True, False])
@pytest.mark.parametrize("kind,name", [(k, n) for k in KINDS for n in CASES_16 + (("hd72",) if k == "fp32" else ())])
def test_input_gradients_vs_oracle(dev, kind, name, inference):
    ref = oracle_grads(name, inference)
    dx64, dt64 = ref["f64"]
    m = build_hip_model(TINY_CASES[name]["cfg"], dev, 11)
    m.precision = kind
    dx, dt = hip_grads(m, dev, name, inference)
    assert dx is not None and dt is not None, "x.grad / t.grad missing"
    assert dx.dtype == torch.float32 and dx.shape == dx64.shape and dt.shape == dt64.shape
    dx, dt = dx.cpu().double(), dt.cpu().double()
    cs, dn = cos(dx, dx64), abs(float(dx.norm() / dx64.norm()) - 1)
    gap = float((dt - dt64).abs().max())
    rcs, rdn = cos(ref["bf16"][0], dx64), abs(float(ref["bf16"][0].norm() / dx64.norm()) - 1)
    rgap = float((ref["bf16"][1] - dt64).abs().max())
    scale = float(dt64.abs().max())
    print(f"[input grads {kind} {name} inference={inference}] dx cosine {cs:.8f} |norm ratio - 1| {dn:.2e}; dt worst |gap| {gap:.3e} "
          f"= {gap / scale:.2e} of max|dt64| {scale:.3f} || bf16-autocast oracle vs fp64: dx cosine {rcs:.8f} norm {rdn:.2e}, "
          f"dt gap {rgap:.3e}")
    if kind == "fp32":
        assert cs > 1 - 1e-6 and dn < 1e-4, (cs, dn)
        assert gap <= 1e-4 * scale, (gap, scale)
    else:
        assert cs >= GRAD_BAR[0] and dn <= GRAD_BAR[1], (cs, dn)
        assert gap <= 3 * rgap, (gap, rgap)


@pytest.mark.parametrize("kind", KINDS)
def test_input_gradient_properties(dev, kind):
    cfg = TINY_CASES["hd64"]["cfg"]
    m = build_hip_model(cfg, dev, 11)
    m.precision = kind
    # parameters alone, as before: a graph, no input gradient
    assert hip_grads(m, dev, "hd64", False, x_grad=False, t_grad=False) == (None, None)
    base = {k: p.grad.clone() for k, p in m.named_parameters() if p.requires_grad}
    assert base and all(bool(torch.isfinite(g).all()) for g in base.values())
    # with x and t requiring grad every parameter gradient keeps its bits
    _drop_grads(m)
    dx, dt = hip_grads(m, dev, "hd64", False)
    for k, p in m.named_parameters():
        if p.requires_grad:
            assert torch.equal(bits(p.grad), bits(base[k])), k
    # two runs: the same bits
    _drop_grads(m)
    dx2, dt2 = hip_grads(m, dev, "hd64", False)
    assert torch.equal(bits(dx), bits(dx2)) and torch.equal(bits(dt), bits(dt2))
    # one of the two alone: the same bits, the other stays None
    _drop_grads(m)
    dxa, none = hip_grads(m, dev, "hd64", False, t_grad=False)
    assert none is None and torch.equal(bits(dxa), bits(dx))
    _drop_grads(m)
    none, dta = hip_grads(m, dev, "hd64", False, x_grad=False)
    assert none is None and torch.equal(bits(dta), bits(dt))
    # inputs of another dtype: the gradient comes back in it
    _drop_grads(m)
    dx64, dt64 = hip_grads(m, dev, "hd64", False, x_dtype=torch.float64, t_dtype=torch.float64)
    assert dx64.dtype == torch.float64 and dt64.dtype == torch.float64
    assert torch.equal(dx64, dx.double()) and torch.equal(dt64, dt.double())
    # a partly frozen model computes every gradient, as it does without input gradients
    _drop_grads(m)
    m.x_embedder.proj.weight.requires_grad_(False)
    dxp, dtp = hip_grads(m, dev, "hd64", False)
    assert torch.equal(bits(dxp), bits(dx)) and torch.equal(bits(dtp), bits(dt))
    assert m.x_embedder.proj.weight.grad is None
    assert torch.equal(bits(m.final_layer.linear.weight.grad), bits(base["final_layer.linear.weight"]))
    # the frozen-weight backward: the same dx and dt, no parameter gradient, no gradient arena
    f = build_hip_model(cfg, dev, 11).requires_grad_(False)
    f.precision = kind
    for inference in (False, True):
        dxf, dtf = hip_grads(f, dev, "hd64", inference)
        if not inference:
            assert torch.equal(bits(dxf), bits(dx)) and torch.equal(bits(dtf), bits(dt))
        assert bool(torch.isfinite(dxf).all()) and bool(torch.isfinite(dtf).all())
    assert all(p.grad is None for p in f.parameters()) and f._arena.grad is None
    # ... refused with a gradient reducer attached
    f.engine().reducer = object()
    with pytest.raises(RuntimeError, match="reducer"):
        hip_grads(f, dev, "hd64", False)
    f.engine().reducer = None
    # no input requires grad: a frozen model builds no graph, and no_grad none either
    _, x, t, y, _ = _case("hd64")
    out, zs = f(x.to(dev), t.to(dev), y.to(dev), inference=False)
    assert not out.requires_grad and not any(z.requires_grad for z in zs)
    with torch.no_grad():
        out, _ = f(x.to(dev).requires_grad_(True), t.to(dev), y.to(dev))
    assert not out.requires_grad
