"""The split kernel of the fp32 build (csrc/gemm_f32.hip: gemm_f32_split_kernel, ops.f32_split) against fp64, every case held to
the budget of tests/tf32_ref.py (derived from the arithmetic; proven on the CPU in tests/test_tf32_budgets_cpu.py).

Buffers are gemm_ref.call_buffers' (own leading dimensions, NaN outside the live elements, inputs too); the launch, the guard
checks and the comparison of every element are tests/test_gemm_epilogues_gpu.py's.  Each case first asks the planner whether the
call runs kernel "f32_split"."""
import pytest
import torch

from tests import gemm_ref as G
from tests import tf32_ref as T
from tests.test_gemm_epilogues_gpu import _launch

pytestmark = pytest.mark.gpu

_INP = {}


def _inputs(sh):
    if sh not in _INP:
        _INP[sh] = G.inputs(sh, T.KIND)               # computed once, shared, never modified
    return _INP[sh]


@pytest.fixture()
def split(dev):
    from reed_amd import ops
    with ops.build("fp32", tf32=True):
        yield ops
    assert not ops.f32_split_on()


def _check(ops, dev, layout, epi, sh, var):
    a = G.plan_args(T.row(layout), epi, sh, var)
    rc, launches = ops.gemm_plan(a.pop("lay"), a.pop("epi"), a.pop("M"), a.pop("N"), a.pop("K"), a.pop("split_k"), **a, precision="fp32")
    assert rc == 0 and [l["kernel"] for l in launches] == ["f32_split"], (rc, launches)
    inp = _inputs(sh)
    got = _launch(inp, T.row(layout), epi, var, dev)
    rat = G.ratios(got, T.reference(inp, epi, var, got))
    shown = {k: v for k, v in var.items() if k != "_bias"}
    print(f"[f32_split {G.LAY_NAME[layout]} {G.EPI_NAME[epi]} {tuple(sh[:3])} {shown}] worst error / budget: "
          + ", ".join(f"{k} {r:.3f} at {i}" for k, (r, i) in rat.items()))
    for k, (r, i) in rat.items():
        assert r <= 1, (k, r, i, tuple(sh[:3]), shown)


CASES = [(lay, e) for lay, epis in ((T.NT, T.EPIS_NT), (T.NN, T.EPIS_NN)) for e in epis]


@pytest.mark.parametrize("layout,epi", CASES, ids=[f"{G.LAY_NAME[l]}-{G.EPI_NAME[e]}" for l, e in CASES])
def test_split_gemm_vs_fp64(dev, split, layout, epi):
    """NT and NN: every epilogue at every shape (M < 16, ragged M and N, K % 8 == 4, K < one K step, five K tiles of 64)."""
    for sh in T.SHAPES:
        for var in T.calls(layout, epi, sh):
            _check(split, dev, layout, epi, sh, var)


@pytest.mark.parametrize("i", range(len(T.TN_CASES)), ids=[f"tokens{s.K}-{s.M}x{s.N}" for s, _ in T.TN_CASES])
def test_split_weight_gradient_vs_fp64(dev, split, i):
    """TN with the fused bias gradient (a plain fp32 column sum), split-K into slabs + reduce_slabs, and the atomic epilogue."""
    sh, vs = T.TN_CASES[i]
    for v in vs:
        epi = G.ATOMIC_F32 if v.get("split") == 4 else G.F32
        _check(split, dev, T.TN, epi, sh, G.with_bias(T.row(T.TN), epi, v))


def _conv_ref(x, w, bias, up, down):
    """fp64 3x3 convolution of NHWC x [B, H, W, C] with w [N, 9 C] in (ky, kx, ci) order -> ([B * Ho * Wo, N], sum of |terms|)."""
    B, H, W, C = x.shape
    N = w.shape[0]
    F = torch.nn.functional

    def conv(xx, ww, bb):
        xx = xx.permute(0, 3, 1, 2)
        if up:
            xx = F.interpolate(xx, scale_factor=2, mode="nearest")
        k = ww.view(N, 3, 3, C).permute(0, 3, 1, 2)
        y = F.conv2d(F.pad(xx, (0, 1, 0, 1)), k, bb, stride=2) if down else F.conv2d(xx, k, bb, padding=1)
        return y.permute(0, 2, 3, 1).reshape(-1, N)
    return conv(x.double(), w.double(), bias.double()), conv(x.double().abs(), w.double().abs(), bias.double().abs())


@pytest.mark.parametrize("form", ["plain", "upsample", "down", "plain-accumulate"])
def test_split_conv3x3_vs_fp64(dev, split, form):
    """The window gather (reed_conv3x3, plain and nearest x2; reed_conv3x3_down) on the split kernel: B = 1, 6 x 6, C = N = 8, so
    K = 72 = two K steps and a quarter, every tap of every border pixel outside the grid, M = 36 / 144 / 9 rows of one tile."""
    ops = split
    B, H, C, N, ldc = 1, 6, 8, 8, 24
    g = torch.Generator().manual_seed(606)
    x = torch.randn(B, H, H, C, generator=g)
    w = torch.randn(N, 9 * C, generator=g) / (9 * C) ** 0.5
    bias = torch.randn(N, generator=g)
    up, down, acc = form == "upsample", form == "down", form.endswith("accumulate")
    ref, mag = _conv_ref(x, w, bias, up, down)
    M, K = ref.shape[0], 9 * C
    prior = torch.randn(M, N, generator=g) if acc else torch.zeros(M, N)
    out = torch.full((M + G.GUARD, ldc), float("nan"))
    if acc:
        out[:M, :N] = prior
    # NaN behind the activation and the weights: a tap read from beyond the image would poison its output
    xb = torch.cat([x.flatten(), torch.full((64,), float("nan"))]).to(dev)
    wb = torch.cat([w.flatten(), torch.full((64,), float("nan"))]).to(dev)
    d = out.to(dev)
    if down:
        ops.conv3x3_down(xb, wb, bias.to(dev), d, ldc, B, H, H, C, N, accumulate=acc)
    else:
        ops.conv3x3(xb, wb, bias.to(dev), d, ldc, B, H, H, C, N, upsample=up, accumulate=acc)
    torch.cuda.synchronize()
    got = d.cpu()
    assert torch.isfinite(got[:M, :N]).all() and torch.isnan(got[:M, N:]).all() and torch.isnan(got[M:]).all()
    want = ref + prior.double()
    budget = (T.SPLIT_TERM + (3 * K + 1) * 2 * T.U) * mag + T.U * (ref.abs() + prior.abs() + want.abs())
    r, i = G.worst((got[:M, :N].double() - want).abs(), budget)
    print(f"[f32_split conv3x3 {form}] worst error / budget: {r:.3f} at {i}")
    assert r <= 1


def test_split_mode_is_isolated(dev):
    """The same call before the knob is ever touched by this test, with the mode off, on, and off again: the exact kernel's
    results are bit-identical all three times, the split kernel's differs from them, and the mode is off afterwards."""
    from reed_amd import ops
    M, N, K = 200, 132, 36
    g = torch.Generator().manual_seed(77)
    A, W = torch.randn(M, K, generator=g).to(dev), (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)

    def run():
        C = torch.full((M, N), float("nan"), device=dev)
        ops.gemm(ops.NT, ops.EPI_F32, A, W, M, N, K, C, K, K, N)
        torch.cuda.synchronize()
        return C.cpu()

    prev = ops.use("fp32")
    try:
        assert not ops.f32_split_on()
        untouched = run()
        assert ops.f32_split(False) is False
        off0 = run()
        assert ops.f32_split(True) is False
        assert ops.gemm_plan(ops.NT, ops.EPI_F32, M, N, K, precision="fp32")[1][0]["kernel"] == "f32_split"
        on = run()
        assert ops.f32_split(False) is True
        assert ops.gemm_plan(ops.NT, ops.EPI_F32, M, N, K, precision="fp32")[1][0]["kernel"] == "f32"
        off1 = run()
    finally:
        ops.f32_split(False)
        ops.use(prev)
    assert torch.equal(untouched, off0) and torch.equal(off0, off1)
    assert torch.isfinite(on).all() and not torch.equal(on, off0)
    ref = A.cpu().double() @ W.cpu().double().T
    assert (on.double() - ref).abs().max() < 1e-4 * ref.abs().max()      # the other kernel, not another problem
