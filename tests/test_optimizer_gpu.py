"""The optimiser pass (csrc/optim.hip) at the sizes and in the forms production uses: the grid-stride loops, the scalar tail,
idle blocks, the frozen tail of the arena, the optional outputs, the loss scaler, and the pointer-offset segment form of
reed_amd/optim.py.  References: fp64 restatements of torch's clip_grad_norm_ / AdamW / update_ema and a plain-Python
GradScaler.update().
"""
import math

import pytest
import torch

from tests.rowpass_ref import DTYPE, U, Guarded, bits

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS, WD, DECAY = 1e-2, 0.9, 0.999, 1e-8, 0.01, 0.99


@pytest.fixture(params=["bf16", "fp16"])
def build16(request, dev):
    from reed_amd import ops
    prev = ops.use(request.param)
    yield request.param
    ops.use(prev)


def randn(n, seed, dev, scale=1.0):
    return (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale).to(dev)


def sqnorm(ops, g, n, nblocks, dev):
    """grad_sqnorm into NaN-pre-filled partials (an idle block must still write its 0) with a canary behind."""
    partial = Guarded(nblocks, torch.float32, dev)
    ops.grad_sqnorm(g, n, partial.t, nblocks)
    torch.cuda.synchronize()
    assert partial.intact() and not torch.isnan(partial.t).any(), "a partial was not written"
    return partial


# ------------------------------------------------------------------------------------------- grad_sqnorm + clip_finalize
# idle blocks and n < 4 (the tail alone); one block; three grid-stride laps plus the tail; two laps in some blocks only
SQ_CASES = [(72, 2048), (3, 64), (7, 1), (64 * 256 * 4 * 3 + 7, 64), (2048 * 256 * 4 + 4 * 300 + 2, 2048)]


@pytest.mark.parametrize("n,nblocks", SQ_CASES)
def test_grad_norm_and_clip_coefficient(dev, n, nblocks):
    """The terms are all positive and the reduction is a tree: per thread at most 3 laps x 5 roundings + 2 for the tail, 8 for the
    wave and block sums, the rest in fp64, so the sum is within 26 u relative and the norm (the square root halves it, its
    cast to fp32 adds u / 2) well within 64 u."""
    from reed_amd import ops
    for scale, max_norm in ((3.0, 1.0), (1e-3, 1.0)):          # clipped; not clipped (coefficient exactly 1 for the small sizes)
        g = randn(n, n + nblocks, dev, scale)
        partial = sqnorm(ops, g, n, nblocks, dev)
        nc = Guarded(2, torch.float32, dev)
        ops.clip_finalize(partial.t, nblocks, max_norm, nc.t)
        torch.cuda.synchronize()
        assert nc.intact()
        ref = math.sqrt(float((g.double() ** 2).sum()))
        norm, coef = float(nc.t[0]), float(nc.t[1])
        r = abs(norm - ref) / (64 * U * ref)
        print(f"[grad norm n={n} blocks={nblocks} scale={scale}] error / (64 u norm) = {r:.3f}")
        assert r <= 1.0, (norm, ref)
        want = min(1.0, max_norm / (ref + 1e-6))
        assert abs(coef - want) <= 66 * U * want and coef <= 1.0, (coef, want)
        # ... and exactly the fp32 expression of the kernel's own norm
        c32 = torch.minimum(torch.ones(()), torch.tensor(max_norm) / (nc.t[0].cpu() + torch.tensor(1e-6)))
        assert abs(coef - float(c32)) <= 2 * U * float(c32)
        if ref < 0.5:
            assert coef == 1.0
    for bad in (float("inf"), float("nan")):
        g = randn(n, n, dev)
        g[n // 2] = bad
        partial = sqnorm(ops, g, n, nblocks, dev) if bad == bad else None
        if partial is None:                                    # a NaN partial is the point here: no unwritten-slot check
            partial = Guarded(nblocks, torch.float32, dev, fill=-1.0)
            ops.grad_sqnorm(g, n, partial.t, nblocks)
        nc = torch.zeros(2, device=dev)
        ops.clip_finalize(partial.t, nblocks, 1.0, nc)
        assert (math.isinf(float(nc[0])) and float(nc[0]) > 0) if bad == bad else math.isnan(float(nc[0]))


def test_grad_sqnorm_refuses_bad_arguments(dev):
    from reed_amd import ops
    g, partial = torch.ones(16, device=dev), torch.full((4,), 7.0, device=dev)
    with pytest.raises(RuntimeError, match="misaligned"):
        ops.grad_sqnorm(g.data_ptr() + 4, 8, partial, 4)
    with pytest.raises(RuntimeError, match="bad args"):
        ops.grad_sqnorm(g, 8, partial, 0)
    with pytest.raises(RuntimeError, match="bad args"):
        ops.grad_sqnorm(None, 8, partial, 4)
    torch.cuda.synchronize()
    assert (partial == 7.0).all()


# -------------------------------------------------------------------------------------------------- clip_finalize_scaled
def scaler_update(state, found_inf, growth, backoff, interval):
    """torch.amp.GradScaler.update() on [scale, growth_tracker, found_inf, steps_taken] (steps_taken: optimiser steps not skipped)."""
    scale, tracker, _, steps = state
    if found_inf:
        return [scale * backoff, 0.0, 1.0, steps]
    tracker += 1.0
    if tracker == interval:
        scale, tracker = scale * growth, 0.0
    return [scale, tracker, 0.0, steps + 1.0]


@pytest.mark.parametrize("case", ["below", "reaches", "inf", "nan", "no_clip"])
def test_clip_finalize_scaled_vs_grad_scaler(dev, case):
    from reed_amd import ops
    n, nblocks, growth, backoff, interval = 4 * 300 + 2, 16, 2.0, 0.5, 3
    state0 = {"below": [1024.0, 0.0, 1.0, 5.0], "reaches": [1024.0, 2.0, 0.0, 6.0], "inf": [1024.0, 2.0, 0.0, 7.0],
              "nan": [4096.0, 1.0, 0.0, 7.0], "no_clip": [65536.0, 0.0, 0.0, 1.0]}[case]
    max_norm = 0.0 if case == "no_clip" else 1.0
    g = randn(n, 5, dev, 0.2)                                   # the true gradient: norm about 7, so it is clipped
    gs = g * state0[0]                                          # what the arena holds (a power-of-two scale: exact)
    if case in ("inf", "nan"):
        gs[17] = float(case)
    partial = Guarded(nblocks, torch.float32, dev, fill=-1.0)
    ops.grad_sqnorm(gs, n, partial.t, nblocks)
    nc, st = Guarded(2, torch.float32, dev), Guarded(4, torch.float32, dev)
    st.t.copy_(torch.tensor(state0))
    ops.clip_finalize_scaled(partial.t, nblocks, max_norm, nc.t, st.t, growth, backoff, interval)
    torch.cuda.synchronize()
    assert nc.intact() and st.intact() and partial.intact()
    bad = case in ("inf", "nan")
    assert st.t.tolist() == scaler_update(state0, bad, growth, backoff, interval)
    norm, coef = float(nc.t[0]), float(nc.t[1])
    if bad:
        assert (math.isinf(norm) if case == "inf" else math.isnan(norm)) and coef == 0.0
        return
    ref = math.sqrt(float((g.double() ** 2).sum()))             # norm_clip[0] is the UNSCALED norm
    assert abs(norm - ref) <= 65 * U * ref, (norm, ref)
    if case == "no_clip":
        assert coef == 1.0 / state0[0]                          # exactly 1 / scale
    else:
        want = min(1.0, max_norm / (ref + 1e-6)) / state0[0]
        assert want < 0.5 / state0[0] and abs(coef - want) <= 68 * U * want, (coef, want)


# --------------------------------------------------------------------------------------------------------- adamw_ema
N_TOTAL = 4 * (8192 * 256 + 300)      # the smallest arena that enters the grid-stride loop (8192 blocks of 256 x 4)
N_TRAIN = N_TOTAL - 4 * 1000          # a frozen tail: EMA and shadow move there, p / m / v do not


class Arena:
    """One set of optimiser state on the device, cloned from shared seeded tensors."""

    def __init__(self, base, dt):
        self.p, self.m, self.v, self.ema = (base[k].clone() for k in ("p", "m", "v", "ema"))
        self.shadow = torch.full((N_TOTAL,), 7.0, dtype=dt, device=self.p.device)

    def step(self, ops, g, nc, t, ema=True, shadow=True, scaler=None, bc=None, segments=None):
        bc1, bc2 = bc if bc is not None else (1 - B1 ** t, 1 - B2 ** t)
        hb = self.shadow.element_size()
        for b, e in segments or [(0, N_TOTAL)]:
            nt = max(0, min(e, N_TRAIN) - b)
            ptr = lambda x, w=4: x.data_ptr() + w * b   # noqa: E731
            ops.adamw_ema(ptr(self.p), ptr(g) if nt else None, ptr(self.m) if nt else None, ptr(self.v) if nt else None,
                          ptr(self.ema) if ema else None, ptr(self.shadow, hb) if shadow else None, nt, e - b, nc,
                          LR, B1, B2, EPS, WD, bc1, bc2, DECAY, scaler_state=scaler)
        return self

    def same(self, other, names=("p", "m", "v", "ema", "shadow")):
        return [k for k in names if not torch.equal(bits(getattr(self, k)), bits(getattr(other, k)))]


def adamw_ema_fp64(p, m, v, ema, g, clip, t):
    """torch.optim.AdamW (decoupled decay, lerp / addcmul moments, bias corrections) + update_ema, in place on fp64 tensors;
    the first N_TRAIN elements train, the EMA follows everything."""
    s = slice(0, N_TRAIN)
    gg = g[s].double() * clip
    p[s] *= 1 - LR * WD
    m[s] += (1 - B1) * (gg - m[s])
    v[s] = v[s] * B2 + (1 - B2) * gg * gg
    bc1, bc2 = 1 - B1 ** t, 1 - B2 ** t
    p[s] -= (LR / bc1) * (m[s] / (v[s].sqrt() / math.sqrt(bc2) + EPS))
    ema.mul_(DECAY).add_(p, alpha=1 - DECAY)


def close(tag, got, ref, rtol=2e-6, atol=5e-7):
    """The project's tolerance for this update (test_fused_optimizer_vs_reference_toy: fp32 FMA-contraction noise)."""
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / (atol + rtol * ref.abs()))   # 0 / 0 (the frozen tail's zero moments)
    r = float(torch.where(torch.isfinite(err), ratio, torch.full_like(err, float("inf"))).max())
    print(f"[adamw_ema] {tag}: worst error / (atol + rtol |ref|) = {r:.3f}")
    assert r <= 1.0, tag
    return r


@pytest.fixture(scope="module")
def base(dev):
    p = randn(N_TOTAL, 1, dev)
    return dict(p=p, ema=p + randn(N_TOTAL, 2, dev, 0.01), m=torch.zeros(N_TOTAL, device=dev), v=torch.zeros(N_TOTAL, device=dev),
                g=[randn(N_TOTAL, 3, dev, 0.1), randn(N_TOTAL, 4, dev, 0.02)])


def test_adamw_ema_two_steps_vs_fp64(dev, build16, base):
    from reed_amd import ops
    dt = DTYPE[build16]
    a = Arena(base, dt)
    p64, m64, v64, e64 = (base[k].double() for k in ("p", "m", "v", "ema"))
    tail = slice(N_TRAIN, N_TOTAL)
    for t in (1, 2):
        g = base["g"][t - 1]
        partial, nc = torch.empty(2048, device=dev), torch.empty(2, device=dev)
        ops.grad_sqnorm(g, N_TRAIN, partial, 2048)
        ops.clip_finalize(partial, 2048, 1.0, nc)
        ema_before = a.ema.clone()
        a.step(ops, g, nc, t)
        torch.cuda.synchronize()
        clip = float(nc[1])
        assert 0 < clip < 0.1                                   # the coefficient really scales the gradient
        adamw_ema_fp64(p64, m64, v64, e64, g, clip, t)
        close(f"{build16} step {t} p", a.p, p64)
        close(f"{build16} step {t} ema", a.ema, e64)
        close(f"{build16} step {t} exp_avg", a.m, m64)
        # exp_avg_sq is far below the absolute term, so it is held relatively: the kernel forms 1 - beta2 from the fp32 beta2 it
        # is handed (1 - fl(0.999) = 0.99998713e-3, exact in fp32) where torch rounds the double 0.001: 1.29e-5 apart, plus a few u
        close(f"{build16} step {t} exp_avg_sq", a.v, v64, rtol=2e-5, atol=0.0)
        # the frozen tail: p, m, v bit-unchanged, the EMA and the shadow still move
        for k in ("p", "m", "v"):
            assert torch.equal(bits(getattr(a, k)[tail]), bits(base[k][tail])), k
        assert not torch.equal(a.ema[tail], ema_before[tail])
        # the shadow is the updated p in the operand type, bit for bit, everywhere
        assert torch.equal(bits(a.shadow), bits(a.p.to(dt)))


def test_adamw_ema_optional_outputs_and_segments_change_no_bit(dev, build16, base):
    from reed_amd import ops
    dt = DTYPE[build16]
    g = base["g"][0]
    nc = torch.tensor([123.0, 0.25], device=dev)
    full = Arena(base, dt).step(ops, g, nc, 1)
    assert Arena(base, dt).step(ops, g, nc, 1, ema=False).same(full, ("p", "m", "v", "shadow")) == []
    no_sh = Arena(base, dt).step(ops, g, nc, 1, shadow=False)
    assert no_sh.same(full, ("p", "m", "v", "ema")) == [] and (no_sh.shadow == 7.0).all()
    one = torch.tensor([123.0, 1.0], device=dev)                # a coefficient of exactly 1 is what no clipping means
    assert Arena(base, dt).step(ops, g, None, 1).same(Arena(base, dt).step(ops, g, one, 1)) == []
    # the pointer-offset segment form of reed_amd/optim.py: an uneven split, a segment across the end of the trained part,
    # and one wholly inside the frozen tail (g = m = v = NULL there)
    b = 4 * (1000 * 256 + 77)
    for segs in ([(0, b), (b, N_TOTAL)], [(0, b), (b, N_TRAIN + 400), (N_TRAIN + 400, N_TOTAL)], [(0, N_TRAIN), (N_TRAIN, N_TOTAL)]):
        assert Arena(base, dt).step(ops, g, nc, 1, segments=segs).same(full) == [], segs
    torch.cuda.synchronize()


def test_adamw_ema_with_a_loss_scaler(dev, build16, base):
    from reed_amd import ops
    dt = DTYPE[build16]
    g = base["g"][0]
    nc = torch.tensor([123.0, 0.25 / 1024], device=dev)        # coefficient / scale, as clip_finalize_scaled leaves it
    gs = g * 1024
    # a skipped step (found_inf = 1): p, m, v bit-unchanged, the EMA and the shadow are updated
    skip = torch.tensor([1024.0, 0.0, 1.0, 0.0], device=dev)
    a = Arena(base, dt).step(ops, gs, nc, 1, scaler=skip)
    for k in ("p", "m", "v"):
        assert torch.equal(bits(getattr(a, k)), bits(base[k])), k
    e64 = base["ema"].double() * DECAY + base["p"].double() * (1 - DECAY)
    close(f"{build16} skipped step ema", a.ema, e64)
    assert torch.equal(bits(a.shadow), bits(base["p"].to(dt)))
    # with a scaler the bias corrections come from state[3] (the steps actually taken): the host's are ignored
    st = torch.tensor([1024.0, 1.0, 0.0, 2.0], device=dev)
    right = Arena(base, dt).step(ops, gs, nc, 2, scaler=st)
    wrong = Arena(base, dt).step(ops, gs, nc, 2, scaler=st, bc=(0.5, 0.123))
    assert wrong.same(right) == []
    p64, m64, v64, e64 = (base[k].double() for k in ("p", "m", "v", "ema"))
    adamw_ema_fp64(p64, m64, v64, e64, g, 0.25, 2)
    close(f"{build16} scaler, bias corrections of step 2: p", right.p, p64)
    close(f"{build16} scaler, bias corrections of step 2: ema", right.ema, e64)
    # ... and differ from a step-1 correction by far more than the tolerance (the check above is not vacuous)
    assert float((Arena(base, dt).step(ops, g, torch.tensor([1.0, 0.25], device=dev), 1).p.double() - p64).abs().max()) > 1e-3
    torch.cuda.synchronize()


def test_adamw_ema_refuses_bad_sizes(dev):
    from reed_amd import ops
    x = torch.full((64,), 7.0, device=dev)
    for n_train, n_total in ((30, 64), (32, 62), (68, 64)):
        with pytest.raises(RuntimeError, match="multiples of 4"):
            ops.adamw_ema(x, x, x, x, None, None, n_train, n_total, None, LR, B1, B2, EPS, WD, 0.1, 0.001, DECAY)
    with pytest.raises(RuntimeError, match="null pointer"):
        ops.adamw_ema(x, None, x, x, None, None, 32, 64, None, LR, B1, B2, EPS, WD, 0.1, 0.001, DECAY)
    torch.cuda.synchronize()
    assert (x == 7.0).all()
