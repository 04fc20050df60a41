"""The reductions and casts of csrc/norm.hip that the rest of the suite reaches only through whole models: token_mean_fwd / bwd,
cast_bf16, rowsum_f32, colsum_bf16, reduce_slabs.

Rules for every case: the reference is fp64 (or the same fp32 chain where the kernel's order is one chain with no products,
which makes it bit-exact); the budget is n u sum|terms| over the n values summed into one output, plus ulp_out(ref) where the
output is 16-bit (tests/rowpass_ref.py; proven on the CPU in tests/test_rowpass_budgets_cpu.py); outputs are pre-filled with
NaN unless accumulating, a canary band follows every output, and every case runs twice and must give the same bits.
"""
import pytest
import torch

from tests.rowpass_ref import DTYPE, KINDS, U, Guarded, bits, ulp_out

pytestmark = pytest.mark.gpu


@pytest.fixture(params=KINDS)
def build(request, dev):
    from reed_amd import ops
    prev = ops.use(request.param)
    yield request.param
    ops.use(prev)


@pytest.fixture(params=["bf16", "fp16"])
def build16(request, dev):
    from reed_amd import ops
    prev = ops.use(request.param)
    yield request.param
    ops.use(prev)


def rand(shape, seed, dev, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def inside(tag, got, ref, budget):
    """Worst |got - ref| / budget over the elements (device tensors), printed; outside, the element is named."""
    err = (got.double() - ref).abs().flatten()
    ratio = torch.where(torch.isfinite(err), err / budget.flatten(), torch.full_like(err, float("inf")))
    ratio = torch.where((err == 0) & (budget.flatten() == 0), torch.zeros_like(ratio), ratio)
    i = int(torch.argmax(ratio))
    r = float(ratio[i])
    assert r <= 1.0, (f"{tag}: element {i}: got {float(got.flatten()[i])!r}, fp64 {float(ref.flatten()[i])!r}, budget "
                      f"{float(budget.flatten()[i]):.3e}, ratio {r:.3g}")
    return r


def twice(fn):
    """Run fn() -> tuple of Guarded twice: canaries intact, the same bits both times.  Returns the first run's outputs."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert x.intact() and y.intact(), "written past the end of an output"
        assert torch.equal(bits(x.full), bits(y.full)), "two runs differ"
    return a


# ---------------------------------------------------------------------------------------------------------- token_mean
@pytest.mark.parametrize("B,T,D", [(3, 16, 384), (2, 256, 1152), (1, 1, 100), (2, 64, 260)])
def test_token_mean_fwd_bwd(dev, build, B, T, D):
    from reed_amd import ops
    kind, dt = build, DTYPE[build]
    x = rand((B, T, D), 7 * T + D, dev) + 0.3

    def fwd():
        out = Guarded(B * D, dt, dev)
        ops.token_mean_fwd(x, out.t, B, T, D)
        return (out,)

    out, = twice(fwd)
    terms = x.double() / T
    ref = terms.sum(1)
    budget = T * U * terms.abs().sum(1)
    if kind != "fp32":
        budget = budget + ulp_out(ref.cpu(), kind).to(dev)
    r_f = inside(f"token_mean_fwd {kind} {(B, T, D)}", out.t.view(B, D), ref, budget)

    # backward: adds g / T onto a non-zero dx
    g = rand((B, D), 11 * T + D, dev, 0.05).to(dt)
    dx0 = rand((B, T, D), 13 * T + D, dev)

    def bwd():
        dx = Guarded(B * T * D, torch.float32, dev)
        dx.t.copy_(dx0.flatten())
        ops.token_mean_bwd(g, dx.t, B, T, D)
        return (dx,)

    dx, = twice(bwd)
    gt = g.float() / T                                       # fp32(g) / T, correctly rounded
    want = (dx0 + gt[:, None, :]).double()                   # fp32(dx0 + fp32(g) / T)
    budget = 2 * U * (dx0.double().abs() + gt.double().abs()[:, None, :].expand(B, T, D))
    r_b = inside(f"token_mean_bwd {kind} {(B, T, D)}", dx.t.view(B, T, D), want, budget)
    print(f"[token_mean {kind} {(B, T, D)}] worst error / budget: fwd {r_f:.3f}, bwd {r_b:.3f}")


def test_token_mean_refuses_bad_arguments(dev, build):
    from reed_amd import ops
    x = torch.ones(2 * 4 * 8, device=dev)
    out = torch.full((2 * 8,), 7.0, dtype=DTYPE[build], device=dev)
    for B, T, D in ((0, 4, 8), (2, 0, 8), (2, 4, 0), (2, -1, 8)):
        with pytest.raises(RuntimeError, match="token_mean_fwd"):
            ops.token_mean_fwd(x, out, B, T, D)
        with pytest.raises(RuntimeError, match="token_mean_bwd"):
            ops.token_mean_bwd(out, x, B, T, D)
    for a in ((None, out), (x, None)):
        with pytest.raises(RuntimeError, match="null pointer"):
            ops.token_mean_fwd(*a, 2, 4, 8)
    for a in ((None, x), (out, None)):
        with pytest.raises(RuntimeError, match="null pointer"):
            ops.token_mean_bwd(*a, 2, 4, 8)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (x == 1.0).all()          # nothing was launched


# ------------------------------------------------------------------------------------------------------------ cast_bf16
def _specials(kind):
    t = 2.0 ** -8 if kind == "bf16" else 2.0 ** -11           # half an ulp of the 16-bit type at 1.0: exact ties
    return torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1 + t, 1 + 3 * t, -(1 + t), -(1 + 3 * t),
                         1 + t + 2.0 ** -20, 1 + t - 2.0 ** -20, 65504.0, 65519.996, 65520.0, -65520.0, 65536.0, 3.38e38, 3.39e38,
                         3.4e38, -3.4e38, 1e-45, -1e-45, 1e-40, 2.0 ** -126, 2.0 ** -127, 2.0 ** -133, 2.0 ** -134, 1.5 * 2.0 ** -134,
                         2.0 ** -14, 2.0 ** -15, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, -(2.0 ** -25), 6.1e-5, 5.97e-8, 1.0, -2.5],
                        dtype=torch.float32)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 4096 * 256 * 4 + 1027])
def test_cast_to_the_16_bit_type_bit_exact(dev, build16, n):
    """Against torch's own cast (round to nearest even, subnormals kept, overflow to inf: 65520 in fp16, 3.4e38 in bf16).  A NaN
    stays a NaN; every other value has torch's bits.  The last size is a grid-stride lap plus the scalar tail."""
    from reed_amd import ops
    kind, dt = build16, DTYPE[build16]
    sp = _specials(kind)
    src = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 3
    k = min(n, sp.numel())
    src[:k] = sp.roll(n % 7)[:k]                            # head: the vector path
    src[n - k:] = sp.roll(n % 5)[:k].flip(0)                # tail: the last n & 3 elements take the scalar path
    want = src.to(dt).to(dev)
    src = src.to(dev)

    def run():
        dst = Guarded(n, dt, dev)
        ops.cast_bf16(src, dst.t, n)
        return (dst,)

    dst, = twice(run)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(dst.t), nan)
    assert torch.equal(bits(dst.t)[~nan], bits(want)[~nan])
    if n >= 8:      # a misaligned source (16 bytes) or destination (8 bytes) is refused
        d2 = torch.full((n,), 7.0, dtype=dt, device=dev)
        with pytest.raises(RuntimeError, match="misaligned"):
            ops.cast_bf16(src.data_ptr() + 4, d2, n - 4)
        with pytest.raises(RuntimeError, match="misaligned"):
            ops.cast_bf16(src, d2.data_ptr() + 2, n - 4)
        torch.cuda.synchronize()
        assert (d2 == 7.0).all()


# ----------------------------------------------------------------------------------------------------------- rowsum_f32
@pytest.mark.parametrize("R", [1, 3, 255, 256, 257, 1000, 4097])
def test_rowsum_f32(dev, R):
    """R = 256 / 257 is the switch to the two-stage form (with ws), 4097 its ragged last 64-row stage; N = 288 is the engine's
    4 x head_dim 72, 100 is no multiple of 64."""
    from reed_amd import ops
    top = 0.0
    for N in (288, 100, 64, 1152):
        part = rand((R, N), R * 7 + N, dev) * torch.exp(rand((R, 1), R + N, dev)) + 0.25
        base = rand((N,), N, dev)
        ws = torch.full(((R + 63) // 64 * N,), float("nan"), device=dev)
        for use_ws in (False, True):
            for acc in (False, True):
                def run():
                    out = Guarded(N, torch.float32, dev)
                    if acc:
                        out.t.copy_(base)
                    ops.rowsum_f32(part, R, out.t, N, acc, ws=ws if use_ws else None)
                    return (out,)

                out, = twice(run)
                terms = torch.cat([part, base[None]]) if acc else part
                ref = terms.double().sum(0)
                budget = terms.shape[0] * U * terms.double().abs().sum(0)
                top = max(top, inside(f"rowsum_f32 R={R} N={N} ws={use_ws} accumulate={acc}", out.t, ref, budget))
    print(f"[rowsum_f32 R={R}] worst error / budget {top:.3f}")


# ---------------------------------------------------------------------------------------------------------- colsum_bf16
@pytest.mark.parametrize("M", [1, 255, 256, 257, 1000])
def test_colsum(dev, build, M):
    """M = 255 / 256 / 257: the edge of the whole-slice fast path; N = 2052: a second 1024-column block with 4 columns in it;
    ld = N + 8 with the pad columns at 1e4: a read through the wrong stride, or past N, shows."""
    from reed_amd import _lib, ops
    kind, dt = build, DTYPE[build]
    top = 0.0
    for N in (4, 132, 1152, 2052):
        nws = int(_lib.load(kind).reed_colsum_ws_floats(M, N))
        assert nws == -(-M // 256) * N == ops.colsum_ws_floats(M, N)
        base = rand((N,), N + 1, dev)
        for ld in (N, N + 8):
            x = torch.full((M, ld), 1e4, dtype=dt, device=dev)
            x[:, :N] = (rand((M, N), M * 3 + N, dev) * torch.exp(rand((M, 1), M + N, dev)) + 0.25).to(dt)
            for acc in (False, True):
                def run():
                    out, ws = Guarded(N, torch.float32, dev), Guarded(nws, torch.float32, dev)
                    if acc:
                        out.t.copy_(base)
                    ops.colsum_bf16(x, ld, ws.t, out.t, M, N, acc)
                    return out, ws

                out, ws = twice(run)
                assert not torch.isnan(ws.t).any()
                terms = x[:, :N].double()
                if acc:
                    terms = torch.cat([terms, base.double()[None]])
                ref = terms.sum(0)
                budget = terms.shape[0] * U * terms.abs().sum(0)
                top = max(top, inside(f"colsum {kind} M={M} N={N} ld={ld} accumulate={acc}", out.t, ref, budget))
    print(f"[colsum {kind} M={M}] worst error / budget {top:.3f}")


# --------------------------------------------------------------------------------------------------------- reduce_slabs
@pytest.mark.parametrize("n", [1, 255, 257, 1152 * 384 + 3])
def test_reduce_slabs_bit_exact(dev, n):
    """out[i] (+)= sum_z slabs[z * stride + i]: one sequential fp32 chain without products, so the same chain in torch fp32
    gives the same bits.  The pad between slabs holds 1e4."""
    from reed_amd import ops
    base = rand((n,), n, dev)
    for nslabs in (1, 2, 7):
        for stride in (n, n + 12):
            slabs = torch.full((nslabs, stride), 1e4, device=dev)
            slabs[:, :n] = rand((nslabs, n), n + nslabs, dev) * 3
            for acc in (False, True):
                def run():
                    out = Guarded(n, torch.float32, dev)
                    if acc:
                        out.t.copy_(base)
                    ops.reduce_slabs(slabs, stride, nslabs, out.t, n, acc)
                    return (out,)

                out, = twice(run)
                want = base.clone() if acc else torch.zeros(n, device=dev)
                for z in range(nslabs):
                    want = want + slabs[z, :n]
                assert torch.equal(bits(out.t), bits(want)), (n, nslabs, stride, acc)
