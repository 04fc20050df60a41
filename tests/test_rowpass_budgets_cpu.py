"""The error budgets of tests/rowpass_ref.py, proven on the CPU before the GPU tests rely on them.

Two conditions keep a budget honest: (a) the fp32 restatement of the kernel's own arithmetic stays at or below 0.6 of it,
which leaves the kernel the rest for the hardware's rsqrt and for FMA contraction, and (b) every realistic bug (a wrong
divisor, a dropped eps, swapped affine vectors, a sum over the wrong length, a dropped row or tail) leaves it, by a factor of
at least 20 for the qk-norm mutations.
"""
import pytest
import torch

from tests.rowpass_ref import (DTYPE, KINDS, MUTATIONS, QK_SHAPES, U, qk_inputs, qk_ratios, qk_reference, qk_restatement,
                               seq_sum_f32, sum_budget, ulp_out, worst)

_CACHE = {}


def _case(kind, shape):
    """(inputs, fp64 reference) of one (build type, shape): computed once, shared, never modified."""
    key = (kind, shape)
    if key not in _CACHE:
        inp = qk_inputs(*shape, kind)
        _CACHE[key] = (inp, qk_reference(inp))
    return _CACHE[key]


@pytest.mark.parametrize("shape", QK_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_stays_inside_the_budgets(kind, shape):
    inp, ref = _case(kind, shape)
    ratios = qk_ratios(qk_restatement(inp), ref)
    print(f"[qk-norm restatement, {kind}, {shape}] worst error / budget: " + ", ".join(f"{k} {v[0]:.3f}" for k, v in ratios.items()))
    assert set(ratios) == {"out", "stats", "dpre", "part", "total"}
    for k, (r, i) in ratios.items():
        assert r <= 0.6, (k, r, i)


# a sum of a2 over the first 64 elements is the whole sum at head_dim 64 (no bug there): that mutation runs at head_dim 72 only
@pytest.mark.parametrize("shape,mutation", [(s, m) for m in MUTATIONS for s in QK_SHAPES if not (m == "a2_64" and s[2] == 64)])
@pytest.mark.parametrize("kind", KINDS)
def test_budgets_reject_the_realistic_bugs(kind, shape, mutation):
    inp, ref = _case(kind, shape)
    ratios = qk_ratios(qk_restatement(inp, mutation=mutation), ref)
    top = max(r for r, _ in ratios.values())
    print(f"[qk-norm {mutation}, {kind}, {shape}] worst error / budget: " + ", ".join(f"{k} {v[0]:.3g}" for k, v in ratios.items()))
    assert top > 20, ratios
    # the fault shows where it is made: a forward bug in the forward output, a backward bug in the backward
    where = {"eps": "out", "var_unbiased": "out", "swap_w": "out", "a2_64": "dpre", "no_w_bwd": "dpre"}[mutation]
    assert ratios[where][0] > 20, (where, ratios)


def test_constant_segment_outputs_the_bias():
    """Variance 0: eps decides, xhat is exactly 0 and the output is b rounded to the output type."""
    for kind in KINDS:
        inp, ref = _case(kind, (5, 2, 64))
        assert torch.equal(ref["out"][0, 1, 1], inp["kb"].double())
        assert torch.equal(qk_restatement(inp)["out"][0, 1, 1], inp["kb"].to(DTYPE[kind]))


def _spacing(x, kind):
    """Distance from |x| to the next larger number of the type, through the bit pattern (nextafter for every type)."""
    t = torch.tensor([abs(x)], dtype=DTYPE[kind])
    it = torch.int32 if kind == "fp32" else torch.int16
    up = (t.view(it) + 1).view(DTYPE[kind])
    return float(up.double() - t.double())


@pytest.mark.parametrize("kind", KINDS)
def test_ulp_out_is_the_spacing_of_the_type(kind):
    p, emin, emax = {"bf16": (7, -126, 127), "fp16": (10, -14, 15), "fp32": (23, -126, 127)}[kind]
    vals = [2.0 ** e for e in range(emin - p, emax + 1)]                  # every power of two, the subnormal range included
    vals += [1.5 * 2.0 ** e for e in (emin - 3, emin, -1, 0, 1, emax - 1)] + [3.0, 0.1, 1 - 2.0 ** -9]
    vals = [float(torch.tensor(v, dtype=DTYPE[kind])) for v in vals]       # representable in the type
    for v in vals:
        for s in (v, -v):
            assert float(ulp_out(torch.tensor(s, dtype=torch.float64), kind)) == _spacing(v, kind), (kind, s)
    # a reference between two numbers of the type has the spacing of the one below
    assert float(ulp_out(torch.tensor(3.0 + 2.0 ** -30, dtype=torch.float64), kind)) == _spacing(3.0, kind)
    # the largest finite value: the step up is infinite, the spacing is the one below it
    big = torch.finfo(DTYPE[kind]).max
    t = torch.tensor([big], dtype=DTYPE[kind])
    it = torch.int32 if kind == "fp32" else torch.int16
    down = (t.view(it) - 1).view(DTYPE[kind])
    assert float(ulp_out(torch.tensor(big, dtype=torch.float64), kind)) == float(t.double() - down.double())
    # zero and everything below the minimum normal: the subnormal spacing
    sub = 2.0 ** (emin - p)
    assert float(ulp_out(torch.tensor(0.0, dtype=torch.float64), kind)) == sub
    assert float(ulp_out(torch.tensor(sub * 0.25, dtype=torch.float64), kind)) == sub
    if kind == "fp16":
        for v in (2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -15, 1023 * 2.0 ** -24):
            assert float(ulp_out(torch.tensor(v, dtype=torch.float64), kind)) == 2.0 ** -24 == _spacing(v, kind)


@pytest.mark.parametrize("R,N", [(1, 100), (3, 64), (16, 384), (64, 260), (257, 288), (1000, 100), (4097, 64)])
def test_sequential_sum_stays_inside_and_a_dropped_row_leaves(R, N):
    g = torch.Generator().manual_seed(R * 131 + N)
    x = torch.randn(R, N, generator=g) * torch.exp(torch.randn(R, 1, generator=g)) + 0.25
    ref, b = sum_budget(x, 0)
    r_ok, _ = worst((seq_sum_f32(x).double() - ref).abs(), b)
    print(f"[sequential fp32 sum, R={R}, N={N}] worst error / budget {r_ok:.3f}")
    assert r_ok <= 0.6
    if R > 1:
        r_bad, _ = worst((seq_sum_f32(x[:-1]).double() - ref).abs(), b)
        print(f"[sequential fp32 sum, R={R}, N={N}] without the last row: {r_bad:.3g}")
        assert r_bad > 1, r_bad
    # with a 16-bit output the budget gains that type's rounding; a row dropped from up to 64 still leaves it (one row of
    # several hundred is below the resolution of an 8-bit mantissa: the kernels with such an output are tested at T <= 64 too)
    for kind in ("bf16", "fp16"):
        ref_k, b_k = sum_budget(x.to(DTYPE[kind]), 0, kind)
        got = seq_sum_f32(x.to(DTYPE[kind])).to(DTYPE[kind])
        assert worst((got.double() - ref_k).abs(), b_k)[0] <= 0.6
        if 1 < R <= 64:
            assert worst((seq_sum_f32(x.to(DTYPE[kind])[:-1]).to(DTYPE[kind]).double() - ref_k).abs(), b_k)[0] > 1


@pytest.mark.parametrize("n", [7, 1027, 4 * 300 + 2, 64 * 256 * 4 + 3])
def test_sum_of_squares_stays_inside_and_a_dropped_tail_leaves(n):
    """The optimiser's norm: positive terms, so the relative bound n u holds for a chain and 64 u covers the kernel's tree
    (at most 2 laps x 4 + 2 + 6 + 2 + 12 additions deep for the sizes tested, plus the squares' own rounding)."""
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g)
    sq = (x * x)
    ref, b = sum_budget(sq.double(), 0)
    assert worst((seq_sum_f32(sq).double() - ref).abs(), b)[0] <= 0.6
    # the kernel's shape: four elements per thread, a tree over the rest; its norm is within 64 u relative
    n4 = n & ~3
    per = (x[:n4].reshape(-1, 4) ** 2).double().float().sum(1)
    tree = float(per.sum()) + float((x[n4:] ** 2).sum())
    exact = float((x.double() ** 2).sum())
    assert abs(tree ** 0.5 - exact ** 0.5) <= 64 * U * exact ** 0.5
    # dropping the n & 3 tail elements moves the norm by far more than 64 u once the tail is not negligible
    x2 = x.clone()
    x2[n4:] = 3.0
    exact2 = float((x2.double() ** 2).sum())
    dropped = float((x2[:n4].double() ** 2).sum())
    assert abs(dropped ** 0.5 - exact2 ** 0.5) > 20 * 64 * U * exact2 ** 0.5
