"""The budget of tests/tf32_ref.py proven on the CPU, and the host side of the split fp32 GEMM (no GPU): the knob in the three
builds of the library, the planner's kernel id, and the command lines that select the mode.

Budget: the fp32 restatement of the split (hi / lo, three exact products, fp32 sums in the kernel's order) stays at or below 0.6
of it on every shape of the GPU test; each realistic bug of the split leaves it by more than 20 times; and the two modes the
kernel stands in for — operands rounded once to TF32 or to IEEE half — exceed it too: it is sharper than either."""
import pytest
import torch

from tests import gemm_ref as G
from tests import tf32_ref as T

_INP = {}


def _inputs(sh):
    if sh not in _INP:
        _INP[sh] = G.inputs(sh, T.KIND)
    return _INP[sh]


def _ratios(inp, layout, epi, var, mutation=None):
    got = {k: v.double() for k, v in T.restatement(inp, layout, epi, var, mutation).items()}
    return {k: r for k, (r, _) in G.ratios(got, T.reference(inp, epi, var, got)).items()}


def _all_calls():
    for layout, epis in ((T.NT, T.EPIS_NT), (T.NN, T.EPIS_NN)):
        for sh in T.SHAPES:
            for epi in epis:
                for var in T.calls(layout, epi, sh):
                    yield layout, epi, sh, var
    for sh, vs in T.TN_CASES:
        for v in vs:
            epi = G.ATOMIC_F32 if v.get("split") == 4 else G.F32
            yield T.TN, epi, sh, G.with_bias(T.row(T.TN), epi, v)


def test_restatement_within_0p6_of_budget():
    worst = 0.0
    for layout, epi, sh, var in _all_calls():
        for k, r in _ratios(_inputs(sh), layout, epi, var).items():
            assert r <= 0.6, (G.LAY_NAME[layout], G.EPI_NAME[epi], tuple(sh[:3]), var, k, r)
            worst = max(worst, r)
    print(f"split restatement: worst error / budget {worst:.3f}")


@pytest.mark.parametrize("mutation", T.MUTATIONS)
def test_mutations_leave_the_budget(mutation):
    """Every bug of the split itself shows in the plain accumulator output (epilogue 0 / 6 on NT and NN, the slabs' sum on TN) by
    more than 20 budgets.  lo from x, hi for both halves and the missing zero fill do so at every shape they apply to.  A DROPPED
    CROSS TERM is different in kind: it loses up to 2^-9 |a||b| per product, but with the sign of a rounding error, so over a
    K-term sum of these random inputs it grows like sqrt(K) while the budget, a worst-case bound, grows like K (and its
    accumulator term like K^2): the error / budget ratio falls roughly as 2^-9 / (sqrt(K) (3 * 2^-16 + 3 K u')) — about 60 at
    K = 8, 25 at K = 36 / 40, 13 at K = 64, 4 at K = 320 and below 1 at K = 1000.  So the 20 x is asserted where K <= 40 (three
    shapes, all three layouts) and the ratio is printed for the rest: at large K no worst-case budget can tell a dropped cross
    term from rounding on random data; the kernel-level guard against it is the K <= 40 shapes of the GPU test, whose budgets the
    same bug leaves by the same factors."""
    cross = mutation.startswith("drop_")
    hit = 0
    for layout, epi, sh, var in _all_calls():
        if epi not in (G.BF16, G.F32) or not T.mutation_applies(mutation, sh):
            continue
        r = _ratios(_inputs(sh), layout, epi, var, mutation)["C"]
        if cross and sh.K > 40:
            print(f"{mutation} {G.LAY_NAME[layout]} {tuple(sh[:3])}: error / budget {r:.1f} (not asserted: K > 40)")
            continue
        assert r > 20, (mutation, G.LAY_NAME[layout], tuple(sh[:3]), var, r)
        hit += 1
    assert hit >= (2 if mutation == "lo_not_zero_filled" else 8), hit


@pytest.mark.parametrize("how", ["tf32", "fp16"])
def test_budget_is_sharper_than_the_modes_it_stands_in_for(how):
    """A @ W^T with both operands rounded once to TF32 (10 mantissa bits) or to IEEE half, accumulated exactly: outside the budget.
    As with the dropped cross terms above, these are rounding errors of random sign — 2 * 2^-11 |a||b| per product at most, about
    2e-3 / sqrt(K) of sum|a||b| at the worst element of a shape — against a worst-case budget of 3 * 2^-16 + (3 K + 1) u': the
    ratio is about 2e-3 / (sqrt(K) (4.6e-5 + 3.6e-7 K)), i.e. 8 at K = 8, 2 at K = 128 and 0.7 at K = 320.  Asserted where
    K <= 128 (four of the five shapes), printed at K = 320."""
    for sh in T.SHAPES:
        inp = _inputs(sh)
        var = G.with_bias(T.row(T.NT), G.F32, {})
        got = {"C": T.rounded_operands(inp, how) + inp["bias"].double()}
        r = G.ratios(got, T.reference(inp, G.F32, var, got))["C"][0]
        print(f"{how} operands at {tuple(sh[:3])}: worst error / split budget {r:.1f}" + (" (not asserted: K > 128)" if sh.K > 128 else ""))
        assert r > 1 or sh.K > 128, (how, tuple(sh[:3]), r)


def test_split_helpers():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -9, 3.14159274, -1e-3, 65504.0 * 3, 0.0])
    hi, lo = T.split(x)
    assert torch.equal(hi, x.bfloat16().float()) and torch.equal(lo, (x - hi).bfloat16().float())
    assert ((x - hi - lo).abs() <= 2.0 ** -17 * x.abs()).all()
    t = T.tf32_round(torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -10, -(1.0 + 2.0 ** -12)]))
    assert torch.equal(t, torch.tensor([1.0, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -10, -1.0]))     # ties to even, then exact, then down
    assert abs(T.scale(64) * 65 * 2 * T.U - (T.SPLIT_TERM + 193 * 2 * T.U)) < 1e-18


# ------------------------------------------------------------------------------------------------------------------- ABI
def test_knob_in_the_three_builds():
    """reed_gemm_f32_split: the fp32-operand library takes 0 and 1; the 16-bit libraries take 0 and refuse 1 with 1002 and a
    message (their operands are 16-bit already)."""
    from reed_amd import _lib
    for prec in ("bf16", "fp16"):
        L = _lib.load(prec)
        assert L.reed_gemm_f32_split(0) == 0
        assert L.reed_gemm_f32_split(1) == 1002 and b"16-bit" in L.reed_last_error()
        assert L.reed_gemm_f32_split(0) == 0
    L = _lib.load("fp32")
    try:
        assert L.reed_gemm_f32_split(1) == 0
    finally:
        assert L.reed_gemm_f32_split(0) == 0


def test_plan_names_the_split_kernel_while_the_mode_is_on():
    from reed_amd import ops
    assert ops.f32_split_on() is False
    shapes = [(ops.NT, ops.EPI_BF16, 200, 132, 36, 1, {}), (ops.NN, ops.EPI_MUL, 300, 256, 128, 1, {}),
              (ops.TN, ops.EPI_F32, 132, 64, 1000, 3, dict(dbias=True, slab=True)), (ops.TN_TALL, ops.EPI_ATOMIC_F32, 256, 384, 1000, 4, {})]

    def plans():
        out = []
        for lay, epi, M, N, K, s, kw in shapes:
            rc, launches = ops.gemm_plan(lay, epi, M, N, K, s, precision="fp32", **kw)
            assert rc == 0 and len(launches) == 1
            out.append(launches[0])
        return out

    off = plans()
    assert [l["kernel"] for l in off] == ["f32"] * 4
    with ops.f32_split_mode(True):
        assert ops.f32_split_on() is True
        on = plans()
        with ops.build("fp32", tf32=False):             # a pass that asks for exact products inside one that asked for the split
            assert plans() == off
        assert plans() == on
    assert ops.f32_split_on() is False and plans() == off
    for (lay, epi, M, N, K, s, kw), a, b in zip(shapes, off, on):
        assert b["kernel"] == "f32_split" and {k: v for k, v in b.items() if k != "kernel"} == {k: v for k, v in a.items() if k != "kernel"}
        assert b["grid"] == -(-M // 128) * -(-N // 128) and (b["rows"], b["cols"]) == (M, N)   # the kernel's 128 x 128 tile
        assert b["splits"] == G.eff_splits(K, s)[0] and b["ksplit_len"] == G.eff_splits(K, s)[1]
    # the refusals are the same in both modes
    with ops.f32_split_mode(True):
        assert ops.gemm_plan(ops.NT, ops.EPI_BF16, 8, 130, 36, precision="fp32")[0] == 1001
        assert ops.gemm_plan(ops.NT, ops.EPI_SWIGLU, 128, 128, 64, precision="fp32")[0] == 1001
    # the 16-bit builds do not know the mode: f32_split leaves them alone
    with ops.f32_split_mode(True):
        assert ops.gemm_plan(ops.NT, ops.EPI_BF16, 256, 256, 128, precision="bf16")[1][0]["kernel"] in ops.GEMM_KERNELS[:9]


def test_mode_is_restored_when_a_block_raises():
    from reed_amd import ops
    with pytest.raises(RuntimeError, match="boom"):
        with ops.build("fp32", tf32=True):
            assert ops.f32_split_on() and ops._PRECISION == "fp32"
            raise RuntimeError("boom")
    assert not ops.f32_split_on() and ops._PRECISION == "bf16"
    assert ops.build_of("tf32") == ("fp32", True) and ops.build_of("fp32") == ("fp32", False) and ops.build_of("fp16") == ("fp16", False)
    from reed_amd import _lib
    assert _lib.PRECISIONS == ("bf16", "fp16", "fp32") and ops.precision_of(torch.float32) == "fp32"


# ------------------------------------------------------------------------------------------------------------------- CLI
def test_command_lines_select_the_mode():
    from reed_amd import dataset, generate, train
    from reed_amd.models.sit import SiT_models
    base = ["--exp-name", "x", "--model", "SiT-S/2", "--enc-type", "None"]
    a = train.parse_args(base + ["--mixed-precision", "no", "--allow-tf32"])
    assert a.gemm_tf32 is True and train.resolve_tf32(True, "no") is True
    for mp in ("fp16", "bf16"):
        assert train.parse_args(base + ["--mixed-precision", mp, "--allow-tf32"]).gemm_tf32 is False
    assert train.parse_args(base + ["--mixed-precision", "no"]).gemm_tf32 is False
    assert train.parse_args(base + ["--allow-tf32"]).gemm_tf32 is False                    # the default is fp16
    assert SiT_models["SiT-S/2"]().tf32 is False
    g = generate.build_parser().parse_args(["--sample-precision", "tf32"])
    assert generate.sample_precision(g) == "tf32"
    # --tf32 / --no-tf32 select what they selected before
    assert generate.sample_precision(generate.build_parser().parse_args([])) == "fp16"
    assert generate.sample_precision(generate.build_parser().parse_args(["--no-tf32"])) == "fp32"
    p = dataset.build_parser()
    assert p.parse_args(["encode", "src", "dst", "--vae-ckpt", "v", "--precision", "tf32"]).precision == "tf32"
    assert p.parse_args(["encode", "src", "dst", "--vae-ckpt", "v"]).precision == "fp32"
    assert p.parse_args(["convert", "src", "dst", "--resolution", "256", "--vae-sd-dest", "m", "--vae-ckpt", "v", "--precision",
                         "tf32"]).precision == "tf32"
