"""The two input-gradient kernels of csrc/embed.hip against fp64, in all three builds: reed_patch_embed_bwd_x (the streaming K = 16
form and the generic kernel at K = 8, 16, 64, 256) and reed_timestep_sinusoid_bwd.  tests/input_grad_ref.py holds the references
and the budgets (proven on the CPU in tests/test_input_grad_budgets_cpu.py).  The protocol of tests/test_embed_gpu.py: every output
lives in a NaN pre-filled buffer with a canary band behind it, every call runs twice and must give the same bits, every element is
held to its budget and the worst one is named, bad shapes are refused without a launch.  profiles/input_grad_tests.txt records the
measured ratios.

Patch-embed shapes (B, C, HW, P, D) — embed_ref.PATCH_SHAPES and one more:
  (1, 4, 2, 2, 4)      one token (a pair with its second token missing), one live lane
  (5, 4, 18, 2, 1280)  405 tokens = 12 blocks of 32 + 21: ten pairs and a single token in the last block; five full groups of 64 loads
  (5, 4, 18, 2, 1284)  past the streaming form's width: the generic kernel at K = 16, 21 columns in the first 4 lanes' chains
  (3, 4, 12, 4, 260)   K = 64; 27 tokens (a tail of 3 in a block of 4 waves)
  (3, 2, 6, 2, 72)     K = 8
  (1, 4, 16, 8, 128)   K = 256
  (2, 4, 6, 2, 328)    added for the streaming form's own tail: 82 loads per row, the second group of 64 with 18 live lanes; 18
                       tokens: 9 pairs over 4 waves
At K = 16 the 16-bit builds run a second time with the weight at 8 (mod 16): the entry point then takes the generic kernel.
"""
import pytest
import torch

from tests import embed_ref as E
from tests import input_grad_ref as R
from tests.rowpass_ref import Guarded
from tests.test_embed_gpu import _show, build, twice  # noqa: F401  (build: the fixture over the three libraries)
from tests.test_final_layer_gpu import _at, _placements, inside

pytestmark = pytest.mark.gpu
F32 = torch.float32


def _refused(fn, out):
    """fn() must raise without a launch: the NaN pre-fill of `out` is still there."""
    with pytest.raises(RuntimeError, match="code 1001"):
        fn()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.t).all()) and out.intact()


@pytest.mark.parametrize("B,C,HW,P,D", R.PATCH_SHAPES)
def test_patch_embed_bwd_x(dev, build, B, C, HW, P, D):
    from reed_amd import ops
    kind = build
    inp = R.bwdx_inputs(B, C, HW, P, D, kind)
    K, n = inp["K"], B * C * HW * HW
    dtok = inp["dtok"].to(dev)
    assert dtok.data_ptr() % 16 == 0
    seen = []
    for residue in (_placements(kind) if K == 16 else (0,)):
        w = _at(inp["w"].to(dev), residue, dev)
        form = R.bwdx_form(K, D, residue == 0)
        seen.append(form)
        ref = R.bwdx_reference(inp, form)

        def run():
            dx = Guarded(n, F32, dev)
            ops.patch_embed_bwd_x(dtok, w, dx.t, B, C, HW, P, D)
            return (dx,)

        (dx,) = twice(run)
        tag = f"patch embed dL/dx {kind} {(B, C, HW, P, D)} K={K} weight at {residue} (mod 16): {form}"
        _show(tag, {"dx": inside(tag, dx.t, ref["dx"], ref["b_dx"])})
    assert seen[0] == ("generic" if K != 16 or D > 1280 else "stream16") and all(f == "generic" for f in seen[1:])


def test_patch_embed_bwd_x_refuses_bad_shapes(dev, build):
    from reed_amd import ops
    dt = R.DTYPE[build]
    dtok, w = torch.zeros(64, 8, device=dev), torch.zeros(8, 64, device=dev, dtype=dt)
    out = Guarded(4 * 4 * 8 * 8, F32, dev)
    for B, C, HW, P in ((1, 4, 7, 2), (1, 3, 8, 2), (0, 4, 8, 2), (1, 4, 8, 0)):        # HW % P, C P P % 8, no samples, no patch
        _refused(lambda: ops.patch_embed_bwd_x(dtok, w, out.t, B, C, HW, P, 8), out)    # noqa: B023
    _refused(lambda: ops.patch_embed_bwd_x(dtok, w, out.t, 1, 4, 8, 2, 0), out)
    _refused(lambda: ops.patch_embed_bwd_x(None, w, out.t, 1, 4, 8, 2, 8), out)


@pytest.mark.parametrize("dim,max_period", E.SIN_CASES)
def test_timestep_sinusoid_bwd(dev, build, dim, max_period):
    from reed_amd import ops
    inp = R.sinb_inputs(dim)
    ref = R.sinb_reference(inp, max_period)
    t, dsin = inp["t"].to(dev), inp["dsin"].to(dev)
    Bn = len(t)

    def run():
        dt = Guarded(Bn, F32, dev)
        ops.timestep_sinusoid_bwd(t, dsin, dt.t, Bn, dim, max_period)
        return (dt,)

    (dt,) = twice(run)
    tag = f"sinusoid dL/dt {build} dim {dim} max_period {max_period:g}"
    _show(tag, {"dt": inside(tag, dt.t, ref["dt"], ref["b_dt"])})
    out = Guarded(Bn, F32, dev)
    _refused(lambda: ops.timestep_sinusoid_bwd(t, dsin, out.t, Bn, 1, max_period), out)
    _refused(lambda: ops.timestep_sinusoid_bwd(t, dsin, out.t, 0, dim, max_period), out)
