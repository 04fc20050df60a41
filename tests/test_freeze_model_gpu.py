"""Partly frozen reed_amd.SiT (reed_amd/freeze.py, Engine): requires_grad_(False) on part of the model is honoured by the forward
(a graph is built whenever anything trains), the backward (only the launches a trainable parameter needs; the chain stops where
nothing upstream trains) and autograd's bookkeeping (frozen p.grad stays None).

The bar is equality: at these sizes the launches that survive are the fully trainable model's kernels with the same arguments, so
every trainable gradient, dx and dt have the bits of the fully trainable run on the same inputs (the inputs and the functional of
tests/test_input_grad_model_gpu.py)."""
import fnmatch
import os

import pytest
import torch

from tests.rowpass_ref import KINDS, bits
from tests.test_input_grad_model_gpu import _case, _drop_grads, functional, hip_grads
from tests.test_model_gpu import build_hip_model
from tests.test_oracle_golden import TINY_CASES, inputs, tiny_cfg

pytestmark = pytest.mark.gpu

# name -> (freeze patterns | None, train-only patterns | None); depth 3: block 2 is the last one
SETS = {
    "a_x_embedder": (["x_embedder.*"], None),
    "b_last_block_final": (None, ["blocks.2.*", "final_layer.*"]),
    "c_projectors": (None, ["projectors.*"]),
    "d_biases": (["*.weight"], None),
    "e_one_fc1": (None, ["blocks.1.mlp.fc1.*"]),
    "f_one_adaln": (None, ["blocks.1.adaLN_modulation.*"]),
    "g_t_embedder": (None, ["t_embedder.*"]),
}
CASES = ("hd64", "two_split")
_FULL = {}


def apply_set(m, which):
    from reed_amd.freeze import select_parameters
    freeze, only = SETS[which] if isinstance(which, str) else which
    named = [(n, p) for n, p in m.named_parameters() if n != "pos_embed"]
    on = select_parameters([n for n, _ in named], freeze, only)
    for n, p in named:
        p.requires_grad_(n in on)
    return on


def grads_of(m):
    return {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


def full_run(dev, kind, case):
    """The fully trainable model on the case's inputs: parameter gradients, dx, dt.  Computed once, shared, never modified."""
    key = (kind, case)
    if key not in _FULL:
        m = build_hip_model(TINY_CASES[case]["cfg"], dev, 11)
        m.precision = kind
        dx, dt = hip_grads(m, dev, case, False)
        _FULL[key] = (grads_of(m), dx.clone(), dt.clone())
    return _FULL[key]


def check(m, on, base, tag):
    for n, p in m.named_parameters():
        if n in on:
            assert p.grad is not None, f"{tag}: {n} is trainable and has no gradient"
            assert torch.equal(bits(p.grad), bits(base[n])), f"{tag}: {n} differs from the fully trainable run"
        else:
            assert p.grad is None, f"{tag}: {n} is frozen and has a gradient"


# every set on hd64 and two_split; qknorm for the q/k-norm row sum: the sets that keep it, drop it with a block, and run it truncated
PARAMS = [(k, c, w) for k in KINDS for c in CASES for w in SETS] + \
         [(k, "qknorm", w) for k in KINDS for w in ("a_x_embedder", "b_last_block_final", "d_biases")]


@pytest.mark.parametrize("kind,case,which", PARAMS)
def test_partly_frozen_model(dev, kind, case, which):
    base, dx_full, dt_full = full_run(dev, kind, case)
    m = build_hip_model(TINY_CASES[case]["cfg"], dev, 11)
    m.precision = kind
    on = apply_set(m, which)
    assert on and len(on) < len(base)
    # no input requires grad: a graph all the same (with x_embedder frozen there was none), gradients where they belong
    assert hip_grads(m, dev, case, False, x_grad=False, t_grad=False) == (None, None)
    check(m, on, base, "parameters only")
    assert m._arena.grad is not None
    # twice: the same bits
    first = grads_of(m)
    _drop_grads(m)
    hip_grads(m, dev, case, False, x_grad=False, t_grad=False)
    again = grads_of(m)
    assert first.keys() == again.keys() and all(torch.equal(bits(first[n]), bits(again[n])) for n in first)
    # x and t require grad as well: dx / dt of the fully trainable model, the parameter gradients unchanged
    _drop_grads(m)
    dx, dt = hip_grads(m, dev, case, False)
    assert torch.equal(bits(dx), bits(dx_full)) and torch.equal(bits(dt), bits(dt_full))
    check(m, on, base, "with input gradients")
    # a flip between forward and backward is refused
    _drop_grads(m)
    cfg, x, t, y, drop = _case(case)
    m.force_drop_mask = drop
    out, zs = m(x.to(dev), t.to(dev), y.to(dev), inference=False)
    p = m.blocks[0].attn.qkv.weight
    p.requires_grad_(not p.requires_grad)
    with pytest.raises(RuntimeError, match="requires_grad changed"):
        functional(out, zs).backward()
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", KINDS)
def test_qk_norm_parameters_alone(dev, kind):
    """Only one block's q/k-norm affine trains: the chain stops behind that block's row sum."""
    base, _, _ = full_run(dev, kind, "qknorm")
    m = build_hip_model(TINY_CASES["qknorm"]["cfg"], dev, 11)
    m.precision = kind
    on = apply_set(m, (None, ["blocks.1.attn.?_norm.*"]))
    assert len(on) == 4
    hip_grads(m, dev, "qknorm", False, x_grad=False, t_grad=False)
    check(m, on, base, "q/k norm of block 1")


@pytest.mark.parametrize("kind", KINDS)
def test_truncated_backward_holds_fewer_activations(dev, kind):
    """Set (b): blocks 0 and 1 run no backward, so their forward saves nothing: the peak of forward + backward is strictly below the
    fully trainable model's on the same inputs (a condition, not a number: fewer tensors are alive)."""
    peaks = {}
    for which in (None, "b_last_block_final"):
        m = build_hip_model(TINY_CASES["hd64"]["cfg"], dev, 11)
        m.precision = kind
        if which:
            apply_set(m, which)
        hip_grads(m, dev, "hd64", False, x_grad=False, t_grad=False)      # workspaces, the gradient arena, the shadow
        _drop_grads(m)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        hip_grads(m, dev, "hd64", False, x_grad=False, t_grad=False)
        peaks[which] = torch.cuda.max_memory_allocated(dev) - before
        del m
    print(f"[freeze {kind}] peak of forward + backward over the resting state: fully trainable {peaks[None]} B, "
          f"last block + final layer {peaks['b_last_block_final']} B")
    assert peaks["b_last_block_final"] < peaks[None]


XL2 = tiny_cfg(D=1152, heads=16, depth=2, input_size=32, projector_dim=256)    # SiT-XL width, depth 2, T = 256


def _xl_grads(dev, kind, freeze=None):
    T = (XL2["input_size"] // XL2["patch_size"]) ** 2
    x, _, t, y, drop_u, _ = inputs(1, 4, XL2["input_size"], 11, [(128, "i")], T, XL2["num_classes"])
    m = build_hip_model(XL2, dev, 11)
    m.precision = kind
    on = apply_set(m, (freeze, None)) if freeze else {n for n, _ in m.named_parameters() if n != "pos_embed"}
    m.train()
    m.force_drop_mask = drop_u < XL2["class_dropout_prob"]
    out, zs = m(x.to(dev), t.to(dev), y.to(dev), inference=False)
    functional(out, zs).backward()
    torch.cuda.synchronize()
    return on, grads_of(m)


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_grouped_weight_gradients_beside_a_frozen_linear(dev, kind, monkeypatch):
    """The smallest size at which a block's four weight gradients go out as one grouped launch.  One linear of block 0 frozen:
    block 1 keeps the grouped launch (the fully trainable bits), block 0 takes the per-GEMM launches for its other three (the bits
    of a fully trainable run under REED_WGRAD_GROUP=0)."""
    from reed_amd import ops
    D, Hm = 1152, 4608
    with ops.build(kind):
        assert ops.wgrad_group_fits([(D, Hm), (Hm, D), (D, D), (3 * D, D)])
    _, grouped = _xl_grads(dev, kind)
    on, part = _xl_grads(dev, kind, freeze=["blocks.0.attn.proj.*"])
    monkeypatch.setenv("REED_WGRAD_GROUP", "0")
    _, single = _xl_grads(dev, kind)
    assert set(part) == on and "blocks.0.attn.proj.weight" not in part
    for n in part:
        want = single if (n.startswith("blocks.0.") and ".adaLN" not in n) else grouped
        assert torch.equal(bits(part[n]), bits(want[n])), n


@pytest.mark.parametrize("which", ["a_x_embedder", "b_last_block_final"])
def test_with_a_gradient_reducer_attached(dev, which):
    """Every bucket fires (at world 1 a no-op) and the backward completes with the bits it has without a reducer."""
    import torch.distributed as dist
    from reed_amd.parallel import GradReducer
    os.environ["REED_COMM"] = "torch"
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29741")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    base, _, _ = full_run(dev, "bf16", "hd64")
    m = build_hip_model(TINY_CASES["hd64"]["cfg"], dev, 11)
    on = apply_set(m, which)
    fired = []
    red = GradReducer(m, rank=0, world=1)
    ready = red.ready
    red.ready = lambda name: (fired.append(name), ready(name))[1]
    try:
        hip_grads(m, dev, "hd64", False, x_grad=False, t_grad=False)
        red.sync()
        torch.cuda.synchronize()
    finally:
        m.engine().reducer = None
        red.close()
    check(m, on, base, "with a reducer")
    assert sorted(fired) == sorted(red.buckets), (fired, list(red.buckets))
    assert fired[-1] == "embed" and len(set(fired)) == len(fired)
    assert set(fnmatch.filter(fired, "block*")) == {"block0", "block1", "block2"}
