"""Activation recomputation through reed_amd.SiT (reed_amd/recompute.py, Engine._recompute_block) on the tiny cases of
tests/test_oracle_golden.py, with the inputs and the functional of tests/test_input_grad_model_gpu.py.

The bar is equality: a recomputed block's backward reads arrays rebuilt by the forward's own launches on the forward's operands, so
every parameter gradient, dx and dt have the bits of the run of the same model on the same inputs with recompute = 0.  Setting an
unknown attribute on an nn.Module succeeds silently, so every test also checks that the recomputation HAPPENED: Engine.recomputed
(the blocks the last backward rebuilt) or the kind of record the forward left on the tape."""
import fnmatch
import os

import pytest
import torch

from reed_amd import lora
from reed_amd.recompute import block_bytes
from tests.rowpass_ref import KINDS, bits
from tests.test_freeze_model_gpu import SETS, apply_set
from tests.test_input_grad_model_gpu import _case, _drop_grads, functional, hip_grads
from tests.test_lora_model_gpu import build_lora_model
from tests.test_model_gpu import build_hip_model
from tests.test_oracle_golden import TINY_CASES, inputs, tiny_cfg

pytestmark = pytest.mark.gpu
DEPTH = 3
CASES = ("hd64", "two_split", "qknorm", "patch4")
_BASE = {}


def grads_of(m):
    return {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


def run(m, dev, case, value, inference=False, fresh=True, **kw):
    """One forward and backward at SiT.recompute = value: (parameter gradients, x.grad, t.grad, blocks the backward rebuilt)."""
    if fresh:
        _drop_grads(m)
    m.recompute = value
    dx, dt = hip_grads(m, dev, case, inference, **kw)
    return grads_of(m), dx, dt, m.engine().recomputed


def same(a, b, tag=""):
    ga, dxa, dta = a[:3]
    gb, dxb, dtb = b[:3]
    assert ga.keys() == gb.keys(), tag
    for n in ga:
        assert torch.equal(bits(ga[n]), bits(gb[n])), f"{tag}: {n} differs from the run without recomputation"
    for u, v, what in ((dxa, dxb, "x.grad"), (dta, dtb, "t.grad")):
        assert (u is None) == (v is None), (tag, what)
        if u is not None:
            assert torch.equal(bits(u), bits(v)), f"{tag}: {what} differs from the run without recomputation"


def base_run(dev, kind, case, inference):
    """(model, its run with recompute = 0): once per (build, case, inference), shared, the gradients never modified."""
    key = (kind, case, inference)
    if key not in _BASE:
        m = build_hip_model(TINY_CASES[case]["cfg"], dev, 11)
        m.precision = kind
        res = run(m, dev, case, 0, inference)
        assert res[3] == 0 and len(res[0]) > 10
        _BASE[key] = (m, res)
    return _BASE[key]


@pytest.mark.parametrize("inference", [True, False])
@pytest.mark.parametrize("kind,case", [(k, c) for k in KINDS for c in CASES + (("hd72",) if k == "fp32" else ())])
def test_gradients_keep_their_bits(dev, kind, case, inference):
    m, base = base_run(dev, kind, case, inference)
    try:
        for value, n in ((1, 1), (DEPTH - 1, DEPTH - 1), ("all", DEPTH)):
            res = run(m, dev, case, value, inference)
            assert res[3] == n, f"recompute={value}: the backward rebuilt {res[3]} blocks, not {n}"
            same(res, base, f"{kind} {case} inference={inference} recompute={value}")
    finally:
        m.recompute = 0


@pytest.mark.parametrize("sag", [False, True])
@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_both_forms_of_the_activation_backward(dev, kind, sag):
    """engine.save_act_grad pinned: the rebuilt fc1 runs the epilogue the tape's forward would have (derivative-saving or plain)."""
    m = build_hip_model(TINY_CASES["hd64"]["cfg"], dev, 11)
    m.precision = kind
    m.engine().save_act_grad = sag
    base = run(m, dev, "hd64", 0)
    res = run(m, dev, "hd64", "all")
    assert res[3] == DEPTH
    same(res, base, f"{kind} save_act_grad={sag}")


@pytest.mark.parametrize("which,blocks", [("b_last_block_final", 1), ("e_one_fc1", 2), ("c_projectors", 0), ("d_biases", 3)])
@pytest.mark.parametrize("kind", KINDS)
def test_with_freezing(dev, kind, which, blocks):
    """A partly frozen model: only the blocks that have a backward are recomputed (set b: block 2; e: blocks 1 and 2, block 1
    stopping behind fc1; c: none; d: all three), trainable gradients keep the bits of the partly frozen run, frozen ones stay None."""
    assert which in SETS
    m = build_hip_model(TINY_CASES["hd64"]["cfg"], dev, 11)
    m.precision = kind
    on = apply_set(m, which)
    for kw in (dict(x_grad=False, t_grad=False), dict()):
        base = run(m, dev, "hd64", 0, **kw)
        res = run(m, dev, "hd64", "all", **kw)
        want = blocks if kw else DEPTH      # with dx wanted the chain runs to the bottom: every block has a backward
        assert res[3] == want == sum(m.engine().plan_for(not kw, not kw).save), (res[3], want)
        same(res, base, f"{kind} {which} {kw}")
        assert set(res[0]) == on and all(p.grad is None for n, p in m.named_parameters() if n not in on)
    # a requires_grad flip between forward and backward is refused as ever
    _drop_grads(m)
    cfg, x, t, y, drop = _case("hd64")
    m.force_drop_mask = drop
    out, zs = m(x.to(dev), t.to(dev), y.to(dev), inference=False)
    p = m.blocks[0].attn.qkv.weight
    p.requires_grad_(not p.requires_grad)
    with pytest.raises(RuntimeError, match="requires_grad changed"):
        functional(out, zs).backward()
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", KINDS)
def test_frozen_weight_backward(dev, kind):
    """Everything requires_grad_(False), x and t require grad: the same dx and dt bits, no gradient arena."""
    f = build_hip_model(TINY_CASES["hd64"]["cfg"], dev, 11).requires_grad_(False)
    f.precision = kind
    base = run(f, dev, "hd64", 0)
    res = run(f, dev, "hd64", "all")
    assert res[3] == DEPTH and res[0] == {} and res[1] is not None and res[2] is not None
    same(res, base, f"{kind} frozen weights")
    assert all(p.grad is None for p in f.parameters()) and f._arena.grad is None
    _, _, dt_full, _ = base_run(dev, kind, "hd64", False)[1]
    assert torch.equal(bits(res[2]), bits(dt_full))


@pytest.mark.parametrize("case", ["hd64", "qknorm"])
@pytest.mark.parametrize("kind", KINDS)
def test_with_lora(dev, kind, case):
    """Adapters of rank 8 on all four linears: reed_lora_grads reads the rebuilt h, o, h2 and u."""
    m = build_lora_model(TINY_CASES[case]["cfg"], dev, 11, 8, 16)
    m.precision = kind
    base = run(m, dev, case, 0, x_grad=False, t_grad=False)
    res = run(m, dev, case, "all", x_grad=False, t_grad=False)
    assert res[3] == DEPTH
    ad = [n for n in res[0] if lora.is_adapter_key(n)]
    assert len(ad) == 2 * 4 * DEPTH and all(float(res[0][n].abs().max()) > 0 for n in ad)
    same(res, base, f"{kind} {case} lora")


@pytest.mark.parametrize("kind", ["bf16", "fp32"])
def test_accumulation_into_live_gradients(dev, kind):
    m, single = base_run(dev, kind, "hd64", False)
    try:
        acc = {}
        for value in (0, "all"):
            run(m, dev, "hd64", value)
            assert m.engine().grad_live
            acc[value] = run(m, dev, "hd64", value, fresh=False)      # the second micro-step adds to the first's gradients
        assert acc["all"][3] == DEPTH
        same(acc["all"], acc[0], f"{kind} two micro-steps")
        n = "blocks.1.mlp.fc1.weight"
        assert not torch.equal(bits(acc[0][0][n]), bits(single[0][n]))
    finally:
        m.recompute = 0
        _drop_grads(m)


@pytest.mark.parametrize("case", ["hd64", "xl3"])
def test_with_a_gradient_reducer_attached(dev, case):
    """The set-up of tests/test_freeze_model_gpu.py::test_with_a_gradient_reducer_attached: every bucket fires once, the bits are
    those of the run without recomputation.  xl3 is D = 1152, the width at which the planner has a choice of kernels on long
    token counts; at this test's few dozen tokens it picks the same kernel for the forward and the rebuild (see below)."""
    import torch.distributed as dist
    from reed_amd.parallel import GradReducer
    os.environ["REED_COMM"] = "torch"
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29741")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    m = build_hip_model(TINY_CASES[case]["cfg"], dev, 11)
    base = run(m, dev, case, 0, x_grad=False, t_grad=False)
    fired = []
    red = GradReducer(m, rank=0, world=1)
    ready = red.ready
    red.ready = lambda name: (fired.append(name), ready(name))[1]
    try:
        res = run(m, dev, case, "all", x_grad=False, t_grad=False)
        red.sync()
        torch.cuda.synchronize()
    finally:
        m.engine().reducer = None
        red.close()
    assert res[3] == DEPTH
    same(res, base, f"{case} with a reducer")
    assert sorted(fired) == sorted(red.buckets), (fired, list(red.buckets))
    assert fired[-1] == "embed" and len(set(fired)) == len(fired)
    assert set(fnmatch.filter(fired, "block*")) == {"block0", "block1", "block2"}


@pytest.mark.parametrize("case", ["hd64", "xl3"])
def test_rebuilt_beside_a_collective(dev, case):
    """The backward of a data-parallel step runs inside ops.set_concurrent_comm(True), the forward outside it: the rebuild's launches
    go through the planner in that state and give the bits the forward's would have saved.  What this shows is the plumbing: the
    switch only trades the persistent form of the four-wave 256^2 kernel for its one-shot form, which needs several tiles per
    workgroup, and at these token counts forward and rebuild run the same kernel.  That two different GEMM kernels give the same
    bits on one problem is what tests/test_gemm_gpu.py holds (test_concurrent_comm_switch_keeps_results and the forced-tile
    256 / 257 / 258 comparisons): the rebuild's equality at scale rests on those."""
    from reed_amd import ops
    m = build_hip_model(TINY_CASES[case]["cfg"], dev, 11)
    cfg, x, t, y, drop = _case(case)
    m.train()
    m.force_drop_mask = drop
    got = {}
    for value in (0, "all"):
        _drop_grads(m)
        m.recompute = value
        out, zs = m(x.to(dev), t.to(dev), y.to(dev), inference=False)
        ops.set_concurrent_comm(True)
        try:
            functional(out, zs).backward()
            torch.cuda.synchronize()
        finally:
            ops.set_concurrent_comm(False)
        got[value] = (grads_of(m), None, None, m.engine().recomputed)
    assert got["all"][3] == DEPTH and got[0][3] == 0
    same(got["all"], got[0], f"{case} backward beside a collective")


def _run_cfg(m, dev, cfg, zspec, B, value):
    T = (cfg["input_size"] // cfg["patch_size"]) ** 2
    x, _, t, y, drop_u, _ = inputs(B, 4, cfg["input_size"], 11, zspec, T, cfg["num_classes"])
    _drop_grads(m)
    m.train()
    m.force_drop_mask = drop_u < cfg["class_dropout_prob"]
    m.recompute = value
    xr, tr = x.to(dev).requires_grad_(True), t.to(dev).requires_grad_(True)
    out, zs = m(xr, tr, y.to(dev), inference=False)
    tape = out.grad_fn.tape
    functional(out, zs).backward()
    torch.cuda.synchronize()
    return (grads_of(m), xr.grad, tr.grad, m.engine().recomputed), tape


@pytest.mark.parametrize("kind", ["bf16", "fp32"])
def test_t1024(dev, kind):
    """512^2 training's token count: the long attention backward behind a recomputed attention forward."""
    cfg = tiny_cfg(input_size=64, depth=2)
    m = build_hip_model(cfg, dev, 11)
    m.precision = kind
    assert m.num_patches == 1024
    base, _ = _run_cfg(m, dev, cfg, [(128, "i")], 2, 0)
    res, _ = _run_cfg(m, dev, cfg, [(128, "i")], 2, "all")
    assert res[3] == 2 and base[3] == 0
    same(res, base, f"{kind} T = 1024")


BIG = tiny_cfg(depth=8, input_size=32)      # D = 128, T = 256; at B = 16, M = 4096 tokens
BIG_B = 16


def tape_bytes(tape):
    """Bytes of the distinct tensors a forward's tape holds."""
    seen = {}

    def walk(v):
        if torch.is_tensor(v):
            seen[v.data_ptr()] = v.numel() * v.element_size()
        elif isinstance(v, (list, tuple)):
            for e in v:
                walk(e)
        elif isinstance(v, dict):
            walk(list(v.values()))
        elif hasattr(v, "__dict__") and type(v).__name__ == "SimpleNamespace":
            walk(list(vars(v).values()))

    walk([v for k, v in vars(tape).items() if k != "plan"])
    return sum(seen.values())


@pytest.mark.parametrize("value,records", [(0, 0), (3, 3), ("all", 8)])
def test_accounting_is_exact(dev, value, records):
    m = build_hip_model(BIG, dev, 11)
    m.train()
    x, _, t, y, drop_u, _ = inputs(BIG_B, 4, 32, 11, [(128, "i")], 256, BIG["num_classes"])
    m.force_drop_mask = drop_u < BIG["class_dropout_prob"]
    m.recompute = value
    out, zs = m(x.to(dev), t.to(dev), y.to(dev), inference=False)
    tape = out.grad_fn.tape
    assert [bool(bk.rc) for bk in tape.blocks] == [i < records for i in range(8)]
    held = tape_bytes(tape)
    eng = m.engine()
    want = eng.saved_activation_bytes(BIG_B, recompute=value, plan=tape.plan)
    print(f"[recompute accounting] recompute={value}: the tape holds {held} B, the closed form says {want} B")
    assert held == want
    assert want == eng.saved_activation_bytes(BIG_B)      # the defaults: the model's setting, the current plan
    functional(out, zs).backward()
    torch.cuda.synchronize()
    assert eng.recomputed == records


def test_memory_really_drops(dev):
    """The peak of one forward and backward over the resting state, with 0 and with "all": lower by at least half of what the
    closed form predicts (what 0 saves, less the checkpoints and one block's live set) — a condition that keeps this from passing
    vacuously, not a measurement."""
    m = build_hip_model(BIG, dev, 11)
    eng = m.engine()
    peaks = {}
    for value in (0, "all"):
        _run_cfg(m, dev, BIG, [(128, "i")], BIG_B, value)        # workspaces, the gradient arena, the shadow
        _drop_grads(m)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        res, _ = _run_cfg(m, dev, BIG, [(128, "i")], BIG_B, value)
        assert res[3] == (8 if value else 0)
        peaks[value] = torch.cuda.max_memory_allocated(dev) - before
        del res
    live = block_bytes(BIG_B * 256, 128, 512, 2, 2)
    predicted = eng.saved_activation_bytes(BIG_B, recompute=0) - (eng.saved_activation_bytes(BIG_B, recompute="all") + live)
    print(f"[recompute memory] peak over the resting state: {peaks[0]} B with 0, {peaks['all']} B with all; the closed form predicts "
          f"{predicted} B less")
    assert predicted > 100e6
    assert peaks[0] - peaks["all"] >= predicted / 2


def test_more_tokens_than_the_kernels_index_raises_before_any_launch(dev):
    """The tiny model's widest weight-gradient operand is [M, 512]: 2^31 bytes are 2 097 151 tokens, one short of 131 072 images of
    16 tokens.  The forward that would build a graph refuses by name of the bound and allocates nothing."""
    m, _ = base_run(dev, "bf16", "hd64", False)
    eng = m.engine()
    assert eng.max_tokens() == 2097151 and eng.max_tokens("fp32") == 2 ** 31 - 257
    B = 131072
    x, t, y = torch.empty(B, 4, 8, 8, device=dev), torch.full((B,), 0.5, device=dev), torch.zeros(B, dtype=torch.long, device=dev)
    mask, training = m.force_drop_mask, m.training
    try:
        m.force_drop_mask = None
        m.eval()
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        with pytest.raises(ValueError, match="2097151 tokens"):
            m(x, t, y, inference=True)
        assert torch.cuda.max_memory_allocated(dev) == before
    finally:
        m.force_drop_mask = mask
        m.train(training)


def test_tape_is_final(dev):
    """Flipping SiT.recompute between a forward and its backward changes nothing for that backward; fp8 with a graph keeps raising."""
    m, base = base_run(dev, "bf16", "hd64", False)
    cfg, x, t, y, drop = _case("hd64")
    try:
        for at_forward, after, n in (("all", 0, DEPTH), (0, "all", 0), (2, "all", 2)):
            _drop_grads(m)
            m.train()
            m.force_drop_mask = drop
            m.recompute = at_forward
            xr, tr = x.to(dev).requires_grad_(True), t.to(dev).requires_grad_(True)
            out, zs = m(xr, tr, y.to(dev), inference=False)
            assert [bool(bk.rc) for bk in out.grad_fn.tape.blocks] == [i < n for i in range(DEPTH)]
            m.recompute = after
            functional(out, zs).backward()
            torch.cuda.synchronize()
            assert m.engine().recomputed == n
            same((grads_of(m), xr.grad, tr.grad), base, f"recompute {at_forward} -> {after}")
        m.recompute = "all"
        m.fp8 = True
        with pytest.raises(RuntimeError, match="fp8 is a sampling mode"):
            m(x.to(dev), t.to(dev), y.to(dev), inference=False)
        m.recompute = -1
        m.fp8 = False
        with pytest.raises(ValueError, match="negative"):
            m(x.to(dev), t.to(dev), y.to(dev), inference=False)
    finally:
        m.fp8 = False
        m.recompute = 0
        _drop_grads(m)
