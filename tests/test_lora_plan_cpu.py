"""LoRA on the host: the constructor and the arena layout with adapters, the FreezePlan of the usual trainable sets, the flag surface
of train.py and how --lora-rank composes with --train-only / --freeze.  No GPU."""
import pytest
import torch

from reed_amd import lora
from reed_amd.freeze import LINEARS, FreezePlan
from reed_amd.models.sit import SiT

KW = dict(input_size=8, patch_size=2, in_channels=4, hidden_size=128, decoder_hidden_size=128, depth=3, num_heads=2, num_classes=10,
          z_dims=[128], z_types=["i"], encoder_depth=2, projector_dim=128)
TAP = [2]


def _model(**kw):
    torch.manual_seed(5)
    return SiT(**KW, **kw)


def _plan(m, on, **kw):
    names = [n for n, _ in m.named_parameters()]
    return FreezePlan(m.depth, TAP, [n for n in names if on(n)], all_names=names, **kw)


def test_constructor_surface_and_defaults():
    m = _model(lora_rank=8)
    assert (m.lora_rank, m.lora_alpha, m.lora_targets) == (8, 8.0, lora.TARGETS) and m._layout.lora_scale == 1.0
    m = _model(lora_rank=16, lora_alpha=32, lora_targets=("mlp.fc2", "attn.qkv"))
    assert m.lora_targets == ("attn.qkv", "mlp.fc2") and m._layout.lora_scale == 2.0
    sd = m.state_dict()
    assert sd["blocks.1.attn.qkv.lora_A"].shape == (16, 128) and sd["blocks.1.attn.qkv.lora_B"].shape == (384, 16)
    assert sd["blocks.2.mlp.fc2.lora_A"].shape == (16, 512) and sd["blocks.2.mlp.fc2.lora_B"].shape == (128, 16)
    assert "blocks.0.attn.proj.lora_A" not in sd and "blocks.0.mlp.fc1.lora_B" not in sd
    for bad in (dict(lora_rank=12), dict(lora_rank=8, lora_targets=("attn.q",)), dict(lora_alpha=4.0), dict(lora_rank=8, lora_targets=())):
        with pytest.raises(ValueError):
            _model(**bad)
    plain = _model()
    assert plain.lora_rank == 0 and not any(lora.is_adapter_key(k) for k in plain.state_dict()) and plain._layout.lora == []


def test_base_weights_do_not_depend_on_the_adapters():
    a, b = _model().state_dict(), _model(lora_rank=8, lora_alpha=16).state_dict()
    assert list(a) == [k for k in b if not lora.is_adapter_key(k)]
    assert all(torch.equal(a[k], b[k]) for k in a)
    m = _model(lora_rank=8)
    for i in range(m.depth):
        for lin in lora.TARGETS:
            A, B = b[f"blocks.{i}.{lin}.lora_A"], b[f"blocks.{i}.{lin}.lora_B"]
            assert float(B.abs().max()) == 0.0 and 0 < float(A.abs().max()) <= A.shape[1] ** -0.5 and float(A.std()) > 0.3 * A.shape[1] ** -0.5
    req = {n: p.requires_grad for n, p in m.named_parameters()}
    assert not req["blocks.0.attn.qkv.weight"] and not req["blocks.2.mlp.fc1.bias"] and req["blocks.0.attn.qkv.lora_A"]
    assert req["blocks.0.adaLN_modulation.1.weight"] and req["x_embedder.proj.weight"] and all(p.is_leaf for p in m.parameters())
    part = _model(lora_rank=8, lora_targets=("attn.qkv",))
    req = {n: p.requires_grad for n, p in part.named_parameters()}
    assert not req["blocks.0.attn.qkv.bias"] and req["blocks.0.attn.proj.weight"]


def test_arena_layout_keeps_adapters_in_their_block():
    m = _model(lora_rank=8)
    L = m._layout
    names = list(L.seg)
    for i, w, a, b in L.lora:
        k = names.index(w)
        assert names[k + 1:k + 4] == [w[:-6] + "bias", a, b]
    buckets = dict(L.buckets())
    chunks = L.update_chunks(TAP)
    by_name = {n: (b, e) for n, b, e in chunks}
    for i, w, a, b in L.lora:
        for n in (a, b):
            off, end = L.off(n), L.off(n) + L.numel(n)
            assert buckets[f"block{i}"][0] <= off and end <= buckets[f"block{i}"][1]
            assert by_name[f"block{i}"][0] <= off and end <= by_name[f"block{i}"][1]
    cover = sorted((b, e) for _, b, e in chunks)
    assert cover[0][0] == 0 and cover[-1][1] == L.n_total and all(x[1] == y[0] for x, y in zip(cover, cover[1:]))
    assert len(L.lora) == 4 * m.depth and [t[0] for t in L.lora] == sorted(t[0] for t in L.lora)


def test_plan_adapters_only():
    m = _model(lora_rank=8)
    pl = _plan(m, lora.is_adapter_key)
    assert pl.mode == "partial" and pl.trunc and pl.k == 0 and pl.stage == [4, 5, 5] and pl.save == [True] * 3
    assert not any(pl.group) and not pl.any_ada and not pl.final_w and pl.final_ln and not pl.dmod
    assert pl.launches() == [f"block{i}.lora.{n}" for i in (2, 1, 0) for n in LINEARS]
    # a frozen projector above blocks that train: its chain runs for the trunk's dx alone, no weight gradient
    assert pl.proj[0]["run"] and pl.proj[0]["dx"] and not any(pl.proj[0]["w"].values())


def test_plan_adapters_plus_projectors():
    m = _model(lora_rank=8)
    pl = _plan(m, lambda n: lora.is_adapter_key(n) or n.startswith("projectors."))
    want = []
    for i in (2, 1, 0):
        if i == 1:
            want += [f"proj0.wgrad.{k}" for k in (4, 2, 0)]
        want += [f"block{i}.lora.{n}" for n in LINEARS]
    assert pl.launches() == want and pl.proj[0]["dx"] and pl.stage == [4, 5, 5]


def test_plan_base_switched_back_on_and_top_block_only():
    m = _model(lora_rank=8)
    pl = _plan(m, lambda n: lora.is_adapter_key(n) or n == "blocks.1.mlp.fc1.weight")
    assert "block1.wgrad.mlp.fc1" in pl.launches() and "block1.lora.mlp.fc1" in pl.launches()
    assert pl.launches().index("block1.wgrad.mlp.fc1") + 1 == pl.launches().index("block1.lora.mlp.fc1") and not any(pl.group)
    full = _plan(m, lambda n: n != "pos_embed")
    assert full.mode == "all" and all(full.group) and all(all(d.values()) for d in full.lora)
    top = _plan(m, lambda n: lora.is_adapter_key(n) and n.startswith("blocks.2."))
    assert top.k == 2 and top.stage == [0, 0, 4] and top.save == [False, False, True]
    assert top.launches() == [f"block2.lora.{n}" for n in LINEARS]
    fc2 = _plan(_model(lora_rank=8, lora_targets=("mlp.fc2",)), lambda n: lora.is_adapter_key(n) and n.startswith("blocks.2."))
    assert fc2.stage == [0, 0, 1] and fc2.launches() == ["block2.lora.mlp.fc2"]
    plain = _plan(_model(), lambda n: n != "pos_embed")
    assert not any(any(d.values()) for d in plain.lora) and not any(".lora." in x for x in plain.launches())


def test_flag_surface_and_freeze_composition():
    from reed_amd import train
    base = ["--exp-name", "t", "--model", "SiT-B/2"]
    a = train.parse_args(base)
    assert (a.lora_rank, a.lora_alpha, a.lora_targets) == (0, None, None)
    a = train.parse_args(base + ["--lora-rank", "16"])
    assert (a.lora_rank, a.lora_alpha, a.lora_targets) == (16, 16.0, list(lora.TARGETS))
    a = train.parse_args(base + ["--lora-rank", "8", "--lora-alpha", "4", "--lora-targets", "mlp.fc1", "attn.qkv"])
    assert (a.lora_rank, a.lora_alpha, a.lora_targets) == (8, 4.0, ["attn.qkv", "mlp.fc1"])
    for bad in (["--lora-rank", "12"], ["--lora-alpha", "4"], ["--lora-rank", "8", "--lora-targets", "attn.q"]):
        with pytest.raises(SystemExit):
            train.parse_args(base + bad)

    def on(m):
        return {n for n, p in m.named_parameters() if p.requires_grad}

    m = _model(lora_rank=8)
    adapters = {n for n, _ in m.named_parameters() if lora.is_adapter_key(n)}
    n_on = train.apply_lora_freeze(m)
    assert on(m) == adapters and n_on == sum(p.numel() for n, p in m.named_parameters() if n in adapters)
    train.apply_lora_freeze(m, train_only=["projectors.*"])
    assert on(m) == adapters | {n for n, _ in m.named_parameters() if n.startswith("projectors.")}
    train.apply_lora_freeze(m, freeze=["blocks.0.*", "x_embedder.*"])
    assert on(m) == {n for n, _ in m.named_parameters() if n != "pos_embed" and not n.startswith(("blocks.0.", "x_embedder."))}
    with pytest.raises(ValueError):
        train.apply_lora_freeze(m, train_only=["nothing.*"])


def test_base_checkpoint_loads_into_an_adapted_model_and_nothing_else_may_be_missing():
    from reed_amd import train
    plain, m = _model(), _model(lora_rank=8)
    sd = {k: v + 1 for k, v in plain.state_dict().items()}
    before = {k: v.clone() for k, v in m.state_dict().items() if lora.is_adapter_key(k)}
    train.load_base_state_dict(m, sd)
    after = m.state_dict()
    assert all(torch.equal(after[k], sd[k]) for k in sd) and all(torch.equal(after[k], before[k]) for k in before)
    short = dict(sd)
    del short["blocks.1.mlp.fc1.bias"]
    with pytest.raises(RuntimeError, match="blocks.1.mlp.fc1.bias"):
        train.load_base_state_dict(m, short)
    with pytest.raises(RuntimeError):
        train.load_base_state_dict(m, dict(sd, extra=torch.zeros(1)))
    with pytest.raises(RuntimeError):   # a plain model keeps torch's strict load
        train.load_base_state_dict(plain, short)
    full = m.state_dict()
    train.load_base_state_dict(m, full)   # a checkpoint with adapters: the strict load
    del full["blocks.0.attn.qkv.lora_B"]
    with pytest.raises(RuntimeError):
        train.load_base_state_dict(m, full)
