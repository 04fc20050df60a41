"""The freeze plan (reed_amd/freeze.py) as host arithmetic on the tiny configuration (depth 3, one image projector tapping the
output of block 1; `two_split`: an image projector behind block 0 and a text projector behind block 2), the trainable ranges the
optimiser walks, and the --freeze / --train-only / --init-from command line.  No GPU."""
import fnmatch

import pytest

from reed_amd.freeze import LINEARS, FreezePlan, select_parameters, trainable_ranges
from tests.test_oracle_golden import TINY_CASES


def model_of(case):
    from reed_amd.models.sit import SiT
    cfg = TINY_CASES[case]["cfg"]
    return SiT(input_size=cfg["input_size"], patch_size=cfg["patch_size"], in_channels=cfg["in_channels"],
               hidden_size=cfg["hidden_size"], decoder_hidden_size=cfg["hidden_size"], depth=cfg["depth"],
               num_heads=cfg["num_heads"], num_classes=cfg["num_classes"], z_dims=cfg["z_dims"], z_types=cfg["z_types"],
               encoder_depth=cfg["encoder_depth"], encoder_depth_text=cfg["encoder_depth_text"],
               projector_dim=cfg["projector_dim"], class_dropout_prob=cfg["class_dropout_prob"], qk_norm=cfg["qk_norm"])


def names_of(case):
    return [n for n, _ in model_of(case).named_parameters() if n != "pos_embed"]


def taps(case):
    cfg = TINY_CASES[case]["cfg"]
    split = cfg["encoder_depth_text"] is not None and cfg["encoder_depth_text"] != cfg["encoder_depth"]
    return [cfg["encoder_depth"] if (zt == "i" or not split) else cfg["encoder_depth_text"] for zt in cfg["z_types"]]


def plan(case, freeze=None, train_only=None, **kw):
    names = names_of(case)
    cfg = TINY_CASES[case]["cfg"]
    on = select_parameters(names, freeze, train_only)
    return FreezePlan(cfg["depth"], taps(case), on, qk_norm=cfg["qk_norm"], all_names=names, **kw)


FULL = (["final.smallk_wgrad"] + [f"block2.wgrad.{n}" for n in LINEARS] + ["proj0.wgrad.4", "proj0.wgrad.2", "proj0.wgrad.0"]
        + [f"block1.wgrad.{n}" for n in LINEARS] + [f"block0.wgrad.{n}" for n in LINEARS]
        + ["ada.wgrad", "label_scatter", "t.wgrad.2", "t.wgrad.0", "x.smallk_wgrad"])


def test_all_trainable_is_the_unchanged_plan():
    p = plan("hd64")
    assert p.mode == "all" and not p.trunc and p.k == 0 and p.stage == [5, 5, 5] and p.save == [True] * 3
    assert p.launches() == FULL
    assert all(p.group) and p.cond and p.final_run and p.final_ln and all(p.mod_reduce)
    assert p.proj == [{"run": True, "dx": True, "stop": -1, "w": {4: True, 2: True, 0: True}, "tap": 2}]
    # pos_embed never trains: listing it or not changes nothing
    names = names_of("hd64")
    assert FreezePlan(3, [2], names + ["pos_embed"], all_names=names + ["pos_embed"]).mode == "all"


@pytest.mark.parametrize("need_x,need_t", [(True, True), (True, False), (False, True)])
def test_nothing_trainable_is_the_frozen_weight_backward(need_x, need_t):
    p = plan("hd64", freeze=["*"], need_x=need_x, need_t=need_t)
    assert p.mode == "none" and not p.any and p.launches() == []
    # the whole activation-gradient chain, as before: every block to its last stage, the conditioning tail, the tap into dx
    assert not p.trunc and p.stage == [5, 5, 5] and p.save == [True] * 3 and p.cond and p.final_ln and p.dmod
    assert p.proj[0]["run"] and p.proj[0]["dx"] and not any(p.group)


def test_set_a_patch_embedder_frozen():
    p = plan("hd64", freeze=["x_embedder.*"])
    assert p.mode == "partial" and not p.trunc and p.save == [True] * 3 and p.stage == [5, 5, 5]
    assert p.launches() == FULL[:-1]                      # everything but the patch embedder's small-K weight gradient
    assert all(p.group)


def test_set_b_last_block_and_final_layer():
    p = plan("hd64", train_only=["blocks.2.*", "final_layer.*"])
    assert p.trunc and p.k == 2 and p.stage == [0, 0, 5] and p.save == [False, False, True]
    assert p.launches() == ["final.smallk_wgrad"] + [f"block2.wgrad.{n}" for n in LINEARS] + ["ada.wgrad"]
    assert not p.cond and p.group == [False, False, True]
    assert p.mod_reduce == [False, False, True, True]     # the trainable adaLN rows only
    assert p.proj[0] == {"run": False, "dx": False, "stop": None, "w": {4: False, 2: False, 0: False}, "tap": 2}
    # an input that requires grad takes the chain to the bottom again
    for kw in (dict(need_x=True), dict(need_t=True)):
        q = plan("hd64", train_only=["blocks.2.*", "final_layer.*"], **kw)
        assert not q.trunc and q.save == [True] * 3 and q.proj[0]["dx"] and q.launches() == p.launches()


def test_set_c_projectors_only():
    p = plan("two_split", train_only=["projectors.*"])
    assert p.trunc and p.k == 3 and p.stage == [0, 0, 0] and p.save == [False] * 3
    assert not p.final_run and not p.final_ln and not p.dmod and not p.cond
    assert p.launches() == [f"proj{j}.wgrad.{k}" for j in (1, 0) for k in (4, 2, 0)]     # the deeper tap first
    assert all(pj["run"] and not pj["dx"] and pj["stop"] == 0 for pj in p.proj)
    # one layer of one projector: its chain stops behind that layer
    q = plan("two_split", train_only=["projectors.1.2.*"])
    assert q.launches() == ["proj1.wgrad.2"] and q.proj[1]["stop"] == 2 and not q.proj[0]["run"]


def test_set_d_weights_frozen_biases_trainable():
    p = plan("hd64", freeze=["*.weight"])
    # every launch is mixed (it writes a bias gradient): the fully trainable launches, the label scatter (a weight alone) aside
    assert p.mode == "partial" and not p.trunc and all(p.group)
    assert p.launches() == [n for n in FULL if n != "label_scatter"]


def test_set_e_one_linear():
    p = plan("hd64", train_only=["blocks.1.mlp.fc1.*"])
    assert p.trunc and p.k == 1 and p.stage == [0, 2, 5] and p.save == [False, True, True]
    assert p.launches() == ["block1.wgrad.mlp.fc1"] and not any(p.group) and not p.dmod
    assert p.final_run and p.final_ln and not p.final_w
    assert p.proj[0]["run"] and p.proj[0]["dx"] and p.proj[0]["stop"] == -1   # the tap feeds block 1, which runs: no weight gradient
    # per linear: the stage that completes it
    for lin, stage in (("mlp.fc2", 1), ("mlp.fc1", 2), ("attn.proj", 3), ("attn.qkv", 4)):
        assert plan("hd64", train_only=[f"blocks.0.{lin}.bias"]).stage == [stage, 5, 5]
    # a block with one linear frozen takes the per-GEMM launches, its neighbours the grouped one
    q = plan("hd64", freeze=["blocks.0.attn.proj.*"])
    assert q.group == [False, True, True] and "block0.wgrad.attn.proj" not in q.launches() and len(q.launches()) == len(FULL) - 1


def test_set_f_one_blocks_adaln():
    p = plan("hd64", train_only=["blocks.1.adaLN_modulation.*"])
    assert p.trunc and p.k == 1 and p.stage == [0, 5, 5] and p.launches() == ["ada.wgrad"]
    assert p.dmod and p.mod_reduce == [False, True, False, False]


def test_set_g_timestep_embedder_only():
    p = plan("hd64", train_only=["t_embedder.*"])
    assert not p.trunc and p.cond and p.stage == [5, 5, 5] and p.save == [True] * 3
    assert p.launches() == ["t.wgrad.2", "t.wgrad.0"] and all(p.mod_reduce)


def test_qk_norm_rowsum():
    full = plan("qknorm")
    assert [n for n in full.launches() if "qknorm" in n] == [f"block{i}.qknorm_rowsum" for i in (2, 1, 0)]
    p = plan("qknorm", train_only=["blocks.1.attn.q_norm.*"])
    assert p.launches() == ["block1.qknorm_rowsum"] and p.stage == [0, 4, 5]
    assert "block1.qknorm_rowsum" not in plan("qknorm", freeze=["blocks.1.attn.?_norm.*"]).launches()


def test_trainable_ranges_are_sorted_merged_and_aligned():
    m = model_of("two_split")
    L = m._layout
    names = [n for n in L.seg if n != "pos_embed"]
    assert trainable_ranges(L, set(names)) == [(0, L.n_train)]
    assert trainable_ranges(L, set()) == []
    for pats in (["blocks.2.*", "final_layer.*"], ["*.bias"], ["projectors.*"], ["blocks.1.mlp.fc1.weight"]):
        on = select_parameters(names, train_only=pats)
        rg = trainable_ranges(L, on)
        assert rg == sorted(rg) and all(b % 4 == 0 and e % 4 == 0 and b < e for b, e in rg)
        assert all(e0 < b1 for (_, e0), (b1, _) in zip(rg, rg[1:]))          # disjoint, and merged where adjacent
        inside = lambda off: any(b <= off < e for b, e in rg)                # noqa: E731
        for n in names:
            off, numel = L.off(n), L.numel(n)
            assert inside(off) == inside(off + numel - 1) == (n in on), n
    assert len(trainable_ranges(L, select_parameters(names, train_only=["*.bias"]))) <= 1024


def test_cli_patterns():
    names = names_of("hd64")
    assert select_parameters(names) == set(names)
    assert select_parameters(names, freeze=["x_embedder.*"]) == {n for n in names if not n.startswith("x_embedder.")}
    only = select_parameters(names, train_only=["final_layer.*", "blocks.1.*"])
    assert only == set(fnmatch.filter(names, "final_layer.*")) | set(fnmatch.filter(names, "blocks.1.*"))
    with pytest.raises(ValueError, match="matches no parameter"):
        select_parameters(names, freeze=["x_embedder.*", "blocks.7.*"])
    with pytest.raises(ValueError, match="matches no parameter"):
        select_parameters(names, train_only=["projector.*"])
    with pytest.raises(ValueError, match="mutually exclusive"):
        select_parameters(names, freeze=["a"], train_only=["b"])


def test_cli_arguments(capsys):
    from reed_amd import train
    a = train.parse_args(["--exp-name", "e", "--train-only", "final_layer.*", "blocks.1.*", "--init-from", "x.pt"])
    assert a.train_only == ["final_layer.*", "blocks.1.*"] and a.freeze is None and a.init_from == "x.pt"
    a = train.parse_args(["--exp-name", "e", "--freeze", "x_embedder.*"])
    assert a.freeze == ["x_embedder.*"] and a.train_only is None and a.init_from is None
    for bad in (["--freeze", "a", "--train-only", "b"], ["--init-from", "x.pt", "--resume-step", "3"], ["--freeze"]):
        with pytest.raises(SystemExit):
            train.parse_args(["--exp-name", "e"] + bad)
    capsys.readouterr()
    m = model_of("hd64")
    n_on = train.apply_freeze(m, None, ["final_layer.*", "blocks.1.*"])
    on = {n for n, p in m.named_parameters() if p.requires_grad}
    assert on == set(fnmatch.filter(names_of("hd64"), "final_layer.*")) | set(fnmatch.filter(names_of("hd64"), "blocks.1.*"))
    assert n_on == sum(p.numel() for p in m.parameters() if p.requires_grad) and not m.pos_embed.requires_grad
    with pytest.raises(ValueError, match="matches no parameter"):
        train.apply_freeze(m, ["nothing.*"], None)
