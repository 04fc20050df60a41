"""The recompute plan (reed_amd/recompute.py) as host arithmetic: which blocks keep a checkpoint for a value of SiT.recompute, with
and without a truncated FreezePlan; the closed form of the bytes a forward's tape holds against sums written out by hand; the
--recompute-blocks command line.  No GPU."""
import numpy as np
import pytest

from reed_amd import recompute as rcp
from reed_amd.recompute import block_bytes, normalize, recomputed_blocks, saved_activation_bytes
from tests.test_freeze_plan_cpu import model_of, plan

DEPTH = 3   # of the tiny cases


@pytest.mark.parametrize("value,want", [(0, []), (False, []), (None, []), (1, [0]), (DEPTH - 1, [0, 1]), (DEPTH, [0, 1, 2]),
                                        ("all", [0, 1, 2]), (True, [0, 1, 2]), (np.int64(2), [0, 1])])
def test_which_blocks_are_recomputed(value, want):
    got = recomputed_blocks(value, plan("hd64").save)
    assert got == [i in want for i in range(DEPTH)]


def test_the_lowest_blocks_with_a_backward_count_under_a_truncated_plan():
    p = plan("hd64", train_only=["blocks.1.mlp.fc1.*"])        # blocks 1 and 2 run a backward, block 0 saves nothing already
    assert p.trunc and p.k == 1 and p.save == [False, True, True]
    assert recomputed_blocks(0, p.save) == [False, False, False]
    assert recomputed_blocks(1, p.save) == [False, True, False]
    assert recomputed_blocks(2, p.save) == [False, True, True]
    assert recomputed_blocks("all", p.save) == [False, True, True]
    p = plan("hd64", train_only=["projectors.*"])              # no block has a backward: nothing to recompute
    assert p.save == [False] * 3 and recomputed_blocks("all", p.save) == [False] * 3


def test_more_than_there_are_clamps():
    assert recomputed_blocks(DEPTH + 5, [True] * DEPTH) == [True] * DEPTH
    assert recomputed_blocks(3, [False, False, True]) == [False, False, True]
    assert normalize(10 ** 6) == 10 ** 6


@pytest.mark.parametrize("bad", [-1, -3, 1.5, 2.0, "3", "some", "ALL", [1], (2,), {}])
def test_bad_values_raise(bad):
    with pytest.raises(ValueError):
        normalize(bad)
    with pytest.raises(ValueError):
        recomputed_blocks(bad, [True] * DEPTH)


def test_the_model_attribute_defaults_to_off():
    m = model_of("hd64")
    assert m.recompute == 0 and normalize(m.recompute) == 0


def _dims(case, B, hb, p, value):
    """The closed form's arguments for a tiny case."""
    m = model_of(case)
    T, D = m.num_patches, m.hidden_size
    projs = [(B * T if zt == "i" else B, m.projector_dim) for j, zt in enumerate(m.z_types) if p.proj[j]["run"]]
    return dict(B=B, T=T, D=D, Hm=int(D * m.mlp_ratio), H=m.num_heads, depth=m.depth, hb=hb, save=p.save,
                recomputed=recomputed_blocks(value, p.save), in_channels=m.in_channels, input_size=m.input_size,
                ada_rows=m._layout.ada_rows, qk_norm=m.qk_norm, projectors=projs)


def test_bytes_of_the_fully_trainable_tiny_model_by_hand():
    """hd64: D = 128, 2 heads, MLP width 512, depth 3, T = 16, 4 x 8 x 8 inputs, one image projector of width 128 behind block 1,
    3 * 6 * 128 + 2 * 128 = 2560 modulation rows; B = 4 (M = 64 tokens), 16-bit operands, nothing recomputed."""
    hand = sum([
        4 * 4 * 8 * 8 * 4, 4 * 4,                                  # x, t
        4 * 256 * 2, 3 * (4 * 128 * 2), 4 * 2560 * 2,              # sinusoid; t1p, t1, silu(c); modulation
        4 * 128 * 4, 4 * 8,                                        # c, labels
        4 * (64 * 128 * 4),                                        # tokens and three block outputs
        3 * (64 * (8 * 128 + 2 * 512) * 2                          # per block: h qkv o h2 y1 y2 (8 D) and u a1 (2 x 512)
             + 64 * 128 * 4 + 4 * 64 * 4 + 4 * 2 * 16 * 4),        #   xmid, four row statistics, lse [4, 2, 16]
        2 * 64 * 4,                                                # the final layer's row statistics
        64 * 128 * 2 + 4 * (64 * 128 * 2),                         # projector: its input and four [64, 128] arrays
    ])
    assert hand == 1134640
    assert saved_activation_bytes(**_dims("hd64", 4, 2, plan("hd64"), 0)) == hand


def test_bytes_of_a_truncated_recomputed_fp32_qknorm_model_by_hand():
    """qknorm, fp32 operands, only block 2 and the final layer train (blocks 0 and 1 save nothing, the projector has no record),
    recompute = 2 clamps to the one block with a backward: its input, its y2."""
    p = plan("qknorm", train_only=["blocks.2.*", "final_layer.*"])
    assert p.save == [False, False, True] and not p.proj[0]["run"]
    hand = sum([
        4 * 4 * 8 * 8 * 4, 4 * 4,
        4 * 256 * 4, 3 * (4 * 128 * 4), 4 * 2560 * 4,
        4 * 128 * 4, 4 * 8,
        2 * (64 * 128 * 4),                                        # block 2's input and its output
        64 * 128 * 4,                                              # y2
        2 * 64 * 4,
    ])
    assert hand == 156208
    assert saved_activation_bytes(**_dims("qknorm", 4, 4, p, 2)) == hand
    # the same block saved: the qk-norm extras are the normalised qkv and [M, 2, H, 2] fp32 statistics
    saved = saved_activation_bytes(**_dims("qknorm", 4, 4, p, 0))
    assert saved - hand == (64 * (8 * 128 + 2 * 512) * 4 + 64 * 128 * 4 + 4 * 64 * 4 + 4 * 2 * 16 * 4
                            + 64 * 3 * 128 * 4 + 64 * 2 * 2 * 2 * 4) - 64 * 128 * 4


def test_six_bytes_against_forty_per_token_and_channel():
    """One more block at mlp_ratio 4 in a 16-bit build: 40 bytes per token and channel saved (32 in eight 16-bit arrays, xmid, and
    the block's output) plus the row statistics and lse; 6 recomputed (y2 and the block's output)."""
    M, D, H = 4096, 1152, 16
    stats = 4 * M * 4 + M * H * 4
    kw = dict(B=16, T=256, D=D, Hm=4 * D, H=H, hb=2, in_channels=4, input_size=32, ada_rows=0)

    def total(depth, value):
        save = [True] * depth
        return saved_activation_bytes(depth=depth, save=save, recomputed=recomputed_blocks(value, save), **kw)

    assert total(8, 0) - total(7, 0) == 40 * M * D + stats
    assert total(8, "all") - total(7, "all") == 6 * M * D
    assert block_bytes(M, D, 4 * D, H, 2) + 4 * M * D == 40 * M * D + stats
    assert block_bytes(M, D, 4 * D, H, 2, recomputed=True) + 4 * M * D == 6 * M * D
    # a recomputed block in place of a saved one changes nothing else
    assert total(8, 0) - total(8, 3) == 3 * (34 * M * D + stats)


def test_a_blocks_input_is_the_output_of_the_block_below_counted_once():
    M, D = 64, 128
    kw = dict(B=4, T=16, D=D, Hm=512, H=2, depth=3, hb=2, in_channels=4, input_size=8, ada_rows=2560)
    head = saved_activation_bytes(save=[False] * 3, recomputed=[False] * 3, **kw)      # no block: the last output alone
    for value in (0, "all"):
        for save in ([True] * 3, [False, True, True], [False, False, True]):
            rc = recomputed_blocks(value, save)
            blocks = sum(block_bytes(M, D, 512, 2, 2, recomputed=r) for s, r in zip(save, rc) if s)
            # depth - k + 1 residual arrays, not two per block
            assert saved_activation_bytes(save=save, recomputed=rc, **kw) == head + blocks + sum(save) * M * D * 4


def test_token_bound():
    """SiT-XL/2's widest token-major weight-gradient operand is the MLP's [M, 4608]: 2^31 bytes at 16 bits are 233 016 tokens — 910
    images at 256^2, 227 at 512^2 (the modulation array's bound, 5482 images, is further out).  The fp32 build: the int alone."""
    assert rcp.max_tokens(4608, 2) == 233016 == (2 ** 31 - 1) // 9216
    ada = 28 * 6 * 1152 + 2 * 1152
    assert rcp.max_tokens(4608, 2, 256, ada) == 233016 and rcp.max_tokens(4608, 2, 1024, ada) == 233016
    assert 233016 // 256 == 910 and 233016 // 1024 == 227
    assert rcp.max_tokens(512, 2, 4, ada) == 4 * 5482       # a deep model on 4 tokens per image: the modulation array first
    assert rcp.max_tokens(4608, 4) == 2 ** 31 - 257
    assert 233016 * 4608 * 2 < 2 ** 31 <= 233017 * 4608 * 2


def test_command_line():
    from reed_amd import train
    parser = train.build_parser()
    assert parser.parse_args(["--exp-name", "x"]).recompute_blocks == 0
    assert parser.parse_args(["--exp-name", "x", "--recompute-blocks", "all"]).recompute_blocks == "all"
    assert parser.parse_args(["--exp-name", "x", "--recompute-blocks", "3"]).recompute_blocks == 3
    assert train.parse_args(["--exp-name", "x", "--recompute-blocks", "3", "--lora-rank", "16", "--resolution", "512",
                             "--gradient-accumulation-steps", "2", "--train-only", "blocks.2?.*"]).recompute_blocks == 3
    for bad in ("-1", "some", "1.5", ""):
        with pytest.raises(SystemExit):
            parser.parse_args(["--exp-name", "x", "--recompute-blocks", bad])
    assert rcp.parse_flag("0") == 0
