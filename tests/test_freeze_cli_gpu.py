"""python -m reed_amd.train --train-only / --freeze / --init-from: short synthetic runs on SiT-S/2; the checkpoints hold what the
flags promise, bit for bit."""
import fnmatch
import json
import logging
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_train_only_and_init_from(dev, tmp_path, caplog):
    caplog.set_level(logging.INFO, logger="reed_amd.train")
    from reed_amd import train
    from reed_amd.models.sit import SiT_models
    out = str(tmp_path / "exps")
    common = ["--model", "SiT-S/2", "--output-dir", out, "--mixed-precision", "bf16", "--batch-size", "8", "--synthetic", "32",
              "--num-workers", "0", "--diffusion-warm-up-steps", "0", "--report-to", "none", "--enc-type", "None", "--seed", "3"]
    # four steps: at the reference's initial weights (zero final layer, zero adaLN) the first step moves the final layer only, the
    # second the adaLN rows, the third the gated linears
    a = train.parse_args(["--exp-name", "part", "--max-train-steps", "4", "--checkpointing-steps", "4",
                          "--train-only", "final_layer.*", "blocks.1.*"] + common)
    d = train.main(a)
    torch.set_grad_enabled(True)
    ck = torch.load(os.path.join(d, "checkpoints", "0000004.pt"), map_location="cpu", weights_only=False)
    # the initial weights: the model as train.main builds it from the seed
    torch.manual_seed(3)
    init = SiT_models["SiT-S/2"](input_size=32, num_classes=a.num_classes, use_cfg=(a.cfg_prob > 0), z_dims=[], z_types=[],
                                 encoder_depth=a.encoder_depth, encoder_depth_text=a.encoder_depth_text, fused_attn=a.fused_attn,
                                 qk_norm=a.qk_norm).state_dict()
    names = [n for n in ck["model"] if n != "pos_embed"]
    on = set(fnmatch.filter(names, "final_layer.*")) | set(fnmatch.filter(names, "blocks.1.*"))
    assert on and "blocks.10.mlp.fc1.weight" not in on
    for n in names:
        same = torch.equal(ck["model"][n].view(torch.int32), init[n].view(torch.int32))
        assert same != (n in on), f"{n}: {'moved' if not same else 'did not move'}"
    # the optimiser state holds the trainable parameters only, and the log names the count
    assert len(ck["opt"]["state"]) == len(on)
    log = caplog.text
    n_on = sum(ck["model"][n].numel() for n in on)
    assert f"--train-only final_layer.* blocks.1.*: {n_on:,} trainable parameters" in log
    logs = [json.loads(l) for l in open(os.path.join(d, "metrics.jsonl"))]
    assert len(logs) == 4 and all(np.isfinite(r["training_denoising_loss"]) and np.isfinite(r["grad_norm"]) for r in logs)
    # --init-from that checkpoint, the blocks frozen: step 0, the blocks keep the checkpoint's bits, the rest moves
    b = train.parse_args(["--exp-name", "ft", "--max-train-steps", "1", "--checkpointing-steps", "1", "--freeze", "blocks.*",
                          "--init-from", os.path.join(d, "checkpoints", "0000004.pt")] + common)
    d2 = train.main(b)
    torch.set_grad_enabled(True)
    ck2 = torch.load(os.path.join(d2, "checkpoints", "0000001.pt"), map_location="cpu", weights_only=False)
    assert ck2["steps"] == 1 and {v["step"].item() for v in ck2["opt"]["state"].values()} == {1.0}
    for n in names:
        same = torch.equal(ck2["model"][n].view(torch.int32), ck["model"][n].view(torch.int32))
        assert same == n.startswith("blocks."), n
    log = caplog.text
    assert "--init-from" in log and "--freeze blocks.*: " in log
    # a pattern that matches nothing is an error, before anything is trained
    c = train.parse_args(["--exp-name", "bad", "--max-train-steps", "1", "--freeze", "block.*"] + common)
    with pytest.raises(ValueError, match="matches no parameter"):
        train.main(c)
