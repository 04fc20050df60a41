"""--recompute-blocks on the GPU, in the manner of tests/test_lora_cli_gpu.py: two steps of `reed_amd.train --synthetic` on a small
model with --recompute-blocks all log exactly the losses and gradient norms of the run without the flag; the checkpoint's args carry
the flag; the start-up log has the saved-activation line, for the chosen setting and for 0."""
import json
import logging
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_recompute_blocks_trains_the_same(dev, tmp_path, caplog):
    from reed_amd import train
    caplog.set_level(logging.INFO, logger="reed_amd.train")
    out = str(tmp_path / "exps")
    common = ["--model", "SiT-S/2", "--output-dir", out, "--mixed-precision", "bf16", "--batch-size", "8", "--enc-type", "None",
              "--synthetic", "32", "--num-workers", "0", "--diffusion-warm-up-steps", "0", "--report-to", "none",
              "--checkpointing-steps", "2", "--max-train-steps", "2", "--seed", "0"]
    runs = {}
    for name, flags in (("plain", []), ("all", ["--recompute-blocks", "all"]), ("five", ["--recompute-blocks", "5"])):
        caplog.clear()
        d = train.main(train.parse_args(["--exp-name", name] + flags + common))
        line = [r.getMessage() for r in caplog.records if "saved activations at" in r.getMessage()]
        assert len(line) == 1 and f"with --recompute-blocks {flags[1] if flags else 0}, " in line[0] and "GiB with 0" in line[0]
        logs = [json.loads(l) for l in open(os.path.join(d, "metrics.jsonl"))]
        ck = torch.load(os.path.join(d, "checkpoints", "0000002.pt"), map_location="cpu", weights_only=False)
        runs[name] = (d, logs, ck)
    _, plain, ck0 = runs["plain"]
    assert len(plain) == 2 and vars(ck0["args"])["recompute_blocks"] == 0
    for name, want in (("all", "all"), ("five", 5)):
        d, logs, ck = runs[name]
        assert len(logs) == 2
        for a, b in zip(logs, plain):      # the logged values, exactly
            for k in ("training_denoising_loss", "proj_loss", "grad_norm", "img_proj_loss"):
                assert a[k] == b[k], (name, k, a[k], b[k])
        assert vars(ck["args"])["recompute_blocks"] == want
        assert json.load(open(os.path.join(d, "args.json")))["recompute_blocks"] == want
        for k, v in ck0["model"].items():      # and the weights after two steps
            assert torch.equal(ck["model"][k], v), k
