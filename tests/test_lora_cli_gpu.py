"""The LoRA command line on the GPU, a small model for two steps at a time: train without adapters, --init-from that checkpoint with
--lora-rank 8, --resume-step, `python -m reed_amd.lora merge` / `extract`, generate.py on the merged checkpoint; a base checkpoint
missing any key but the adapters' is refused."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from reed_amd import lora

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lora_train_resume_merge_generate(dev, tmp_path):
    from reed_amd import generate, train
    out = str(tmp_path / "exps")
    common = ["--model", "SiT-S/2", "--output-dir", out, "--mixed-precision", "bf16", "--batch-size", "8", "--enc-type", "None",
              "--synthetic", "32", "--num-workers", "0", "--diffusion-warm-up-steps", "0", "--report-to", "none",
              "--checkpointing-steps", "2"]
    base_dir = train.main(train.parse_args(["--exp-name", "base", "--max-train-steps", "2"] + common))
    base_ck = os.path.join(base_dir, "checkpoints", "0000002.pt")
    base = torch.load(base_ck, map_location="cpu", weights_only=False)
    assert not any(lora.is_adapter_key(k) for k in base["model"])
    # adapters on the pre-trained base
    flags = ["--lora-rank", "8", "--lora-alpha", "16", "--learning-rate", "1e-3"]
    d = train.main(train.parse_args(["--exp-name", "ft", "--max-train-steps", "2", "--init-from", base_ck] + flags + common))
    rec = json.load(open(os.path.join(d, "args.json")))
    assert (rec["lora_rank"], rec["lora_alpha"], rec["lora_targets"]) == (8, 16.0, list(lora.TARGETS))
    ck_path = os.path.join(d, "checkpoints", "0000002.pt")
    ck = torch.load(ck_path, map_location="cpu", weights_only=False)
    ad = [k for k in ck["model"] if lora.is_adapter_key(k)]
    assert len(ad) == 2 * 4 * 12 and [k for k in ck["ema"] if lora.is_adapter_key(k)] == ad
    for k, v in base["model"].items():      # only the adapters trained: the base has the bits it was loaded with
        assert torch.equal(ck["model"][k], v), k
    assert all(float(ck["model"][k].abs().max()) > 0 for k in ad)
    assert sorted(ck["opt"]["state"]) == [i for i, k in enumerate(ck["model"]) if lora.is_adapter_key(k)]
    logs = [json.loads(l) for l in open(os.path.join(d, "metrics.jsonl"))]
    assert len(logs) == 2 and all(np.isfinite(r["training_denoising_loss"]) and r["grad_norm"] > 0 for r in logs)
    # resume
    train.main(train.parse_args(["--exp-name", os.path.basename(d), "--max-train-steps", "4", "--resume-step", "2"] + flags + common))
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(d, "checkpoints", "*.pt"))) == ["0000002.pt", "0000004.pt"]
    ck4_path = os.path.join(d, "checkpoints", "0000004.pt")
    ck4 = torch.load(ck4_path, map_location="cpu", weights_only=False)
    assert ck4["steps"] == 4 and any(not torch.equal(ck4["model"][k], ck["model"][k]) for k in ad)
    # merge and extract, as commands
    merged_path, adapter_path = str(tmp_path / "merged.pt"), str(tmp_path / "adapter.pt")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for cmd, dst in (("merge", merged_path), ("extract", adapter_path)):
        r = subprocess.run([sys.executable, "-m", "reed_amd.lora", cmd, ck4_path, dst], env=env, cwd=ROOT, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
    merged = torch.load(merged_path, map_location="cpu", weights_only=False)
    assert set(merged) == {"model", "ema", "args", "steps"} and merged["steps"] == 4
    assert list(merged["model"]) == list(base["model"]) and list(merged["ema"]) == list(base["ema"])
    assert not [k for k in vars(merged["args"]) if k.startswith("lora_")]
    w = "blocks.3.mlp.fc1"
    want = ck4["model"][w + ".weight"].double() + 2.0 * ck4["model"][w + ".lora_B"].double() @ ck4["model"][w + ".lora_A"].double()
    assert merged["model"][w + ".weight"].dtype == torch.float32
    torch.testing.assert_close(merged["model"][w + ".weight"].double(), want, rtol=0, atol=1e-6)
    assert torch.equal(merged["model"]["blocks.3.mlp.fc1.bias"], ck4["model"]["blocks.3.mlp.fc1.bias"])
    adapter = torch.load(adapter_path, map_location="cpu", weights_only=False)
    assert adapter["lora_rank"] == 8 and adapter["lora_alpha"] == 16.0 and list(adapter["adapter"]) == ad
    assert all(torch.equal(adapter["adapter"][k], ck4["model"][k]) and torch.equal(adapter["ema_adapter"][k], ck4["ema"][k]) for k in ad)
    # generate.py loads the merged checkpoint as it loads any other
    g = generate.build_parser().parse_args(["--ckpt", merged_path, "--model", "SiT-S/2", "--sample-dir", str(tmp_path / "samples"),
                                            "--per-proc-batch-size", "4", "--num-fid-samples", "4", "--num-steps", "2",
                                            "--cfg-scale", "1.0", "--save-latents"])
    folder = generate.main(g)
    torch.set_grad_enabled(True)
    lat = np.load(folder + "_latents.npz")["arr_0"]
    assert lat.shape == (4, 4, 32, 32) and np.isfinite(lat).all()
    # a base checkpoint missing anything else is refused
    del base["model"]["blocks.5.attn.proj.bias"]
    bad = str(tmp_path / "bad.pt")
    torch.save(base, bad)
    with pytest.raises(RuntimeError, match="blocks.5.attn.proj.bias"):
        train.main(train.parse_args(["--exp-name", "bad", "--max-train-steps", "1", "--init-from", bad] + flags + common))
