#!/usr/bin/env python
"""tests/golden/xl2_infer_mxfp8.npz: the fp32 oracle (oracle/sit.py) evaluating SiT-XL/2 with its four block linears on MX-fp8
quantise-decoded operands (tests/mxfp8_ref.py: mx_emulation), on the inputs of tests/golden/xl2_infer.npz (the CFG-doubled
evaluation [x; x], labels [y; 1000], n = 2) at t = 0.9 and 0.35.  Two [4, 4, 32, 32] f32 arrays, "mx.t0.9" and "mx.t0.35":
what tests/test_mxfp8_model_gpu.py holds the fp8 sampling path of the HIP model to.  About a minute on the CPU.
usage: python tools/gen_mxfp8_golden.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import detfill                                   # noqa: E402
from oracle import sit as osit                               # noqa: E402
from tests import mxfp8_ref as R                             # noqa: E402
from tests.test_oracle_golden import inputs                  # noqa: E402


def xl2_oracle():
    cfg = osit.make_config("SiT-XL/2", input_size=32, num_classes=1000, z_dims=[1024], z_types=["i"], encoder_depth=8,
                           fused_attn=True, qk_norm=False)
    P = detfill.fill_state_dict(osit.init_params(cfg), base_seed=0)
    return osit.OracleModel(P, cfg), cfg


def main():
    torch.manual_seed(0)
    om, cfg = xl2_oracle()
    x, _, _, y, _, _ = inputs(2, 4, 32, 77, [], 256, 1000)
    xx, yy = torch.cat([x, x]), torch.cat([y, torch.tensor([1000, 1000])])
    ref = np.load(os.path.join(ROOT, "tests", "golden", "xl2_infer.npz"))
    out = {}
    with torch.no_grad():
        for tv in (0.9, 0.35):
            tt = torch.full((4,), tv)
            plain = om(xx, tt, yy)[0]
            rf = torch.from_numpy(ref[f"fp32.t{tv}"])
            print(f"t={tv}: the oracle against the fixture's fp32 array: rel L2 {R.rel_l2(plain, rf):.2e}")
            with R.mx_emulation(om.P, cfg["depth"]) as count:
                mx = om(xx, tt, yy)[0]
            assert count[0] == 4 * cfg["depth"]
            d = (mx - rf).abs().max().item() / rf.abs().max().item()
            cs = torch.nn.functional.cosine_similarity(mx.flatten().double(), rf.flatten().double(), dim=0).item()
            print(f"t={tv}: MX emulation against fp32: rel L2 {R.rel_l2(mx, rf):.2e}, 1 - cos {1 - cs:.2e}, max/scale {d:.2e}; "
                  f"the fixture's bf16 array: rel L2 {R.rel_l2(torch.from_numpy(ref[f'bf16.t{tv}']), rf):.2e}")
            out[f"mx.t{tv}"] = mx.float().numpy()
    np.savez(os.path.join(ROOT, "tests", "golden", "xl2_infer_mxfp8.npz"), **out)


if __name__ == "__main__":
    main()
