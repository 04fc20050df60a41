#!/usr/bin/env python
"""attn_fwd_kernel<64, true> (the attention forward with the <= 16-row query tail folded into the last full block, T = 1025 / 1029)
in both 16-bit builds: the instantiation exists, loads its tiles by LDS-DMA, and spills nothing: no scratch instructions, and the
compiler reports ScratchSize 0, VGPRs Spill 0 and SGPRs Spill 0 (a spill would be memory or lane traffic in the tile loop).
usage: python tools/check_attn_tail_isa.py"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bad = 0
for flags in ([], ["-DREED_FP16"]):
    out = os.path.join(tempfile.mkdtemp(), "attn.s")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), "-I",
                        "/opt/rocm/include", "-x", "hip", "--cuda-device-only", "-S", os.path.join(ROOT, "reed_amd/csrc/attention.hip"),
                        "-o", out, "-Rpass-analysis=kernel-resource-usage"] + flags + sys.argv[1:], check=True, capture_output=True,
                       text=True)
    # the compiler's own account of the instantiation: scratch size and spilled VGPRs / SGPRs (SGPRs go to VGPR lanes, not scratch)
    rem = r.stderr.split("Function Name: ")
    usage = next((blk for blk in rem[1:] if blk.startswith("_ZN12_GLOBAL__N_115attn_fwd_kernelILi64ELb1E")), "")
    nums = {k: int(v) for k, v in re.findall(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill): (\d+)", usage)}
    if not usage or any(nums.get(k, 0) for k in ("ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill")):
        bad += 1
        print("BAD", " ".join(flags or ["bf16"]), "resource usage of attn_fwd_kernel<64, true>:", nums or "not reported")
    else:
        print("ok  ", " ".join(flags or ["bf16"]), "resource usage:", nums)
    s = open(out).read()
    parts = re.split(r"\n(_Z\w+):[^\n]*\n", s)
    seen = 0
    for i in range(1, len(parts), 2):
        if "attn_fwd_kernelILi64ELb1E" not in parts[i]:
            continue
        seen += 1
        body = parts[i + 1].split("s_endpgm")[0]
        nscratch = sum("scratch_" in l for l in body.split("\n"))
        mfma = sum("v_mfma" in l for l in body.split("\n"))
        dma = sum("buffer_load_dwordx4" in l and " lds" in l for l in body.split("\n"))
        ok = nscratch == 0 and dma > 0
        bad += not ok
        print(("ok  " if ok else "BAD ") + " ".join(flags or ["bf16"]) + " " + parts[i][:64], "scratch instructions", nscratch,
              "mfma", mfma, "lds-dma loads", dma)
    if seen != 1:
        bad += 1
        print("BAD", flags, "expected 1 instantiation of attn_fwd_kernel<64, true>, found", seen)
sys.exit(1 if bad else 0)
