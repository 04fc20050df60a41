#!/usr/bin/env python
"""attn_bwd_long_kernel (the 16-bit attention backward past 256 tokens) in both 16-bit builds: its waits are the compiler's, so what
is checked is what the design rests on — no scratch (a spill is vector-memory traffic inside the chunk loop), and the next chunk's
Q / dO prefetch stays in flight under phase A: between the prefetch's last global load and the first MFMA behind it there is no
s_waitcnt vmcnt(0).  usage: python tools/check_attn_long_isa.py"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bad = 0
for flags in ([], ["-DREED_FP16"]):
    out = os.path.join(tempfile.mkdtemp(), "attn.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), "-I",
                    "/opt/rocm/include", "-x", "hip", "--cuda-device-only", "-S", os.path.join(ROOT, "reed_amd/csrc/attention.hip"),
                    "-o", out] + flags + sys.argv[1:], check=True, stderr=subprocess.DEVNULL)
    s = open(out).read()
    parts = re.split(r"\n(_Z\w+):[^\n]*\n", s)
    seen = 0
    for i in range(1, len(parts), 2):
        if "attn_bwd_long_kernel" not in parts[i]:
            continue
        seen += 1
        lines = parts[i + 1].split("s_endpgm")[0].split("\n")
        scratch = any("scratch_" in l for l in lines)
        loads = [k for k, l in enumerate(lines) if l.strip().startswith("global_load_dwordx4")]
        # the chunk loop's prefetch: the last run of 16-byte global loads that has an MFMA behind it
        mf = [k for k, l in enumerate(lines) if "v_mfma" in l]
        pre = [k for k in loads if any(m > k for m in mf)]
        last = pre[-1] if pre else None
        first_mfma = next((m for m in mf if last is not None and m > last), None)
        drained = last is None or first_mfma is None or any("vmcnt(0)" in l for l in lines[last:first_mfma])
        ok = not scratch and not drained
        bad += not ok
        print(("ok  " if ok else "BAD ") + " ".join(flags or ["bf16"]) + " " + parts[i][:64], "scratch", scratch,
              "prefetch drained before phase A", drained)
    if seen != 2:
        bad += 1
        print("BAD", flags, "expected 2 instantiations of attn_bwd_long_kernel, found", seen)
sys.exit(1 if bad else 0)
