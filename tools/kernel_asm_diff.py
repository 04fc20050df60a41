"""Compare two hipcc -S --cuda-device-only dumps kernel by kernel: which kernels exist in only one, which differ in text.
Kernel order and the function index inside local labels (.LBB<n>_, .Lfunc_end<n>) follow position in the file, so they are
normalised away; comments and trailing blanks are stripped.  A kernel's text is its code up to .Lfunc_end plus its
.amdhsa_kernel descriptor (registers, LDS, scratch).  Exit status 1 if any kernel differs.
Usage: python tools/kernel_asm_diff.py OLD.s NEW.s"""
import hashlib
import re
import sys


def kernels(path):
    s = re.sub(r"(\.L[A-Za-z_]+?)\d+", r"\1", open(path).read())            # .LBB12_3 -> .LBB_3, .Lfunc_end12 -> .Lfunc_end
    s = "\n".join(re.sub(r"\s*;.*", "", l).rstrip() for l in s.split("\n"))   # comments, trailing whitespace
    parts = re.split(r"\n(_Z\w+):\n", s)
    out = {}
    for name, body in zip(parts[1::2], parts[2::2]):
        desc = re.search(r"\.amdhsa_kernel %s\n.*?\.end_amdhsa_kernel" % re.escape(name), s, re.S)
        text = body.split(".Lfunc_end")[0] + (desc.group(0) if desc else "")
        out[name] = hashlib.sha256(text.encode()).hexdigest()
    return out


old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
differ = sorted(k for k in old.keys() & new.keys() if old[k] != new[k])
print(f"{sys.argv[1]} -> {sys.argv[2]}: {len(old)} / {len(new)} kernels, {len(old.keys() & new.keys()) - len(differ)} identical")
for title, names in (("only in old", sorted(old.keys() - new.keys())), ("only in new", sorted(new.keys() - old.keys())),
                     ("differ", differ)):
    print(f"  {title}: {len(names)}")
    for k in names:
        print(f"    {k}")
sys.exit(1 if differ else 0)
