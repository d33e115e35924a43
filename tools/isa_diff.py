#!/usr/bin/env python3
"""isa_diff.py REV: is the gfx950 device code of the working tree that of commit REV?

Exports REV with `git archive` into a temporary directory, compiles csrc/murbhip.hip of both trees to device assembly
(no GPU needed) and prints per kernel either `identical` or the vector / scalar register counts and the scratch of both
sides.  Lines holding __hip_cuid_ are left out: that symbol is random per compile and the only difference between two
builds of one source.  Exit status 1 if any kernel, or anything else in the assembly (kernel order, data), differs."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join("nbody-eurohpc_amd", "csrc", "murbhip.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def assembly(tree, out):
    subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-S", "--cuda-device-only", os.path.join(tree, SRC), "-o", out],
                   check=True, stderr=subprocess.DEVNULL)
    return "".join(line for line in open(out) if "__hip_cuid_" not in line)


def kernels(text):
    """{symbol: (code and kernel descriptor, 'vgpr sgpr scratch' from the metadata)}"""
    found = {}
    for name, meta in re.findall(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S):
        code = text[text.index("\n" + name + ":"):]
        code = code[:code.index(".end_amdhsa_kernel")]
        num = [re.search(r"\." + f + r":\s+(\d+)", meta).group(1) for f in ("vgpr_count", "sgpr_count", "private_segment_fixed_size")]
        found[name] = (code, "vgpr {} sgpr {} scratch {}".format(*num))
    return found


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        old_tree = os.path.join(tmp, "old")
        os.mkdir(old_tree)
        tar = subprocess.run(["git", "-C", ROOT, "archive", sys.argv[1], "nbody-eurohpc_amd/csrc", "include"], check=True, capture_output=True)
        subprocess.run(["tar", "-x", "-C", old_tree], input=tar.stdout, check=True)
        with ThreadPoolExecutor(2) as pool:
            old, new = pool.map(assembly, (old_tree, ROOT), (os.path.join(tmp, "old.s"), os.path.join(tmp, "new.s")))
    ko, kn = kernels(old), kernels(new)
    differ = 0
    for name in sorted(set(ko) | set(kn)):
        if name in ko and name in kn and ko[name][0] == kn[name][0]:
            print("identical ", name)
            continue
        differ += 1
        print("DIFFERS   ", name)
        print("    " + sys.argv[1] + ": " + (ko[name][1] if name in ko else "absent"))
        print("    working tree: " + (kn[name][1] if name in kn else "absent"))
    rest = old != new and not differ
    print(f"{len(kn)} kernels, {differ} differ" + ("; the assembly differs outside the kernels' code (their order, data, metadata)" if rest else ""))
    sys.exit(1 if differ or rest else 0)


if __name__ == "__main__":
    main()
