"""The gfx950 device assembly of nbody-eurohpc_amd/csrc/murbhip.hip for the host tests that inspect the code object: compiled
once per process (hipcc -S --cuda-device-only, about 13 s, no GPU needed), then read by kernel.  A caller decides for itself
what a missing compiler means (hipcc() is None): some tests skip, some fail."""
import os
import re
import shutil
import subprocess
import tempfile
from functools import lru_cache

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIELDS = ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count", "sgpr_count")


def hipcc():
    return "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")


@lru_cache(maxsize=None)
def text():
    """The whole assembly file, metadata included."""
    src = os.path.join(ROOT, "nbody-eurohpc_amd", "csrc", "murbhip.hip")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "murbhip.s")
        subprocess.run([hipcc(), "-O3", "--offload-arch=gfx950", "-std=c++17", "-S", "--cuda-device-only", src, "-o", asm],
                       check=True, stderr=subprocess.DEVNULL)
        return open(asm).read()


def metadata(kernel):
    """{symbol: {field: number}} of every kernel whose symbol holds a match of the regular expression `kernel`; FIELDS names the fields."""
    found = re.findall(r"\.name:\s+(\S*(?:" + kernel + r")\S*)\n(.*?)\.wavefront_size", text(), re.S)
    return {name: {f: int(re.search(r"\." + f + r":\s+(\d+)", meta).group(1)) for f in FIELDS} for name, meta in found}


def symbol(kernel):
    """The first symbol of the code that holds `kernel`: murb_force_jerk_kernel, not murb_force_jerk_kernel_something."""
    return next(k for k in re.findall(r"^(_Z\w*" + kernel + r"\w*):", text(), re.M))


def body(kernel):
    """A kernel's instructions, from its label to the end of the function; `kernel` is a symbol or a name symbol() finds."""
    name = kernel if kernel.startswith("_Z") else symbol(kernel)
    code = text()[text().index(name + ":"):]
    return code[:code.index(".Lfunc_end")]   # not the first s_endpgm: an early exit can come first


def ops(kernel, pattern):
    """Every match of `pattern` (multi-line mode) in the kernel's body, in order."""
    return re.findall(pattern, body(kernel), re.M)
