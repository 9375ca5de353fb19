"""gfx950 assembly of a .hip of the package for the ISA tests: one `hipcc -S` per source and process, whichever tests ask.
Compiling dpe_bcm.hip takes minutes (134 kernels); five test modules read it."""
import functools
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "navlab-dpe-sdr_amd", "csrc")


def hipcc():
    for c in ("/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


@functools.lru_cache(maxsize=None)
def _compile(name):
    """(assembly text, None), or (None, the compiler's message): a failed compile is cached like a good one."""
    with tempfile.TemporaryDirectory(prefix="isa_") as d:
        out = os.path.join(d, os.path.splitext(name)[0] + ".s")
        p = subprocess.run([hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-Wno-pass-failed",
                            "-S", "--cuda-device-only", os.path.join(CSRC, name), "-o", out], cwd=CSRC,
                           stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        if p.returncode != 0:
            return None, "hipcc -S %s failed (exit %d):\n%s" % (name, p.returncode, p.stderr[-4000:])
        with open(out) as f:
            return f.read(), None


def asm_of(name):
    """The assembly text of csrc/<name> (device code only, no GPU needed); skips the calling test where hipcc is absent and
    fails it, with the compiler's message, where the compile fails."""
    if hipcc() is None:
        pytest.skip("hipcc not available")
    text, err = _compile(name)
    assert err is None, err
    return text
