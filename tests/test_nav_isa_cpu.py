"""The scalar navigation kernel (csrc/dpe_nav.hip), read from its gfx950 assembly: no scratch memory, no register spills, no LDS,
fp64 arithmetic, and only vector stores to memory.  Compiles with hipcc -S (no GPU needed); skips where hipcc is absent."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "navlab-dpe-sdr_amd", "csrc", "dpe_nav.hip")
KERNEL = "_ZN3dpe20nav_solve_log_kernel"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = next((c for c in ("/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "dpe_nav.s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-Wno-pass-failed",
                           "-S", "--cuda-device-only", SRC, "-o", out], cwd=os.path.dirname(SRC),
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return open(out).read()


def _metadata(text):
    m = re.search(r"\.name:\s+%s\w*\n(.*?)(?=\n  - \.|\namdhsa\.target)" % re.escape(KERNEL), text, flags=re.S)
    body = text[max(0, m.start() - 1500):m.end()]
    return {k: v for k, v in re.findall(r"\.(\w+):\s+(\S+)", body)}


def _instructions(text):
    lines = text.split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(KERNEL) and l.split(";")[0].rstrip().endswith(":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return [l.strip().split(";")[0].strip() for l in lines[start + 1:end] if l.startswith("\t") and not l.strip().startswith((".", ";"))]


def test_no_scratch_no_spills_no_lds(asm, capsys):
    md = _metadata(asm)
    assert md["private_segment_fixed_size"] == "0" and md["uses_dynamic_stack"] == "false", md
    assert md["sgpr_spill_count"] == "0" and md["vgpr_spill_count"] == "0", md
    assert md["group_segment_fixed_size"] == "0", md
    with capsys.disabled():
        print("\nnav_solve_log_kernel: %s VGPRs, %s SGPRs" % (md["vgpr_count"], md["sgpr_count"]))
    assert int(md["vgpr_count"]) <= 128          # two blocks of four waves per SIMD pair stay resident
    ins = _instructions(asm)
    assert not [i for i in ins if i.startswith(("scratch_", "buffer_"))]
    assert not [i for i in ins if i.startswith("s_") and ("store" in i or "atomic" in i)]       # memory is written by vector stores alone
    assert any(i.startswith("global_store") for i in ins) and not any(i.startswith(("ds_read", "ds_write")) for i in ins)
    assert sum(1 for i in ins if re.match(r"v_\w+_f64", i)) > 500 and any(i.startswith(("ds_bpermute", "v_readlane")) for i in ins)
