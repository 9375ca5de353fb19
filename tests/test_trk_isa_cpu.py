"""Scalar tracking kernels (csrc/dpe_trk.hip), read from their gfx950 assembly: no scratch memory, no register spills, and no
fp64 vector instruction in the sample loop -- carrier and code phase advance there as 64-bit integers, the arithmetic is fp32;
fp64 belongs to the per-window seeds, the reduction and the one-lane loop phase.  Compiles with hipcc -S (no GPU needed);
skips where hipcc is absent."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "navlab-dpe-sdr_amd", "csrc", "dpe_trk.hip")
KERNELS = ("_ZN3dpe17trk_scalar_kernel", "_ZN3dpe20trk_correlate_kernel")


def _hipcc():
    for c in ("/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "dpe_trk.s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-Wno-pass-failed",
                           "-S", "--cuda-device-only", SRC, "-o", out], cwd=os.path.dirname(SRC),
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return open(out).read()


def _kernel_blocks(text, prefix):
    lines = text.split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(prefix) and l.split(";")[0].rstrip().endswith(":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    blocks, cur = [], None
    for l in lines[start + 1:end]:
        m = re.match(r"^(\.LBB\w+|; %bb\.\d+):\s*(;.*)?$", l)
        if m:
            cur = dict(name=m.group(1), note=m.group(2) or "", ins=[])
            blocks.append(cur)
            continue
        t = l.strip()
        if cur is None or not t or t.startswith(";") or t.startswith("."):
            continue
        cur["ins"].append(t.split(";")[0].strip())
    return blocks


def _metadata(text, prefix):
    """The kernel's entry in the amdhsa.kernels metadata: {key: value}."""
    m = re.search(r"\.name:\s+%s\w*\n(.*?)(?=\n  - \.|\namdhsa\.target)" % re.escape(prefix), text, flags=re.S)
    body = text[max(0, m.start() - 1500):m.end()]
    return {k: v for k, v in re.findall(r"\.(\w+):\s+(\S+)", body)}


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_no_spills(asm, kernel):
    md = _metadata(asm, kernel)
    assert md["private_segment_fixed_size"] == "0" and md["uses_dynamic_stack"] == "false", md
    assert md["sgpr_spill_count"] == "0" and md["vgpr_spill_count"] == "0", md
    blocks = _kernel_blocks(asm, kernel)
    assert not [i for b in blocks for i in b["ins"] if i.startswith("scratch_") or i.startswith("buffer_store") or i.startswith("buffer_load")]


@pytest.mark.parametrize("kernel,depth", [(KERNELS[0], 2), (KERNELS[1], 1)])
def test_sample_loop_holds_no_fp64(asm, kernel, depth):
    """The sample loop is the loop that loads the samples (16 bytes per lane) and reads the chip table from LDS: the innermost
    loop of the window loop in trk_scalar_kernel, the only long loop of trk_correlate_kernel."""
    blocks = _kernel_blocks(asm, kernel)
    headers = {}
    for b in blocks:
        m = re.search(r"(?:in Loop: Header=|Inner Loop Header: Depth=|Loop Header: Depth=)(\w*)", b["note"])
        if not m:
            continue
        h = re.search(r"Header=(BB\w+) Depth=(\d+)", b["note"])
        key = (h.group(1), int(h.group(2))) if h else (b["name"][2:], int(re.search(r"Depth=(\d+)", b["note"]).group(1)))
        headers.setdefault(key, []).append(b)
    loops = [v for (hd, d), v in headers.items() if d == depth and any(i.startswith("global_load_dwordx4") for b in v for i in b["ins"])]
    assert len(loops) == 1, [k for k in headers]
    ins = [i for b in loops[0] for i in b["ins"]]
    assert any(i.startswith("ds_read_i8") for i in ins) and sum(1 for i in ins if re.match(r"v_(pk_)?fma", i)) >= 30
    f64 = [i for i in ins if re.match(r"v_\w+_f64", i) or re.match(r"v_cvt_\w*f64", i)]
    assert not f64, f64
