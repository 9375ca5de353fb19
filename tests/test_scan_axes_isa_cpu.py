"""Instruction budget of the grid-axes scan (bcm_scan_axes_kernel<1, false, false, false>), read from the gfx950 assembly of
dpe_bcm.hip and set against the point-cloud headline (bcm_scan_kernel<1, false, false, false, false>) in the same assembly:
vector instructions per (point, SV) in the innermost (SV) loop of each manifold, registers, scratch.  Compiles with hipcc -S
(no GPU needed); skips where hipcc is absent."""
import re

import pytest

from tests.isa_asm import asm_of

AXES = "_ZN3dpe20bcm_scan_axes_kernelILi1ELb0ELb0ELb0EEE"
POINTS = "_ZN3dpe15bcm_scan_kernelILi1ELb0ELb0ELb0ELb0EEE"
PER_POINT_SV_MAX = 7.5


@pytest.fixture(scope="module")
def asm():
    return asm_of("dpe_bcm.hip")


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


def _sv_loops(blocks):
    """The SV loops: single-block loops nested in a tile loop (by the compiler's annotations, "Parent Loop ... Depth=1") that read
    the banks from LDS.  Returns [(VALU count, ds_read count)] per loop."""
    out = []
    for b in blocks:
        if not re.search(r"Parent Loop BB\w+ Depth=1", b["note"]):
            continue
        ds = sum(1 for i in b["ins"] if i.startswith("ds_read"))
        if ds:
            out.append((sum(1 for i in b["ins"] if i.startswith("v_")), ds))
    return out


def _per_point_sv(text, prefix, ds_per_point):
    """Vector instructions per (point, SV) of each manifold's SV loop: the loop's count over the points x SVs it scores, which
    its bank reads give (ds_per_point reads per (point, SV))."""
    return sorted(v / (ds / ds_per_point) for v, ds in _sv_loops(_kernel_blocks(text, prefix)))


def _meta(text, prefix, key):
    m = re.search(r"\.name:\s+" + prefix + r".*?\n(?:.*\n)*?\s+\." + key + r":\s+(\d+)", text)
    return int(m.group(1))


def test_axes_sv_loop_budget(asm):
    axes = _per_point_sv(asm, AXES, 2)     # ds_read_b64 {A, B} + ds_read_b32 {C} per (point, SV)
    points = _per_point_sv(asm, POINTS, 2)
    assert len(axes) == 2, "expected one SV loop per manifold, found %d" % len(axes)
    assert len(set(points)) == 2, points   # (two SV loops per manifold: the tile loop is unrolled by two)
    for a in axes:
        assert a <= PER_POINT_SV_MAX, "axes SV loop: %.2f vector instructions per (point, SV)" % a
    # cheaper manifold against cheaper manifold (velocity), dearer against dearer (position)
    assert axes[0] < min(points) and axes[1] < max(points), (axes, points)


def test_axes_no_scratch_and_registers(asm):
    assert _meta(asm, AXES, "private_segment_fixed_size") == 0
    assert _meta(asm, AXES, "vgpr_spill_count") == 0
    assert _meta(asm, AXES, "vgpr_count") <= _meta(asm, POINTS, "vgpr_count")
