"""Instruction budget of the headline scan variant (bcm_scan_kernel<1, false, false, false, false>), read from the gfx950
assembly of dpe_bcm.hip: the vector instructions a full tile spends outside the per-SV loop, and no 64-bit compare in
the full-tile loop.  Compiles with hipcc -S (no GPU needed); skips where hipcc is absent."""
import re

import pytest

from tests.isa_asm import asm_of

HEADLINE = "_ZN3dpe15bcm_scan_kernelILi1ELb0ELb0ELb0ELb0EEE"
# full-tile loop, vector instructions outside the SV loop, counted statically over the loop body (the loop holds two tiles;
# cold blocks such as the K = 0 path and the hand-over to the ragged tile are included): 27 (velocity) / 33 (position)
# when this budget was set, against ~100 per tile of the predicated loop it replaced
VALU_PER_TILE_MAX = 36
SV_LOOP_VALU_MAX = 41   # one SV of four points (position side; the velocity side needs 35)


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


def _tile_loops(blocks):
    """Outermost loops (depth 1, by the compiler's loop annotations) that contain an inner loop: the full-tile loops of the
    two manifolds.  Returns {header: (blocks outside the inner loops, inner-loop blocks)}."""
    loops = {}
    for b in blocks:
        m = re.search(r"(?:Header=|Parent Loop )(BB\w+) Depth=1", b["note"])
        if m:
            key = m.group(1)
        elif "=>This Loop Header: Depth=1" in b["note"]:
            key = b["name"][2:]
        else:
            continue
        outer, inner = loops.setdefault(key, ([], []))
        (inner if "Parent Loop" in b["note"] else outer).append(b)
    return {k: v for k, v in loops.items() if v[1]}


def _valu(b):
    return sum(1 for i in b["ins"] if i.startswith("v_"))


def test_headline_full_tile_budget(asm):
    loops = _tile_loops(_kernel_blocks(asm, HEADLINE))
    assert len(loops) == 2, "expected one full-tile loop per manifold, found %d" % len(loops)
    for header, (outer, inner) in loops.items():
        # the loop body holds two tiles (the prefetch alternates between two register sets): two SV loops
        assert len([b for b in inner if any(i.startswith("ds_read") for i in b["ins"])]) == 2, header
        per_tile = sum(_valu(b) for b in outer) / 2.0
        assert per_tile <= VALU_PER_TILE_MAX, "%s: %.1f VALU per full tile outside the SV loop" % (header, per_tile)
        for b in inner:
            assert _valu(b) <= SV_LOOP_VALU_MAX, "%s: SV loop grew to %d VALU" % (header, _valu(b))
        cmp64 = [i for b in outer for i in b["ins"] if re.match(r"v_cmp\w*_[iu]64", i)]
        assert not cmp64, "64-bit compares in the full-tile loop: %s" % cmp64
        # the tile's grid points arrive by four 16-byte buffer loads per tile, no vector address arithmetic
        loads = [i for b in outer for i in b["ins"] if i.startswith("buffer_load_dwordx4")]
        assert len(loads) == 8, header
