"""Register and scratch budget of the coarse-to-fine scan (bcm_scan_refine_kernel), read from the kernel descriptors in the
gfx950 assembly of dpe_bcm.hip: every template variant emitted, no scratch, no dynamic stack, and VGPRs / SGPRs / static LDS
pinned a few above what the build shows; VGPRs stay at or below 128 (four waves per SIMD, i.e. four 256-thread blocks per CU).
Measured when this budget was set, over the four clamp variants: VGPRs 89 .. 104 (LPower 1), 99 .. 113 (LPower 2), 69 (general
powf); SGPRs 100; static LDS 96 bytes (wave keys and counts).  Only kernel descriptors are read.  Compiles with hipcc -S (no GPU
needed); skips where hipcc is absent."""
import re

import pytest

from tests.isa_asm import asm_of

KERNEL = "_ZN3dpe22bcm_scan_refine_kernelILi%dELb%dELb%dEEE"
VGPR_MAX = {1: 108, 2: 117, 0: 73}
SGPR_MAX = 104
LDS_MAX = 128


@pytest.fixture(scope="module")
def asm():
    return asm_of("dpe_bcm.hip")


def _descriptor(text, prefix):
    m = re.search(r"\.amdhsa_kernel (%s\S*)\n(.*?)\.end_amdhsa_kernel" % re.escape(prefix), text, flags=re.S)
    assert m, prefix
    return dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))


@pytest.mark.parametrize("lp", [1, 2, 0])
def test_no_scratch_and_register_budget(asm, lp):
    for cp in (0, 1):
        for cv in (0, 1):
            name = KERNEL % (lp, cp, cv)
            d = _descriptor(asm, name)
            assert int(d["private_segment_fixed_size"]) == 0, name
            assert int(d.get("uses_dynamic_stack", "0")) == 0, name
            assert int(d["next_free_vgpr"]) <= VGPR_MAX[lp] <= 128, (name, d["next_free_vgpr"])
            assert int(d["next_free_sgpr"]) <= SGPR_MAX, (name, d["next_free_sgpr"])
            assert int(d["group_segment_fixed_size"]) <= LDS_MAX, (name, d["group_segment_fixed_size"])


def test_every_variant_is_emitted(asm):
    names = set(re.findall(r"\.amdhsa_kernel (_ZN3dpe22bcm_scan_refine_kernel\S+)", asm))
    assert len(names) == 12, sorted(names)
