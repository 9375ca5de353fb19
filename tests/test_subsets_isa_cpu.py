"""Register and scratch budget of the subsets scan (bcm_scan_subsets_kernel), read from the kernel descriptors in the gfx950
assembly of dpe_bcm.hip: no scratch, no dynamic stack, every template variant emitted, and register counts inside the budget
of a 256-thread block (512 VGPRs per lane at one block per CU; the LPower 1 / 2 variants with subsets stay below 170, which
leaves three waves per SIMD, the plain variants below 80); SGPRs and static LDS are pinned a few above what was measured.  Compiles with hipcc -S (no GPU needed); skips where hipcc is absent."""
import re

import pytest

from tests.isa_asm import asm_of

KERNEL = "_ZN3dpe23bcm_scan_subsets_kernelILi%dELb%dELb%dELb%dEEE"
# (LPower variant, SUBS) -> VGPR budget.  Measured when this budget was set: with subsets 156 .. 158 (LPower 1), 162 .. 164 (2),
# 231 .. 233 (general powf); without 65 .. 68 (1), 68 (2), 135 .. 137 (general powf)
VGPR_MAX = {(1, 1): 162, (2, 1): 168, (0, 1): 237, (1, 0): 72, (2, 0): 72, (0, 0): 141}
# SGPRs, measured: with subsets 80 .. 86 (LPower 1 / 2), without 68 .. 80; the general powf variants take 100 either way
SGPR_MAX = {(1, 1): 90, (2, 1): 90, (0, 1): 104, (1, 0): 84, (2, 0): 84, (0, 0): 104}
# static LDS in bytes, measured: with subsets 1408 .. 1728 (wave keys, 4 x 16 subset keys, per-SV counters and membership words),
# without 80 .. 384
LDS_MAX = {1: 1792, 0: 448}


@pytest.fixture(scope="module")
def asm():
    return asm_of("dpe_bcm.hip")


def _descriptor(text, prefix):
    m = re.search(r"\.amdhsa_kernel (%s\S*)\n(.*?)\.end_amdhsa_kernel" % re.escape(prefix), text, flags=re.S)
    assert m, prefix
    return dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))


@pytest.mark.parametrize("subs", [1, 0])
@pytest.mark.parametrize("lp", [1, 2, 0])
def test_no_scratch_and_register_budget(asm, lp, subs):
    for cp in (0, 1):
        for cv in (0, 1):
            name = KERNEL % (lp, cp, cv, subs)
            d = _descriptor(asm, name)
            assert int(d["private_segment_fixed_size"]) == 0, name
            assert int(d.get("uses_dynamic_stack", "0")) == 0, name
            assert int(d["next_free_vgpr"]) <= VGPR_MAX[(lp, subs)], (name, d["next_free_vgpr"])
            assert int(d["next_free_sgpr"]) <= SGPR_MAX[(lp, subs)], (name, d["next_free_sgpr"])
            assert int(d["group_segment_fixed_size"]) <= LDS_MAX[subs], (name, d["group_segment_fixed_size"])


def test_every_variant_is_emitted(asm):
    names = set(re.findall(r"\.amdhsa_kernel (_ZN3dpe23bcm_scan_subsets_kernel\S+)", asm))
    assert len(names) == 24, sorted(names)
