"""Register and scratch budget of the multi-epoch scan (bcm_scan_epochs_kernel), read from the kernel descriptors in the
gfx950 assembly of dpe_bcm.hip: no scratch, no spills, and register counts that leave the scan kernels' occupancy (two
256-thread blocks per CU need <= 128 VGPRs per lane for the LPower 1 / 2 variants).  Compiles with hipcc -S (no GPU
needed); skips where hipcc is absent."""
import re

import pytest

from tests.isa_asm import asm_of

KERNEL = "_ZN3dpe22bcm_scan_epochs_kernelILi%dELb%dELb%dEEE"
VGPR_MAX = {1: 96, 2: 96, 0: 160}      # measured when this budget was set: 76 .. 87 (LPower 1), 80 .. 89 (2), 121 .. 140 (general powf)


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
            assert int(d["next_free_vgpr"]) <= VGPR_MAX[lp], (name, d["next_free_vgpr"])
            assert int(d["next_free_sgpr"]) <= 104, (name, d["next_free_sgpr"])
            m = re.search(r"^%s\S*:.*?^\.Lfunc_end" % re.escape(name), asm, flags=re.S | re.M)
            assert m and "scratch_" not in m.group(0), name


def test_every_variant_is_emitted(asm):
    names = set(re.findall(r"\.amdhsa_kernel (_ZN3dpe22bcm_scan_epochs_kernel\S+)", asm))
    assert len(names) == 12, sorted(names)
