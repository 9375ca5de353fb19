"""Register and scratch budget of the synthesiser kernel (syn_kernel, both forms), read from the kernel descriptors in the gfx950
assembly of dpe_syn.hip: no scratch, no dynamic stack, at most 128 VGPRs (four waves per SIMD), no static LDS (the K x 1023 chip table
is the launch's dynamic allocation).  Only kernel descriptors are read.  Compiles with hipcc -S (no GPU needed); skips where hipcc is
absent."""
import re

import pytest

from tests.isa_asm import asm_of

KERNEL = "_ZN3dpe10syn_kernelILb%dEEE"


@pytest.fixture(scope="module")
def asm():
    return asm_of("dpe_syn.hip")


def _descriptor(text, prefix):
    m = re.search(r"\.amdhsa_kernel (%s\S*)\n(.*?)\.end_amdhsa_kernel" % re.escape(prefix), text, flags=re.S)
    assert m, prefix
    return dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))


@pytest.mark.parametrize("name", [KERNEL % 0, KERNEL % 1])
def test_no_scratch_and_register_budget(asm, name):
    d = _descriptor(asm, name)
    assert int(d["private_segment_fixed_size"]) == 0, name
    assert int(d.get("uses_dynamic_stack", "0")) == 0, name
    assert int(d["next_free_vgpr"]) <= 128, (name, d["next_free_vgpr"])
    assert int(d["group_segment_fixed_size"]) == 0, (name, d["group_segment_fixed_size"])


def test_both_forms_are_emitted(asm):
    names = set(re.findall(r"\.amdhsa_kernel (_ZN3dpe10syn_kernel\S+)", asm))
    assert len(names) == 2 and {n[:len(KERNEL % 0)] for n in names} == {KERNEL % 0, KERNEL % 1}, sorted(names)
