"""Budget of the measurement kernel with the manifold moments' covariance (chm_k1_cov_kernel, csrc/dpe_chm_dev.h), read from the
kernel descriptors in the gfx950 assembly of dpe_chanmgr.hip: emitted, no scratch, no dynamic stack, and LDS and VGPRs within what
its one 64-thread block needs -- the figures the build gives, pinned: 6608 bytes of LDS (chm_k1_kernel's 5832 plus the 30 sums, two
counts, R and the fallback word) and 132 VGPRs -- 64 of them the 32 block partials a lane keeps in flight while it folds a row (one wave per SIMD is all the kernel ever runs: up to 512 are free).  chm_k1_kernel
stays emitted beside it, with the LDS it had.  Only kernel descriptors are read.  Compiles with hipcc -S; skips where hipcc is absent."""
import re

import pytest

from tests.isa_asm import asm_of

COV = "_ZN3dpeL17chm_k1_cov_kernelE"
K1 = "_ZN3dpeL13chm_k1_kernelE"


@pytest.fixture(scope="module")
def asm():
    return asm_of("dpe_chanmgr.hip")


def _descriptor(text, prefix):
    m = re.search(r"\.amdhsa_kernel (%s\S*)\n(.*?)\.end_amdhsa_kernel" % re.escape(prefix), text, flags=re.S)
    assert m, prefix
    return dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))


def test_cov_kernel_is_emitted_without_scratch(asm):
    d = _descriptor(asm, COV)
    assert int(d["private_segment_fixed_size"]) == 0, d["private_segment_fixed_size"]
    assert int(d.get("uses_dynamic_stack", "0")) == 0


def test_cov_kernel_lds_and_vgprs_are_pinned(asm):
    d = _descriptor(asm, COV)
    assert int(d["group_segment_fixed_size"]) == 6608, d["group_segment_fixed_size"]
    assert int(d["next_free_vgpr"]) <= 132, d["next_free_vgpr"]


def test_plain_kernel_keeps_its_lds(asm):
    d = _descriptor(asm, K1)
    assert int(d["group_segment_fixed_size"]) == 5832, d["group_segment_fixed_size"]
    assert int(d.get("uses_dynamic_stack", "0")) == 0
