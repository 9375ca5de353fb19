"""The additive C-ABI of the device loop's measurement covariance (dpe_bcm_moments_rval, dpe_chm_dev_set_measurement_cov,
dpe_chm_dev_rval, dpe_rval_record): declared, exported, wrapped, laid out as the header says, refused where no device is needed
to refuse -- and DPE_ABI_VERSION stays 4.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dpe_bcm_moments_rval", "dpe_chm_dev_set_measurement_cov", "dpe_chm_dev_rval")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return dpe.engine.lib()


def test_exports_present_and_version_unchanged(built):
    hdr = open(os.path.join(ROOT, "include", "dpe_hip.h")).read()
    for n in NEW:
        assert hasattr(built, n), n
        assert n in dpe.engine.EXPORTS, n
        assert re.search(r"\bint %s\(" % n, hdr), n
    assert built.dpe_abi_version() == 4 and re.search(r"#define DPE_ABI_VERSION 4\b", hdr)
    assert callable(dpe.engine.ChanMgrDev.set_measurement_cov) and callable(dpe.engine.ChanMgrDev.rval) and callable(dpe.engine.moments_rval)
    assert "128 a block of the" in hdr and "fell back to the identity" in hdr   # the status bit, documented beside the others


def test_rval_record_has_the_headers_layout():
    """The struct as the header declares it, field by field (natural alignment, no padding beyond `reserved`)."""
    hdr = open(os.path.join(ROOT, "include", "dpe_hip.h")).read()
    body = re.search(r"typedef struct dpe_rval_record \{(.*?)\} dpe_rval_record;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = [d.strip() for d in body.split(";") if d.strip()]
    assert decl == ["uint64_t seq", "double R[64]", "double sums[2][15]", "int64_t nAbove[2]", "float threshold[2]", "int32_t fallback",
                    "int32_t reserved"], decl
    r = dpe.engine.RvalRecord
    want = (("seq", 0, 8), ("R", 8, 512), ("sums", 520, 240), ("nAbove", 760, 16), ("threshold", 776, 8), ("fallback", 784, 4),
            ("reserved", 788, 4))
    assert [(n, getattr(r, n).offset, getattr(r, n).size) for n, _ in r._fields_] == list(want)
    assert C.sizeof(r) == 792


def test_refusals_that_need_no_device(built):
    dp = C.POINTER(C.c_double)
    rho, fl = (C.c_double * 2)(0.5, 0.5), np.zeros(4)
    with pytest.raises(dpe.DpeError, match="set_measurement_cov: null handle"):
        dpe.engine._check(built.dpe_chm_dev_set_measurement_cov(None, rho, fl.ctypes.data_as(dp), fl.ctypes.data_as(dp)))
    rec = dpe.engine.RvalRecord()
    with pytest.raises(dpe.DpeError, match="rval: null argument"):
        dpe.engine._check(built.dpe_chm_dev_rval(None, C.c_int64(0), C.byref(rec), None))
    # rho and the floors are looked at before the handle's state: any non-null pointer serves as a handle here
    fake = C.create_string_buffer(4096)
    for bad in (1.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(dpe.DpeError, match=r"set_measurement_cov: rho\[1\] = .* outside \[0, 1\) \(velocity manifold\)"):
            dpe.engine._check(built.dpe_chm_dev_set_measurement_cov(fake, (C.c_double * 2)(0.5, bad), fl.ctypes.data_as(dp), fl.ctypes.data_as(dp)))
    neg = np.array([0.0, -1.0, 0.0, 0.0])
    with pytest.raises(dpe.DpeError, match=r"posFloorVar\[1\] = -1 is negative or not finite"):
        dpe.engine._check(built.dpe_chm_dev_set_measurement_cov(fake, rho, neg.ctypes.data_as(dp), fl.ctypes.data_as(dp)))
    with pytest.raises(dpe.DpeError, match=r"velFloorVar\[1\] = -1 is negative or not finite"):
        dpe.engine._check(built.dpe_chm_dev_set_measurement_cov(fake, rho, fl.ctypes.data_as(dp), neg.ctypes.data_as(dp)))
