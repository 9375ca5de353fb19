"""CPU: the manifold-moments calls exist in the header, the library and the Python layer, each has its INTEGRATION.md row, the
two structs have the header's layout, DPE_ABI_VERSION is unchanged (the change is additive), the refusals that need no device
refuse, and the library's host-only dpe_bcm_moments_from_sums gives the numbers the numpy restatement was held to."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import moments_ref as mr
from tests.test_moments_ref_cpu import check_from_sums, rotation_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dpe_bcm_moments", "dpe_bcm_moments_results", "dpe_bcm_moments_dev", "dpe_bcm_moments_from_sums")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return dpe.engine.lib()


def test_new_symbols_exported_and_documented(built):
    hdr = open(os.path.join(ROOT, "include", "dpe_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("## 1b."):]
    rows = dict(re.findall(r"^\| `(dpe_[a-z0-9_]+)` \| (.+) \|$", sec, flags=re.M))
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(built, n) and n in dpe.engine.EXPORTS, n
        assert len(rows.get(n, "")) > 20, n
    assert built.dpe_abi_version() == 4 and re.search(r"#define DPE_ABI_VERSION 4\b", hdr)
    assert "typedef struct dpe_bcm_moments_config" in hdr and "typedef struct dpe_bcm_moments_result" in hdr
    bcm = open(os.path.join(ROOT, "navlab-dpe-sdr_amd", "csrc", "dpe_bcm.hip")).read()
    assert bcm.index('#include "dpe_bcm_subsets.h"') < bcm.index('#include "dpe_bcm_moments.h"')
    assert "2.4h" in open(os.path.join(ROOT, "DESIGN.md")).read() and "dpe_bcm_moments.h" in open(os.path.join(ROOT, "README.md")).read()


def _header_fields(hdr, name):
    """(type, field, array dims) of every member of `typedef struct name { ... }`, comments removed, in order."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.match(r"(const )?(\w+) (.+)", decl)
        for item in m.group(3).split(","):
            item = item.strip()
            ptr = item.startswith("*")
            f = re.match(r"\*?(\w+)((\[\d+\])*)", item)
            out.append(("ptr" if ptr else m.group(2), f.group(1), [int(d) for d in re.findall(r"\[(\d+)\]", f.group(2))]))
    return out


SIZES = {"double": 8, "int64_t": 8, "int32_t": 4, "float": 4, "ptr": 8}


@pytest.mark.parametrize("cname,pytype", [("dpe_bcm_moments_config", "BcmMomentsConfig"), ("dpe_bcm_moments_result", "BcmMomentsResult")])
def test_struct_layout_against_the_header(cname, pytype):
    hdr = open(os.path.join(ROOT, "include", "dpe_hip.h")).read()
    st = getattr(dpe.engine, pytype)
    off = 0
    fields = _header_fields(hdr, cname)
    assert [f for _, f, _ in fields] == [f[0] for f in st._fields_]
    for ctype, field, dims in fields:      # natural alignment: every member of these structs is 4 or 8 bytes
        size = SIZES[ctype]
        off = (off + size - 1) // size * size
        assert getattr(st, field).offset == off, (cname, field)
        assert getattr(st, field).size == size * int(np.prod(dims)) if dims else getattr(st, field).size == size, (cname, field)
        off += getattr(st, field).size
    assert C.sizeof(st) == (off + 7) // 8 * 8
    assert C.sizeof(dpe.engine.BcmMomentsConfig) == 64 and C.sizeof(dpe.engine.BcmMomentsResult) == 840


def test_python_face():
    sig = inspect.signature(dpe.BatchCorrManifold.moments)
    assert list(sig.parameters) == ["self", "rho", "keys", "pos_scores", "vel_scores", "n_windows", "stream"]
    assert callable(dpe.engine.moments_from_sums) and len(dpe.engine.MOMENT_NAMES) == 15 == len(mr.NAMES)
    assert tuple(dpe.engine.MOMENT_NAMES) == mr.NAMES
    assert inspect.signature(dpe.pipeline.run_closed_loop).parameters["measurement_cov"].default is None


def _refused(built, h, cfg, pattern):
    assert built.dpe_bcm_moments(h, cfg, None) != 0
    msg = built.dpe_last_error().decode()
    assert msg.startswith("[BatchCorrManifold] moments:") and re.search(pattern, msg), msg


def test_refusals_that_need_no_device(built):
    _refused(built, None, None, "null config")
    for rho, pat in (((1.0, 0.5), r"rho\[0\]"), ((0.5, 1.0), r"rho\[1\]"), ((float("nan"), 0.0), r"rho\[0\]"), ((0.0, float("inf")), r"rho\[1\]"),
                     ((-0.1, 0.0), r"rho\[0\]")):
        cfg = dpe.engine.BcmMomentsConfig((C.c_double * 2)(*rho), None, None, None, 0, 0, 0, 0)
        _refused(built, None, C.byref(cfg), pat + ".*outside \\[0, 1\\)")
    cfg = dpe.engine.BcmMomentsConfig((C.c_double * 2)(0.0, 0.999), None, None, None, 0, 0, 0, 0)
    _refused(built, None, C.byref(cfg), "null handle")
    assert built.dpe_bcm_moments_results(None, None, None) != 0 and built.dpe_bcm_moments_dev(None, None, None) != 0
    assert built.dpe_bcm_moments_from_sums(None, None, None, None, None) != 0


def test_library_from_sums_after_rotation(built):
    grid, iso, ax = mr.gaussian_case()
    _, cor, _ = mr.gaussian_case(mr.SIGMA_XY)
    pos, vel, R, centre = rotation_case((grid, iso, cor, ax))
    z, Rv = check_from_sums(dpe.engine.moments_from_sums, pos, vel, R, centre)
    z2, R2 = mr.from_sums([pos["sums"], vel["sums"]], centre, R)
    assert np.abs(z2 - z).max() < 1e-8 and np.abs(R2 - Rv).max() < 1e-12
    # a single point: the covariance is exactly 0 (raw-score weights: w x is exact in fp64, so S2 - mu S1 cancels bit for bit)
    one = mr.moments(np.array([0.37], dtype=np.float32), np.array([[1.7, -0.3, 2.9, 0.11]], dtype=np.float32), np.float32(0.37), 0.0)
    z1, R1 = dpe.engine.moments_from_sums([one["sums"], one["sums"]], centre, R)
    assert not R1.any() and one["nAbove"] == 1
