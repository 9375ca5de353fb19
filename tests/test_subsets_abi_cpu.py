"""CPU: the subsets calls exist in the header, the library and the Python layer, each has its INTEGRATION.md row, and the
result struct has the header's layout; DPE_ABI_VERSION is unchanged (the change is additive)."""
import ctypes as C
import inspect
import os
import re

import pytest

import navlab_dpe_sdr_amd as dpe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dpe_bcm_create_subsets", "dpe_bcm_update_subsets", "dpe_bcm_results_subsets")


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
    assert built.dpe_abi_version() == 4
    assert "typedef struct dpe_bcm_subset_result" in hdr and "dpe_bcm_subsets.h" in open(
        os.path.join(ROOT, "navlab-dpe-sdr_amd", "csrc", "dpe_bcm.hip")).read()
    assert "2.4f" in open(os.path.join(ROOT, "DESIGN.md")).read() and "dpe_bcm_subsets.h" in open(os.path.join(ROOT, "README.md")).read()


def test_result_struct_layout_and_python_face():
    r = dpe.engine.BcmSubsetResult
    assert C.sizeof(r) == 8 * 8 + 8 * 8 + 8 + 8 + 4 + 4 + 8 + 8 == 168
    assert r.offset.offset == 64 and r.posIndex.offset == 128 and r.velIndex.offset == 136 and r.posScore.offset == 144
    assert r.velScore.offset == 148 and r.posOutOfWindow.offset == 152 and r.velOutOfWindow.offset == 160
    assert issubclass(dpe.SubsetManifold, dpe.BatchCorrManifold) and dpe.engine.SUBSET_MAX == 16
    for m in ("Start", "Update", "results", "read_scores", "read_keys", "last_split", "Stop"):
        assert callable(getattr(dpe.SubsetManifold, m)), m
    assert callable(dpe.pipeline.run_fde_closed_loop) and callable(dpe.engine.leave_one_out_masks)
    # the threshold of the separation test is the caller's decision: no default
    p = inspect.signature(dpe.pipeline.solution_separation).parameters["threshold_m"]
    assert p.default is inspect.Parameter.empty
    assert inspect.signature(dpe.pipeline.run_fde_closed_loop).parameters["threshold_m"].default is inspect.Parameter.empty
    ax = dpe.GridAxes.uniform(3, 10.0)
    with pytest.raises(dpe.DpeError, match="point-list grids only"):
        dpe.SubsetManifold(2.5e6, 5000, dpe.engine.carr_fft_len(5000), ax, ax, 8)
