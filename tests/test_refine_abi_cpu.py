"""CPU: the coarse-to-fine calls exist in the header, the library and the Python layer, each has its INTEGRATION.md row, and
the result struct has the header's layout; DPE_ABI_VERSION is unchanged (the change is additive)."""
import ctypes as C
import inspect
import os
import re

import pytest

import navlab_dpe_sdr_amd as dpe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dpe_bcm_create_refine", "dpe_bcm_update_refine", "dpe_bcm_results_refine", "dpe_bcm_refine_scores", "dpe_bcm_refine_keys")


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
    assert "typedef struct dpe_bcm_refine_result" in hdr and re.search(r"#define DPE_REFINE_MAX_LEVELS 4\b", hdr)
    bcm = open(os.path.join(ROOT, "navlab-dpe-sdr_amd", "csrc", "dpe_bcm.hip")).read()
    assert bcm.index('#include "dpe_bcm_axes.h"') < bcm.index('#include "dpe_bcm_refine.h"')
    assert "2.4g" in open(os.path.join(ROOT, "DESIGN.md")).read() and "dpe_bcm_refine.h" in open(os.path.join(ROOT, "README.md")).read()


def test_result_struct_layout_and_python_face():
    r = dpe.engine.BcmRefineResult
    assert dpe.engine.REFINE_MAX_LEVELS == 4
    assert C.sizeof(r) == 8 * 8 + 8 * 8 + 4 * 8 + 4 * 8 + 4 * 4 + 4 * 4 + 4 * 8 + 4 * 8 == 288
    assert r.zVal.offset == 0 and r.offset.offset == 64 and r.posIndex.offset == 128 and r.velIndex.offset == 160
    assert r.posScore.offset == 192 and r.velScore.offset == 208 and r.posOutOfWindow.offset == 224 and r.velOutOfWindow.offset == 256
    for m in ("Start", "Update", "results", "read_scores", "read_keys", "last_split", "Stop"):
        assert callable(getattr(dpe.RefineManifold, m)), m
    assert "level" in inspect.signature(dpe.RefineManifold.read_scores).parameters
    assert "level" in inspect.signature(dpe.RefineManifold.read_keys).parameters
    assert callable(dpe.pipeline.run_refine_closed_loop) and callable(dpe.pipeline.bank_half_widths_refine)
    # levels are pairs of whole GridAxes; the half-widths follow the SUMMED extents of the levels
    ax = dpe.GridAxes.uniform(3, 10.0)
    with pytest.raises(dpe.DpeError, match="pair of whole GridAxes"):
        dpe.RefineManifold(2.5e6, 5000, dpe.engine.carr_fft_len(5000), [(ax, ax.shard(0, 5))])
    nfft = dpe.engine.carr_fft_len(5000)
    one = dpe.pipeline.bank_half_widths(ax.points(), ax.points(), 2.5e6, nfft)
    assert dpe.pipeline.bank_half_widths_refine([(ax, ax)], 2.5e6, nfft) == one
    big = dpe.GridAxes.uniform(3, 500.0)
    two = dpe.pipeline.bank_half_widths_refine([(big, big), (ax, ax)], 2.5e6, nfft)
    both = dpe.GridAxes.uniform(3, 510.0)
    assert two == dpe.pipeline.bank_half_widths(both.points(), both.points(), 2.5e6, nfft)
