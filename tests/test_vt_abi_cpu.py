"""CPU: the vector tracker's C-ABI (include/dpe_hip.h, additive): symbols, struct sizes, every limit dpe_vt_create refuses with its
message, and the scalar tracker's interface as it was."""
import ctypes as C
import os
import re

import pytest

import navlab_dpe_sdr_amd as dpe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VT_SYMBOLS = ("dpe_vt_create", "dpe_vt_destroy", "dpe_vt_set_ephemerides", "dpe_vt_init", "dpe_vt_init_from_trk", "dpe_vt_track",
              "dpe_vt_read_log", "dpe_vt_read_corr", "dpe_vt_state", "dpe_vt_dev_status", "dpe_vt_filter_step_host")
TRK_SYMBOLS = ("dpe_trk_create", "dpe_trk_destroy", "dpe_trk_set_params", "dpe_trk_track", "dpe_trk_correlate", "dpe_trk_read_log",
               "dpe_trk_read_cp_signs", "dpe_trk_state", "dpe_trk_dev_status")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return dpe.engine.lib()


def test_symbols_and_struct_sizes(built):
    hdr = open(os.path.join(ROOT, "include", "dpe_hip.h")).read()
    names = set(re.findall(r"\b(dpe_vt_[a-z0-9_]+)\s*\(", hdr))
    assert names == set(VT_SYMBOLS)
    for n in VT_SYMBOLS:
        assert hasattr(built, n) and n in dpe.engine.EXPORTS, n
    e = dpe.engine
    assert C.sizeof(e.VtConfig) == 280 and C.sizeof(e.VtChan) == 624 and C.sizeof(e.VtStateRec) == 10592
    assert e.VectorTracker.LOG_HEAD + e.VectorTracker.MAX_CHAN * e.VectorTracker.LOG_CHAN == 212
    assert re.search(r"#define DPE_VT_LOG_HEAD 20\b", hdr) and re.search(r"#define DPE_VT_LOG_CHAN 12\b", hdr) and re.search(r"#define DPE_VT_MAX_CHAN 16\b", hdr)
    assert built.dpe_abi_version() == 4                      # additive: the version check stays as it is


def test_scalar_tracker_interface_unchanged(built):
    hdr = open(os.path.join(ROOT, "include", "dpe_hip.h")).read()
    assert set(re.findall(r"\b(dpe_trk_[a-z0-9_]+)\s*\(", hdr)) == set(TRK_SYMBOLS)
    for n in TRK_SYMBOLS:
        assert hasattr(built, n), n
    assert C.sizeof(dpe.engine.TrkConfig) == 208 and C.sizeof(dpe.engine.TrkChanState) == 104
    for proto in ("int dpe_trk_create(const dpe_trk_config *cfg, dpe_trk **out);",
                  "int dpe_trk_track(dpe_trk *h, const int16_t *samples_dev, int32_t nWindows, dpe_stream_t stream);",
                  "int dpe_trk_set_params(dpe_trk *h, const dpe_acq_track_init *init /* [nChan] */, dpe_stream_t stream);",
                  "int dpe_trk_read_log(dpe_trk *h, int64_t firstWindow, int32_t nWindows, double *out, dpe_stream_t stream);"):
        assert proto in hdr, proto


@pytest.mark.parametrize("kw,prns,msg", [
    (dict(), list(range(1, 18)), r"at most 16 channels .*got 17"),
    (dict(N=7), [1, 2, 3, 4], r"N must be even and in 2 \.\. 20 .*got 7"),
    (dict(N=1), [1, 2, 3, 4], r"N must be even and in 2 \.\. 20 .*got 1"),
    (dict(N=22), [1, 2, 3, 4], r"N must be even and in 2 \.\. 20 .*got 22"),
    (dict(T=1.6e-3), [1, 2, 3, 4], r"the window must be at most 1\.5 ms"),
    (dict(T=0.5002e-3), [1, 2, 3, 4], r"round\(T fs\) = 1251 samples per window must be even"),
    (dict(num_prev=40), [1, 2, 3, 4], r"numPrev must be in 2 \.\. 32"),
    (dict(), [1, 2, 3, 40], r"PRN 40 out of range"),
])
def test_create_refusals(built, kw, prns, msg):
    with pytest.raises(dpe.DpeError, match=msg):
        dpe.VectorTracker(2.5e6, prns, **kw)


def test_null_arguments(built):
    with pytest.raises(dpe.DpeError, match=r"\[VectorTracker\] create: null argument"):
        dpe.engine._check(built.dpe_vt_create(None, None))
    with pytest.raises(dpe.DpeError, match=r"\[VectorTracker\] filter_step_host: null argument"):
        dpe.engine._check(built.dpe_vt_filter_step_host(None, None, None, None, None, None, None))
    assert built.dpe_vt_destroy(None) == 0
