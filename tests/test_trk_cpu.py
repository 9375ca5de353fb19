"""CPU: scalar tracking -- the numpy restatement tests/trk_ref.py against the twin's own logs (fixture O14), the fixture's
own properties, gen_iq_record, and the header / INTEGRATION / struct-layout checks of the dpe_trk_ symbols.

Measured (this fixture, fp64 numpy on x86-64): trk_ref reproduces every logged quantity of the twin, all 361 rows x 4 channels
x 22 names, the cp_sign streams and the carried p_a, with a residual of exactly 0 -- both do the same IEEE operations in the
same order.  Ten times that is still 0: the assertions below are equalities."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import trk_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRK_SYMBOLS = {"dpe_trk_create", "dpe_trk_destroy", "dpe_trk_set_params", "dpe_trk_track", "dpe_trk_correlate", "dpe_trk_read_log",
               "dpe_trk_read_cp_signs", "dpe_trk_state", "dpe_trk_dev_status"}


@pytest.fixture(scope="module")
def o14(golden):
    g = golden("o14_scalar_track")
    return g, trk_ref.o14_iq(g)


@pytest.fixture(scope="module")
def ref_run(o14):
    g, iq = o14
    return trk_ref.track(iq, float(g["fs"]), float(g["T"]), g["prn"], g["start"], int(g["M"]))


def test_trk_ref_equals_the_twin(o14, ref_run):
    g, _ = o14
    log, case, signs, seg, ps = ref_run
    M = int(g["M"])
    for n in trk_ref.LOG_NAMES:
        a, b = log[n], g["log_" + n]
        assert a.shape == b.shape == (M + 1, len(g["prn"]))
        assert np.array_equal(np.isnan(a), np.isnan(b)), n
        res = np.nanmax(np.abs(a - b))
        print("%-8s residual %.3e" % (n, res))
        assert res == 0.0, n                      # 10 x the measured residual (0)
    for k in range(len(g["prn"])):
        n = int(g["cp_sign_n"][k])
        assert signs[k].size == n and np.array_equal(signs[k], g["cp_sign"][k, :n])
        assert log["cp"][M, k] == n


def test_o14_is_the_recording_the_issue_asks_for(o14, ref_run):
    """K >= 4 with Dopplers of both signs, M >= 300, every channel declared locked inside the record, >= 10 nav bits, one channel
    visiting all three boundary cases, start parameters off the truth, and no prompt sign decided on less than 1 % of the
    channel's median prompt magnitude (so the GPU test's allowance for such signs is never needed by the twin itself)."""
    g, _ = o14
    log, case, signs, seg, ps = ref_run
    M, K = int(g["M"]), len(g["prn"])
    assert K >= 4 and M >= 300 and (g["syn_fi"] > 0).any() and (g["syn_fi"] < 0).any()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "o14_scalar_track.npz")) < \
        max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden"))
            if f.endswith(".npz") and not f.startswith("o14"))
    assert (g["log_lock"][0] == 0).all() and (g["log_lock"][M - 1] == 1).all()
    assert all(np.argmax(g["log_lock"][:M, k] > 0) > 240 for k in range(K))
    assert (g["nav_bits_n"] >= 10).all()
    assert any(set(case[:, k]) == {0, 1, 2} for k in range(K))
    d_rc = np.abs((g["start"][:, 0] - g["syn_rc"] + 511.5) % 1023.0 - 511.5)
    assert (d_rc > 0.01).all() and (d_rc < 0.5).all() and (np.abs(g["start"][:, 3] - g["syn_fi"]) > 5.0).all()
    for k in range(K):
        med = np.median(np.hypot(g["log_iP"][:M, k], g["log_qP"][:M, k]))
        assert np.abs(ps[k]).min() > 0.01 * med, (k, np.abs(ps[k]).min() / med)


def test_twin_recovers_the_nav_bits(o14):
    """Once the loops have pulled in, the twin's cp_sign stream is the synthesised bit stream up to one sign per channel."""
    g, _ = o14
    for k in range(len(g["prn"])):
        n = int(g["cp_sign_n"][k])
        s = g["cp_sign"][k, :n]
        agree = trk_ref.nav_bit_agreement(s, g["nav_bits"][k], int(g["syn_cp_ref"][k]), skip=100)
        assert agree in (0.0, 1.0), (k, agree)


def test_gen_iq_record_is_continuous():
    """A record cut into windows equals gen_iq's single windows where the two overlap in meaning: no noise, one channel, no bit
    edge -- the second window continues the first one's code and carrier phase."""
    fs, S = 2.5e6, 2500
    ch = dpe.synth.random_channels(3, 1, prns=[7])
    ch["cp_ref"] = np.array([1])       # the first nav-bit edge is the first code-period boundary
    iq, bits = dpe.synth.gen_iq_record(1, fs, 3 * S, ch, amp=100.0, sigma=0.0, nav_bits=[np.ones(2, dtype=np.int8)])
    t = np.arange(3 * S) / fs
    chips = dpe.synth.ca_code(7).astype(np.float64)
    x = 100.0 * chips[np.mod(np.floor(t * ch["fc"][0] + ch["rc"][0]).astype(np.int64), 1023)] * np.exp(2j * np.pi * (ch["fi"][0] * t + ch["ri"][0]))
    assert np.array_equal(iq[0::2], np.rint(x.real).astype(np.int16)) and np.array_equal(iq[1::2], np.rint(x.imag).astype(np.int16))
    # a sign change exactly at the first code-period boundary when the first edge is there
    iq2, _ = dpe.synth.gen_iq_record(1, fs, 3 * S, ch, amp=100.0, sigma=0.0, nav_bits=[np.array([1, -1], dtype=np.int8)])
    edge = int(np.argmax(np.floor(t * ch["fc"][0] + ch["rc"][0]) >= 1023))
    assert np.array_equal(iq2[:2 * edge], iq[:2 * edge]) and np.array_equal(iq2[2 * edge:], -iq[2 * edge:])
    assert bits[0].size == 2


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return dpe.engine.lib()


def test_trk_symbols_in_header_library_and_integration_md(built):
    hdr = open(os.path.join(ROOT, "include", "dpe_hip.h")).read()
    names = set(re.findall(r"\b(dpe_trk_[a-z0-9_]+)\s*\(", hdr))
    assert names == TRK_SYMBOLS
    for n in names:
        assert hasattr(built, n) and n in dpe.engine.EXPORTS, n
    assert built.dpe_abi_version() == 4 and "#define DPE_ABI_VERSION 4 " in hdr
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("## 1b."):]
    rows = dict(re.findall(r"^\| `(dpe_trk_[a-z0-9_]+)` \| (.+) \|$", sec, flags=re.M))
    assert set(rows) == TRK_SYMBOLS
    for n, v in rows.items():       # every row cites the twin by file:line, or says why there is nothing to cite
        assert re.search(r"\.py:\d+", v) or v.startswith("none"), n
    assert "ScalarTracker" in dpe.__all__ and dpe.ScalarTracker is dpe.engine.ScalarTracker


def test_trk_struct_layouts_match_header():
    e = dpe.engine
    assert C.sizeof(e.TrkConfig) == 208 and e.TrkConfig.prn.offset == 56 and e.TrkConfig.logCapacityWindows.offset == 48
    assert C.sizeof(e.TrkChanState) == 104 and e.TrkChanState.rc.offset == 40
    hdr = open(os.path.join(ROOT, "include", "dpe_hip.h")).read()
    assert "#define DPE_TRK_LOG_DOUBLES %d" % len(e.ScalarTracker.LOG_NAMES) in hdr
    assert e.ScalarTracker.LOG_NAMES[:22] == trk_ref.LOG_NAMES


def test_trk_create_fails_loudly_without_a_gpu_and_checks_its_config(built):
    import torch
    with pytest.raises(dpe.DpeError):
        dpe.ScalarTracker(2.5e6, [4, 9], T=0.02)            # the twin's boundary cases cover one code period
    with pytest.raises(dpe.DpeError):
        dpe.ScalarTracker(2.5e6, [4, 99])
    if not torch.cuda.is_available():
        with pytest.raises(dpe.DpeError):
            dpe.ScalarTracker(2.5e6, [4, 9])                # hipMalloc fails -> error, never a CPU path
