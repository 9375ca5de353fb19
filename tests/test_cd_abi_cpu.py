"""Collective detection's C-ABI without a GPU: the dpe_cd_ symbols are declared, exported and wrapped, the structs have the
header's layout, the ABI version stays 4, create refuses what it can check before it touches a device, and dpe_cd_predict (host,
fp64, no device) agrees with tests/cd_ref.py's prediction from oracle.sat_pos."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import cd_ref, cd_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dpe_cd_create", "dpe_cd_destroy", "dpe_cd_predict", "dpe_cd_update", "dpe_cd_results", "dpe_cd_map"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return dpe.engine.lib()


def test_symbols_and_version(built):
    hdr = open(os.path.join(ROOT, "include", "dpe_hip.h")).read()
    declared = set(re.findall(r"\b(dpe_cd_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(NAMES)
    for n in NAMES:
        assert hasattr(built, n) and n in dpe.engine.EXPORTS
    assert built.dpe_abi_version() == 4
    assert re.search(r"#define DPE_ABI_VERSION 4\b", hdr)
    assert callable(dpe.CollectiveDetector.update) and callable(dpe.pipeline.collective_detection)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in NAMES:
        assert re.search(r"^\| `%s` \| no reference counterpart: .+ \|$" % n, doc, flags=re.M), n


def test_struct_layouts_match_header():
    e = dpe.engine
    assert C.sizeof(e.CdConfig) == 64 and e.CdConfig.enuGrid.offset == 24 and e.CdConfig.dopplerSign.offset == 56
    assert C.sizeof(e.CdSv) == 64 and e.CdSv.sat.offset == 8 and e.CdSv.delay0.offset == 32 and e.CdSv.dopplerHz.offset == 56
    assert C.sizeof(e.CdResult) == 72 and e.CdResult.score.offset == 24 and e.CdResult.fixEcef.offset == 32
    assert C.sizeof(e.CdSvResult) == 48 and e.CdSvResult.rc.offset == 16 and e.CdSvResult.peak.offset == 40


def _create(**kw):
    a = dict(fs=2.5e6, M=2500, bins=np.arange(-20, 21) * 100.0, grid=np.zeros((1, 3)), J=0, max_sv=8, ds=1.0)
    a.update(kw)
    return dpe.CollectiveDetector(a["fs"], a["M"], a["bins"], a["grid"], drift_half_width=a["J"], max_sv=a["max_sv"], ds=a["ds"])


@pytest.mark.parametrize("kw,msg", [
    (dict(M=8), "M outside 16..32768"), (dict(M=40000), "M outside"), (dict(max_sv=17), "maxSv outside 1..16"),
    (dict(max_sv=0), "maxSv outside"), (dict(J=33), "driftHalfWidth outside 0..32"), (dict(J=-1), "driftHalfWidth outside"),
    (dict(fs=0.0), "sampling frequency not positive"), (dict(bins=np.array([0.0, 0.0])), "zero bin step"),
    (dict(ds=0.5), "dopplerSign is neither"), (dict(grid=np.array([[0.0, np.nan, 0.0]])), "not finite"),
    (dict(grid=np.array([[0.0, 0.0, 0.0], [45455.0, 0.0, 0.0]])), "1.1 Hz per km"),
    (dict(grid=np.zeros((0, 3))), "nPoints outside"),
])
def test_create_refusals_need_no_device(built, kw, msg):
    """Everything create can check it checks before the first device call, with a message that says what."""
    with pytest.raises(dpe.DpeError, match=re.escape(msg)):
        _create(**kw)


def test_largest_allowed_grid_passes_the_check(built):
    """45 454 m at 100 Hz bins is inside (0.5 x 100 / 1.1 km): without a device the call then fails on the allocation, with one
    it succeeds -- either way not on the grid."""
    import torch
    try:
        cd = _create(grid=np.array([[0.0, 0.0, 0.0], [45454.0, 0.0, 0.0]]))
    except dpe.DpeError as e:
        assert not torch.cuda.is_available() and "no device memory" in str(e)
    else:
        cd.close()


def test_null_and_range_arguments(built):
    e = dpe.engine
    with pytest.raises(dpe.DpeError, match="create: null argument"):
        e._check(built.dpe_cd_create(None, None))
    with pytest.raises(dpe.DpeError, match="results: null argument"):
        e._check(built.dpe_cd_results(None, None, None))
    with pytest.raises(dpe.DpeError, match="update: null argument"):
        e._check(built.dpe_cd_update(None, None, 0, None, None, 0, None, None))
    with pytest.raises(dpe.DpeError, match="map: null handle"):
        e._check(built.dpe_cd_map(None, None, None))
    with pytest.raises(dpe.DpeError, match="predict: null argument"):
        e._check(built.dpe_cd_predict(None, 1, None, None, None, None, C.c_double(0.0), None))
    assert built.dpe_cd_destroy(None) == 0
    g = cd_world.geometry()
    b = cd_world.bins()
    with pytest.raises(dpe.DpeError, match="nSv 17 outside 1..16"):
        e.cd_predict(2.5e6, 2500, b, np.tile(g["eph"][:1], (17, 1)), [1] * 17, [0] * 17, g["p0"], g["rx_time"])
    with pytest.raises(dpe.DpeError, match="PRN outside 1..37"):
        e.cd_predict(2.5e6, 2500, b, g["eph"][:1], [40], [0], g["p0"], g["rx_time"])
    bad = g["eph"][:1].copy()
    bad[0, 3] = np.nan
    with pytest.raises(dpe.DpeError, match="ephemeris not finite"):
        e.cd_predict(2.5e6, 2500, b, bad, [2], [0], g["p0"], g["rx_time"])
    with pytest.raises(dpe.DpeError, match="range outside"):
        e.cd_predict(2.5e6, 2500, b, g["eph"][:1], [2], [0], -g["p0"], g["rx_time"])
    with pytest.raises(dpe.DpeError, match="p0 or the receive time is not finite"):
        e.cd_predict(2.5e6, 2500, b, g["eph"][:1], [2], [0], g["p0"], np.inf)


@pytest.mark.parametrize("ds", [1.0, -1.0])
def test_predict_matches_reference(built, oracle, ds):
    """delay0 to 1e-6 sample and bin0 to 1e-6 bin against cd_ref.predict, at the truth, at p0 and a second later."""
    g = cd_world.geometry()
    b = cd_world.bins()
    rows = list(range(len(g["prns"])))
    for p, t in ((g["truth"], g["rx_time"]), (g["p0"], g["rx_time"]), (g["p0"], g["rx_time"] + 1.0)):
        got = dpe.engine.cd_predict(cd_world.FS, cd_world.M, b, g["eph"], g["prns"], rows, p, t, ds=ds)
        want = cd_ref.predict(oracle, g["eph"], g["prns"], rows, p, t, cd_world.FS, cd_world.M, float(b[0]), 100.0, ds=ds)
        for a, w in zip(got, want):
            d = abs(a["delay0"] - w["delay0"])
            assert min(d, cd_world.M - d) < 1e-6 and abs(a["bin0"] - w["bin0"]) < 1e-6
            assert np.abs(a["sat"] - w["sat"]).max() < 1e-4 and abs(a["range0"] - w["range0"]) < 1e-4
            assert (a["prn"], a["row"]) == (w["prn"], w["row"]) and 0.0 <= a["delay0"] < cd_world.M
            assert abs(a["doppler_hz"] - (b[0] + 100.0 * a["bin0"])) < 1e-9


def test_grid_and_frame_helpers(oracle):
    g = dpe.synth.enu_disc_grid(3000.0, 150.0)
    assert g.shape == (1257, 3) and (g[:, 2] == 0).all() and np.sqrt((g ** 2).sum(1)).max() <= 3000.0
    assert (np.abs(g).sum(1) == 0).sum() == 1 and len({tuple(r) for r in g}) == 1257
    assert dpe.synth.enu_disc_grid(100.0, 150.0).shape == (1, 3)
    p0 = cd_world.geometry()["p0"]
    assert np.abs(dpe.synth.enu2ecef_matrix(p0).ravel() - oracle.enu2ecef(oracle.ecef2ll(p0))).max() < 1e-14
