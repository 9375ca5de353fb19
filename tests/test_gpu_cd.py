"""GPU: collective detection (dpe_cd_*, CollectiveDetector, pipeline.collective_detection) against tests/cd_ref.py.

Parity on injected random surfaces is the sensitive test -- any wrong index shows.  Tolerance (derived, tests/cd_ref.py TOL): every
term is non-negative, so nothing cancels; the fp32 chain of K <= 16 lerps and adds is within (K + 3) 2^-24 <= 1.2e-6 of the score, the
rounding of the lerp weight adds 2^-24 of the row maximum: |GPU - reference| <= 2e-6 max(score, row maximum).  A point's (j, m) and
the global arg-max must be the reference's wherever the reference's own top-two margin exceeds that; elsewhere either candidate
within the tolerance is accepted, at no more than 1 % of a case's points (tests/test_cd_world_cpu.py shows the inputs meet that cap
by themselves).  Then the two worlds of tests/cd_world.py through the real Acquisition surface, and the handle's behaviour."""
import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import cd_ref, cd_world

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


def _scan(torch, c, p0=None, cd=None):
    own = cd is None
    if own:
        cd = dpe.CollectiveDetector(c["fs"], c["M"], c["bins"], c["grid"], drift_half_width=c["J"], max_sv=c["K"])
    surf = torch.from_numpy(c["surface"]).cuda()
    cd.update(surf, c["sv"], c["p0"] if p0 is None else p0, c["R"])
    fix, per = cd.results()
    score, jm = cd.read_map()
    if own:
        cd.close()
    return fix, per, score, jm


@pytest.mark.parametrize("name", list(cd_world.RANDOM_CASES))
def test_parity_on_random_surfaces(torch_cuda, name):
    c = cd_world.random_case(name)
    ref, tol = c["ref"], cd_world.tolerance(c["ref"])
    J, M = c["J"], c["M"]
    fix, per, score, jm = _scan(torch_cuda, c)
    d = np.abs(score.astype(np.float64) - ref["map_score"])
    print("%s: largest |GPU - reference| / tolerance over the map: %.3f (tolerance %.3g)" % (name, (d / tol).max(), tol.max()))
    assert (d <= tol).all()
    same = (jm == ref["map_jm"]).all(1)
    assert same[ref["map_margin"] > tol].all()
    staged = cd_ref.staged_rows(c["surface"], c["sv"], J)
    for p in np.nonzero(~same)[0]:            # the other candidate has to be within the tolerance of the reference's best
        assert -J <= jm[p, 0] <= J and 0 <= jm[p, 1] < M
        alt = cd_ref.point_terms(c["surface"], c["sv"], ref["tau"][p], J, staged).sum(0)[jm[p, 0] + J, jm[p, 1]]
        assert ref["map_score"][p] - alt <= tol[p]
    assert (~same).mean() <= 0.01
    # the global arg-max
    bp = ref["point"]
    if ref["margin"] > tol[bp]:
        assert (fix["point"], fix["j"], fix["m"]) == (bp, ref["j"], ref["m"])
    else:
        assert ref["score"] - ref["map_score"][fix["point"]] <= tol[bp]
    assert (fix["j"], fix["m"]) == tuple(jm[fix["point"]]) and fix["score"] == score[fix["point"]]
    assert abs(fix["score"] - ref["score"]) <= tol[bp]
    assert fix["bins_out_of_range"] == ref["bins_out_of_range"]
    assert np.abs(fix["fix_ecef"] - (c["p0"] + c["R"] @ c["grid"][fix["point"]])).max() < 1e-6
    assert abs(fix["clock_bias_m"] - fix["m"] / c["fs"] * cd_ref.C_LIGHT) < 1e-6
    assert abs(fix["clock_drift_mps"] + fix["j"] * cd_world.RANDOM_BIN_STEP * cd_ref.C_LIGHT / cd_ref.F_L1) < 1e-9
    # per SV at the arg-max
    if (fix["point"], fix["j"], fix["m"]) == (bp, ref["j"], ref["m"]):
        rc, fc, fi = cd_ref.sv_results(ref, c["fs"], float(c["bins"][0]), cd_world.RANDOM_BIN_STEP)
        for k, r in enumerate(per):
            inside = 0 <= ref["dopp_idx"][k] < c["bins"].size
            assert (r["prn"], r["max_code_idx"], r["max_dopp_idx"], r["found"]) == (k + 1, ref["code_idx"][k], ref["dopp_idx"][k], inside)
            assert abs(r["peak"] - ref["peak"][k]) <= cd_ref.TOL * ref["row_max"]
            assert abs(r["rc"] - rc[k]) < 1e-9 and abs(r["fc"] - fc[k]) < 1e-6 and abs(r["fi"] - fi[k]) < 1e-9
        assert abs(sum(r["peak"] for r in per) - fix["score"]) <= tol[bp]


def _world_run(torch, cn0):
    g = cd_world.geometry()
    acq = dpe.Acquisition(cd_world.FS, cd_world.S, g["prns"], cd_world.bins(), mode="coherent")
    samples = torch.from_numpy(cd_world.window(cn0)).cuda()
    out = dpe.pipeline.collective_detection(acq, samples, g["eph"], g["prns"], g["p0"], g["rx_time"], g["grid"], cd_world.J)
    return g, acq, samples, out


def test_noiseless_world_through_acquisition(torch_cuda):
    """The real Acquisition surface: the fix is the truth point, every SV's index pair is Acquisition.results()' own, and fine on
    the collective per-SV results returns what fine on the ordinary results returns."""
    g, acq, samples, out = _world_run(torch_cuda, None)
    fix = out["fix"]
    assert fix["point"] == g["true_point"] and fix["m"] == cd_world.M_TRUE and fix["j"] == cd_world.J_TRUE
    assert np.abs(fix["fix_ecef"] - g["truth"]).max() < 1e-6 and fix["bins_out_of_range"] == 0
    assert all(r["found"] for r in out["ordinary"])
    for c, r in zip(out["coarse"], out["ordinary"]):
        assert (c["prn"], c["max_code_idx"], c["max_dopp_idx"]) == (r["prn"], r["max_code_idx"], r["max_dopp_idx"])
        assert abs(c["rc"] - r["rc"]) < 1e-9 and c["fi"] == r["fi"] and abs(c["fc"] - r["fc"]) < 1e-6
    fine = acq.fine(samples, out["ordinary"])
    for a, b in zip(out["tracker_init"], fine):
        assert a["fi"] == b["fi"] and abs(a["rc"] - b["rc"]) < 1e-9 and abs(a["ri"] - b["ri"]) < 1e-6 and a["found"]
    # the device prediction is the reference's
    for a, w in zip(out["sv"], g["sv"]):
        assert abs(a["delay0"] - w["delay0"]) < 1e-6 and abs(a["bin0"] - w["bin0"]) < 1e-6
    acq.close()


def test_weak_world_cold_start(torch_cuda):
    """Acquisition alone finds at most half of the SVs; the collective fix is the truth point, and every SV's delay index there is
    within one sample of the truth's, the unfound ones included.  The per-SV results go into the tracker as they are."""
    g, acq, samples, out = _world_run(torch_cuda, cd_world.WEAK_CN0)
    K = len(g["prns"])
    found = sum(int(r["found"]) for r in out["ordinary"])
    print("Acquisition found %d of %d; collective point %d (truth %d)" % (found, K, out["fix"]["point"], g["true_point"]))
    assert found <= K // 2
    assert out["fix"]["point"] == g["true_point"]
    assert np.abs(out["fix"]["fix_ecef"] - g["truth"]).max() < 1e-6
    _, delay = cd_world.channels()
    for c, want in zip(out["coarse"], np.round(delay).astype(np.int64)):
        d = abs(c["max_code_idx"] - int(want))
        assert min(d, cd_world.M - d) <= 1
    trk = dpe.ScalarTracker(cd_world.FS, g["prns"])
    trk.set_params(out["tracker_init"])
    trk.close()
    acq.close()


def test_handle_behaviour(torch_cuda):
    c = cd_world.random_case("lds-2500-k8")
    p0b = c["p0"] + c["R"] @ np.array([400.0, -300.0, 20.0])
    alone_a, alone_b = _scan(torch_cuda, c), _scan(torch_cuda, c, p0=p0b)
    assert not np.array_equal(alone_a[2], alone_b[2])
    cd = dpe.CollectiveDetector(c["fs"], c["M"], c["bins"], c["grid"], drift_half_width=c["J"], max_sv=c["K"])
    with pytest.raises(dpe.DpeError, match="results: no update yet"):
        cd.results()
    surf = torch_cuda.from_numpy(c["surface"]).cuda()
    # two updates back to back on one stream: the second's results are those of the second alone, and the first's come back
    cd.update(surf, c["sv"], c["p0"], c["R"])
    cd.update(surf, c["sv"], p0b, c["R"])
    fix, per = cd.results()
    score, jm = cd.read_map()
    assert np.array_equal(score, alone_b[2]) and np.array_equal(jm, alone_b[3]) and per == alone_b[1]
    assert {k: v for k, v in fix.items() if k != "fix_ecef"} == {k: v for k, v in alone_b[0].items() if k != "fix_ecef"}
    again = _scan(torch_cuda, c, cd=cd)
    assert np.array_equal(again[2], alone_a[2]) and np.array_equal(again[3], alone_a[3]) and again[1] == alone_a[1]
    assert np.array_equal(again[0]["fix_ecef"], alone_a[0]["fix_ecef"])
    # refused on the host, before anything is launched: the map stays what it was
    with pytest.raises(dpe.DpeError, match="surface row outside the surface"):
        cd.update(surf, c["sv"], c["p0"], c["R"], n_rows=max(s["row"] for s in c["sv"]))
    bad = [dict(s) for s in c["sv"]]
    bad[3]["delay0"] = float(c["M"])
    with pytest.raises(dpe.DpeError, match=r"delay0 outside \[0, M\)"):
        cd.update(surf, bad, c["p0"], c["R"])
    small = dpe.CollectiveDetector(c["fs"], c["M"], c["bins"], c["grid"], drift_half_width=c["J"], max_sv=4)
    with pytest.raises(dpe.DpeError, match="nSv 8 outside 1..4"):
        small.update(surf, c["sv"], c["p0"], c["R"])
    small.close()
    assert np.array_equal(cd.read_map()[0], alone_a[2])
    cd.close()
