"""GPU: collective detection (dpe_cd_*, CollectiveDetector, pipeline.collective_detection) against tests/cd_ref.py.

Parity on injected random surfaces is the sensitive test -- any wrong index shows.  Tolerance (derived, tests/cd_ref.py TOL): every
term is non-negative, so nothing cancels; the fp32 chain of K <= 16 lerps and adds is within (K + 3) 2^-24 <= 1.2e-6 of the score, the
rounding of the lerp weight adds 2^-24 of the row maximum: |GPU - reference| <= 2e-6 max(score, row maximum).  A point's (j, m) and
the global arg-max must be the reference's wherever the reference's own top-two margin exceeds that; elsewhere either candidate
within the tolerance is accepted, at no more than 1 % of a case's points (tests/test_cd_world_cpu.py shows the inputs meet that cap
by themselves).  The assertions are tests/cd_checks.py's, which tests/test_cd_checks_cpu.py feeds wrong scans on the CPU.  The second
table of tests/cd_world.py adds the cases in which the drift axis decides, exact ties, repeated points and the shapes at the launch
plan's edges.  Then the two worlds of tests/cd_world.py through the real Acquisition surface, and the handle's behaviour."""
import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import cd_checks, cd_ref, cd_world

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


def _scan(torch, c, p0=None, cd=None, n_sv=None, max_sv=None, ds=1.0, stream=None):
    own = cd is None
    if own:
        cd = dpe.CollectiveDetector(c["fs"], c["M"], c["bins"], c["grid"], drift_half_width=c["J"], max_sv=max_sv or c["K"], ds=ds)
    surf = torch.from_numpy(c["surface"]).cuda()
    torch.cuda.synchronize()
    cd.update(surf, c["sv"][:n_sv], c["p0"] if p0 is None else p0, c["R"], stream=stream)
    fix, per = cd.results()
    score, jm = cd.read_map(stream)
    if own:
        cd.close()
    return fix, per, score, jm


def _same(a, b):
    """Two scans' outputs (fix, per, score, jm), byte for byte."""
    return (np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and a[1] == b[1] and np.array_equal(a[0]["fix_ecef"], b[0]["fix_ecef"]) and
            {k: v for k, v in a[0].items() if k != "fix_ecef"} == {k: v for k, v in b[0].items() if k != "fix_ecef"})


def _first_svs(c, n):
    """The case cut to its first n SVs, with the reference of those."""
    sv = c["sv"][:n]
    return dict(c, sv=sv, K=n, ref=cd_ref.scan(c["surface"], sv, c["p0"], c["R"], c["grid"], c["fs"], c["J"]))


@pytest.mark.parametrize("name", list(cd_world.RANDOM_CASES))
def test_parity_on_random_surfaces(torch_cuda, name):
    c = cd_world.random_case(name)
    fix, per, score, jm = _scan(torch_cuda, c)
    cd_checks.check_parity(c, fix, per, score, jm, name=name)


@pytest.mark.parametrize("name", list(cd_world.PARITY_CASES))
def test_parity_on_new_cases(torch_cuda, name):
    """The second table's parity cases (tests/cd_world.py: drift decided, an SV outside the raster at the arg-max, the plan's edge
    shapes, long walks, a surface spanning orders of magnitude), held to the same assertions and the same tolerance.  The repeated
    offsets in addition: the device's arithmetic for a point depends on its coordinates alone, so the three copies of an offset --
    scored by different blocks, in different flush slots -- have the same bytes, and the fix is the first copy."""
    c = cd_world.new_case(name)
    fix, per, score, jm = _scan(torch_cuda, c)
    cd_checks.check_parity(c, fix, per, score, jm, name=name)
    if cd_world.NEW_CASES[name][1].get("grid") == "repeat3":
        n = c["P"] // 3
        assert np.array_equal(score[:n], score[n:2 * n]) and np.array_equal(score[:n], score[2 * n:])
        assert np.array_equal(jm[:n], jm[n:2 * n]) and np.array_equal(jm[:n], jm[2 * n:])
        assert fix["point"] < n
        print("%s: the three copies of every offset agree bit for bit" % name)


@pytest.mark.parametrize("name", list(cd_world.TIE_CASES))
def test_exact_ties(torch_cuda, name):
    """The first-maximum rule ("first maximum in (point, j, m) index order", include/dpe_hip.h) where scores are equal: in a lane
    (the strict >), across lanes, passes and waves (the packed key ~(jj M + m)), across a block's points and the drift blocks (the
    LDS and device atomicMax) and across points (~p in cd_final_kernel).  Every grid point is (0, 0, 0), every delay0 a whole number
    (0 and M - 1 among them), every surface value a multiple of 2^-8 no larger than 1.

    Why equality with the fp64 reference is exact.  The reference: tau is a whole number, f = 0, a score is a sum of K <= 3 surface
    values, and np.argmax is the first maximum (tests/test_cd_world_cpu.py asserts all of it, and an independent integer-roll sum).
    The device: range - range0 may differ from 0 by an ulp of the range (the host's and the device's square roots need not contract
    their sums of squares alike), about 3e-11 sample.  Then tau is a whole number n plus or minus that.  Below n: floor gives n - 1
    and f = (float)(1 - 3e-11) = 1.0f exactly, w0 = 0: the lerp selects sample i0 + 1, which is sample n.  Above n (or equal): f <=
    3e-11 and w0 = 1.0f: each SV adds its sample exactly and then f times the next one, at most 3e-11, which rounds away against any
    sum that is a non-zero multiple of 2^-8 (half an ulp of 2^-8 is 2.3e-10) and is exactly zero on the all-zero surface; a sum that
    is zero on another surface may come out as at most 1e-10 instead, far below the maximum (>= 0.5), which alone is compared.  So
    every score that ties for the maximum is the same fp32 number as in the reference, and no other reaches it."""
    c = cd_world.new_case(name)
    fix, per, score, jm = _scan(torch_cuda, c)
    cd_checks.check_exact(c, fix, score, jm)
    cd_checks.check_parity(c, fix, per, score, jm, name=name)          # the per-SV results at that arg-max
    if cd_world.NEW_CASES[name][1]["surface"] == "zeros":
        assert (fix["point"], fix["j"], fix["m"], fix["score"]) == (0, -c["J"], 0, 0.0) and all(r["peak"] == 0 for r in per)
    print("%s: map, every row and the global (point, j, m) = (%d, %d, %d) equal the reference bit for bit" % (name, fix["point"], fix["j"], fix["m"]))


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


def test_permuted_subset_through_acquisition(torch_cuda):
    """prns a reversed six of acq.prns' eight, eph in that order: the surface rows are 7, 5, 4, 3, 1, 0 and not 0..5.  The fix is the
    truth point with the world's m and j (tests/test_cd_world_cpu.py: the reference's, by 5 % of the score); the six collective
    entries sit at their own rows of `coarse` with the ordinary results' index pairs, the other two are the ordinary results."""
    g = cd_world.geometry()
    prns, eph, sv = cd_world.subset()
    acq = dpe.Acquisition(cd_world.FS, cd_world.S, g["prns"], cd_world.bins(), mode="coherent")
    samples = torch_cuda.from_numpy(cd_world.window(None)).cuda()
    out = dpe.pipeline.collective_detection(acq, samples, eph, prns, g["p0"], g["rx_time"], g["grid"], cd_world.J)
    fix = out["fix"]
    assert fix["point"] == g["true_point"] and fix["m"] == cd_world.M_TRUE and fix["j"] == cd_world.J_TRUE
    assert np.abs(fix["fix_ecef"] - g["truth"]).max() < 1e-6 and fix["bins_out_of_range"] == 0
    assert len(out["coarse"]) == len(g["prns"]) == len(out["ordinary"]) and len(out["sv"]) == len(prns)
    for a, w in zip(out["sv"], sv):
        assert (a["prn"], a["row"]) == (w["prn"], w["row"]) and abs(a["delay0"] - w["delay0"]) < 1e-6 and abs(a["bin0"] - w["bin0"]) < 1e-6
    for row, (c, r) in enumerate(zip(out["coarse"], out["ordinary"])):
        assert c["prn"] == r["prn"] == g["prns"][row]
        if row in cd_world.SUBSET_ROWS:
            assert (c["max_code_idx"], c["max_dopp_idx"], c["found"]) == (r["max_code_idx"], r["max_dopp_idx"], True)
            assert abs(c["rc"] - r["rc"]) < 1e-9 and c["fi"] == r["fi"] and abs(c["fc"] - r["fc"]) < 1e-6
            assert c["peak"] > 0
        else:
            assert c == r
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


def test_sv_count_changes_on_one_handle(torch_cuda):
    """One handle of max_sv = 16 at M = 2 500: 16 SVs (rows from L2), then the first 8 of them (rows in LDS), then 16 again.  Each
    update's map, fix and per-SV list are, byte for byte, those of a fresh handle of exactly that many SVs given that update alone
    -- nothing of an earlier update's SVs, weights or keys is left -- and the 8-SV one is the reference's of those 8.  Then nSv
    below maxSv without a change: 3 SVs on a handle of 8 against a handle of 3."""
    c = cd_world.new_case("plant-minus-l2-2500-k16")
    assert c["M"] == 2500 and c["K"] == 16
    alone16, alone8 = _scan(torch_cuda, c), _scan(torch_cuda, c, n_sv=8, max_sv=8)
    assert len(alone16[1]) == 16 and len(alone8[1]) == 8 and not np.array_equal(alone16[2], alone8[2])
    c8 = _first_svs(c, 8)
    cd_checks.check_parity(c8, *alone8, name="the first 8 of plant-minus-l2-2500-k16")
    cd = dpe.CollectiveDetector(c["fs"], c["M"], c["bins"], c["grid"], drift_half_width=c["J"], max_sv=16)
    assert _same(_scan(torch_cuda, c, cd=cd), alone16)
    assert _same(_scan(torch_cuda, c, cd=cd, n_sv=8), alone8)
    assert _same(_scan(torch_cuda, c, cd=cd), alone16)
    cd.close()
    k8 = cd_world.random_case("lds-2500-k8")
    alone3 = _scan(torch_cuda, k8, n_sv=3, max_sv=3)
    assert _same(_scan(torch_cuda, k8, n_sv=3, max_sv=8), alone3) and len(alone3[1]) == 3
    cd_checks.check_parity(_first_svs(k8, 3), *alone3, name="the first 3 of lds-2500-k8")


def test_update_on_another_stream(torch_cuda):
    """The same update on a non-default stream, results() and the map read on it: the bytes of the default-stream run."""
    c = cd_world.new_case("interior-2500-k8")
    default = _scan(torch_cuda, c)
    stream = torch_cuda.cuda.Stream()
    assert stream.cuda_stream != torch_cuda.cuda.current_stream().cuda_stream
    other = _scan(torch_cuda, c, stream=stream)
    stream.synchronize()
    assert _same(other, default)
    cd_checks.check_parity(c, *other, name="interior-2500-k8 on another stream")


def test_doppler_sign_minus_one(torch_cuda):
    """dopplerSign = -1 on the handle, on a case whose arg-max has j != 0: the scan is the same, the clock drift changes its sign,
    and each SV's fc is formed with the negative sign (cd_ref.sv_results(ds=-1))."""
    c = cd_world.new_case("interior-2500-k8")
    assert c["ref"]["j"] != 0
    plus, minus = _scan(torch_cuda, c), _scan(torch_cuda, c, ds=-1.0)
    cd_checks.check_parity(c, *minus, ds=-1.0, name="interior-2500-k8 at dopplerSign -1")
    assert np.array_equal(plus[2], minus[2]) and np.array_equal(plus[3], minus[3])
    assert minus[0]["clock_drift_mps"] == -plus[0]["clock_drift_mps"] != 0.0
    _, fc, _ = cd_ref.sv_results(c["ref"], c["fs"], float(c["bins"][0]), cd_world.RANDOM_BIN_STEP, ds=-1.0)
    for a, b, want in zip(plus[1], minus[1], fc):
        assert abs(b["fc"] - want) < 1e-6 and (a["fi"], a["rc"], a["peak"]) == (b["fi"], b["rc"], b["peak"])
        assert abs((a["fc"] - cd_ref.F_CA) + (b["fc"] - cd_ref.F_CA)) < 1e-9
