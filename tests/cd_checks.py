"""What a collective-detection scan's outputs are held to (tests/test_gpu_cd.py), as functions that the CPU can call too:
tests/test_cd_checks_cpu.py feeds them the outputs of deliberately wrong numpy scans, so that what the cases reject is on record.

check_parity: the tolerance is tests/cd_ref.py's TOL, derived there; a point's (j, m) and the global arg-max must be the reference's
wherever the reference's own top-two margin exceeds it, elsewhere either candidate within the tolerance is accepted, at no more than
1 % of a case's points.  check_exact: the tie cases, bit for bit.  numpy_scan: the specification's scan with a hook on each point's
[2J + 1, M] scores and a choice of the first or the last maximum, in the shape CollectiveDetector returns."""
import numpy as np

from tests import cd_ref, cd_world


def check_parity(c, fix, per, score, jm, ds=1.0, name=""):
    """c: a case of tests/cd_world.py; fix, per: CollectiveDetector.results(); score, jm: read_map().  Returns the largest
    |score - reference| / tolerance over the map."""
    ref, tol = c["ref"], cd_world.tolerance(c["ref"])
    J, M = c["J"], c["M"]
    n_bins = c["bins"].size
    d = np.abs(score.astype(np.float64) - ref["map_score"])
    ratio = float((d / np.where(tol > 0, tol, 1.0)).max())
    print("%s: largest |GPU - reference| / tolerance over the map: %.3f (tolerance %.3g)" % (name, ratio, tol.max()))
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
    assert abs(fix["clock_drift_mps"] + ds * fix["j"] * cd_world.RANDOM_BIN_STEP * cd_ref.C_LIGHT / cd_ref.F_L1) < 1e-9
    # per SV at the arg-max
    if (fix["point"], fix["j"], fix["m"]) == (bp, ref["j"], ref["m"]):
        rc, fc, fi = cd_ref.sv_results(ref, c["fs"], float(c["bins"][0]), cd_world.RANDOM_BIN_STEP, ds)
        assert len(per) == len(c["sv"])
        for k, r in enumerate(per):
            inside = 0 <= ref["dopp_idx"][k] < n_bins
            assert (r["prn"], r["max_code_idx"], r["max_dopp_idx"], r["found"]) == (k + 1, ref["code_idx"][k], ref["dopp_idx"][k], inside)
            assert abs(r["peak"] - ref["peak"][k]) <= cd_ref.TOL * ref["row_max"]
            if not inside:                    # an SV whose bin leaves the raster at j*: no term, and an index pair that says so
                assert r["found"] is False and r["peak"] == 0 and (r["max_dopp_idx"] < 0 or r["max_dopp_idx"] >= n_bins)
            assert abs(r["rc"] - rc[k]) < 1e-9 and abs(r["fc"] - fc[k]) < 1e-6 and abs(r["fi"] - fi[k]) < 1e-9
        assert abs(sum(r["peak"] for r in per) - fix["score"]) <= tol[bp]
    return ratio


def check_exact(c, fix, score, jm):
    """The tie cases: every point is the same point, and every sum is exact in fp32 and in fp64 alike (tests/test_gpu_cd.py
    test_exact_ties has the argument), so the map, every row of it and the global (point, j, m) equal the reference's first maximum
    bit for bit."""
    ref = c["ref"]
    assert score.dtype == np.float32 and np.array_equal(score, ref["map_score"].astype(np.float32))
    assert np.array_equal(score.astype(np.float64), ref["map_score"])
    assert np.array_equal(jm, ref["map_jm"])
    assert (score == score[0]).all() and (jm == jm[0]).all()
    assert fix["point"] == 0
    assert (fix["point"], fix["j"], fix["m"]) == (ref["point"], ref["j"], ref["m"])
    assert fix["score"] == ref["score"]


def numpy_scan(c, mutate=None, last=False, ds=1.0):
    """The specification's scan in numpy fp64, in the shape the device returns: (fix, per, score fp32 [P], jm int32 [P, 2]).
    mutate(sc [2J + 1, M]) -> the scores a wrong scan would compare; last: the last maximum instead of the first, over (j, m) and
    over the points.  With neither this is cd_ref.scan rounded to fp32."""
    ref, J, M = c["ref"], c["J"], c["M"]
    P = ref["tau"].shape[0]
    n_bins = c["bins"].size
    staged = cd_ref.staged_rows(c["surface"], c["sv"], J)
    score, jm = np.zeros(P), np.zeros((P, 2), dtype=np.int32)
    for p in range(P):
        sc = cd_ref.point_terms(c["surface"], c["sv"], ref["tau"][p], J, staged).sum(0)
        if mutate is not None:
            sc = mutate(sc)
        sc = sc.ravel()
        i = sc.size - 1 - int(sc[::-1].argmax()) if last else int(sc.argmax())
        score[p], jm[p] = sc[i], (i // M - J, i % M)
    bp = P - 1 - int(score[::-1].argmax()) if last else int(score.argmax())
    j, m = int(jm[bp, 0]), int(jm[bp, 1])
    terms = cd_ref.point_terms(c["surface"], c["sv"], ref["tau"][bp], J, staged)[:, j + J, m]
    res = dict(code_idx=np.mod(np.round(ref["tau"][bp] + m).astype(np.int64), M), dopp_idx=cd_ref.bins_of(c["sv"]) + j)
    rc, fc, fi = cd_ref.sv_results(res, c["fs"], float(c["bins"][0]), cd_world.RANDOM_BIN_STEP, ds)
    score32 = score.astype(np.float32)
    fix = dict(point=bp, m=m, j=j, score=float(score32[bp]), bins_out_of_range=ref["bins_out_of_range"],
               fix_ecef=c["p0"] + c["R"] @ c["grid"][bp], clock_bias_m=m / c["fs"] * cd_ref.C_LIGHT,
               clock_drift_mps=-ds * j * cd_world.RANDOM_BIN_STEP * cd_ref.C_LIGHT / cd_ref.F_L1)
    per = [dict(prn=s["prn"], found=bool(0 <= res["dopp_idx"][k] < n_bins), max_code_idx=int(res["code_idx"][k]),
                max_dopp_idx=int(res["dopp_idx"][k]), rc=float(rc[k]), fc=float(fc[k]), fi=float(fi[k]), peak=float(np.float32(terms[k])))
           for k, s in enumerate(c["sv"])]
    return fix, per, score32, jm
