"""Collective detection's worlds on the CPU (tests/cd_world.py, tests/cd_ref.py): what the GPU tests of tests/test_gpu_cd.py rely on
is asserted here, so that none of them can silently stop showing anything.  No GPU."""
import numpy as np
import pytest

from tests import cd_ref, cd_world


def test_noiseless_world_pins_both_signs():
    """On the oracle's own coarse-acquisition surfaces of the noiseless window the reference's arg-max is the truth point, every SV's
    (delay, Doppler) index pair there is the oracle's own per-PRN peak, and m / j are the window's common delay and Doppler offset:
    the sign of the delay (a longer range and a clock that is ahead both increase it) and of the Doppler bin are the ones
    Acquisition uses."""
    g = cd_world.geometry()
    _, res = cd_world.oracle_acq(None)
    ref = cd_world.reference(None)
    assert ref["point"] == g["true_point"]
    assert ref["m"] == cd_world.M_TRUE and ref["j"] == cd_world.J_TRUE
    assert all(r["found"] for r in res)
    assert list(ref["code_idx"]) == [r["max_code_idx"] for r in res]
    assert list(ref["dopp_idx"]) == [r["max_dopp_idx"] for r in res]
    assert ref["bins_out_of_range"] == 0
    assert ref["point_margin"] > 0.05 * ref["score"]
    # the truth is a grid point to rounding, a few km from p0, and the grid stays within what create accepts for 100 Hz bins
    assert np.abs(g["p0"] + g["R"] @ g["grid"][g["true_point"]] - g["truth"]).max() < 1e-6
    assert 2000.0 < np.linalg.norm(g["truth"] - g["p0"]) < 3000.0
    assert np.sqrt((g["grid"] ** 2).sum(1)).max() < 0.5 * 100.0 / cd_ref.DOPPLER_HZ_PER_KM * 1000.0


def test_weak_world_is_decisive():
    """At the recorded level the oracle's per-PRN acquisition finds at most half of the SVs, the collective arg-max is still the
    truth point, and its margin over every other point is at least ten times the GPU tolerance; one dB above, more than half
    are still found (the recorded level is the first on the way down from 40 dB-Hz)."""
    g = cd_world.geometry()
    K = len(g["prns"])
    found, point, margin, need = cd_world.weak_conditions()
    print("C/N0 %.0f dB-Hz: found %d of %d, point %d (truth %d), margin %.4g against %.4g" % (cd_world.WEAK_CN0, found, K, point,
                                                                                             g["true_point"], margin, need))
    assert found <= K // 2
    assert point == g["true_point"]
    assert margin >= need
    _, res = cd_world.oracle_acq(cd_world.WEAK_CN0 + 1.0)
    assert sum(int(r["found"]) for r in res) > K // 2
    # the per-SV delay indices at the collective arg-max are the truth's, the unfound SVs included
    ref = cd_world.reference(cd_world.WEAK_CN0)
    _, delay = cd_world.channels()
    d = np.abs(ref["code_idx"] - np.round(delay).astype(np.int64))
    assert np.minimum(d, cd_world.M - d).max() <= 1 and ref["m"] == cd_world.M_TRUE and ref["j"] == cd_world.J_TRUE


@pytest.mark.parametrize("name", list(cd_world.RANDOM_CASES))
def test_random_surface_case_is_decisive(name):
    """The reference's own top-two margin exceeds the GPU tolerance at >= 99 % of a case's points and at its global arg-max, so
    the parity test's 1 % cap is met by the inputs themselves; and the case has what it is there for."""
    c = cd_world.random_case(name)
    ref, tol = c["ref"], cd_world.tolerance(c["ref"])
    assert (ref["map_margin"] > tol).mean() >= 0.99
    assert ref["margin"] > tol[ref["point"]]
    M, K, P, J, _ = cd_world.RANDOM_CASES[name]
    assert ref["tau"].shape == (P, K) and c["surface"].dtype == np.float32
    assert (ref["bins_out_of_range"] > 0) == (J > 0)
    fl = np.floor(ref["tau"])
    assert fl[0, 0] == 0 and (K == 1 or fl[0, 1] == M - 1)      # at p0: delays within a sample of 0 and of M ...
    assert P < 5 or (fl < 0).any() or (fl >= M).any()           # ... which the grid's range differences carry across the wrap
    if P >= 5:
        far = np.sqrt((c["grid"] ** 2).sum(1))
        assert far[0] == 0.0 and far[1] == 3000.0 and 0.99 < far[2] / (0.5 * cd_world.RANDOM_BIN_STEP / 1.1 * 1000.0) < 1.0


@pytest.mark.parametrize("name", list(cd_world.PARITY_CASES))
def test_new_parity_case_is_decisive(name):
    """The same two conditions for the second table's parity cases.  The repeated-point case ties with itself by construction:
    there the arg-max's margin is taken over the points at other offsets."""
    c = cd_world.new_case(name)
    ref, tol = c["ref"], cd_world.tolerance(c["ref"])
    (M, K, P, J, _), opts = cd_world.NEW_CASES[name]
    assert ref["tau"].shape == (P, K) and c["surface"].shape == (K + 1, 2 * J + 9, M) and c["surface"].dtype == np.float32
    assert (ref["map_margin"] > tol).mean() >= 0.99
    bp = ref["point"]
    if opts.get("grid") == "repeat3":
        n = P // 3
        assert P == 60 and np.array_equal(c["grid"][:n], c["grid"][n:2 * n]) and np.array_equal(c["grid"][:n], c["grid"][2 * n:])
        assert np.array_equal(ref["map_score"][:n], ref["map_score"][n:2 * n]) and np.array_equal(ref["map_jm"][:n], ref["map_jm"][2 * n:])
        assert bp < n and len(set(map(tuple, c["grid"][:n]))) == n
        others = np.delete(ref["map_score"][:n], bp)
        assert ref["map_margin"][bp] > tol[bp] and ref["score"] - others.max() > tol[bp]
    else:
        assert ref["margin"] > tol[bp]
    if opts.get("surface") == "exp2":         # orders of magnitude: the staged rows' values span more than 1e6 to 1
        v = c["surface"][c["surface"] > 0]
        assert v.max() / np.median(v) > 100.0 and v.max() / v.min() > 1.0e6 and ref["score"] > 1.0e9


def test_drift_cases_decide_the_drift_axis():
    """Interior bins: no (k, j) leaves the raster, so every j competes with all K SVs -- the reference's map takes both signs of j
    in each case, at least 16 distinct values at J = 32, and a global arg-max has j != 0.  Planted rows: an SV sits at each raster
    edge, the surface is four times larger along every SV's row at b_k + plant J, so every point's j is plant J although that drops
    an SV, and that SV's own result at the arg-max is the outside-the-raster branch."""
    off_zero = 0
    for name, (shape, opts) in cd_world.DRIFT_CASES.items():
        c = cd_world.new_case(name)
        ref, J, n_bins = c["ref"], c["J"], c["bins"].size
        j = ref["map_jm"][:, 0]
        b = cd_ref.bins_of(c["sv"])
        if opts.get("bins") == "interior":
            assert ref["bins_out_of_range"] == 0 and (b - J >= 0).all() and (b + J < n_bins).all()
            assert (j < 0).any() and (j > 0).any()
            assert J < 32 or np.unique(j).size >= 16
            off_zero += int(ref["j"] != 0)
        else:
            plant = opts["plant"]
            assert (j == plant * J).all() and ref["j"] == plant * J
            assert ref["bins_out_of_range"] > 0
            outside = (ref["dopp_idx"] < 0) | (ref["dopp_idx"] >= n_bins)
            assert outside.any() and not outside.all() and (ref["peak"][outside] == 0).all()
    assert off_zero >= 1
    shapes = [s[:4] for s, _ in cd_world.DRIFT_CASES.values()]
    assert shapes == [(2500, 8, 49, 2), (2046, 4, 131, 32), (5000, 8, 5, 2), (2500, 8, 9, 2), (2500, 8, 9, 2), (2500, 16, 3, 2)]


@pytest.mark.parametrize("name", list(cd_world.TIE_CASES))
def test_tie_case_is_exact(name):
    """What makes the tie cases' comparison exact: every tau is a whole number, so every score is a sum of K surface values, all
    multiples of 2^-8 -- exact in fp32 as in fp64; the margin is 0 and more than one hypothesis ties at every point; and the
    reference's answer is the first maximum of an independent sum of integer rolls."""
    c = cd_world.new_case(name)
    ref, J, M, K = c["ref"], c["J"], c["M"], c["K"]
    n_bins = c["bins"].size
    assert not c["grid"].any()
    assert np.array_equal(ref["tau"], np.round(ref["tau"])) and (ref["tau"] == ref["tau"][0]).all()
    d0 = [s["delay0"] for s in c["sv"]]
    assert d0[0] == 0.0 and d0[1] == M - 1.0 and np.array_equal(ref["tau"][0], d0)
    assert np.array_equal(c["surface"] * 256.0, np.round(c["surface"] * 256.0)) and c["surface"].max() <= 1.0
    total = np.zeros((2 * J + 1, M), dtype=np.int64)            # in units of 2^-8
    for s, b in zip(c["sv"], cd_ref.bins_of(c["sv"])):
        for jj in range(2 * J + 1):
            if 0 <= b + jj - J < n_bins:
                total[jj] += np.roll(np.round(c["surface"][s["row"], b + jj - J] * 256.0).astype(np.int64), -int(s["delay0"]))
    first = int(total.ravel().argmax())                        # np.argmax: the first maximum
    ties = int((total == total.max()).sum())
    print("%s: (point, j, m) = (%d, %d, %d), score %g, %d tied hypotheses per point" % (name, ref["point"], ref["j"], ref["m"], ref["score"], ties))
    assert ties > 1 and ref["margin"] == 0 and (ref["map_margin"] == 0).all()
    assert (ref["point"], ref["j"], ref["m"]) == (0, first // M - J, first % M) and ref["score"] == total.max() / 256.0
    assert (ref["map_jm"] == (ref["j"], ref["m"])).all() and (ref["map_score"] == ref["score"]).all()
    kind = cd_world.NEW_CASES[name][1]["surface"]
    if kind == "zeros":
        assert (ref["j"], ref["m"], ref["score"]) == (-J, 0, 0.0) and not ref["peak"].any() and ties == (2 * J + 1) * M
    if kind == "ones":                                          # the first j that keeps the most SVs: the edge bins keep all K only at 0
        assert (ref["j"], ref["m"], ref["score"]) == (0, 0, float(K)) and ties == M and ref["bins_out_of_range"] > 0


def test_permuted_subset_of_the_noiseless_world():
    """Six of the eight PRNs in reversed order, rows their own places in the surface: on the oracle's surfaces the reference's
    arg-max is still the truth point with the world's m and j, by a margin over every other point above 5 % of the score."""
    g = cd_world.geometry()
    prns, eph, sv = cd_world.subset()
    assert [s["row"] for s in sv] == list(cd_world.SUBSET_ROWS) and [s["prn"] for s in sv] == prns
    assert [s["row"] for s in sv] != list(range(len(sv))) and len(set(prns)) == 6 and eph.shape == (6, 21)
    surf, res = cd_world.oracle_acq(None)
    ref = cd_ref.scan(surf, sv, g["p0"], g["R"], g["grid"], cd_world.FS, cd_world.J)
    assert ref["point"] == g["true_point"] and ref["m"] == cd_world.M_TRUE and ref["j"] == cd_world.J_TRUE
    assert ref["point_margin"] > 0.05 * ref["score"]
    assert list(ref["code_idx"]) == [res[r]["max_code_idx"] for r in cd_world.SUBSET_ROWS]
    assert list(ref["dopp_idx"]) == [res[r]["max_dopp_idx"] for r in cd_world.SUBSET_ROWS]


def test_reference_lerp_is_continuous_and_circular():
    """The score is continuous in tau and circular over the code period: a delay of M + x scores what x scores, shifted clock values
    are rotations, and whole-sample delays reproduce the surface."""
    rng = np.random.Generator(np.random.PCG64(9))
    M = 64
    surf = rng.random((1, 3, M), dtype=np.float32)
    sv = [dict(prn=1, row=0, sat=np.zeros(3), delay0=0.0, bin0=1.0)]
    t0 = cd_ref.point_terms(surf, sv, np.array([5.0]), 1)
    assert np.array_equal(t0[0, 1], np.roll(surf[0, 1].astype(np.float64), -5))
    assert np.array_equal(t0[0, 0], np.roll(surf[0, 0].astype(np.float64), -5))
    a = cd_ref.point_terms(surf, sv, np.array([5.25]), 1)
    b = cd_ref.point_terms(surf, sv, np.array([5.25 + M]), 1)
    assert np.abs(a - b).max() < 1e-12
    lo, hi = cd_ref.point_terms(surf, sv, np.array([6.0 - 1e-9]), 1), cd_ref.point_terms(surf, sv, np.array([6.0]), 1)
    assert np.abs(lo - hi).max() < 1e-8
    assert np.abs(a[0, 1] - (0.75 * t0[0, 1] + 0.25 * np.roll(t0[0, 1], -1))).max() < 1e-15
