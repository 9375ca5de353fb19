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
