"""CPU: the numpy restatement of the manifold moments (tests/moments_ref.py) held to something it did not compute itself --
Gaussian rows exp(-d^T Sigma^-1 d / 2) on a 21^4 uniform grid of step 0.5, whose covariance is Sigma up to the +-5 sigma
truncation (5e-6 on a unit variance; the lattice sum itself adds ~exp(-2 pi^2 sigma^2 / h^2) = 1e-34).  Passes without the
feature, by design: it proves the yardstick the GPU tests use.

Threshold count.  The issue that asked for these tests expected nAbove == 5^4 at rho = 0.5 on the Sigma = I row, from "5 points
per axis".  Five per axis is right (exp(-x^2 / 2) > 1/2 for |x| < 1.177, i.e. k = -2 .. 2 at step 0.5), but one scalar threshold
on the 4-D row selects the lattice BALL sum k_i^2 < 2 ln 2 / 0.25 = 5.545, not the box: 1 + 8 + 24 + 32 + 24 + 48 = 137 points
with sum k_i^2 = 0 .. 5.  The test asserts both the five per axis and the 137, the latter counted from the integer lattice."""
import itertools

import numpy as np
import pytest

from tests import moments_ref as mr


@pytest.fixture(scope="module")
def rows():
    grid, iso, ax = mr.gaussian_case()
    _, cor, _ = mr.gaussian_case(mr.SIGMA_XY)
    return grid, iso, cor, ax


@pytest.mark.parametrize("which", ["identity", "xy_correlated"])
def test_raw_score_weights_recover_sigma(rows, which):
    grid, iso, cor, _ = rows
    row, sigma = (iso, np.eye(4)) if which == "identity" else (cor, mr.SIGMA_XY)
    r = mr.moments(row, grid, row.max(), 0.0)
    assert r["tau"] == 0.0 and r["nAbove"] == np.count_nonzero(row > 0)
    assert np.abs(r["mean"]).max() < 1e-9
    assert np.abs(r["cov"] - sigma).max() < 1e-4, np.abs(r["cov"] - sigma).max()
    assert (r["cov"] == r["cov"].T).all()


def test_half_maximum_threshold_counts_the_lattice_ball(rows):
    grid, iso, _, ax = rows
    assert iso.max() == np.float32(1.0)
    r = mr.moments(iso, grid, iso.max(), 0.5)
    assert r["tau"] == np.float32(0.5)
    k = np.rint(grid.astype(np.float64) / 0.5).astype(int)
    above = iso > r["tau"]
    for a in range(4):      # exactly 5 points per axis exceed the threshold
        others = [b for b in range(4) if b != a]
        on_axis = above & (k[:, others] == 0).all(axis=1)
        assert on_axis.sum() == 5 and sorted(k[on_axis, a]) == [-2, -1, 0, 1, 2]
        assert k[above, a].min() == -2 and k[above, a].max() == 2
    ball = sum(1 for v in itertools.product(range(-3, 4), repeat=4) if sum(c * c for c in v) * 0.25 < 2 * np.log(2.0))
    assert ball == 137 and r["nAbove"] == ball
    # the thresholded weights are symmetric about the peak: zero mean, isotropic covariance, smaller than Sigma's
    assert np.abs(r["mean"]).max() < 1e-12
    c = r["cov"]
    assert np.abs(c - np.diag(np.diag(c))).max() < 1e-12 and np.ptp(np.diag(c)) < 1e-12 and 0.05 < c[0, 0] < 1.0


def test_nan_scores_contribute_nothing(rows):
    grid, iso, _, _ = rows
    bad = iso.copy()
    hit = np.arange(100) * 1931 + 7
    bad[hit] = np.nan
    zeroed = iso.copy()
    zeroed[hit] = 0.0
    a, b = mr.moments(bad, grid, iso.max(), 0.0), mr.moments(zeroed, grid, iso.max(), 0.0)
    assert (a["sums"] == b["sums"]).all() and a["nAbove"] == b["nAbove"]


def rotation_case(rows):
    """Both manifolds' sums of the correlated row (rho 0 and 0.3), a rotation that moves every axis -- about (1, 2, 3) by 0.7 rad
    (Rodrigues) -- and a centre of ECEF magnitude.  Shared with test_moments_abi_cpu.py, which holds the library's
    dpe_bcm_moments_from_sums to the same numbers."""
    grid, _, cor, _ = rows
    pos, vel = mr.moments(cor, grid, cor.max(), 0.0), mr.moments(cor, grid, cor.max(), 0.3)
    u = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    Kx = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    R = np.eye(3) + np.sin(0.7) * Kx + (1 - np.cos(0.7)) * Kx @ Kx
    centre = np.array([4.0e6, -1.0e6, 4.5e6, 30.0, 1.5, -2.5, 0.25, 0.01])
    return pos, vel, R, centre


def check_from_sums(from_sums, pos, vel, R, centre):
    z, Rv = from_sums([pos["sums"], vel["sums"]], centre, R)
    J = np.eye(4)
    J[:3, :3] = R
    assert np.abs(Rv[:4, :4] - J @ mr.SIGMA_XY @ J.T).max() < 1e-4
    assert np.abs(Rv[:4, :4] - J @ pos["cov"] @ J.T).max() < 1e-12 and np.abs(Rv[4:, 4:] - J @ vel["cov"] @ J.T).max() < 1e-12
    assert (Rv == Rv.T).all() and not Rv[:4, 4:].any() and not Rv[4:, :4].any()
    # (a centre of 4e6 m has an ulp of 1e-9 m)
    assert np.abs(z[:4] - (centre[:4] + J @ pos["mean"])).max() < 1e-8 and np.abs(z[4:] - (centre[4:] + J @ vel["mean"])).max() < 1e-12
    # no point above the threshold: S0 == 0 gives NaN for that manifold only
    z3, R3 = from_sums([np.zeros(15), vel["sums"]], centre, R)
    assert np.isnan(z3[:4]).all() and np.isnan(R3[:4, :4]).all() and (z3[4:] == z[4:]).all() and (R3[4:, 4:] == Rv[4:, 4:]).all()
    assert not R3[:4, 4:].any() and not R3[4:, :4].any()
    return z, Rv


def test_from_sums_after_rotation(rows):
    check_from_sums(mr.from_sums, *rotation_case(rows))
