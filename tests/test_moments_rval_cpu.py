"""dpe_bcm_moments_rval (host export of csrc/dpe_bcm_moments_cov.h, the function the device-resident loop forms its R with) against
a numpy restatement in extended precision.  Every entry of a block is a bilinear form of at most 16 + 16 products,
    R[a][b] = sum_cd J[a][c] C[c][d] J[b][d] + sum_c J[a][c] floor[c] J[b][c],     C[c][d] = (S2[c][d] - mu[c] S1[d]) / S0,
and has to lie within 32 * 2^-53 * (the same sums over absolute values) of the restatement.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe

SECOND = np.array([[5, 6, 7, 8], [6, 9, 10, 11], [7, 10, 12, 13], [8, 11, 13, 14]])
EPS = 32 * 2.0 ** -53


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return dpe.engine.lib()


def sums_of(points, weights):
    """The fifteen sums of weighted points [n, 4], in MOMENT_NAMES' order, accumulated in fp64."""
    s = np.zeros(15)
    for x, w in zip(points, weights):
        s[0] += w
        s[1:5] += w * x
        for a in range(4):
            for b in range(a, 4):
                s[SECOND[a, b]] += w * x[a] * x[b]
    return s


def rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q


def restate(sums, R, floor):
    """-> (blocks [2, 4, 4], bound [2, 4, 4], M [2, 4, 4], F [2, 4, 4]) in long double; the bound from absolute values."""
    ld = np.longdouble
    J = np.eye(4, dtype=ld)
    J[:3, :3] = np.asarray(R, dtype=ld).reshape(3, 3)
    out, bound, Ms, Fs = [], [], [], []
    for m in range(2):
        S = np.asarray(sums[m], dtype=ld)
        mu = S[1:5] / S[0]
        S2 = S[SECOND]
        Cm = (S2 - np.outer(mu, S[1:5])) / S[0]
        Cabs = (np.abs(S2) + np.outer(np.abs(mu), np.abs(S[1:5]))) / np.abs(S[0])
        D = np.diag(np.asarray(floor[m], dtype=ld))
        M, F = J @ Cm @ J.T, J @ D @ J.T
        out.append(M + F)
        bound.append(EPS * (np.abs(J) @ Cabs @ np.abs(J).T + np.abs(J) @ D @ np.abs(J).T))
        Ms.append(M)
        Fs.append(F)
    return np.array(out), np.array(bound), np.array(Ms), np.array(Fs)


@pytest.mark.parametrize("seed", range(8))
def test_random_sums_match_numpy_within_the_rounding_bound(built, seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(5, 40))
    sums = np.array([sums_of(rng.standard_normal((n, 4)) * rng.uniform(0.1, 30.0, 4) + rng.uniform(-5, 5, 4), rng.uniform(0.1, 50.0, n))
                     for _ in range(2)])
    Rm, floor = rotation(rng), rng.uniform(0.0, 2.0, (2, 4))
    R, fb = dpe.engine.moments_rval(sums, Rm, floor)
    want, bound, M, F = restate(sums, Rm, floor)
    assert fb == 0
    for m in range(2):
        blk = R[4 * m:4 * m + 4, 4 * m:4 * m + 4]
        err = np.abs(blk.astype(np.longdouble) - want[m])
        assert (err <= bound[m]).all(), (m, float((err / bound[m]).max()))
    # bit-symmetric, and the off-diagonal blocks exactly 0
    assert R.tobytes() == np.ascontiguousarray(R.T).tobytes()
    assert not R[:4, 4:].any() and not R[4:, :4].any()
    assert not np.signbit(R[:4, 4:]).any() and not np.signbit(R[4:, :4]).any()
    # RValMom of dpe_bcm_moments_from_sums is what R carries on top of the floor: R - F equals it to the same bound
    _, RValMom = dpe.engine.moments_from_sums(sums, np.zeros(8), Rm)
    for m in range(2):
        sl = slice(4 * m, 4 * m + 4)
        err = np.abs((R[sl, sl].astype(np.longdouble) - F[m]) - RValMom[sl, sl].astype(np.longdouble))
        assert (err <= bound[m]).all(), (m, float((err / bound[m]).max()))
        assert (np.abs(RValMom[sl, sl].astype(np.longdouble) - M[m]) <= bound[m]).all()


def test_single_point_gives_the_floor_exactly(built):
    """One point above the threshold at rho = 0: S2 - mu S1 cancels to an exact 0, and the block is F bit for bit -- F by the
    function's own loop order, v = 0; for c: v += (J[a][c] * d[c]) * J[b][c], upper triangle mirrored.  (0 + F: a -0.0 of F reads +0.0.)"""
    rng = np.random.default_rng(21)
    # as the moments kernel meets them: grid offsets with a few mantissa bits (multiples of the spacing) and a weight that is the
    # difference of two fp32 scores -- the products w x and (w x) x are then exact, which is what makes the cancellation exact
    x = rng.integers(-40, 41, (2, 4)) * 0.25
    w = rng.uniform(1.0, 9.0, 2).astype(np.float32).astype(np.float64)
    sums = np.array([sums_of(x[m:m + 1], w[m:m + 1]) for m in range(2)])
    Rm, floor = rotation(rng), rng.uniform(0.01, 2.0, (2, 4))
    R, fb = dpe.engine.moments_rval(sums, Rm, floor)
    assert fb == 0
    J = np.eye(4)
    J[:3, :3] = Rm
    for m in range(2):
        F = np.zeros((4, 4))
        for a in range(4):
            for b in range(a, 4):
                v = 0.0
                for c in range(4):
                    v += (J[a, c] * floor[m, c]) * J[b, c]
                F[a, b] = F[b, a] = v
        assert np.array_equal(R[4 * m:4 * m + 4, 4 * m:4 * m + 4], F), m


@pytest.mark.parametrize("m", [0, 1])
def test_empty_manifold_falls_back_to_the_identity(built, m):
    """S0 = 0 in one manifold: that block is the 4 x 4 identity, bit m of fallback is set, the other block is what it is alone."""
    rng = np.random.default_rng(5 + m)
    full = np.array([sums_of(rng.standard_normal((9, 4)), rng.uniform(0.5, 2.0, 9)) for _ in range(2)])
    Rm, floor = rotation(rng), rng.uniform(0.0, 1.0, (2, 4))
    ref, fb0 = dpe.engine.moments_rval(full, Rm, floor)
    sums = full.copy()
    sums[m] = 0.0
    R, fb = dpe.engine.moments_rval(sums, Rm, floor)
    assert fb0 == 0 and fb == 1 << m
    sl, ot = slice(4 * m, 4 * m + 4), slice(4 * (1 - m), 4 * (1 - m) + 4)
    assert np.array_equal(R[sl, sl], np.eye(4))
    assert R[ot, ot].tobytes() == ref[ot, ot].tobytes()
    assert not R[sl, ot].any() and not R[ot, sl].any()


def test_refusals(built):
    dp = C.POINTER(C.c_double)
    s, R9, f, out, fb = np.ones((2, 15)), np.eye(3).reshape(9), np.zeros((2, 4)), np.zeros(64), C.c_int32(0)
    with pytest.raises(dpe.DpeError, match="moments_rval: null argument"):
        dpe.engine._check(built.dpe_bcm_moments_rval(None, R9.ctypes.data_as(dp), f.ctypes.data_as(dp), out.ctypes.data_as(dp), C.byref(fb)))
    for bad in (-1.0, np.nan, np.inf):
        g = f.copy()
        g[1, 2] = bad
        with pytest.raises(dpe.DpeError, match=r"floorVar\[1\]\[2\]"):
            dpe.engine.moments_rval(s, R9, g)
