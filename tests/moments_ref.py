"""numpy restatement of the manifold moments (include/dpe_hip.h, dpe_bcm_moments).  No GPU code.

For one score row: tau = float32(rho) * smax as one IEEE fp32 multiply; w_i = s_i > tau ? (double)s_i - (double)tau : 0 (a NaN
score fails the compare); the fifteen sums S = sum_i w_i {1, x, y, z, t, xx, xy, xz, xt, yy, yz, yt, zz, zt, tt} about the grid
origin, each term formed in fp64 from the fp32 inputs and the terms added with math.fsum (the correctly rounded sum, whatever
the order).  abs_sums are the sums of the terms' magnitudes: the scale of the bound of any fp64 summation order."""
import math

import numpy as np

NAMES = ("1", "x", "y", "z", "t", "xx", "xy", "xz", "xt", "yy", "yz", "yt", "zz", "zt", "tt")
PAIRS = ((0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3))   # sums[5:] in order


def threshold(smax, rho):
    return np.float32(rho) * np.float32(smax)


def smax_of_key(key):
    """The fp32 whose bits are the high word of a packed (score, index) key."""
    return np.array([int(key) >> 32], dtype=np.uint32).view(np.float32)[0]


def mean_cov(sums):
    """(mu [4], C [4, 4]) from one manifold's sums; C = S2 / S0 - mu mu^T evaluated as (S2 - mu S1^T) / S0, one value per pair.
    NaN where S0 == 0."""
    s = np.asarray(sums, dtype=np.float64)
    mu, C = np.full(4, np.nan), np.full((4, 4), np.nan)
    if s[0] != 0.0 and not np.isnan(s[0]):
        mu = s[1:5] / s[0]
        for k, (a, b) in enumerate(PAIRS):
            C[a, b] = C[b, a] = (s[5 + k] - mu[a] * s[1 + b]) / s[0]
    return mu, C


def moments(scores, grid, smax, rho):
    """scores: float32 [G]; grid: float32 [G, 4] (the offsets the device scored); smax: float32; rho: the manifold's threshold
    ratio.  Returns dict(sums [15], abs_sums [15], nAbove, tau, mean [4], cov [4, 4])."""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    g = np.ascontiguousarray(grid, dtype=np.float32).reshape(-1, 4)
    assert s.shape == (g.shape[0],)
    tau = threshold(smax, rho)
    with np.errstate(invalid="ignore"):
        above = s > tau
        w = np.where(above, s.astype(np.float64) - np.float64(tau), 0.0)
    d = g.astype(np.float64)
    first = [w * d[:, a] for a in range(4)]
    terms = [w] + first + [first[a] * d[:, b] for a, b in PAIRS]
    sums = np.array([math.fsum(t) for t in terms])
    abs_sums = np.array([np.abs(t).sum() for t in terms])      # (a scale, not a value under test: numpy's pairwise sum will do)
    mu, C = mean_cov(sums)
    return dict(sums=sums, abs_sums=abs_sums, nAbove=int(np.count_nonzero(above)), tau=tau, mean=mu, cov=C)


def from_sums(sums2, centre, enu2ecef):
    """numpy twin of dpe_bcm_moments_from_sums: (zValMom [8], RValMom [8, 8]) from both manifolds' sums [2, 15]."""
    J = np.eye(4)
    J[:3, :3] = np.asarray(enu2ecef, dtype=np.float64).reshape(3, 3)
    z, R = np.zeros(8), np.zeros((8, 8))
    for m in range(2):
        mu, C = mean_cov(np.asarray(sums2)[m])
        z[4 * m:4 * m + 4] = np.asarray(centre, dtype=np.float64)[4 * m:4 * m + 4] + J @ mu
        M = J @ C @ J.T
        R[4 * m:4 * m + 4, 4 * m:4 * m + 4] = np.triu(M) + np.triu(M, 1).T   # both triangles from one value
    return z, R


def gaussian_case(sigma=None, dim=21, step=0.5):
    """The analytic yardstick: a dim^4 uniform grid of the given step about the origin (float32 [dim^4, 4], t fastest, and its
    four axes) and the row exp(-d^T Sigma^-1 d / 2) as float32."""
    ax = (np.arange(dim) - (dim - 1) / 2) * step
    X = np.stack(np.meshgrid(ax, ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 4)
    Si = np.linalg.inv(np.eye(4) if sigma is None else np.asarray(sigma, dtype=np.float64))
    row = np.exp(-0.5 * np.einsum("ia,ab,ib->i", X, Si, X)).astype(np.float32)
    return X.astype(np.float32), row, ax


SIGMA_XY = np.eye(4)
SIGMA_XY[0, 1] = SIGMA_XY[1, 0] = 0.6
