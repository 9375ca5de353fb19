"""Collective detection's specification in numpy fp64 (include/dpe_hip.h): the score, the position-domain map, the
arg-max, the per-SV results and the prediction of (delay0, bin0) from ephemerides.  The yardstick of the dpe_cd_ tests; satellite
states come from oracle.sat_pos.

    tau_k(p) = delay0_k + (|sat_k - (p0 + R d_p)| - |sat_k - p0|) fs / c
    u = tau_k(p) + m,  i0 = floor(u) mod M,  i1 = (i0 + 1) mod M,  f = u - floor(u)
    b_k(j) = round_half_even(bin0_k) + j
    score(p, m, j) = sum_k (1 - f) s[row_k][b_k(j)][i0] + f s[row_k][b_k(j)][i1]      (0 where b_k(j) leaves the raster)
"""
import numpy as np

C_LIGHT = 299792458.0
F_L1 = 1.57542e9
F_CA = 1.023e6
L_CA = 1023
T_CA = 1.0e-3
OE_DOT = 7.2921151467e-5
TOL = 2.0e-6           # |GPU - reference| <= TOL max(score, row maximum): (K + 3) 2^-24 <= 1.2e-6 of the score for the fp32 chain of
                       # K <= 16 lerps and adds of non-negative terms, plus 2^-24 of the row maximum for the rounding of f
DOPPLER_HZ_PER_KM = 1.1


def _rot(state, tau):
    """Satellite state rotated by the Earth's turn over the time of flight, velocity in the inertial form (cuchanmgr.cu:383-404)."""
    x = -OE_DOT * tau
    ct, st = np.cos(x), np.sin(x)
    s = state
    o = np.array(s, dtype=np.float64)
    o[0] = ct * s[0] - st * s[1]
    o[1] = st * s[0] + ct * s[1]
    o[4] = ct * s[4] - st * s[5] - OE_DOT * st * s[0] - OE_DOT * ct * s[1]
    o[5] = st * s[4] + ct * s[5] + OE_DOT * ct * s[0] - OE_DOT * st * s[1]
    return o


def predict(oracle, eph, prns, rows, p0, rx_time, fs, M, bin_start, bin_step, ds=1.0):
    """One dict per SV (prn, row, sat, delay0, bin0, range0, doppler_hz): light time by three fixed-point rounds, the ephemeris at
    the SV clock's reading of the transmit time, a receiver at rest in ECEF."""
    p0 = np.asarray(p0, dtype=np.float64)[:3]
    out = []
    for e, prn, row in zip(np.asarray(eph, dtype=np.float64), prns, rows):
        tau, dt = 0.07, 0.0
        for _ in range(3):
            s, rc = oracle.sat_pos(e, rx_time - tau + dt)
            assert rc == 0
            sr = _rot(s, tau)
            los = sr[:3] - p0
            rng = float(np.sqrt(los[0] * los[0] + los[1] * los[1] + los[2] * los[2]))
            tau, dt = rng / C_LIGHT, s[3]
        ev = np.array([-OE_DOT * p0[1], OE_DOT * p0[0], 0.0])
        lrr = float(np.sum(los / rng * (ev - sr[4:7])))            # minus the range rate
        fi = F_L1 * (lrr / C_LIGHT + sr[7]) / ds
        delay0 = float(np.mod(rng / C_LIGHT - sr[3], T_CA) * fs)
        if delay0 >= M:
            delay0 -= M
        out.append(dict(prn=int(prn), row=int(row), sat=sr[:3].copy(), delay0=delay0, bin0=(fi - bin_start) / bin_step, range0=rng,
                        doppler_hz=fi))
    return out


def taus(sv, p0, R, grid, fs):
    """tau [P, K] in samples."""
    p0 = np.asarray(p0, dtype=np.float64)[:3]
    pe = p0[None, :] + np.asarray(grid, dtype=np.float64) @ np.asarray(R, dtype=np.float64).reshape(3, 3).T
    t = np.zeros((pe.shape[0], len(sv)))
    for k, s in enumerate(sv):
        sat = np.asarray(s["sat"], dtype=np.float64)
        rng = np.sqrt(((sat[None, :] - pe) ** 2).sum(1))
        r0 = np.sqrt(((sat - p0) ** 2).sum())
        t[:, k] = s["delay0"] + (rng - r0) * fs / C_LIGHT
    return t


def bins_of(sv):
    return np.array([int(np.round(s["bin0"])) for s in sv], dtype=np.int64)        # np.round: half to even


def staged_rows(surface, sv, J):
    """Per SV: (ok [2J+1] bool, rows fp64 [n_ok, 2 M + 1]: each staged row twice and its first entry again, so that M consecutive
    entries from any start below M are the row read circularly)."""
    n_bins = surface.shape[1]
    b0 = bins_of(sv)
    out = []
    for k, s in enumerate(sv):
        b = b0[k] + np.arange(-J, J + 1)
        ok = (b >= 0) & (b < n_bins)
        rows = surface[s["row"]][b[ok]].astype(np.float64)
        out.append((ok, np.concatenate([rows, rows, rows[:, :1]], axis=1)))
    return out


def point_terms(surface, sv, tau_p, J, staged=None):
    """Per-SV terms [K, 2J+1, M] of one point (fp64 arithmetic on the fp32 surface)."""
    M = surface.shape[2]
    staged = staged if staged is not None else staged_rows(surface, sv, J)
    out = np.zeros((len(sv), 2 * J + 1, M))
    m = np.arange(M, dtype=np.float64)
    mi = np.arange(M, dtype=np.int64)
    for k in range(len(sv)):
        ok, ext = staged[k]
        u = tau_p[k] + m
        fl = np.floor(u)
        f = u - fl
        i0 = np.mod(fl.astype(np.int64), M)
        i1 = np.mod(i0 + 1, M)
        if np.array_equal(i0, np.mod(i0[0] + mi, M)):          # (always, unless tau + m rounds across an integer) a circular shift: slices
            s0, s1 = ext[:, i0[0]:i0[0] + M], ext[:, i0[0] + 1:i0[0] + 1 + M]
        else:
            s0, s1 = ext[:, i0], ext[:, i1]
        out[k, ok] = (1.0 - f)[None, :] * s0 + f[None, :] * s1
    return out


def scan(surface, sv, p0, R, grid, fs, J):
    """-> dict: map_score [P], map_jm [P, 2] (j, m: the first maximum in (j, m) order), map_margin [P] (best minus second best
    over (j, m)), point / j / m / score of the first global maximum in (p, j, m) order, margin (to the best of every other
    hypothesis), point_margin (to the best of every other POINT), bins_out_of_range, row_max (the largest surface value of any
    staged row), tau [P, K], and per SV at the arg-max: code_idx, dopp_idx, peak."""
    surface = np.asarray(surface)
    M = surface.shape[2]
    t = taus(sv, p0, R, grid, fs)
    P, K = t.shape
    nJ = 2 * J + 1
    score, jm, margin = np.zeros(P), np.zeros((P, 2), dtype=np.int64), np.zeros(P)
    staged = staged_rows(surface, sv, J)
    for p in range(P):
        sc = point_terms(surface, sv, t[p], J, staged).sum(0).ravel()                      # (j, m) order
        i = int(sc.argmax())
        score[p], jm[p] = sc[i], (i // M - J, i % M)
        sc[i] = -np.inf
        margin[p] = score[p] - sc.max() if sc.size > 1 else np.inf
    best = int(score.argmax())
    others = np.delete(score, best)
    point_margin = float(score[best] - others.max()) if others.size else np.inf
    b0 = bins_of(sv)
    bj = b0[:, None] + np.arange(-J, J + 1)[None, :]
    ok = (bj >= 0) & (bj < surface.shape[1])
    row_max = max([float(surface[s["row"], bj[k][ok[k]]].max()) for k, s in enumerate(sv) if ok[k].any()] + [0.0])
    j, m = int(jm[best, 0]), int(jm[best, 1])
    terms = point_terms(surface, sv, t[best], J)[:, j + J, m]
    return dict(map_score=score, map_jm=jm, map_margin=margin, point=best, j=j, m=m, score=float(score[best]),
                margin=min(float(margin[best]), point_margin), point_margin=point_margin, bins_out_of_range=int((~ok).sum()),
                row_max=row_max, tau=t, code_idx=np.mod(np.round(t[best] + m).astype(np.int64), M), dopp_idx=b0 + j, peak=terms)


def sv_results(res, fs, bin_start, bin_step, ds=1.0):
    """rc, fc, fi of the per-SV index pairs, as dpe_acq_results forms them (correlator.py:90-92)."""
    rc = L_CA - (res["code_idx"] / fs) * F_CA
    fi = bin_start + bin_step * res["dopp_idx"]
    return rc, F_CA + (ds * F_CA / F_L1) * fi, fi
