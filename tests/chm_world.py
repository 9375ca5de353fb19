"""Channel-manager worlds off the shipped handoff, and the port-by-port comparison the channel-manager tests share.

The builder generalises the fixed point of workload.extend_handoff -- transmit time <-> satellite state <-> pseudorange, through
the host ChanMgr -- to any ephemeris row, receiver state and receive time: make_channel() gives a self-consistent channel
(rc, cp, cp_ref, TOW, fc, fi), place() collects K of them above an elevation mask, world(name) the handoff-shaped dicts that
ChanMgr.from_handoff / ChanMgrDev.from_handoff take as they are.  What each world is for: WORLDS below and DESIGN.md 2.6a.
Everything is seeded and small; the worlds are built once per process."""
import functools

import numpy as np

import navlab_dpe_sdr_amd as dpe

C_LIGHT = 299792458.0
FCA = 1.023e6
OMEGA_E = 7.2921151467e-5
WGS_A, WGS_B = 6378137.0, 6356752.314245
MU = 3.9860050e14
MAX_CHAN = 37      # DPE_MAX_CHAN (include/dpe_hip.h)
I_E, I_OMG0, I_M0, I_DELN, I_TOE, I_TOC = 1, 3, 5, 6, 15, 16
TG9 = np.linspace(-12.0, 12.0, 9)
TG_WIDE = np.array([-100e3, -60e3, -3000.0, -2000.0, 5.0, 2500.0, 50e3, 100e3])   # even; mid entry (index 4) is not 0
TG_LONG = np.array([-2.0, -1.0, 0.0, 1.0, 2.0]) * 6.0
ECC_LIST = (0.0, 0.02, 0.3, 0.0, 0.3, 0.02, 0.3, 0.02)
SITES = {"sydney": (-33.0, 151.0), "arctic": (78.0, -170.0), "equator180": (0.0, 180.0 - 1e-9), "pole": (90.0, 0.0)}
WORLDS = ("week_lo", "week_hi", "ecc", "site_sydney", "site_arctic", "site_equator180", "site_pole", "wide_tg", "full", "kepler_fail",
          "long_1ms", "long_5ms")


def base_handoff():
    return dpe.handoff.read_handoff(dpe.workload.HANDOFF_CSV)


def llh2ecef(lat_deg, lon_deg, h=100.0):
    """Geodetic -> ECEF on the channel manager's ellipsoid; the pole and the equator exactly (x = y = 0, z = 0)."""
    if lat_deg == 90.0:
        return np.array([0.0, 0.0, WGS_B + h])
    lat, lon = np.radians(lat_deg), np.radians(lon_deg)
    e2 = 1.0 - (WGS_B / WGS_A) ** 2
    N = WGS_A / np.sqrt(1.0 - e2 * np.sin(lat) ** 2)
    z = 0.0 if lat_deg == 0.0 else (N * (1.0 - e2) + h) * np.sin(lat)
    return np.array([(N + h) * np.cos(lat) * np.cos(lon), (N + h) * np.cos(lat) * np.sin(lon), z])


def half_week(t):
    return t - 604800.0 if t > 302400.0 else (t + 604800.0 if t < -302400.0 else t)


def make_channel(eph, X, rx_time, T=0.02, elev_min_deg=5.0):
    """The fixed point for one ephemeris row: -> dict(rc, cp, cp_ref, TOW, fc, fi, elev, tx), or None below the mask
    (elev_min_deg None: no visibility asked for)."""
    X = np.asarray(X, dtype=np.float64)
    tow = int(np.floor(rx_time)) - 2
    cp, rc, cpr, fc, fi = 1000, 0.0, 1000, FCA, 0.0
    elev = tx = None
    for it in range(4):
        cm = dpe.engine.ChanMgr([1], [rc], [0.0], [fc], [fi], [cp], [cpr], [tow], eph[None, :], rx_time, T)
        cm.Start(X, X, (0.0,))
        cm.Update(X, X, (0.0,))
        s, e, w, _ = cm.outputs(with_batch=True)
        cm.Stop()
        sat = e["satState"][0]
        R = w["enu2ecef"][0].reshape(3, 3)
        los = sat[:3] - X[:3]
        rng = np.linalg.norm(los)
        elev = np.degrees(np.arcsin((R.T @ (los / rng))[2]))
        if elev_min_deg is not None and elev < elev_min_deg:
            return None
        tx = rx_time - (rng - C_LIGHT * sat[3] + X[3]) / C_LIGHT
        whole = np.floor((tx - tow) * 1000.0)
        cpr = int(cp - whole)
        rc = float((tx - tow - whole * 1e-3) * FCA)
        fc, fi = float(s["codeFrequency"][0]), float(s["carrierFrequency"][0])
    if not (0.0 <= rc < 1023.0):
        return None
    return dict(rc=rc, cp=cp, cp_ref=cpr, TOW=tow, fc=fc, fi=fi, elev=float(elev), tx=float(tx), eph=eph.copy())


def place(X, rx_time, K, tweak=None, T=0.02, elev_min_deg=5.0):
    """K visible channels at receiver state X and receive time rx_time: clones of the handoff's ephemeris rows with OMEGA_0 / M_0
    shifted trial by trial (extend_handoff's scheme), `tweak(eph, j)` applied to the row that would become channel j."""
    ho = base_handoff()
    K0 = len(ho["prn_list"])
    chans = []
    for trial in range(1, 6000):
        if len(chans) == K:
            break
        eph = ho["eph"][trial % K0].copy()
        eph[I_OMG0] += 0.9 * trial
        eph[I_M0] += 1.7 * trial
        if tweak is not None:
            tweak(eph, len(chans))
        ch = make_channel(eph, X, rx_time, T, elev_min_deg)
        if ch is not None:
            ch["ri"] = 0.25 * trial % 1.0
            chans.append(ch)
    if len(chans) != K:
        raise RuntimeError("could not place %d SVs above the mask" % K)
    return handoff_dict(chans, X, rx_time)


def handoff_dict(chans, X, rx_time, prns=None):
    K = len(chans)
    return dict(rxTime=float(rx_time), rxTime_a=float(rx_time), X_ECEF=np.asarray(X, dtype=np.float64).copy(), bytes_read=0,
                prn_list=np.array(prns if prns is not None else range(1, K + 1), dtype=np.int32),
                rc=np.array([c["rc"] for c in chans]), ri=np.array([c["ri"] for c in chans]),
                fc=np.array([c["fc"] for c in chans]), fi=np.array([c["fi"] for c in chans]),
                cp=np.array([c["cp"] for c in chans], dtype=np.int32), cp_timestamp=np.array([c["cp_ref"] for c in chans], dtype=np.int32),
                TOW=np.array([c["TOW"] for c in chans], dtype=np.int32), eph=np.array([c["eph"] for c in chans]),
                tx=np.array([c.get("tx", np.nan) for c in chans]), elev=np.array([c.get("elev", np.nan) for c in chans]))


def subset(ho, sel):
    out = dict(ho)
    for key in ("prn_list", "rc", "ri", "fc", "fi", "cp", "cp_timestamp", "TOW", "eph", "tx", "elev"):
        if key in ho:
            out[key] = np.asarray(ho[key])[list(sel)]
    return out


def kepler_last_step(M, e):
    """The channel manager's Kepler iteration (E = M, 10 Newton steps, stop at |dE| <= 1e-12) in Python: -> the last |dE|
    (<= 1e-12: converged)."""
    import math
    E, dE = M, 1.0
    for it in range(10):
        if abs(dE) <= 1e-12:
            break
        dE = (M - E + e * math.sin(E)) / (1.0 - e * math.cos(E))
        E = math.fmod(E + dE, 6.2831853071796)
    return abs(dE)


def failing_mean_anomaly(oracle, eph, tx, drift=3e-5):
    """e = 0.99 on `eph`: a mean anomaly at transmit time tx for which the oracle's Kepler iteration misses its 10-iteration cap.
    The failing set is ragged at every scale (Newton's iteration from E = M wanders), so a failing neighbourhood proves little.
    What makes the choice safe against the device's sincos last bits is the MARGIN: the tenth step's |dE| is of order 1 where the cap
    asks for 1e-12, and a perturbation of M by 1e-7 rad moves it by a few per cent (amplification ~1e7: a last-bit difference,
    1e-16, moves it by ~1e-9; a margin of 1e-5 is asked for).  Among the points whose neighbours at +-0.04 rad fail too, the one is taken whose smallest
    last step over M - 2e-6 .. M + drift on a 1e-7 rad raster (the mean anomaly moves n x 6 T = 2e-5 rad over a test's windows) is
    largest.  -> (M, M_0, that smallest last step)."""
    eph = eph.copy()
    eph[I_E] = 0.99
    n = np.sqrt(MU / eph[0] ** 6) + eph[I_DELN]
    tk = half_week(tx - eph[I_TOE])

    def fails(m):
        eph[I_M0] = m - n * tk
        return oracle.sat_pos(eph, tx)[1] != 0
    coarse = []
    for m in np.arange(-0.6, 0.6, 0.0001):        # (outside +-0.5 rad nothing fails at e = 0.99)
        mg = min(kepler_last_step(m + d, 0.99) for d in (0.0, -1e-6, 1e-6, 1e-5, 2e-5, 3e-5))
        if mg > 1e-5:
            coarse.append((mg, float(m)))
    coarse.sort(reverse=True)
    best = None
    for _, m in coarse:
        if not (fails(m) and fails(m - 0.04) and fails(m + 0.04)):
            continue
        mg = min(kepler_last_step(m + d, 0.99) for d in np.arange(-2e-6, drift, 1e-7))
        if best is None or mg > best[1]:
            best = (m, mg)
    if best is None or best[1] < 1e-5:
        raise RuntimeError("no robustly failing mean anomaly")
    return best[0], best[0] - n * tk, best[1]


@functools.lru_cache(maxsize=None)
def world(name):
    """-> dict(ho=handoff-shaped dict, T, tg=time grid, plus what the world's branch claim needs).  Do not modify the result."""
    ho = base_handoff()
    X = ho["X_ECEF"].copy()
    if name in ("week_lo", "week_hi"):
        toe, rx = (600000.0, 3000.4) if name == "week_lo" else (7200.0, 601000.4)

        def tweak(eph, j):
            eph[I_TOE] = eph[I_TOC] = toe
        return dict(ho=place(X, rx, 8, tweak), T=0.02, tg=TG9)
    if name == "ecc":
        def tweak(eph, j):
            eph[I_E] = ECC_LIST[j]
        return dict(ho=place(X, ho["rxTime"], 8, tweak), T=0.02, tg=TG9, ecc=np.array(ECC_LIST))
    if name.startswith("site_"):
        lat, lon = SITES[name[5:]]
        Xs = X.copy()
        Xs[:3] = llh2ecef(lat, lon)
        return dict(ho=place(Xs, ho["rxTime"], 8), T=0.02, tg=TG9, latlon=(lat, lon))
    if name == "wide_tg":
        return dict(ho=ho, T=0.02, tg=TG_WIDE)
    if name == "full":
        return dict(ho=dpe.workload.extend_handoff(ho, MAX_CHAN), T=0.02, tg=TG9)
    if name == "kepler_fail":
        from oracle import oracle
        oracle.lib()
        good = subset(ho, [1, 2, 3, 4])
        bad = subset(ho, [0])
        tx = float(bad["TOW"][0] + (bad["cp"][0] - bad["cp_timestamp"][0]) * 1e-3 + bad["rc"][0] / FCA)
        m, m0, margin = failing_mean_anomaly(oracle, bad["eph"][0], tx)
        bad["eph"] = bad["eph"].copy()
        bad["eph"][0, I_E] = 0.99
        bad["eph"][0, I_M0] = m0
        five = dict(good)
        for key in ("prn_list", "rc", "ri", "fc", "fi", "cp", "cp_timestamp", "TOW", "eph"):
            five[key] = np.concatenate([good[key][:2], bad[key], good[key][2:]])
        return dict(ho=five, good=good, T=0.02, tg=TG9, bad_chan=2, bad_tx=tx, bad_M=m, bad_margin=margin)
    if name in ("long_1ms", "long_5ms"):
        T, n, seed = (0.001, 200, 3) if name == "long_1ms" else (0.005, 150, 2)
        return dict(ho=ho, T=T, tg=TG_LONG, n=n, seed=seed)
    raise KeyError(name)


def moving_fixes(X, n, seed=5):
    """The fixes of test_device_channel_manager_matches_the_host_form: tens of metres and m/s per window, clock terms included.
    -> list of (x_k|k, x_k+1|k)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = np.array(X, dtype=np.float64).copy()
    out = []
    for it in range(n):
        x1 = x + np.concatenate([rng.uniform(-30, 30, 3), rng.uniform(-40, 40, 1), rng.uniform(-3, 3, 3), rng.uniform(-1, 1, 1)])
        xk = x1 + np.concatenate([rng.uniform(-2, 2, 4), rng.uniform(-0.2, 0.2, 4)])
        out.append((x1, xk))
        x = x1
    return out


def long_run_fixes(X, T, n, seed):
    """The recipe of test_chanmgr_long_runs_random_subsets: a receiver that accelerates and whose fix is noisy.
    -> list of (fix fed back, grid centre); entry 0 is for Start."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = np.array(X, dtype=np.float64).copy()
    v = rng.uniform(-30.0, 30.0, 3)
    out = []
    for it in range(n):
        x[:3] += v * T
        v += rng.uniform(-2.0, 2.0, 3) * T
        x[4:7] = v
        xk = x + np.concatenate([rng.normal(0, 2.0, 4), rng.normal(0, 0.1, 4)])
        out.append((xk, xk + np.concatenate([rng.normal(0, 1.0, 4), np.zeros(4)])))
    return out


def compare(dev, host, dev_chans=None, scale=None):
    """Every port of the device form (ChanMgrDev.outputs(with_batch=True)) against the host form's (ChanMgr.outputs(with_batch=True)).
    Bounds: 1e-4 chips (the raster argument of tests/test_gpu_chm_dev.py), 1e-9 on phase and fi, 1e-12 relative on fc, positions
    and velocities, 1e-14 on the ENU matrix, exact integers, state port and rxTime.
    dev_chans: the device channels that correspond to the host's (default: all, in order).
    scale: per compared channel, a factor on the satellite-state and fc bounds (1 / (1 - e) for an eccentric orbit: the conditioning
    of Kepler's equation, dE = dM / (1 - e cos E)); default 1.  -> worst deviation per port, in units of its bound where it has one."""
    sd, ed, wd, bd = dev
    sh, eh, wh, bh = host
    if dev_chans is not None:
        idx = list(dev_chans)
        sd, ed, bd = sd[idx], ed[idx], bd[idx]
    sc = np.ones(len(sh)) if scale is None else np.asarray(scale, dtype=np.float64)
    for f in ("cpElapsedStart", "cpReference", "prn"):
        assert np.array_equal(sd[f], sh[f]), f
    for f in ("cpRefTOW", "cpElapsedEnd", "cpRef"):
        assert np.array_equal(ed[f], eh[f]), f
    worst = {}
    for name, a, b, tol, rel in (("rcStart", sd["codePhaseStart"], sh["codePhaseStart"], 1e-4, False),
                                 ("rcEnd", ed["codePhaseEnd"], eh["codePhaseEnd"], 1e-4, False),
                                 ("riStart", sd["carrierPhaseStart"], sh["carrierPhaseStart"], 1e-9, False),
                                 ("fc", sd["codeFrequency"], sh["codeFrequency"], 1e-12, True),
                                 ("fi", sd["carrierFrequency"], sh["carrierFrequency"], 1e-9, False),
                                 ("R", wd["enu2ecef"], wh["enu2ecef"], 1e-14, False),
                                 ("x", wd["xCurrkk1"], wh["xCurrkk1"], 0.0, False)):
        d = np.abs(np.asarray(a) - np.asarray(b))
        err = (d / sc).max() if name == "fc" else d.max()
        if rel:
            err /= np.abs(np.asarray(b)).max()
        worst[name] = err / tol if tol else err
        assert err <= tol, (name, err)
    assert wd["rxTime"][0] == wh["rxTime"][0] and wd["dopplerSign"][0] == wh["dopplerSign"][0]
    # batch satellite states: positions relative to the orbit radius, velocities to the speed, clock terms absolutely
    s3 = sc[:, None, None]
    pos = (np.abs(bd[..., :3] - bh[..., :3]) / s3).max() / 2.6e7
    vel = (np.abs(bd[..., 4:7] - bh[..., 4:7]) / s3).max() / 3.0e3
    clk = max((np.abs(bd[..., 3] - bh[..., 3]) / sc[:, None]).max(), (np.abs(bd[..., 7] - bh[..., 7]) / sc[:, None]).max())
    assert pos < 1e-12 and vel < 1e-12 and clk < 1e-17, (pos, vel, clk)
    assert np.array_equal(ed["satState"], bd[:, bd.shape[1] // 2])
    worst.update(satPos=pos / 1e-12, satVel=vel / 1e-12, satClk=clk / 1e-17)
    return worst


def merge_worst(acc, w):
    for k, v in w.items():
        acc[k] = max(acc.get(k, 0.0), float(v))
    return acc


# ---------------------------------------------------------------------------------------------------------------------------------
# P_k|k-1 matrices that take the filter's LU inverse (dpe_ekf.hip::invert, dpe_ekf_dev.h::ekf_lu_column) off the diagonal-pivot
# path.  The filter forms S = P + I (H = I, R = I) -- exactly, for the entries used here.

def lu_pivots(Smat):
    """numpy copy of the host form's pivot rule (first largest |.| at or below the diagonal, `>`): -> (rows chosen per column,
    pivot values, the column at which the matrix is singular or None, the candidates of every column before its swap)."""
    lu = np.array(Smat, dtype=np.float64).copy()
    rows, vals, cands = [], [], []
    for c in range(8):
        p = c
        for r in range(c + 1, 8):
            if abs(lu[r, c]) > abs(lu[p, c]):
                p = r
        cands.append(lu[c:, c].copy())
        if lu[p, c] == 0.0:
            return rows, vals, c, cands
        rows.append(p)
        vals.append(lu[p, c])
        if p != c:
            lu[[p, c]] = lu[[c, p]]
        for r in range(c + 1, 8):
            lu[r, c] = lu[r, c] / lu[c, c]
            lu[r, c + 1:] = lu[r, c + 1:] - lu[r, c] * lu[c, c + 1:]
    return rows, vals, None, cands


def _sym(rng, scale):
    a = rng.uniform(-scale, scale, (8, 8))
    return (a + a.T) / 2.0


def swaps_wanted(rows):
    sw = [c for c, p in enumerate(rows) if p != c]
    return (len(sw) >= 4 and 0 in sw and 6 in sw and any(rows[c] == 7 for c in sw if c < 6)
            and any(rows[c] == c + 1 for c in sw if c < 6))


@functools.lru_cache(maxsize=None)
def filter_case(name):
    """-> P_k|k-1 [8, 8] for the case (the claims are asserted by tests/test_chm_world_cpu.py)."""
    if name == "fresh":             # an ordinary SPD covariance, for the window after a singular one
        rng = np.random.Generator(np.random.PCG64(99))
        b = rng.uniform(-1.0, 1.0, (8, 8))
        return b @ b.T + 2.0 * np.eye(8)
    if name == "swaps":             # SPD, small leading diagonals and large couplings: D^1/2 C D^1/2 with a steep D
        for seed in range(1, 5000):
            rng = np.random.Generator(np.random.PCG64(seed))
            b = rng.uniform(-1.0, 1.0, (8, 3))
            Cm = b @ b.T + 0.05 * np.eye(8)
            dinv = 1.0 / np.sqrt(np.diag(Cm))
            Cm = Cm * dinv[:, None] * dinv[None, :]                      # a correlation matrix with large couplings
            d = np.sqrt(0.02 * 4.0 ** rng.permutation(8))
            P = Cm * d[:, None] * d[None, :]
            P = (P + P.T) / 2.0
            rows, vals, sing, _ = lu_pivots(P + np.eye(8))
            if sing is None and swaps_wanted(rows) and np.linalg.eigvalsh(P).min() > 0.0:
                return P
        raise RuntimeError("no seed gives the swap pattern")
    if name == "tie":               # column 0: +3 in row 2, -3 in row 5, nothing larger: the FIRST is the pivot row
        rng = np.random.Generator(np.random.PCG64(7))
        P = _sym(rng, 0.3) + 1.5 * np.eye(8)
        P[0, 0] = 0.5
        P[2, 0] = P[0, 2] = 3.0
        P[5, 0] = P[0, 5] = -3.0
        return P
    if name == "negative":          # symmetric, indefinite: negative pivots, one of them chosen over a smaller positive candidate
        for seed in range(1, 5000):
            rng = np.random.Generator(np.random.PCG64(seed))
            P = _sym(rng, 2.0) - 3.0 * np.eye(8)
            rows, vals, sing, cands = lu_pivots(P + np.eye(8))
            if sing is not None or np.linalg.cond(P + np.eye(8)) > 200.0:
                continue
            neg_swap = [c for c in range(7) if rows[c] != c and vals[c] < 0.0 and (cands[c] > 0.0).any()]
            if sum(v < 0.0 for v in vals) >= 3 and sum(v > 0.0 for v in vals) >= 1 and neg_swap:
                return P
        raise RuntimeError("no seed gives negative pivots")
    if name == "singular0":         # S's column 0 is zero: P[:, 0] = -e_0
        rng = np.random.Generator(np.random.PCG64(21))
        P = _sym(rng, 0.5) + 2.0 * np.eye(8)
        P[:, 0] = 0.0
        P[0, 0] = -1.0
        return P
    if name == "singular5":         # block diagonal: five clean eliminations, then a 3 x 3 block whose first column is zero
        rng = np.random.Generator(np.random.PCG64(22))
        P = np.zeros((8, 8))
        P[:5, :5] = _sym(rng, 0.5)[:5, :5] + 2.0 * np.eye(5)
        P[5:, 5:] = rng.uniform(0.5, 1.5, (3, 3))
        P[5:, 5] = 0.0
        P[5, 5] = -1.0
        return P
    raise KeyError(name)


FILTER_CASES = ("swaps", "tie", "negative", "singular0", "singular5")
EKF_KEYS = ("xk1k1", "xkk1", "Pk1k1", "Pkk1", "K", "Q")
