"""fp64 numpy restatement of the vector-tracking loop of DESIGN.md 7e (test infrastructure, no GPU): correlations as direct sums in
the manner of tests/trk_ref.py, then per epoch the discriminators, the lock gate, W, the Kalman update through the Cholesky factor
of S, the predict step and the steering.  The satellite routine is the oracle's (the reference's CHM_Get_Sat_Pos), which the world
of tests/vt_world.py is built with too.  `ls_fix` is the twin's single-epoch least squares (naveng.py:132-224) on the same
measurements -- the yardstick a filtered loop has to beat."""
import math

import numpy as np

import navlab_dpe_sdr_amd as dpe
from tests import trk_ref

C, F_CA, F_L1, OE, T_CA, L_CA = 299792458.0, 1.023e6, 1.57542e9, 7.2921151467e-5, 0.001, 1023.0
BAD_WINDOW, NO_UPDATE, PIVOT = 1, 2, 4
CHAN_NAMES = ("rc", "ri", "fc", "fi", "cp", "eR", "eV", "wR", "wV", "lock", "dpc", "dfi")
Q_DEFAULT = np.array([0.0, 0.0, 0.0, 0.0, 6.0, 6.0, 6.0, (2.5e-10 * C) * (2.5e-10 * C)])


class Config:
    def __init__(self, fs, prns, T=1e-3, N=20, ds=1.0, num_prev=20, init_var=(225.0, 1.0), min_var=(1.0, 0.01), q=None, lock_thr=4.0):
        self.fs, self.T, self.N, self.ds, self.num_prev = float(fs), float(T), int(N), float(ds), int(num_prev)
        self.prns = [int(p) for p in prns]
        self.K = len(self.prns)
        self.S = int(round(self.T * self.fs))
        self.NT = float(self.N) * self.T
        self.fcaid = self.ds * F_CA / F_L1
        self.init_var, self.min_var = tuple(init_var), tuple(min_var)
        self.q = Q_DEFAULT.copy() if q is None else np.asarray(q, dtype=np.float64)
        self.lock_thr = float(lock_thr)
        self.round_ms = abs(self.NT * 1000.0 - round(self.NT * 1000.0)) < 1e-9


def new_state(cfg, X, Sigma, rx_time0, chan):
    chan = np.asarray(chan, dtype=np.float64)
    return dict(X=np.array(X, dtype=np.float64), Sigma=np.array(Sigma, dtype=np.float64).reshape(8, 8), rxTime0=float(rx_time0), rxBase=float(rx_time0),
                epochs=0, status=0, rc=chan[:, 0].copy(), ri=chan[:, 1].copy(), fc=chan[:, 2].copy(), fi=chan[:, 3].copy(), cp=chan[:, 4].copy(),
                sat=None, histR=np.zeros((cfg.K, cfg.num_prev)), histV=np.zeros((cfg.K, cfg.num_prev)), histN=np.zeros(cfg.K, dtype=np.int64),
                histPos=np.zeros(cfg.K, dtype=np.int64))


def state_from_rec(cfg, rec):
    """dpe_vt_state_rec (engine.VtStateRec) -> the state dict of new_state: the inverse of tests/test_vt_host_cpu.host_state, with the
    record's status kept."""
    K, P = cfg.K, cfg.num_prev
    ch = [rec.chan[k] for k in range(K)]
    st = dict(X=np.array(rec.X, dtype=np.float64), Sigma=np.array(rec.Sigma, dtype=np.float64).reshape(8, 8), rxTime0=float(rec.rxTime0),
              rxBase=float(rec.rxBase), epochs=int(rec.epochs), status=int(rec.status))
    for n in ("rc", "ri", "fc", "fi", "cp"):
        st[n] = np.array([getattr(c, n) for c in ch], dtype=np.float64)
    st["sat"] = np.array([list(c.sat) for c in ch], dtype=np.float64) if rec.satValid else None
    st["histR"] = np.array([list(c.histRange)[:P] for c in ch], dtype=np.float64)
    st["histV"] = np.array([list(c.histRate)[:P] for c in ch], dtype=np.float64)
    st["histN"] = np.array([c.histN for c in ch], dtype=np.int64)
    st["histPos"] = np.array([c.histPos for c in ch], dtype=np.int64)
    return st


class Nudge:
    """A model of another maths library and another Kepler solver, for measuring what such a difference does to an epoch's results:
    every atan2 / sin / cos result handed to it moves by up to `ulps` units in the last place, in a seeded random direction; sat()
    moves a satellite state by up to `sat_rel` of the orbit radius (2.6e7 m) and speed (3e3 m/s) and by sat_clk on the clock terms
    -- the bounds tests/test_gpu_chm_dev.py holds sat_state to on the device."""

    def __init__(self, seed, ulps=2, sat_rel=1e-12, sat_clk=1e-17):
        self.rng, self.ulps, self.sat_rel, self.sat_clk = np.random.default_rng(seed), int(ulps), float(sat_rel), float(sat_clk)

    def __call__(self, v):
        return float(v + float(self.rng.integers(-self.ulps, self.ulps + 1)) * np.spacing(abs(v)))

    def sat(self, s):
        u = self.rng.uniform(-1.0, 1.0, 8)
        scale = np.array([2.6e7 * self.sat_rel] * 3 + [self.sat_clk] + [3.0e3 * self.sat_rel] * 3 + [self.sat_clk])
        return np.asarray(s, dtype=np.float64) + u * scale


def window_params(st, k, j, T):
    return (np.mod(st["rc"][k] + j * st["fc"][k] * T, L_CA), np.mod(st["ri"][k] + j * st["fi"][k] * T, 1.0), st["fc"][k], st["fi"][k])


def correlate_epoch(iq, first_sample, cfg, st, chips=None, round_epl=None):
    """-> sums [N, K, 8] = iE qE iP qP iL qL case periods of the epoch that starts at complex sample `first_sample`."""
    chips = chips or [dpe.synth.ca_code(p).astype(np.float64) for p in cfg.prns]
    out = np.zeros((cfg.N, cfg.K, 8))
    for j in range(cfg.N):
        a = 2 * (first_sample + j * cfg.S)
        wv = iq[a:a + 2 * cfg.S]
        x = wv[0::2] + 1j * wv[1::2]
        for k in range(cfg.K):
            rc, ri, fc, fi = window_params(st, k, j, cfg.T)
            if not (fi == fi and ri == ri):            # vt_correlate_kernel's own test: such a window is case -1, its sums stay 0
                out[j, k, 6] = -1.0
                continue
            e, p, l, compl_, _, _, case, _ = trk_ref.correlate(x, chips[k], cfg.fs, rc, ri, fc, fi, 0j)
            if case < 0:
                out[j, k, 6] = -1.0
                continue
            v = np.array([e.real, e.imag, p.real, p.imag, l.real, l.imag])
            if round_epl is not None:
                v = v.astype(round_epl).astype(np.float64)
            out[j, k, :6], out[j, k, 6], out[j, k, 7] = v, case, compl_
    return out


def transmit(tow, cps, cp, rc, rx_time):
    ci, cf = (cp - cps) * T_CA, rc / F_CA
    return tow + ci + cf, ((rx_time - tow) - ci) - cf


def geometry(sat, d, X, ds, nudge=None):
    """-> los [3], Doppler / ds and predicted minus NCO code phase (chips) for the state X; sat at the NCO's transmit time.
    nudge: a Nudge that moves the cos and sin results (None: as computed)."""
    tau = d - (X[3] / C) + sat[3]
    a = -OE * tau
    ct, s_ = math.cos(a), math.sin(a)
    if nudge is not None:
        ct, s_ = nudge(ct), nudge(s_)
    p = np.array([ct * sat[0] - s_ * sat[1], s_ * sat[0] + ct * sat[1], sat[2]])
    v = np.array([ct * sat[4] - s_ * sat[5] - OE * s_ * sat[0] - OE * ct * sat[1], s_ * sat[4] + ct * sat[5] + OE * ct * sat[0] - OE * s_ * sat[1], sat[6]])
    lv = p - X[:3]
    rng = math.sqrt(lv[0] * lv[0] + lv[1] * lv[1] + lv[2] * lv[2])
    los = lv / rng
    e = np.array([X[4] - OE * X[1], X[5] + OE * X[0], X[6]])
    lrr = (los[0] * (e[0] - v[0])) + (los[1] * (e[1] - v[1])) + (los[2] * (e[2] - v[2]))
    bc_fi = F_L1 * ((lrr - X[7]) / C + sat[7]) / ds
    pr = rng - C * sat[3] + X[3]
    return los, bc_fi, (d - pr / C) * F_CA, p, pr


def discriminate(cfg, s, nudge=None):
    """s [N, 8] of one channel -> bad, dpc, dfi, lock.  nudge: a Nudge that moves the atan2 result."""
    bad = bool(np.any(~(s[:, 6] >= 0.0)) or not np.all(np.isfinite(s[:, :6])))
    E = L = m1 = m2 = cross = dot = 0.0
    with np.errstate(all="ignore"):
        for j in range(cfg.N):
            iE, qE, iP, qP, iL, qL = s[j, :6]
            E += math.sqrt(iE * iE + qE * qE) if not bad else 0.0
            L += math.sqrt(iL * iL + qL * qL) if not bad else 0.0
            if bad:
                continue
            p = math.sqrt(iP * iP + qP * qP)
            m1 += p
            m2 += p * p
            if j > 0:
                i0, q0 = s[j - 1, 2], s[j - 1, 3]
                cr, dt = i0 * qP - iP * q0, i0 * iP + q0 * qP
                if dt < 0.0:
                    cr, dt = -cr, -dt
                cross += cr
                dot += dt
    if bad:
        return True, 0.0, 0.0, 0.0
    dpc = (E - L) / (2.0 * (E + L)) if E + L != 0.0 else 0.0
    at = math.atan2(cross, dot)
    if nudge is not None:
        at = nudge(at)
    dfi = at / (2.0 * math.pi * cfg.T)
    m1, m2 = m1 / cfg.N, m2 / cfg.N
    var = m2 - m1 * m1
    lock = m1 / math.sqrt(var) if var > 0.0 else (1.0e30 if m1 > 0.0 else 0.0)
    return False, dpc, dfi, lock


def variance(h, n):
    s = 0.0
    for i in range(n):
        s += h[i]
    m = s / n
    v = 0.0
    for i in range(n):
        a = h[i] - m
        v += a * a
    return v / n


def filter_step(cfg, oracle, eph, tow, cps, st, sums, order=None, nudge=None):
    """One epoch's steps b - f on `st` (in place).  order: the sequence the included channels' rows are taken in (None: channel
    order) -- the result's spread over such orders is the restatement's own rounding noise.  nudge: a Nudge applied to every atan2,
    sin and cos result and, in the epoch that computes them (st["sat"] None), to the satellite states of the epoch's start -- the
    spread over such nudges is what another maths library may change.  Returns the epoch's record (dict)."""
    K, N = cfg.K, cfg.N
    X, P = st["X"], st["Sigma"]
    rec = {n: np.zeros(K) for n in CHAN_NAMES}
    bad, incl, los = np.zeros(K, dtype=bool), np.zeros(K, dtype=bool), np.zeros((K, 3))
    if st["sat"] is None:
        st["sat"] = np.zeros((K, 8))
        for k in range(K):
            tt, _ = transmit(tow[k], cps[k], st["cp"][k], st["rc"][k], st["rxTime0"])
            st["sat"][k], _ = oracle.sat_pos(eph[k], tt)
            if nudge is not None:
                st["sat"][k] = nudge.sat(st["sat"][k])
    rho = np.zeros(K)
    for k in range(K):
        b, dpc, dfi, lock = discriminate(cfg, sums[:, k, :], nudge)
        wR, wV = cfg.init_var
        if st["histN"][k] >= cfg.num_prev:
            wR = max(variance(st["histR"][k], cfg.num_prev), cfg.min_var[0])
            wV = max(variance(st["histV"][k], cfg.num_prev), cfg.min_var[1])
        _, d = transmit(tow[k], cps[k], st["cp"][k], st["rc"][k], st["rxTime0"])
        with np.errstate(all="ignore"):
            los[k], _, d_chips, _, pr = geometry(st["sat"][k], d, X, cfg.ds, nudge)
        if not np.all(np.isfinite(los[k])):
            b = True
        bad[k] = b
        incl[k] = (not b) and lock > cfg.lock_thr
        rec["dpc"][k], rec["dfi"][k], rec["lock"][k] = dpc, dfi, lock
        rec["eR"][k], rec["eV"][k] = -dpc * (C / F_CA), -dfi * (cfg.ds * C / F_L1)
        rec["wR"][k], rec["wV"][k] = wR, wV
        rho[k] = C * d - dpc / F_CA * C                # measured pseudorange: the NCO's, corrected by the discriminator (for ls_fix)
    status = (BAD_WINDOW if bad.any() else 0) | (NO_UPDATE if incl.sum() < 4 else 0)
    sel = [k for k in range(K) if incl[k]] if order is None else [k for k in order if incl[k]]
    nI = len(sel)
    if nI >= 4:
        n = 2 * nI
        H = np.zeros((n, 8))
        e, w = np.zeros(n), np.zeros(n)
        for r, k in enumerate(sel):
            H[r, 0:3], H[r, 3] = -los[k], 1.0
            H[nI + r, 4:7], H[nI + r, 7] = -los[k], 1.0
            e[r], e[nI + r] = rec["eR"][k], rec["eV"][k]
            w[r], w[nI + r] = rec["wR"][k], rec["wV"][k]
        A = H @ P
        S = A @ H.T + np.diag(w)
        Lm = np.zeros((n, n))
        fail = False
        for c in range(n):
            col = S[c:, c] - Lm[c:, :c] @ Lm[c, :c]
            if not (col[0] > 0.0) or not np.isfinite(col[0]):
                fail = True
                break
            Lm[c:, c] = col / math.sqrt(col[0])
            Lm[c, c] = math.sqrt(col[0])
        if fail:
            status |= PIVOT
        else:
            Y = np.linalg.solve(Lm, A)
            y = np.linalg.solve(Lm, e)
            X = X + Y.T @ y
            P = P - Y.T @ Y
    # predict
    dt = cfg.NT
    F = np.eye(8)
    for i in range(4):
        F[i, i + 4] = dt
    P = 0.5 * (P + P.T)
    P = F @ P @ F.T + np.diag(cfg.q)
    X = F @ X
    epochs = st["epochs"] + 1
    rxN = st["rxBase"] + float(epochs) * cfg.NT
    if cfg.round_ms:
        r = math.floor(rxN * 1000.0 + 0.5) / 1000.0
        if abs(r - rxN) < 1.0e-7:
            rxN = r
    # steer
    for k in range(K):
        adv, turn = st["rc"][k] + N * st["fc"][k] * cfg.T, st["ri"][k] + N * st["fi"][k] * cfg.T
        rcN, cpN, riN = np.mod(adv, L_CA), st["cp"][k] + math.floor(adv / L_CA), np.mod(turn, 1.0)
        tt, d = transmit(tow[k], cps[k], cpN, rcN, rxN)
        sat, rc_ = oracle.sat_pos(eph[k], tt)
        fiN, fcN = st["fi"][k], st["fc"][k]
        if rc_ == 0:
            with np.errstate(all="ignore"):
                _, bc_fi, d_chips, _, _ = geometry(sat, d, X, cfg.ds, nudge)
            fcB = F_CA + cfg.fcaid * bc_fi + d_chips / cfg.NT
            if np.isfinite(bc_fi) and np.isfinite(fcB):
                fiN, fcN = bc_fi, fcB
        if incl[k]:
            p = st["histPos"][k]
            st["histR"][k, p], st["histV"][k, p] = rec["eR"][k], rec["eV"][k]
            st["histPos"][k] = 0 if p + 1 >= cfg.num_prev else p + 1
            st["histN"][k] = min(st["histN"][k] + 1, cfg.num_prev)
        st["rc"][k], st["ri"][k], st["fc"][k], st["fi"][k], st["cp"][k] = rcN, riN, fcN, fiN, cpN
        st["sat"][k] = sat
        for nme, v in zip(CHAN_NAMES[:5], (rcN, riN, fcN, fiN, cpN)):
            rec[nme][k] = v
    st["X"], st["Sigma"], st["rxTime0"], st["epochs"] = X, P, rxN, epochs
    st["status"] |= status
    rec.update(X=X.copy(), diag=np.diag(P).copy(), rxTime0=rxN, mask=int(sum(1 << k for k in range(K) if incl[k])), status=status, n_incl=int(incl.sum()),
               rho=rho, los=los, incl=incl.copy())
    return rec


def ls_fix(rec, st_before, cfg, oracle, eph, tow, cps, X0):
    """The twin's perform_least_sqrs on one epoch's measured pseudoranges (included channels): Gauss-Newton from X0, <= 10 steps.
    The satellites stand at the NCOs' transmit times of the epoch's start; the small difference to the measured transmit time
    (< 1e-6 s x 800 m/s) is below a millimetre."""
    sel = np.flatnonzero(rec["incl"])
    x = np.array(X0[:4], dtype=np.float64)
    sats = []
    for k in sel:
        _, d = transmit(tow[k], cps[k], st_before["cp"][k], st_before["rc"][k], st_before["rxTime0"])
        sats.append((st_before["sat"][k], d))
    for _ in range(10):
        H, r = np.zeros((sel.size, 4)), np.zeros(sel.size)
        for i, (k, (sat, d)) in enumerate(zip(sel, sats)):
            Xs = np.concatenate([x, np.zeros(4)])
            los, _, _, _, pr = geometry(sat, d, Xs, cfg.ds)
            H[i, :3], H[i, 3] = -los, 1.0
            r[i] = rec["rho"][k] - pr
        dx = np.linalg.lstsq(H, r, rcond=None)[0]
        x = x + dx
        if np.linalg.norm(dx) < 1e-7:
            break
    return x


def run(iq, cfg, oracle, start, X0, Sigma0, n_epochs, round_epl=None, with_ls=False, first_sample=0):
    """The closed loop from `start` (vt_world's form) over n_epochs epochs.  Returns dict(recs = the epoch records, sums
    [n_epochs, N, K, 8], params [n_epochs, K, 5] = every epoch's start parameters, ls [n_epochs, 4] when with_ls, state)."""
    eph, tow, cps = start["eph"], start["tow"], start["cps"]
    st = new_state(cfg, X0, Sigma0, start["rxTime0"] + first_sample / cfg.fs, start["chan"])
    chips = [dpe.synth.ca_code(p).astype(np.float64) for p in cfg.prns]
    recs, sums, params, ls = [], [], [], []
    for e in range(n_epochs):
        params.append(np.stack([st["rc"], st["ri"], st["fc"], st["fi"], st["cp"]], axis=1))
        s = correlate_epoch(iq, first_sample + e * cfg.N * cfg.S, cfg, st, chips, round_epl)
        before = dict(cp=st["cp"].copy(), rc=st["rc"].copy(), rxTime0=st["rxTime0"], sat=None)
        x_before = st["X"].copy()
        rec = filter_step(cfg, oracle, eph, tow, cps, st, s)
        if with_ls:
            if before["sat"] is None:
                before["sat"] = np.array([oracle.sat_pos(eph[k], transmit(tow[k], cps[k], before["cp"][k], before["rc"][k], before["rxTime0"])[0])[0]
                                          for k in range(cfg.K)])
            ls.append(ls_fix(rec, before, cfg, oracle, eph, tow, cps, x_before) if rec["n_incl"] >= 4 else np.full(4, np.nan))
        recs.append(rec)
        sums.append(s)
    return dict(recs=recs, sums=np.array(sums), params=np.array(params), ls=np.array(ls), state=st)


def table(recs):
    """{name: array over epochs} of every logged quantity, in the device log's terms."""
    out = dict(X=np.array([r["X"] for r in recs]), diag=np.array([r["diag"] for r in recs]), rxTime0=np.array([r["rxTime0"] for r in recs]),
               mask=np.array([r["mask"] for r in recs]), status=np.array([r["status"] for r in recs]))
    for n in CHAN_NAMES:
        out[n] = np.array([r[n] for r in recs])
    return out
