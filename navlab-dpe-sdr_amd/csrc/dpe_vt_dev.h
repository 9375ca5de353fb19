// dpe_vt_dev.h -- one epoch of the vector-tracking loop behind the correlations: discriminators, lock gate, measurement
// variances, the Kalman update through the Cholesky factor of S, the predict step and the steering of every channel.  One source, two
// forms: vt_filter_kernel (dpe_vt.hip) runs it as one 64-lane block, dpe_vt_filter_step_host as a loop over the same 64 "lanes".
// The function is a sequence of PHASES; inside a phase every lane works on its own elements and reads only what earlier phases left
// in the work area (LDS on the device), between phases stands a barrier.  The host form runs a phase's lanes one after the other, so
// both forms perform the same operations on every element in the same order (contraction off); what differs between them is the
// math library behind sincos / atan2 / sqrt.  Rows of the update are the included channels in channel order -- range rows, then rate
// rows -- so the arithmetic does not depend on which lanes the channels occupy.
#pragma once
#include "../../include/dpe_hip.h"
#include "dpe_sat.h"   // Eph, sat_state, rotate_state, wrap_pos

namespace dpe {

constexpr int kVtLanes = 64, kVtMaxChan = DPE_VT_MAX_CHAN, kVtMaxRows = 2 * DPE_VT_MAX_CHAN;

struct VtEph { Eph eph; double tow, cps; };   // ephemerides and their timestamp (TOW at code period cps)

struct VtCfg {
    double fs, T, ds, NT, fcaid;
    int N, K, numPrev, roundMs;   // roundMs: N T is a whole number of milliseconds (rxTime0 on the ms grid is rounded to it, receiver.py:713)
    double initVarR, initVarV, minVarR, minVarV, q[8], lockThr;
};

struct VtWork {
    double X[8], P[64], Xn[8], Pn[64];
    double A[kVtMaxRows * 8];               // H Sigma, then Y = L^-1 H Sigma
    double S[kVtMaxRows * kVtMaxRows];      // S, its lower triangle becomes L
    double e[kVtMaxRows], w[kVtMaxRows];    // residuals (then L^-1 e) and the diagonal of W, by row
    double los[kVtMaxChan * 3];
    double eR[kVtMaxChan], eV[kVtMaxChan], wR[kVtMaxChan], wV[kVtMaxChan], lock[kVtMaxChan], dpc[kVtMaxChan], dfi[kVtMaxChan];
    double piv;
    int incl[kVtMaxChan], bad[kVtMaxChan], chanOf[kVtMaxChan];   // chanOf[r]: the r-th included channel
    int n, nIncl, status, fail, mask;
};

#ifdef __HIP_DEVICE_COMPILE__
#define VT_LANES(l) { const int l = threadIdx.x; {
#define VT_END }} __syncthreads();
#else
#define VT_LANES(l) { for (int l = 0; l < kVtLanes; ++l) {
#define VT_END }}
#endif

DPE_HD static inline bool vt_finite(double v) { return std::fabs(v) <= 1.7976931348623157e308; }   // false for NaN

// transmit time the NCO state (cp, rc) stands for, and the part of (rxTime - transmit time) that stays well conditioned:
// d = ((rxTime - TOW) - (cp - cps) 1 ms) - rc / F_CA has an ulp of 1e-17 s where the transmit time itself has 6e-11 s
DPE_HD static inline double vt_transmit(const VtEph &p, double cp, double rc, double rxTime, double &d)
{
#pragma clang fp contract(off)
    const double ci = (cp - p.cps) * kTCA, cf = rc / kFCA;
    d = ((rxTime - p.tow) - ci) - cf;
    return p.tow + ci + cf;
}

// The satellite state of `sat` (at the NCO's transmit time) rotated into the ECEF frame of the reception instant rxTime - X[3] / c
// (the twin's t_c = rxTime_a, receiver.py:651), line of sight, and what the state X predicts for the channel: Doppler / ds and the
// code phase minus the NCO's, in chips (receiver.py:690-706).
DPE_HD static inline void vt_geometry(const double sat[8], double d, const double *X, double ds, double los[3], double &bcFi, double &dChips)
{
#pragma clang fp contract(off)
    double sr[8];
    const double tau = d - (X[3] / kC) + sat[3];
    rotate_state(sat, tau, sr);
    const double lx = sr[0] - X[0], ly = sr[1] - X[1], lz = sr[2] - X[2];
    const double range = std::sqrt(lx * lx + ly * ly + lz * lz);
    los[0] = lx / range; los[1] = ly / range; los[2] = lz / range;
    const double ex = X[4] - kOEDot * X[1], ey = X[5] + kOEDot * X[0], ez = X[6];
    const double lrr = (los[0] * (ex - sr[4])) + (los[1] * (ey - sr[5])) + (los[2] * (ez - sr[6]));
    bcFi = kFL1 * ((lrr - X[7]) / kC + sr[7]) / ds;
    const double pr = range - kC * sr[3] + X[3];
    dChips = (d - pr / kC) * kFCA;
}

// receive time of the next epoch's first sample: rxBase + epochs N T in one rounding, on the millisecond grid when it lies there
// (receiver.py:713 rounds to the millisecond; a start that is not on that grid is left as it is)
DPE_HD static inline double vt_next_rx_time(const VtCfg &cfg, const dpe_vt_state_rec *st)
{
#pragma clang fp contract(off)
    double rxN = st->rxBase + (double)(st->epochs + 1) * cfg.NT;
    if (cfg.roundMs) {
        const double r = std::floor(rxN * 1000.0 + 0.5) / 1000.0;
        if (std::fabs(r - rxN) < 1.0e-7) rxN = r;
    }
    return rxN;
}

// sums: [N][K][8] = iE qE iP qP iL qL case periods.  st: in / out.  rec: the epoch's log record.
DPE_HD static inline void vt_filter_epoch(const VtCfg &cfg, const VtEph *eph, dpe_vt_state_rec *st, const double *sums, double *rec, VtWork &w)
{
#pragma clang fp contract(off)
    const int K = cfg.K, N = cfg.N;
    // ---- phase 0: per channel -- discriminators, lock metric, measurement variances, line of sight; the state into the work area
    VT_LANES(l)
        w.P[l] = st->Sigma[l];
        if (l < 8) w.X[l] = st->X[l];
        if (l == 0) { w.fail = 0; w.piv = 0.0; }
        if (l < K) {
            const int k = l;
            dpe_vt_chan &c = st->chan[k];
            int bad = 0;
            double E = 0.0, L = 0.0, m1 = 0.0, m2 = 0.0, cross = 0.0, dot = 0.0, i0 = 0.0, q0 = 0.0;
            for (int j = 0; j < N; ++j) {
                const double *s = sums + ((size_t)j * K + k) * DPE_VT_CORR_DOUBLES;
                const double iE = s[0], qE = s[1], iP = s[2], qP = s[3], iL = s[4], qL = s[5];
                if (!(s[6] >= 0.0) || !vt_finite(iE) || !vt_finite(qE) || !vt_finite(iP) || !vt_finite(qP) || !vt_finite(iL) || !vt_finite(qL)) bad = 1;
                E += std::sqrt(iE * iE + qE * qE);
                L += std::sqrt(iL * iL + qL * qL);
                const double p = std::sqrt(iP * iP + qP * qP);
                m1 += p;
                m2 += p * p;
                if (j > 0) {   // discriminator.py:56-69 on the pair (j - 1, j), folded so that dot >= 0
                    double cr = i0 * qP - iP * q0, dt = i0 * iP + q0 * qP;
                    if (dt < 0.0) { cr = -cr; dt = -dt; }
                    cross += cr;
                    dot += dt;
                }
                i0 = iP; q0 = qP;
            }
            double dpc = 0.0, dfi = 0.0, lock = 0.0;
            if (!bad) {
                if (E + L != 0.0) dpc = (E - L) / (2.0 * (E + L));
                dfi = std::atan2(cross, dot) / (2.0 * 3.141592653589793 * cfg.T);
                m1 = m1 / (double)N;
                m2 = m2 / (double)N;
                const double var = m2 - m1 * m1;
                lock = var > 0.0 ? m1 / std::sqrt(var) : (m1 > 0.0 ? 1.0e30 : 0.0);
            }
            // W: the variance of the last numPrev included residuals (receiver.py:607-624), floored; the configured value until they exist
            double wR = cfg.initVarR, wV = cfg.initVarV;
            if (c.histN >= cfg.numPrev) {
                double sR = 0.0, sV = 0.0;
                for (int i = 0; i < cfg.numPrev; ++i) { sR += c.histRange[i]; sV += c.histRate[i]; }
                const double mR = sR / (double)cfg.numPrev, mV = sV / (double)cfg.numPrev;
                double vR = 0.0, vV = 0.0;
                for (int i = 0; i < cfg.numPrev; ++i) {
                    const double a = c.histRange[i] - mR, b = c.histRate[i] - mV;
                    vR += a * a;
                    vV += b * b;
                }
                vR = vR / (double)cfg.numPrev;
                vV = vV / (double)cfg.numPrev;
                wR = vR > cfg.minVarR ? vR : cfg.minVarR;
                wV = vV > cfg.minVarV ? vV : cfg.minVarV;
            }
            // geometry at the epoch's start: the satellite at the NCO's transmit time
            double d;
            const double tt = vt_transmit(eph[k], c.cp, c.rc, st->rxTime0, d);
            double sat[8];
            int kep = 0;
            if (st->satValid) {
#pragma unroll
                for (int i = 0; i < 8; ++i) sat[i] = c.sat[i];
            } else {
                kep = sat_state(eph[k].eph, tt, sat);
            }
            double los[3], bcFi, dChips;
            vt_geometry(sat, d, st->X, cfg.ds, los, bcFi, dChips);
            if (kep || !vt_finite(los[0]) || !vt_finite(los[1]) || !vt_finite(los[2])) bad = 1;
            w.los[3 * k] = los[0]; w.los[3 * k + 1] = los[1]; w.los[3 * k + 2] = los[2];
            w.bad[k] = bad;
            w.incl[k] = (!bad && lock > cfg.lockThr) ? 1 : 0;
            w.dpc[k] = dpc; w.dfi[k] = dfi; w.lock[k] = lock;
            w.eR[k] = -dpc * (kC / kFCA);                 // receiver.py:617, 644: adds to rc
            w.eV[k] = -dfi * (cfg.ds * kC / kFL1);        // receiver.py:618, 645: adds to fi
            w.wR[k] = wR; w.wV[k] = wV;
        }
    VT_END
    // ---- phase 1: the included channels in channel order
    VT_LANES(l)
        if (l < K) {
            int r = 0;
            for (int i = 0; i < l; ++i) r += w.incl[i];
            if (w.incl[l]) w.chanOf[r] = l;
        }
        if (l == 0) {
            int n = 0, anyBad = 0, mask = 0;
            for (int i = 0; i < K; ++i) { n += w.incl[i]; anyBad |= w.bad[i]; mask |= w.incl[i] << i; }
            w.nIncl = n;
            w.n = 2 * n;
            w.mask = mask;
            w.status = (anyBad ? DPE_VT_BAD_WINDOW : 0) | (n < 4 ? DPE_VT_NO_UPDATE : 0);
        }
    VT_END
    const int n = w.n, nI = w.nIncl;
    const bool update = nI >= 4;
    if (update) {
        // ---- A = H Sigma, rows [-los, 1, 0 0 0 0] and [0 0 0 0, -los, 1] (receiver.py:654-661)
        VT_LANES(l)
            for (int idx = l; idx < n * 8; idx += kVtLanes) {
                const int r = idx >> 3, b = idx & 7, hi = r >= nI, k = w.chanOf[hi ? r - nI : r], o = hi ? 4 : 0;
                const double *u = w.los + 3 * k;
                w.A[idx] = (((-u[0]) * w.P[o * 8 + b] + (-u[1]) * w.P[(o + 1) * 8 + b]) + (-u[2]) * w.P[(o + 2) * 8 + b]) + w.P[(o + 3) * 8 + b];
            }
            if (l < n) {
                const int hi = l >= nI, k = w.chanOf[hi ? l - nI : l];
                w.e[l] = hi ? w.eV[k] : w.eR[k];
                w.w[l] = hi ? w.wV[k] : w.wR[k];
            }
        VT_END
        // ---- S = A H^T + W
        VT_LANES(l)
            for (int idx = l; idx < n * n; idx += kVtLanes) {
                const int r = idx / n, cc = idx - r * n, hi = cc >= nI, k = w.chanOf[hi ? cc - nI : cc], o = hi ? 4 : 0;
                const double *u = w.los + 3 * k, *a = w.A + r * 8 + o;
                double s = ((a[0] * (-u[0]) + a[1] * (-u[1])) + a[2] * (-u[2])) + a[3];
                if (r == cc) s += w.w[r];
                w.S[r * kVtMaxRows + cc] = s;
            }
        VT_END
        // ---- Cholesky S = L L^T, a column per step, a row per lane; a pivot that is not positive ends it
        for (int cc = 0; cc < n; ++cc) {
            VT_LANES(l)
                if (l >= cc && l < n) {
                    double s = w.S[l * kVtMaxRows + cc];
                    for (int k = 0; k < cc; ++k) s -= w.S[l * kVtMaxRows + k] * w.S[cc * kVtMaxRows + k];
                    w.S[l * kVtMaxRows + cc] = s;
                    if (l == cc) w.piv = s;
                }
            VT_END
            VT_LANES(l)
                const double pv = w.piv;
                if (!(pv > 0.0) || !vt_finite(pv)) {
                    if (l == 0) w.fail = 1;
                } else if (l >= cc && l < n) {
                    const double dg = std::sqrt(pv);
                    w.S[l * kVtMaxRows + cc] = l == cc ? dg : w.S[l * kVtMaxRows + cc] / dg;
                }
            VT_END
            if (w.fail) break;
        }
    }
    if (update && !w.fail) {
        // ---- forward substitution: Y = L^-1 A (lanes 0 .. 7, a column each) and y = L^-1 e (lane 8)
        VT_LANES(l)
            if (l < 9) {
                for (int r = 0; r < n; ++r) {
                    double s = l < 8 ? w.A[r * 8 + l] : w.e[r];
                    for (int k = 0; k < r; ++k) s -= w.S[r * kVtMaxRows + k] * (l < 8 ? w.A[k * 8 + l] : w.e[k]);
                    s = s / w.S[r * kVtMaxRows + r];
                    if (l < 8) w.A[r * 8 + l] = s; else w.e[r] = s;
                }
            }
        VT_END
        // ---- X += K e = Y^T y;  Sigma = (I - K H) Sigma = Sigma - Y^T Y
        VT_LANES(l)
            const int a = l >> 3, b = l & 7;
            double s = 0.0;
            for (int r = 0; r < n; ++r) s += w.A[r * 8 + a] * w.A[r * 8 + b];
            w.P[l] = w.P[l] - s;
            if (l < 8) {
                double t = 0.0;
                for (int r = 0; r < n; ++r) t += w.A[r * 8 + l] * w.e[r];
                w.X[l] = w.X[l] + t;
            }
        VT_END
    }
    // ---- predict: Sigma symmetrised, F Sigma F^T + Q with the constant-velocity F of step N T (ekf.py:33-42), X = F X
    VT_LANES(l)
        const int i = l >> 3, j = l & 7;
        const double dt = cfg.NT;
        double fp0 = 0.5 * (w.P[i * 8 + j] + w.P[j * 8 + i]);
        if (i < 4) fp0 = fp0 + dt * (0.5 * (w.P[(i + 4) * 8 + j] + w.P[j * 8 + i + 4]));
        double s = fp0;
        if (j < 4) {
            double fp4 = 0.5 * (w.P[i * 8 + j + 4] + w.P[(j + 4) * 8 + i]);
            if (i < 4) fp4 = fp4 + dt * (0.5 * (w.P[(i + 4) * 8 + j + 4] + w.P[(j + 4) * 8 + i + 4]));
            s = s + fp4 * dt;
        }
        if (i == j) s = s + cfg.q[i];
        w.Pn[l] = s;
        if (l < 8) w.Xn[l] = l < 4 ? w.X[l] + dt * w.X[l + 4] : w.X[l];
    VT_END
    // ---- steer every channel from the predicted state (receiver.py:672-720), write the state and the log record
    VT_LANES(l)
        const double rxN = vt_next_rx_time(cfg, st);
        const int status = w.status | (w.fail ? DPE_VT_PIVOT : 0);
        if (l < K) {
            const int k = l;
            dpe_vt_chan &c = st->chan[k];
            const double adv = c.rc + (double)N * c.fc * cfg.T, turn = c.ri + (double)N * c.fi * cfg.T;
            const double rcN = wrap_pos(adv, (double)kLCA), cpN = c.cp + std::floor(adv / (double)kLCA), riN = wrap_pos(turn, 1.0);
            double d;
            const double tt = vt_transmit(eph[k], cpN, rcN, rxN, d);
            double sat[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, los[3], bcFi, dChips;
            double fiN = c.fi, fcN = c.fc;
            if (sat_state(eph[k].eph, tt, sat) == 0) {
                vt_geometry(sat, d, w.Xn, cfg.ds, los, bcFi, dChips);
                const double fcB = kFCA + cfg.fcaid * bcFi + dChips / cfg.NT;
                if (vt_finite(bcFi) && vt_finite(fcB)) { fiN = bcFi; fcN = fcB; }
            }
            if (w.incl[k]) {
                c.histRange[c.histPos] = w.eR[k];
                c.histRate[c.histPos] = w.eV[k];
                c.histPos = c.histPos + 1 >= cfg.numPrev ? 0 : c.histPos + 1;
                if (c.histN < cfg.numPrev) c.histN += 1;
            }
            c.rc = rcN; c.ri = riN; c.fc = fcN; c.fi = fiN; c.cp = cpN;
#pragma unroll
            for (int i = 0; i < 8; ++i) c.sat[i] = sat[i];
            double *o = rec + DPE_VT_LOG_HEAD + k * DPE_VT_LOG_CHAN;
            o[0] = rcN; o[1] = riN; o[2] = fcN; o[3] = fiN; o[4] = cpN;
            o[5] = w.eR[k]; o[6] = w.eV[k]; o[7] = w.wR[k]; o[8] = w.wV[k]; o[9] = w.lock[k]; o[10] = w.dpc[k]; o[11] = w.dfi[k];
        } else if (l < kVtMaxChan) {
            double *o = rec + DPE_VT_LOG_HEAD + l * DPE_VT_LOG_CHAN;
            for (int i = 0; i < DPE_VT_LOG_CHAN; ++i) o[i] = 0.0;
        }
        st->Sigma[l] = w.Pn[l];
        if (l < 8) {
            st->X[l] = w.Xn[l];
            rec[l] = w.Xn[l];
            rec[8 + l] = w.Pn[l * 9];
        }
        if (l == 63) {
            rec[16] = rxN; rec[17] = (double)w.mask; rec[18] = (double)status; rec[19] = (double)w.nIncl;
        }
    VT_END
    // (the scalars every lane of the last phase read are written behind its barrier)
    VT_LANES(l)
        if (l == 0) {
            st->rxTime0 = vt_next_rx_time(cfg, st);
            st->epochs = st->epochs + 1;
            st->status |= w.status | (w.fail ? DPE_VT_PIVOT : 0);
            st->satValid = 1;
        }
    VT_END
}

#undef VT_LANES
#undef VT_END

}  // namespace dpe
