// dpe_chm_arith.h -- the channel manager's arithmetic (cudarecv/modules/src/cuchanmgr.cu:240-923) as plain C++, host and device:
// a channel's state, its transmit time, the back-calculated code phase, the measurement and the time update, the batch satellite
// states.  Shared by the host form (dpe_chm_*, dpe_chanmgr.hip) and the device form (dpe_chm_dev.h, dpe_chm_k2.h).  The orbit
// arithmetic underneath is dpe_sat.h's.
#pragma once
#include <cstddef>

#include "dpe_sat.h"

namespace dpe {

struct Chan {
    int prn, cpElaStart, cpElaEnd, cpRef, cpRefTOW;
    double rcStart, rcEnd, riStart, riEnd, fc, fi, txTime;
    double sat[8];
    Eph eph;
};

DPE_HD static inline double tx_of(const Chan &c, double cpEla, double rc)  // :258-260
{
    return c.cpRefTOW + ((cpEla - c.cpRef) * kTCA) + (rc / kFCA);
}

// back-calculated code phase (chips since the reference code period) for a receiver state x at
// receive time t and a rotated satellite state (:429-432, :763-774)
DPE_HD static inline double back_calc_rc(const Chan &c, const double sat[8], const double *x, double t, double *rangeOut)
{
    const double lx = sat[0] - x[0], ly = sat[1] - x[1], lz = sat[2] - x[2];
    const double range = std::sqrt(lx * lx + ly * ly + lz * lz);
    const double pr = range - kC * sat[3] + x[3];
    const double bcTx = t - pr / kC;
    const double frac = bcTx - c.cpRefTOW - ((c.cpElaEnd - c.cpRef) * kTCA);
    if (rangeOut) *rangeOut = range;
    return frac * kFCA;
}

// time update shared by CHM_TimeUpdateChannels (:675-823) and the tail of CHM_PropagateChannels (:451-602)
struct SatDirect {   // the reference's evaluation (CHM_Get_Sat_Pos)
    DPE_HD int operator()(const Chan &c, double tx, double out[8]) const { return sat_state(c.eph, tx, out); }
};
template <class SatFn>
DPE_HD static inline int advance(Chan &c, const double *x, double rxTime, double T, const SatFn &sat_at)
{
    const double adv = c.fc * T + c.rcEnd;
    const double cpPred = c.cpElaEnd + std::floor(adv / kLCA);
    const double rcPred = wrap_pos(adv, (double)kLCA);
    const double txPred = tx_of(c, cpPred, rcPred);
    double sp[8], sr[8];
    if (sat_at(c, txPred, sp)) return -1;
    const double tau = rxTime + T - (txPred + (x[3] / kC)) + sp[3];
    rotate_state(sp, tau, sr);
    const double bcRc = back_calc_rc(c, sr, x, rxTime + T, nullptr);
    c.cpElaStart = c.cpElaEnd;
    c.rcStart = c.rcEnd;
    c.cpElaEnd += std::floor(bcRc / kLCA);
    c.rcEnd = wrap_pos(bcRc, (double)kLCA);
    c.riStart = c.riEnd;
    c.riEnd = wrap_pos(c.fi * T + c.riEnd, 1.0);
    c.txTime = tx_of(c, c.cpElaEnd, c.rcEnd);
    return sat_at(c, c.txTime, c.sat);
}

// measurement update of fi / fc from the new fix x (CHM_PropagateChannels :380-447): the back-calculated carrier and code frequency.
// One copy for the host form (propagate) and the device form (chm_k1).
DPE_HD static inline void meas_update(const Chan &c, const double *x, double rxTime, double T, int dopplerSign, double &bcFi, double &bcFc)
{
    double sr[8], range;
    const double tau = rxTime - (c.txTime + (x[3] / kC)) + c.sat[3];
    rotate_state(c.sat, tau, sr);
    const double bcRc = back_calc_rc(c, sr, x, rxTime, &range);
    const double ex = x[4] - kOEDot * x[1], ey = x[5] + kOEDot * x[0], ez = x[6];
    const double lx = sr[0] - x[0], ly = sr[1] - x[1], lz = sr[2] - x[2];
    const double lrr = ((lx / range) * (ex - sr[4])) + ((ly / range) * (ey - sr[5])) + ((lz / range) * (ez - sr[6]));
    bcFi = kFL1 * ((lrr - x[7]) / kC + sr[7]) / dopplerSign;
    bcFc = kFCA + (dopplerSign * kFCA / kFL1) * bcFi + (bcRc - c.rcEnd) / T;
}
// the measurement update, then the time update
template <class SatFn>
DPE_HD static inline int propagate(Chan &c, const double *x, double rxTime, double T, int dopplerSign, const SatFn &sat_at)
{
    double bcFi, bcFc;
    meas_update(c, x, rxTime, T, dopplerSign, bcFi, bcFc);
    c.fi = bcFi;
    c.fc = bcFc;
    return advance(c, x, rxTime, T, sat_at);
}

// CHM_GridPrep :892-916 for one channel: the K x dimT batch satellite states.  The entry the ML kernels read (dimT / 2,
// BCM :1775) takes the reference's own evaluation.  The others differ from it by a clock-offset step of metres / c in the
// time of flight, i.e. by d <= 1e-10 rad of Earth rotation: their rotation is the mid one advanced to first order,
// cos(a + d) = cos a - d sin a, sin(a + d) = sin a + d cos a -- the d^2 / 2 <= 1e-20 remainder is far below the last bit --
// instead of 2 (dimT - 1) more sin/cos evaluations per SV.
DPE_HD static inline void batch_states(const Chan &c, double rxTime, const double *xkk1, const double *timeGrid, int dimT, double *out /* [dimT][8] */)
{
    const int mid = dimT / 2;
    const double tau0 = rxTime - (c.txTime + ((timeGrid[mid] + xkk1[3]) / kC)) + c.sat[3];
    double ct0, st0;
    sincos(-kOEDot * tau0, &st0, &ct0);
    for (int t = 0; t < dimT; ++t) {
        double *o = out + (size_t)t * 8;
        if (t == mid) { rotate_state_cs(c.sat, ct0, st0, o); continue; }
        const double tau = rxTime - (c.txTime + ((timeGrid[t] + xkk1[3]) / kC)) + c.sat[3];
        const double d = -kOEDot * (tau - tau0);
        if (std::fabs(d) < 1e-8) rotate_state_cs(c.sat, ct0 - d * st0, st0 + d * ct0, o);
        else rotate_state(c.sat, tau, o);   // a time grid of kilometres: evaluate directly
    }
}

}  // namespace dpe
