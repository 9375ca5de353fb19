// dpe_nav_dev.h -- the scalar navigation solution's arithmetic (pygnss/pythonreceiver/scalar/naveng.py:10-224 with
// libgnss/utils.py:117-228), shared by its host form (dpe_nav_solve) and its device form (nav_solve_log_kernel), both in dpe_nav.hip.
// Satellite clock correction and ECEF state are dpe_sat.h's sat_state_t, which restates libgnss/satpos.py:8-185 operation for
// operation -- satellite_clock_correction at the transmit time, locate_satellite at transmit time - clock bias -- here with the
// twin's remainder: np.mod takes the divisor's sign where the reference's fmod takes the dividend's, and since 2 x 3.1415926535898
// is 1.4e-14 short of a period, an anomaly reduced the other way moves a satellite by 3.7e-7 m (measured against fixture O15: a
// constant 1.2e-7 m in the fix).
#pragma once
#include "../../include/dpe_hip.h"
#include "dpe_sat.h"   // sat_state_t, ModFloor (np.mod)

namespace dpe {

struct NavChan {      // what a channel's decode (or the caller) supplies
    Eph eph;
    double tow, cp;   // Ephemerides.timestamp
    int haveEph, haveTime;
};

// naveng.py:30-39: transmit time from the code-period count and the code phase, then the satellite's ECEF state there
DPE_HD static inline int nav_transmit(const NavChan &c, double cp, double rc, double &tt, double sat[8])
{
#pragma clang fp contract(off)
    const double codeIntDiff = (cp - c.cp) * kTCA;
    const double codeFracDiff = rc / kFCA;
    tt = c.tow + codeIntDiff + codeFracDiff;
    return sat_state_t(c.eph, tt, sat, ModFloor());
}

// naveng.py:60-71: pseudorange, pseudorate and the state rotated to ECI at t_c = rxTime (utils.py:173-228).
// o = {x, y, z, vx, vy, vz, pseudorange, pseudorate}
DPE_HD static inline void nav_observe(const double sat[8], double tt, double fi, double ds, double rxTime, double o[8])
{
#pragma clang fp contract(off)
    const double doppler = fi * ds;
    o[6] = kC * (rxTime - tt) + kC * sat[3];
    o[7] = (-kC / kFL1) * doppler + kC * sat[7];
    const double tgps = tt - sat[3];
    const double otau = kOEDot * (tgps - rxTime);
    double so, co;
    sincos(otau, &so, &co);
    o[0] = co * sat[0] - so * sat[1];
    o[1] = so * sat[0] + co * sat[1];
    o[2] = sat[2];
    o[3] = (co * sat[4] - so * sat[5]) + (-kOEDot * o[1]);
    o[4] = (so * sat[4] + co * sat[5]) + kOEDot * o[0];
    o[5] = sat[6];
}

// 4-unknown least squares by Givens rotations, one row at a time: the triangle and its right-hand side are 14 doubles, so rows
// need not be stored, the row order fixes every rounding, and the result has the backward stability of the twin's SVD lstsq
// (the normal equations would square the geometry's condition number).
struct Ls4 {
    double r00, r01, r02, r03, r11, r12, r13, r22, r23, r33, d0, d1, d2, d3;
};
DPE_HD static inline void ls4_init(Ls4 &s)
{
    s.r00 = s.r01 = s.r02 = s.r03 = s.r11 = s.r12 = s.r13 = s.r22 = s.r23 = s.r33 = s.d0 = s.d1 = s.d2 = s.d3 = 0.0;
}
DPE_HD static inline double ls4_rot(double rjj, double aj, double &c, double &sn)   // returns the new diagonal element
{
#pragma clang fp contract(off)
    const double h = std::sqrt(rjj * rjj + aj * aj);
    const bool z = h == 0.0;
    c = z ? 1.0 : rjj / h;
    sn = z ? 0.0 : aj / h;
    return h;
}
DPE_HD static inline void ls4_apply(double &r, double &a, double c, double sn)
{
#pragma clang fp contract(off)
    const double t = c * r + sn * a;
    a = c * a - sn * r;
    r = t;
}
DPE_HD static inline void ls4_add(Ls4 &s, double a0, double a1, double a2, double a3, double b)
{
    double c, sn;
    s.r00 = ls4_rot(s.r00, a0, c, sn);
    ls4_apply(s.r01, a1, c, sn); ls4_apply(s.r02, a2, c, sn); ls4_apply(s.r03, a3, c, sn); ls4_apply(s.d0, b, c, sn);
    s.r11 = ls4_rot(s.r11, a1, c, sn);
    ls4_apply(s.r12, a2, c, sn); ls4_apply(s.r13, a3, c, sn); ls4_apply(s.d1, b, c, sn);
    s.r22 = ls4_rot(s.r22, a2, c, sn);
    ls4_apply(s.r23, a3, c, sn); ls4_apply(s.d2, b, c, sn);
    s.r33 = ls4_rot(s.r33, a3, c, sn);
    ls4_apply(s.d3, b, c, sn);
}
// false: rank deficient (a diagonal element below 1e-12 of the largest), x is zero
DPE_HD static inline bool ls4_solve(const Ls4 &s, double x[4])
{
#pragma clang fp contract(off)
    const double a0 = std::fabs(s.r00), a1 = std::fabs(s.r11), a2 = std::fabs(s.r22), a3 = std::fabs(s.r33);
    const double mx = std::fmax(std::fmax(a0, a1), std::fmax(a2, a3)), mn = std::fmin(std::fmin(a0, a1), std::fmin(a2, a3));
    if (!(mn > 1e-12 * mx)) {
        x[0] = x[1] = x[2] = x[3] = 0.0;
        return false;
    }
    x[3] = s.d3 / s.r33;
    x[2] = (s.d2 - s.r23 * x[3]) / s.r22;
    x[1] = (s.d1 - s.r12 * x[2] - s.r13 * x[3]) / s.r11;
    x[0] = (s.d0 - s.r01 * x[1] - s.r02 * x[2] - s.r03 * x[3]) / s.r00;
    return true;
}

// perform_least_sqrs (naveng.py:132-224) from rxPos = 0, then naveng.py:76-77: rxTime_a and the rotation back to ECEF.
// get(k, o): observation k of n as nav_observe leaves it.
template <class Get>
DPE_HD static inline void nav_solve_core(int n, const Get &get, double rxTime, dpe_nav_fix &f, int status)
{
#pragma clang fp contract(off)
    double rx[4] = {0.0, 0.0, 0.0, 0.0}, x[4] = {0.0, 0.0, 0.0, 0.0}, o[8];
    int iters = 0;
    double last = 0.0;
    for (int it = 0; it < 10; ++it) {
        Ls4 s;
        ls4_init(s);
        for (int k = 0; k < n; ++k) {
            get(k, o);
            const double dx = o[0] - rx[0], dy = o[1] - rx[1], dz = o[2] - rx[2];
            const double nrm = std::sqrt(dx * dx + dy * dy + dz * dz);
            ls4_add(s, -dx / nrm, -dy / nrm, -dz / nrm, 1.0, o[6] - (nrm + rx[3]));
        }
        ++iters;
        if (!ls4_solve(s, x)) {
            status |= DPE_NAV_SOL_RANK_POS;
            last = 0.0;
            break;
        }
        for (int i = 0; i < 4; ++i) rx[i] = rx[i] + x[i];
        last = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3]);
        if (last < 1.0e-7) break;
    }
    if (last > 1.0e-5) status |= DPE_NAV_SOL_NOT_CONVERGED;
    double rv[4] = {0.0, 0.0, 0.0, 0.0};
    if (!(status & DPE_NAV_SOL_RANK_POS)) {
        Ls4 s;
        ls4_init(s);
        for (int k = 0; k < n; ++k) {
            get(k, o);
            const double dx = o[0] - rx[0], dy = o[1] - rx[1], dz = o[2] - rx[2];
            const double nrm = std::sqrt(dx * dx + dy * dy + dz * dz);
            const double lx = dx / nrm, ly = dy / nrm, lz = dz / nrm;
            ls4_add(s, -lx, -ly, -lz, 1.0, o[7] - (lx * o[3] + ly * o[4] + lz * o[5]));
        }
        if (!ls4_solve(s, rv)) status |= DPE_NAV_SOL_RANK_VEL;
    }
    // ECI -> ECEF at t_gps = rxTime_a, t_c = rxTime (utils.py:117-170)
    const double rxTimeA = rxTime - rx[3] / kC;
    const double otau = kOEDot * (rxTimeA - rxTime);
    double so, co;
    sincos(otau, &so, &co);
    const double wx = rv[0] - (-kOEDot * rx[1]), wy = rv[1] - kOEDot * rx[0];
    f.X_ECEF[0] = co * rx[0] + so * rx[1];
    f.X_ECEF[1] = -so * rx[0] + co * rx[1];
    f.X_ECEF[2] = rx[2];
    f.X_ECEF[3] = rx[3];
    f.X_ECEF[4] = co * wx + so * wy;
    f.X_ECEF[5] = -so * wx + co * wy;
    f.X_ECEF[6] = rv[2];
    f.X_ECEF[7] = rv[3];
    f.rxTime = rxTime;
    f.rxTime_a = rxTimeA;
    f.lastUpdate = last;
    f.iterations = iters;
    f.status = status;
}

}  // namespace dpe
