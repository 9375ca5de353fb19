// dpe_sat.h -- GPS orbit arithmetic as plain C++, host and device: the broadcast ephemeris, Kepler's equation, the satellite's ECEF
// state and clock (CHM_Get_Sat_Pos, cudarecv/modules/src/cuchanmgr.cu:85-210), the Earth rotation over a signal's time of flight and
// the ENU frame of a position.  One copy for the channel manager (dpe_chm_arith.h, dpe_chm_k2.h), the scalar navigator
// (dpe_nav_dev.h), the vector tracker (dpe_vt_dev.h) and collective detection's prediction (dpe_cd_plan.h).  Nothing of HIP is
// included: a host compiler builds it alone, a .hip unit brings the device's math functions with its runtime header.
#pragma once
#include <cmath>

#include "dpe_consts.h"

namespace dpe {

struct Eph {  // subset of eph_t (cudarecv/utils/inc/ephhelper.h:98-125) used by CHM_Get_Sat_Pos
    double sqrtA, e, i0, OMG0, omg, M0, deln, OMGd, idot, crc, crs, cuc, cus, cic, cis, toes, tocs, f0, f1, f2, tgd;
};

constexpr double kMu = 3.9860050e14;       // ephhelper.h MU_GPS
constexpr double kRelF = -4.442807633e-10; // consthelper.h CONST_F
constexpr double k2Pi = 6.2831853071796;   // consthelper.h CONST_2PI
constexpr double kWgsA = 6378137.0, kWgsB = 6356752.314245, kWgsE = 0.08181919084262149, kWgsEp = 0.08209443794969568;

DPE_HD static inline double half_week(double t)  // CHM_Correct_Week_Crossover :26-31
{
    return t > 302400.0 ? t - 604800.0 : (t < -302400.0 ? t + 604800.0 : t);
}

// The remainder the reference takes: C's fmod (the sign of the dividend).  The Python twin's np.mod takes the sign of the divisor
// (ModFloor); with kPi rounded as the ICD rounds it the two differ by more than a period's rounding for a negative angle.
struct ModTrunc {
    DPE_HD double operator()(double a, double m) const { return std::fmod(a, m); }
};
struct ModFloor {   // np.mod
    DPE_HD double operator()(double a, double m) const
    {
        double r = std::fmod(a, m);
        if (r != 0.0 && ((r < 0.0) != (m < 0.0))) r += m;
        return r;
    }
};

// The iteration of :97-107 from wherever E stands (its fixed point does not depend on the start: dpe_chm_k2.h starts it warm)
template <class Mod>
DPE_HD static inline bool kepler_iterate(double M, double e, double &E, const Mod &mod)
{
    double dE = 1.0;
    for (int it = 0; it < 10 && std::fabs(dE) > 1e-12; ++it) {
        double sE, cE;
        sincos(E, &sE, &cE);   // glibc: bit-identical to sin() and cos(), one argument reduction
        dE = (M - E + e * sE) / (1.0 - e * cE);
        E = mod(E + dE, k2Pi);
    }
    return std::fabs(dE) <= 1e-12;
}
template <class Mod>
DPE_HD static inline bool solve_kepler_t(double M, double e, double &E, const Mod &mod)  // :97-107
{
    E = M;
    return kepler_iterate(M, e, E, mod);
}
DPE_HD static inline bool solve_kepler(double M, double e, double &E) { return solve_kepler_t(M, e, E, ModTrunc()); }

// CHM_Get_Sat_Pos :85-210 -> state {x,y,z,clk bias, vx,vy,vz, clk drift}
template <class Mod>
DPE_HD static inline int sat_state_t(const Eph &p, double tx, double out[8], const Mod &mod)
{
    const double A = p.sqrtA * p.sqrtA;
    const double n = std::sqrt(kMu / (A * A * A)) + p.deln;
    double tc = half_week(tx - p.tocs);
    double clkb = p.f2 * tc * tc + p.f1 * tc + p.f0 - p.tgd;
    double tk = half_week(tx - clkb - p.toes);
    double E;
    if (!solve_kepler_t(mod(p.M0 + n * tk, k2Pi), p.e, E, mod)) return -1;
    const double dtr = kRelF * p.e * p.sqrtA * std::sin(E);
    tc = tx - (clkb + dtr) - p.tocs;
    clkb = p.f2 * tc * tc + p.f1 * tc + p.f0 + dtr - p.tgd;
    const double clkd = p.f1 + 2.0 * p.f2 * tc;
    tk = half_week(tx - clkb - p.toes);
    if (!solve_kepler_t(mod(p.M0 + n * tk, k2Pi), p.e, E, mod)) return -1;
    double sE, cE;
    sincos(E, &sE, &cE);
    const double den = 1.0 - p.e * cE;
    const double nu = std::atan2(std::sqrt(1.0 - p.e * p.e) * sE / den, (cE - p.e) / den);
    double u = mod(nu + p.omg, k2Pi);
    double c2, s2;
    sincos(2.0 * u, &s2, &c2);
    u += p.cuc * c2 + p.cus * s2;
    const double r = A * den + p.crc * c2 + p.crs * s2;
    const double inc = p.i0 + p.idot * tk + p.cic * c2 + p.cis * s2;
    const double Om = mod(p.OMG0 + (p.OMGd - kOEDot) * tk - kOEDot * p.toes, k2Pi);
    double su, cu, sO, cO, si, ci;
    sincos(u, &su, &cu);
    sincos(Om, &sO, &cO);
    sincos(inc, &si, &ci);
    const double xo = r * cu, yo = r * su;
    out[0] = xo * cO - yo * sO * ci;
    out[1] = xo * sO + yo * cO * ci;
    out[2] = yo * si;
    out[3] = clkb;
    sincos(2.0 * u, &s2, &c2);  // recomputed with the corrected u (:180-181)
    const double Ed = n / den;
    double snu, cnu;
    sincos(nu, &snu, &cnu);
    const double nud = sE * Ed * (1.0 + p.e * cnu) / (snu * den);
    const double ud = nud + 2.0 * (p.cus * c2 - p.cuc * s2) * nud;
    const double rd = A * p.e * sE * Ed + 2.0 * (p.crs * c2 - p.crc * s2) * nud;
    const double id = p.idot + (p.cis * c2 - p.cic * s2) * 2 * nud;
    const double vxo = rd * cu - yo * ud, vyo = rd * su + xo * ud;
    const double Omd = p.OMGd - kOEDot;
    const double ta = vxo - yo * ci * Omd, tb = xo * Omd + vyo * ci - yo * si * id;
    out[4] = ta * cO - tb * sO;
    out[5] = ta * sO + tb * cO;
    out[6] = vyo * si + yo * ci * id;
    out[7] = clkd;
    return 0;
}
DPE_HD static inline int sat_state(const Eph &p, double tx, double out[8]) { return sat_state_t(p, tx, out, ModTrunc()); }

DPE_HD static inline double wrap_pos(double v, double m)
{
    double t = std::fmod(v, m);
    return t < 0.0 ? t + m : t;
}

// Earth-rotation of a satellite state by the signal time of flight (:383-404, :895-916)
DPE_HD static inline void rotate_state_cs(const double s[8], double ct, double st, double o[8]);
DPE_HD static inline void rotate_state(const double s[8], double tau, double o[8])
{
    double ct, st;
    const double x = -kOEDot * tau;
#ifdef __HIP_DEVICE_COMPILE__
    // The angle is the Earth's rotation over a signal's travel time, ~5e-6 rad: below 2^-10 the series to x^5 / x^6 are exact to the last
    // bit (next terms x^7 / 5040 and x^8 / 40320 are < 2e-22 of sin x and < 3e-29), and the device library's sincos -- argument
    // reduction and all, ~230 instructions of the lone wave of chm_k1, which pays ~5 clocks for each -- is not needed.
    if (fabs(x) < 0x1p-10) {
        const double x2 = x * x;
        st = x * fma(x2, fma(x2, 1.0 / 120.0, -1.0 / 6.0), 1.0);
        ct = fma(x2, fma(x2, fma(x2, -1.0 / 720.0, 1.0 / 24.0), -0.5), 1.0);
    } else
#endif
        sincos(x, &st, &ct);
    rotate_state_cs(s, ct, st, o);
}
DPE_HD static inline void rotate_state_cs(const double s[8], double ct, double st, double o[8])
{
    o[0] = ct * s[0] - st * s[1];
    o[1] = st * s[0] + ct * s[1];
    o[2] = s[2];
    o[3] = s[3];
    o[4] = ct * s[4] - st * s[5] - kOEDot * st * s[0] - kOEDot * ct * s[1];
    o[5] = st * s[4] + ct * s[5] + kOEDot * ct * s[0] - kOEDot * st * s[1];
    o[6] = s[6];
    o[7] = s[7];
}

// CHM_Dev_ECEF2LL_Rad :37-50 + CHM_Dev_R_ENU2ECEF :54-73: row-major ENU -> ECEF at the grid centre
DPE_HD static inline void enu2ecef_matrix(const double *xkk1, double Rm[9])
{
    const double p = std::sqrt(xkk1[0] * xkk1[0] + xkk1[1] * xkk1[1]);
    const double th = std::atan2(xkk1[2] * kWgsA, p * kWgsB);
    const double lat = std::atan2(xkk1[2] + std::pow(kWgsEp, 2) * kWgsB * std::pow(std::sin(th), 3),
                                  p - std::pow(kWgsE, 2) * kWgsA * std::pow(std::cos(th), 3));
    const double lon = std::atan2(xkk1[1], xkk1[0]);
    double sa, ca, so, co;
    sincos(lat, &sa, &ca);
    sincos(lon, &so, &co);
    Rm[0] = -so; Rm[1] = -sa * co; Rm[2] = ca * co;
    Rm[3] = co;  Rm[4] = -sa * so; Rm[5] = ca * so;
    Rm[6] = 0.0; Rm[7] = ca;       Rm[8] = sa;
}

}  // namespace dpe
