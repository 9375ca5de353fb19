// dpe_bcm_moments_cov.h -- from a window's manifold moments to the filter's measurement covariance R: ONE definition, host and device.
//
// dpe_bcm_moments (dpe_bcm_moments.h) leaves fifteen fp64 sums per manifold.  The host export dpe_bcm_moments_from_sums, the host
// export dpe_bcm_moments_rval and the device-resident loop's measurement kernel (chm_k1_cov_kernel, dpe_chm_dev.h) all form the 4 x 4
// covariance block of a manifold through mom_cov_block below, so the three carry the same doubles: every function here runs under
// fp contract(off) (S2 - mu S1 has to cancel to an exact 0 for a single point, and a fused multiply-add on one side only would
// split the host filter from the device filter), and every loop has a fixed order.  DESIGN.md 2.4h.
#pragma once
#include <cmath>

#include "dpe_consts.h"   // DPE_HD

namespace dpe {

constexpr int kMomSums = 15;
constexpr int kMomSlots = 16;    // a block's partial: the 15 sums and, as an integer in the last slot, its count of points above tau

// J = blockdiag(enu2ecef, 1): offsets (E, N, U, t) of a manifold grid -> (ECEF, t)
DPE_HD static inline void mom_frame(const double *R, double J[4][4])
{
    J[0][0] = R[0]; J[0][1] = R[1]; J[0][2] = R[2]; J[0][3] = 0.0;
    J[1][0] = R[3]; J[1][1] = R[4]; J[1][2] = R[5]; J[1][3] = 0.0;
    J[2][0] = R[6]; J[2][1] = R[7]; J[2][2] = R[8]; J[2][3] = 0.0;
    J[3][0] = 0.0;  J[3][1] = 0.0;  J[3][2] = 0.0;  J[3][3] = 1.0;
}

// One manifold's mean mu and M = J C J^T, C = S2 / S0 - mu mu^T, from its sums {1 | x y z t | xx xy xz xt yy yz yt zz zt tt}.
// S0 == 0 (no point above the threshold; a NaN sum goes the same way): mu and M are NaN.
DPE_HD static inline void mom_cov_block(const double *S, const double J[4][4], double mu[4], double M[4][4])
{
#pragma clang fp contract(off)
    // order of the sums: 1 | x y z t | xx xy xz xt yy yz yt zz zt tt -- the pair (a, b), a <= b, is sum 5 + 4 a - a (a - 1) / 2 + (b - a)
    const double S0 = S[0];
    double Cm[4][4], JC[4][4];
    const bool empty = !(S0 != 0.0);
#pragma unroll
    for (int a = 0; a < 4; ++a) mu[a] = empty ? (double)NAN : S[1 + a] / S0;
    // C as (S2 - mu S1^T) / S0: exactly 0 for a single point; one value per pair, both triangles
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = a; b < 4; ++b) Cm[a][b] = Cm[b][a] = empty ? (double)NAN : (S[5 + 4 * a - a * (a - 1) / 2 + (b - a)] - mu[a] * S[1 + b]) / S0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            double v = 0.0;
#pragma unroll
            for (int c = 0; c < 4; ++c) v += J[a][c] * Cm[c][b];
            JC[a][b] = v;
        }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = a; b < 4; ++b) {
            double v = 0.0;
#pragma unroll
            for (int c = 0; c < 4; ++c) v += JC[a][c] * J[b][c];
            if (empty) v = (double)NAN;
            M[a][b] = M[b][a] = v;
        }
}

// F = J diag(d) J^T: the grid's quantisation variance per (E, N, U, t) axis, moved into the frame of the measurement
DPE_HD static inline void mom_floor_block(const double J[4][4], const double *d, double F[4][4])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = a; b < 4; ++b) {
            double v = 0.0;
#pragma unroll
            for (int c = 0; c < 4; ++c) v += (J[a][c] * d[c]) * J[b][c];
            F[a][b] = F[b][a] = v;
        }
}

// One manifold's 4 x 4 block of the filter's R: M + F element by element; the identity where an entry is not finite (S0 == 0),
// and then the return value is true.  blk: row-major [16].
DPE_HD static inline bool mom_rval_block(const double *S, const double *enu2ecef, const double *floorVar, double *blk)
{
#pragma clang fp contract(off)
    double J[4][4], mu[4], M[4][4], F[4][4];
    mom_frame(enu2ecef, J);
    mom_cov_block(S, J, mu, M);
    mom_floor_block(J, floorVar, F);
    bool bad = false;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const double v = M[a][b] + F[a][b];
            bad = bad || !(fabs(v) <= 1.79769313486231570815e308);   // (NaN and +-inf fail the compare)
            blk[4 * a + b] = v;
        }
    if (bad) {
#pragma unroll
        for (int i = 0; i < 16; ++i) blk[i] = (i % 5 == 0) ? 1.0 : 0.0;
    }
    return bad;
}

// Both manifolds: R row-major [64] = blockdiag(block 0, block 1), the off-diagonal blocks exactly 0; returns the fallback bits
DPE_HD static inline int mom_rval(const double *sums /* [2][15] */, const double *enu2ecef, const double *floorVar /* [2][4] */, double *R)
{
    int fallback = 0;
    for (int i = 0; i < 64; ++i) R[i] = 0.0;
    for (int m = 0; m < 2; ++m) {
        double blk[16];
        if (mom_rval_block(sums + kMomSums * m, enu2ecef, floorVar + 4 * m, blk)) fallback |= 1 << m;
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) R[(4 * m + a) * 8 + 4 * m + b] = blk[4 * a + b];
    }
    return fallback;
}

}  // namespace dpe
