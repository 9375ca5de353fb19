// dpe_ekf_dev.h -- cuEKF's filter (cudarecv/modules/src/cuekf.cu:626-742) in its device form: the state block EkfDev and the 8 x 8
// fp64 update and predict steps with one lane per matrix element, run inside the device-resident loop's measurement kernel
// (chm_k1, dpe_chm_dev.h).  Device code only; the host form is dpe_ekf.hip.
#pragma once
#include "dpe_common.h"

#ifdef __HIPCC__
namespace dpe {

// cuEKF's filter (EnableEKF = true) as device state: dsp::cuEKF::StepUpdate / StepPredict (cuekf.cu:626-742) run inside the
// measurement kernel, one lane per matrix element.  Same fields, same row-major layout as the host form (dpe_ekf.hip).
struct EkfDev {
    double F[64], H[64], Q[64], K[64], Pk1k1[64], Pkk1[64], xk1k1[8], xkk1[8];
    double lpfVals[20];
    double lpfAvg;
    int lpfIdx, failed;   // failed: S was singular in some window (the state is then held for that window, bit 32 of the status)
    // the structure dpe_ekf_create gives F and H, which the device form exploits (see ekf_dev_step): H = I; F = I, plus Tc on [i][i + 4],
    // i < 4, when `coupled`
    int coupled, pad;
    double Tc;
};

// ---- cuEKF on the device: the 8 x 8 fp64 steps of dpe_ekf.hip with one lane per matrix element (a block of 64 threads).
// Every element is formed by the same operations in the same order as the host form (sums over k = 0 .. 7 ascending, no fused
// multiply-add), so the two give the same doubles.  sm: 6 x 64 doubles of LDS scratch.
#if defined(DPE_EXPERIMENTS) && defined(DPE_EKF_STAMPS)   // (timing attribution: shader-clock stamps of the phases of chm_k1, left in the fix record's two
#define DPE_EKF_STAMP(i) do { if (threadIdx.x == 0) dpe_ekf_stamps[i] = __builtin_readcyclecounter(); } while (0)   // out-of-window counts)
__shared__ unsigned long long dpe_ekf_stamps[10];
#else
#define DPE_EKF_STAMP(i) do { } while (0)
#endif
// (The filter's pieces are templates on the kernel form for one reason: each measurement kernel then has copies of its own, with the
// callers the single kernel had, and the inliner treats them as it did.  As functions shared by two kernels ekf_dev_invert became a
// call with a stack frame and ekf_dev_mul lost its 16-byte LDS reads -- in BOTH kernels.)
template <bool COV>
__device__ static inline double ekf_dev_mul(const double *a, const double *b, bool bT, double *c)
{
#pragma clang fp contract(off)
    const int l = threadIdx.x, i = l >> 3, j = l & 7;
    double s = 0.0;
    for (int k = 0; k < 8; ++k) s += a[i * 8 + k] * (bT ? b[j * 8 + k] : b[k * 8 + j]);
    __syncthreads();   // (c may alias a or b)
    c[l] = s;
    __syncthreads();
    return s;          // (this lane's element: the caller need not read it back)
}
// inverse through LU with partial pivoting (getrf + getri, cuekf.cu:681-694); false: singular.
// Round 6: the FACTORISATION runs on registers -- lane l = (r, kk) holds lu[r][kk]; the block is one wave, so a column's values at or
// below the diagonal are v_readlane pairs (wave-uniform: the pivot search is the host form's, first largest |.| at or below the
// diagonal), the row swap and the pivot row's element are one ds_bpermute round trip per column, a lane's own row's element of the
// column is a DPP row broadcast (rows c and p change places, so behind the swap row p holds the old diagonal element -- a uniform
// value -- and every other row below the diagonal what it held before), and nothing waits at a barrier.  Through LDS it was five
// dependent round trips and four barriers per column.  A lone wave is ISSUE-bound here (shader-clock stamps, scripts/ekf_stamps.py:
// 954 clocks per column at ~150 instructions, most of them selects): the DPP form of the own-row element replaced a 38-instruction
// select chain per column, and the pivot search became a scalar chain (below): chm_k1 with the filter 9.7-9.9 -> 8.8-9.0 us.  (Measured and
// dropped: the divisions with the divisor's reciprocal refined once, off the chain -- three dependent operations per quotient instead
// of thirteen, bit-identical under an exponent-range guard -- were SLOWER, 9.65-9.9 against 8.75-9.0 us on one box: the guards and
// selects add instructions, and what this wave pays for is instructions, ~5 clocks each, not the latency of a chain.)  Every element still sees the host form's operations in the host form's order: lu[r][c] /= lu[c][c];
// lu[r][k] -= lu[r][c] * lu[c][k] (no fused multiply-add).  The two substitutions (one column of the inverse per lane, 28 dependent
// multiply-subtracts each) read the factors back from LDS as before.
__device__ __forceinline__ double ekf_readlane_d(double v, int lane)
{
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, lane), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), lane);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
// lane N of every 16-lane row to all lanes of the row (row_newbcast); lane l + 4 of the row to lane l (row_shl:4, zero beyond the row)
template <int N>
__device__ __forceinline__ double ekf_row_bcast_d(double v)
{
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)u, 0x150 + N, 0xf, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), 0x150 + N, 0xf, 0xf, false);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double ekf_row_shl4_d(double v)
{
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)u, 0x104, 0xf, 0xf, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), 0x104, 0xf, 0xf, true);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
// column C of the factorisation; false: the column is zero at and below the diagonal (singular)
template <int C>
__device__ __forceinline__ bool ekf_lu_column(double &x, int &pv, int l, int r, int kk)
{
#pragma clang fp contract(off)
    // The pivot row: the first largest |.| at or below the diagonal, as the host form finds it.  The candidates are wave-uniform
    // (v_readlane pairs), and |a| > |b| on finite doubles is the unsigned order of their magnitude bits: the search is a chain of scalar
    // subtract-with-borrow / select steps -- five scalar instructions per candidate; as v_cmp_gt_f64 on scalar operands every step
    // was a vector compare between two scalar selects, each waiting for the other pipe.  (NaN-free input: a NaN in S makes every
    // later state NaN in either form.)
    const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
    unsigned bLo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, C * 8 + C);
    unsigned bHi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), C * 8 + C) & 0x7fffffffu;
    int p = C;
#pragma unroll
    for (int q = C + 1; q < 8; ++q) {
        const unsigned cLo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, q * 8 + C);
        const unsigned cHi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), q * 8 + C) & 0x7fffffffu;
        unsigned t;
        asm("s_sub_u32 %3, %0, %4\n\ts_subb_u32 %3, %1, %5\n\ts_cselect_b32 %0, %4, %0\n\ts_cselect_b32 %1, %5, %1\n\ts_cselect_b32 %2, %6, %2"
            : "+s"(bLo), "+s"(bHi), "+s"(p), "=&s"(t)
            : "s"(cLo), "s"(cHi), "s"(q)
            : "scc");
    }
    if ((bLo | bHi) == 0u) return false;
    const double pivVal = ekf_readlane_d(x, p * 8 + C);
    const double diagOld = ekf_readlane_d(x, C * 8 + C);   // (row p holds it behind the swap)
    // this lane's own row's element of column C before the swap: lane (r, C) = lane C or 8 + C of the lane's 16-lane row
    const double ownEven = ekf_row_bcast_d<C>(x), ownOdd = ekf_row_bcast_d<8 + C>(x);
    const double own = (r & 1) ? ownOdd : ownEven;
    // the row swap and the pivot row's element of this lane's column, both from the values before the swap: one round trip
    const int src = (r == C) ? p * 8 + kk : (r == p) ? C * 8 + kk : l;
    const double xs = __shfl(x, src, 64), xck = __shfl(x, p * 8 + kk, 64);
    const int ps = (l == C) ? p : (l == p) ? C : l;
    pv = __shfl(pv, ps, 64);
    x = xs;
    if (r > C) {
        const double xc = (r == p) ? diagOld : own;   // this lane's row's element of column C after the swap
        const double f = xc / pivVal;
        if (kk == C) x = f;
        else if (kk > C) x -= f * xck;
    }
    return true;
}
template <bool COV>
__device__ static inline bool ekf_dev_invert(const double *a, double *lu, double *inv, int *piv)
{
#pragma clang fp contract(off)
    const int l = threadIdx.x, r = l >> 3, kk = l & 7;
    double x = a[l];
    int pv = l;                      // lanes 0 .. 7: piv[l]
    const bool singular = !(ekf_lu_column<0>(x, pv, l, r, kk) && ekf_lu_column<1>(x, pv, l, r, kk) && ekf_lu_column<2>(x, pv, l, r, kk) &&
                            ekf_lu_column<3>(x, pv, l, r, kk) && ekf_lu_column<4>(x, pv, l, r, kk) && ekf_lu_column<5>(x, pv, l, r, kk) &&
                            ekf_lu_column<6>(x, pv, l, r, kk) && ekf_lu_column<7>(x, pv, l, r, kk));
    if (singular) return false;      // (wave-uniform)
    DPE_EKF_STAMP(3);
    lu[l] = x;
    (void)piv;
    int pvRow[8];                    // (wave-uniform: the row permutation, from lanes 0 .. 7)
#pragma unroll
    for (int i = 0; i < 8; ++i) pvRow[i] = __builtin_amdgcn_readlane(pv, i);
    __syncthreads();
    if (l < 8) {   // one column of the inverse per lane
        const int cl = l;
        double y[8], xx[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            double s = (pvRow[i] == cl) ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < i; ++k) s -= lu[i * 8 + k] * y[k];
            y[i] = s;
        }
#pragma unroll
        for (int i = 7; i >= 0; --i) {
            double s = y[i];
#pragma unroll
            for (int k = i + 1; k < 8; ++k) s -= lu[i * 8 + k] * xx[k];
            xx[i] = s / lu[i * 8 + i];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) inv[i * 8 + cl] = xx[i];
    }
    __syncthreads();
    return true;
}
// StepUpdate (:660-721) with the measurement z and R = I as BatchCorrManifold emits it (:2003-2011), then StepPredict (:626-656).
// Returns false when S is singular (state untouched).  sm: kEkfDevScratch doubles of LDS.
// Round 6: eight of the ten 8 x 8 products have H or F as a factor, and dpe_ekf_create fixes their structure -- H = I, F = I (+ Tc on
// [i][i + 4], i < 4).  A dot product of the host form, s = 0.0; s += a[i][k] * b[k][j] for k = 0 .. 7 without fused multiply-add, then
// reduces to its structural terms IN THE SAME ORDER: the exact-zero factors contribute +-0.0, which leaves a sum that started at +0.0
// unchanged (and +0.0 + x = x exactly, -0.0 included: it becomes +0.0 in both forms -- hence the literal "0.0 +" below).  So
//   H X = X H^T = 0.0 + X,      (F X)[i][j] = (0.0 + X[i][j]) + Tc X[i + 4][j]  (i < 4),      (X F^T)[i][j] = (0.0 + X[i][j]) + X[i][j + 4] Tc  (j < 4)
// give the host form's doubles bit for bit with one or two operations per element instead of sixteen LDS reads and eight dependent
// multiply-adds; the two dense products (K = P S^-1 and (I - K) P) and the LU inverse stay as they were.  chm_k1 with the filter:
// 11.7 -> see profiles/r6_closed_loop_device.txt.
constexpr int kEkfDevScratch = 11 * 64, kEkfDevXk = 640, kEkfDevX1 = 648;   // (x_k+1|k and x_k|k stay at these offsets of the scratch)
// the filter's operands of lane l, requested at the top of chm_k1 -- beside the keys and the grid rows of the measurement, not behind them
// (one ~1.5 us round trip to device memory off the kernel's dependent chain)
struct EkfPre {
    double p, xk, lpf, lpfAvg, Tc;
    int lpfIdx, coupled;
};
__device__ static inline EkfPre ekf_dev_prefetch(const EkfDev *e)
{
    const int l = threadIdx.x;
    EkfPre r;
    r.p = e->Pkk1[l];
    r.xk = l < 8 ? e->xkk1[l] : 0.0;
    r.lpf = l < 20 ? e->lpfVals[l] : 0.0;
    r.lpfAvg = e->lpfAvg;
    r.Tc = e->Tc;
    r.lpfIdx = e->lpfIdx;
    r.coupled = e->coupled;
    return r;
}
// COV: the measurement covariance is Rm (64 doubles of LDS, row-major) instead of the identity: S = (H P) H^T + Rm, the host form's
// S[i] += R[i] (dpe_ekf_step_update), so the states stay the host filter's fed the same R.  (dpe_chm_dev_set_measurement_cov)
template <bool COV>
__device__ static inline bool ekf_dev_step(EkfDev *e, const EkfPre &pre, const double *z, double *sm, int *piv, const double *Rm)
{
#pragma clang fp contract(off)
    const int l = threadIdx.x, i = l >> 3, j = l & 7;
    double *T = sm, *S = sm + 64, *Sinv = sm + 128, *lu = sm + 192, *y = sm + 256, *tmp = sm + 320;
    double *P = sm + 512, *P1 = sm + 576, *xk = sm + 640, *x1 = sm + 648;
    const bool coupled = pre.coupled != 0;
    const double Tc = pre.Tc;
    const double p = pre.p;
    P[l] = p;
    const int lpfIdx = __builtin_amdgcn_readfirstlane(pre.lpfIdx);
    const double lpfAvg0 = pre.lpfAvg;
    const double pz = 0.0 + p;                                     // H P = P H^T = 0.0 + P
    if constexpr (COV) S[l] = (0.0 + pz) + Rm[l];
    else S[l] = (0.0 + pz) + ((l % 9 == 0) ? 1.0 : 0.0);           // S = (H P) H^T + R
    T[l] = pz;                                                     // P H^T, the first factor of K
    if (l < 8) y[l] = z[l] - pre.xk;                               // y = z - H x_k|k-1
    __syncthreads();
    DPE_EKF_STAMP(2);
#if defined(DPE_EXPERIMENTS) && defined(DPE_EKF_SKIP_INV)   // (timing attribution only: wrong results)
    Sinv[l] = S[l];
    __syncthreads();
#else
    if (!ekf_dev_invert<COV>(S, lu, Sinv, piv)) return false;
#endif
    DPE_EKF_STAMP(4);
    const double kv = ekf_dev_mul<COV>(T, Sinv, false, tmp);            // K = (P H^T) S^-1
    e->K[l] = kv;
    double xs1 = 0.0;                                              // lanes 0 .. 7: x_k|k
    if (l < 8) {                                                   // x_k|k = x_k|k-1 + K y
        double s = pre.xk;
        for (int k = 0; k < 8; ++k) s += tmp[l * 8 + k] * y[k];
        x1[l] = s;                                                 // (left in the scratch for the caller: kEkfDevX1)
        e->xk1k1[l] = s;
        xs1 = s;
    }
    {                                                              // P_k|k = (I - K H) P_k|k-1, K H = 0.0 + K
        double t = -(0.0 + kv);
        if (l % 9 == 0) t += 1.0;
        __syncthreads();                                           // (the reads of tmp above)
        T[l] = t;
    }
    __syncthreads();
    DPE_EKF_STAMP(5);
    const double p1 = ekf_dev_mul<COV>(T, P, false, P1);
    DPE_EKF_STAMP(6);
    e->Pk1k1[l] = p1;
    // ---- StepPredict with GetQVal (:733-742) and EKF_Update_Q (:42-78).  The block is one wave: the low-pass state is wave-uniform
    // (every lane forms it from lanes 4 .. 6 of x_k|k and the ring entry of lane lpfIdx), so nothing is broadcast through LDS.
    const double v4 = ekf_readlane_d(xs1, 4), v5 = ekf_readlane_d(xs1, 5), v6 = ekf_readlane_d(xs1, 6);
    const double v = sqrt(v4 * v4 + v5 * v5 + v6 * v6);
    const double av = lpfAvg0 - ekf_readlane_d(pre.lpf, lpfIdx) + (v / 20.0);
    if (l == 0) {
        e->lpfVals[lpfIdx] = v / 20.0;
        e->lpfAvg = av;
        e->lpfIdx = lpfIdx + 1 >= 20 ? 0 : lpfIdx + 1;
    }
    DPE_EKF_STAMP(7);
    const double q = 1.0 + 250.0 / fmin(fmax(av * av, 50.0), 125.0);
    const auto q0 = [&](int r, int c) -> double {                  // Q0: diagonal
        if (r != c) return 0.0;
        if (r == 4 || r == 5 || r == 6) return q;
        if (r == 7) return (2.5e-10) * (2.5e-10) * kC * kC;        // Q_CLOCK_DRIFT, cuekf.h:28
        return 0.0;
    };
    const auto fq = [&](int r, int c) -> double {                  // (F Q0)[r][c]
        double s = 0.0 + q0(r, c);
        if (coupled && r < 4) s += Tc * q0(r + 4, c);
        return s;
    };
    double qv = 0.0 + fq(i, j);                                    // Q = (F Q0) F^T
    if (coupled && j < 4) qv += fq(i, j + 4) * Tc;
    e->Q[l] = qv;
    {                                                              // x_k+1|k = F x_k|k
        const double up = ekf_row_shl4_d(xs1);                     // lane l + 4's value (lanes 0 .. 3 read lanes 4 .. 7)
        if (l < 8) {
            double s = 0.0 + xs1;
            if (coupled && l < 4) s += Tc * up;
            xk[l] = s;                                             // (left in the scratch for the caller: kEkfDevXk)
            e->xkk1[l] = s;
        }
    }
    {                                                              // P_k+1|k = (F P) F^T + Q
        double t = 0.0 + p1;
        if (coupled && i < 4) t += Tc * P1[l + 32];
        const double tr = ekf_row_shl4_d(t);                       // (F P)[i][j + 4]: four lanes on in the lane's own matrix row
        double s2 = 0.0 + t;
        if (coupled && j < 4) s2 += tr * Tc;
        e->Pkk1[l] = s2 + qv;
    }
    __syncthreads();
    return true;
}

}  // namespace dpe
#endif  // __HIPCC__
