// dpe_chm_k2.h -- the device-resident channel manager's state, ports and kernel arguments, and the part of its per-window work
// that rides in the next window's stage-1 launch: the time update chm_k2 and the speculative satellite states chm_k3.  dpe_bcs.hip
// includes this header alone -- its bank kernels carry the two as extra blocks -- and so compiles neither the measurement kernel
// nor the filter; dpe_chm_dev.h adds those for dpe_chanmgr.hip.  Device code only.
#pragma once
#include "dpe_common.h"
#include "dpe_prep.h"
#include "dpe_chm_arith.h"

#ifdef __HIPCC__
namespace dpe {

struct ChmDevState {
    Chan ch[DPE_MAX_CHAN];
    double warmE[DPE_MAX_CHAN], warmM[DPE_MAX_CHAN];   // Kepler warm start: eccentric / mean anomaly of the channel's last evaluation
    int warmOk[DPE_MAX_CHAN];
    double rxTime, T;
    int dopplerSign, K, dimT;
    int status;        // sticky: 1 Kepler iteration failed, 4 an arg-max key was 0 / out of range, 8 / 16 BatchCorrScores input flags
    long long window;  // windows completed (Start does not count)
    // ---- speculative satellite states (chm_k3): the Kepler solutions of the NEXT time update, computed one window ahead beside
    // the current one (two buffers, alternating with the window parity the host passes in ChmKArgs::specPar)
    Eph ephC[DPE_MAX_CHAN];                 // the ephemerides again, never written after create (chm_k3 reads them while chm_k2 rewrites ch[])
    double snapFc[DPE_MAX_CHAN], snapRcEnd[DPE_MAX_CHAN];   // chm_k1's snapshot of what chm_k3 needs of a channel (chm_k2 overwrites ch[] beside it)
    int snapCpElaEnd[DPE_MAX_CHAN], snapCpRef[DPE_MAX_CHAN], snapCpRefTOW[DPE_MAX_CHAN];
    double specTx[2][DPE_MAX_CHAN], specSat[2][2][DPE_MAX_CHAN][8];   // [buffer][at specTx | at specTx + kChmH]
    int specOk[2][DPE_MAX_CHAN];
    double specWE[2][DPE_MAX_CHAN], specWM[2][DPE_MAX_CHAN];          // chm_k3's own Kepler warm start, per wave
    int specWOk[2][DPE_MAX_CHAN];
};
// The reference's output ports of cuChanMgr (cuchanmgr.cu:973-990,1136-1171) and cuEKF (cuekf.cu:277-279) as device arrays,
// plus zVal (BatchCorrManifold, :2297) and the TimeGrid input
struct ChmPorts {
    double *rxTime, *txTime, *rcStart, *riStart, *rcEnd, *riEnd, *fc, *fi, *sat, *enu2ecef, *xk1k1, *xkk1, *zVal, *timeGrid;
    int *dopplerSign, *cpRef, *cpElaStart, *cpElaEnd, *cpRefTOW;
    unsigned char *prn;
};

struct EkfDev;   // dpe_ekf_dev.h: the measurement kernel's filter; chm_k2 and chm_k3 only pass the pointer on

struct ChmKArgs {
    ChmDevState *st;
    ChmPorts p;
    int mode;                       // 0 Start (CHM_ComputeSatStates + time update), 1 Update (measurement + time update)
    int specPar;                    // which speculative buffer chm_k2 reads; chm_k3 (same launch) fills the other one
    const double *xk1k1, *xkk1;     // inputs 10 / 12 on the device; ignored when meas != 0
    // measurement from the attached BatchCorrManifold's keys (BCM_MakePosMeas / MakeVelMeas + EKF_PassMeas)
    int meas;
    const unsigned long long *keys; // {posKey, velKey, posOutOfWindow, velOutOfWindow} of the window just scanned
    const double *posGrid, *velGrid;
    const double *posAx, *velAx;    // grid axes (x, y, z, t back to back) instead of point lists: the index is decoded from them
    int posDim[4], velDim[4];
    long long posG, velG, posOff, velOff;
    dpe_fix_record *ring;           // pinned, device address
    int ringDepth;
    dpe_fix_record *stage;          // device memory: chm_k1 leaves the window's record here, the chm_k2 that follows it sends it over the host link
    EkfDev *ekf;                    // nullptr: EKF_PassMeas (the shipped flow); else the filter runs on the measurement (dpe_chm_dev_set_ekf)
    // parameter blocks of the attached handles for the NEXT window (nullptr: not attached)
    BcsChanDev *bcsChan;
    int *bcsStatus;
    int hintL1;                     // > 0: the attached BatchCorrScores chooses its kernel from nominal values (dpe_bcs_set_dev_hint): check the promise here
    double hintStepMax;
    int *hintViol;
    double fs;
    int S;
    BcmSvDev *svPos, *svVel;
    BcmDevWin *devWin;
    double Cf;
    int L, B;
    long long C;
};

// CHM_Get_Sat_Pos with the Kepler iterations started near their fixed point: the first solve from the channel's previous
// eccentric anomaly advanced by the change of the mean anomaly (two iterations instead of five at e = 0.01), the second -- whose
// mean anomaly differs by n x 1e-8 s -- from the first.  The iteration's fixed point does not depend on where it starts; the
// values agree with the cold start to the last bits (1e-16 in E).
__device__ static inline int sat_state_warm(const Eph &p, double tx, double out[8], double &wE, double &wM, int &wOk)
{
    const double A = p.sqrtA * p.sqrtA;
    const double n = sqrt(kMu / (A * A * A)) + p.deln;
    double tc = half_week(tx - p.tocs);
    double clkb = p.f2 * tc * tc + p.f1 * tc + p.f0 - p.tgd;
    double tk = half_week(tx - clkb - p.toes);
    double M = fmod(p.M0 + n * tk, k2Pi);
    double E = M;
    if (wOk && fabs(M - wM) < 1e-2) E = wE + (M - wM);
    if (!kepler_iterate(M, p.e, E, ModTrunc())) return -1;
    const double dtr = kRelF * p.e * p.sqrtA * sin(E);
    tc = tx - (clkb + dtr) - p.tocs;
    clkb = p.f2 * tc * tc + p.f1 * tc + p.f0 + dtr - p.tgd;
    const double clkd = p.f1 + 2.0 * p.f2 * tc;
    tk = half_week(tx - clkb - p.toes);
    M = fmod(p.M0 + n * tk, k2Pi);
    if (!kepler_iterate(M, p.e, E, ModTrunc())) return -1;
    wE = E; wM = M; wOk = 1;
    double sE, cE;
    sincos(E, &sE, &cE);
    const double den = 1.0 - p.e * cE;
    const double nu = atan2(sqrt(1.0 - p.e * p.e) * sE / den, (cE - p.e) / den);
    double u = fmod(nu + p.omg, k2Pi);
    double c2, s2;
    sincos(2.0 * u, &s2, &c2);
    u += p.cuc * c2 + p.cus * s2;
    const double r = A * den + p.crc * c2 + p.crs * s2;
    const double inc = p.i0 + p.idot * tk + p.cic * c2 + p.cis * s2;
    const double Om = fmod(p.OMG0 + (p.OMGd - kOEDot) * tk - kOEDot * p.toes, k2Pi);
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

// The per-window work in two pieces, so that only the first sits between the scan of window n and the correlator of window n+1:
//
//   chm_k1 (one wave, a kernel of its own behind the scan; dpe_chm_dev.h): the measurement from the scan's keys (BCM_MakePosMeas /
//       MakeVelMeas, batchcorrmanifold.cu:1977-2068), the pass-through (EKF_PassMeas, cuekf.cu:147-159), the measurement update of
//       fi / fc (CHM_PropagateChannels :380-447), BatchCorrScores' parameter block of the next window, the fix for the host (the
//       record's fields leave for the pinned ring as soon as the measurement exists, its sequence word at the kernel's end).
//   chm_k2 (one block of 256 threads): the time update (CHM_TimeUpdateChannels :675-823) with its two Kepler evaluations
//       (:85-210), CHM_GridPrep (:853-923), BatchCorrManifold's coefficient blocks.  Nothing the next window's stage 1 reads
//       -- it runs as an extra block of that window's stage-1 LAUNCH (bcs_bank_kernel, FUSE form), beside the correlator blocks,
//       and is complete when the scan starts.  (As a kernel of its own for a host that keeps the reference's module order.)
//       Waves 0 / 1: a channel's two evaluations lie ~1e-7 s apart, so the second is the first advanced along the difference
//       quotient over h = 2^-10 s (step error a h / 2 x dt = 3e-11 m) and the two run side by side.  Wave 2: the ENU matrix.
//       Then all threads: the K x dimT batch states.
constexpr double kChmH = 0.0009765625;

__device__ __forceinline__ static void chm_k2(const ChmKArgs &a)
{
    __shared__ double sXk[8], sR[9];
    __shared__ double sTx[DPE_MAX_CHAN], sS1[DPE_MAX_CHAN][8], sSat[DPE_MAX_CHAN][8], sTau0[DPE_MAX_CHAN], sCt[DPE_MAX_CHAN], sSt[DPE_MAX_CHAN];
    __shared__ int sFlags;
    ChmDevState *st = a.st;
    const int tid = threadIdx.x, nThreads = blockDim.x, wave = tid >> 6, k = tid & 63, K = st->K, dimT = st->dimT;
    const double rxTime = st->rxTime, T = st->T;
    const int ds = st->dopplerSign;
    const bool live = wave < 2 && k < K;
    if (tid == 0) sFlags = 0;
    if (tid < 8) sXk[tid] = a.p.xkk1[tid];
    // the fix record chm_k1 staged: its fields go out over the host link now (one otherwise idle lane), the sequence word at the end
    // of this kernel, when they have long arrived
    dpe_fix_record *ringRec = nullptr;
    unsigned long long ringSeq = 0ull;
    if (a.meas && tid == nThreads - 1) {
        const dpe_fix_record rec = *a.stage;
        ringSeq = rec.seq;
        ringRec = a.ring + ((long long)(ringSeq - 1ull) % a.ringDepth);
        for (int i = 0; i < 8; ++i) __hip_atomic_store(&ringRec->zVal[i], rec.zVal[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&ringRec->rxTime, rec.rxTime, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&ringRec->posIndex, rec.posIndex, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&ringRec->velIndex, rec.velIndex, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&ringRec->posOutOfWindow, rec.posOutOfWindow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&ringRec->velOutOfWindow, rec.velOutOfWindow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&ringRec->posScore, rec.posScore, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&ringRec->velScore, rec.velScore, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&ringRec->status, rec.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    Chan c;
    double wE = 0.0, wM = 0.0;
    int wOk = 0;
    if (live) {
        c = st->ch[k];
        wE = st->warmE[k]; wM = st->warmM[k]; wOk = st->warmOk[k];
    }
    __syncthreads();
    // ---- 1. predicted transmit time (CHM_TimeUpdateChannels :675-823); at Start first CHM_ComputeSatStates :258-301
    double x1[8];
    for (int i = 0; i < 8; ++i) x1[i] = a.p.xk1k1[i];
    double txPred = 0.0;
    if (wave == 0 && live) {
        if (a.mode == 0) {
            c.txTime = tx_of(c, c.cpElaEnd, c.rcEnd);
            if (sat_state_warm(c.eph, c.txTime, c.sat, wE, wM, wOk)) atomicOr(&sFlags, 1);
        }
        const double adv = c.fc * T + c.rcEnd;
        const double cpPred = c.cpElaEnd + floor(adv / kLCA);
        const double rcPred = wrap_pos(adv, (double)kLCA);
        txPred = tx_of(c, cpPred, rcPred);
        sTx[k] = txPred;
    }
    __syncthreads();
    // ---- 2. the satellite state at the predicted transmit time (wave 0) and a step later (wave 1), side by side; wave 2: the
    //         ENU -> ECEF matrix of the next grid centre (CHM_Dev_R_ENU2ECEF :54-73)
    // A chm_k3 one window earlier has left both states at a transmit time within ~1e-7 s of this one (it could not know this window's
    // fix): they are advanced along their own difference quotient -- the remainder, a delta^2 / 2 with a = 0.6 m/s^2, is 1e-14 m --
    // and the two Kepler solutions, 5 us of a lone wave's fp64 libm calls, are off this kernel's path.  Without a usable
    // speculation (Start, a standalone launch, a jump of the code phase) the solutions are computed here as before.
    double sp[8];
    if (live) {
        const int sb = a.specPar & 1;
        const double dSpec = sTx[k] - st->specTx[sb][k];
        if (a.mode == 1 && st->specOk[sb][k] && fabs(dSpec) < 1e-5) {
            if (wave == 0) {
                for (int i = 0; i < 8; ++i) {
                    const double s0 = st->specSat[sb][0][k][i], s1 = st->specSat[sb][1][k][i];
                    const double adv = (s1 - s0) / kChmH * dSpec;
                    sp[i] = s0 + adv;
                    sS1[k][i] = s1 + adv;
                }
            }
        } else {
            const double tx = sTx[k] + (wave == 1 ? kChmH : 0.0);
            if (sat_state_warm(c.eph, tx, sp, wE, wM, wOk)) atomicOr(&sFlags, 1);
            if (wave == 1)
                for (int i = 0; i < 8; ++i) sS1[k][i] = sp[i];
        }
    }
    if (tid == 128) {
        double Rm[9];
        enu2ecef_matrix(sXk, Rm);
        for (int i = 0; i < 9; ++i) { sR[i] = Rm[i]; a.p.enu2ecef[i] = Rm[i]; }
        a.p.rxTime[0] = rxTime + T;
        a.p.dopplerSign[0] = ds;
        if (a.devWin) {   // the window frame dpe_bcm_results would read (pinned): sent now, it has arrived long before the kernel ends
            for (int i = 0; i < 8; ++i) a.devWin->xCurrkk1[i] = sXk[i];
            for (int i = 0; i < 9; ++i) a.devWin->enu2ecef[i] = Rm[i];
            a.devWin->dopplerSign = ds;
            a.devWin->bad = 0;
        }
    }
    __syncthreads();
    // ---- 3. wave 0: the rest of the time update; the state at the back-calculated transmit time along the difference quotient
    if (wave == 0 && live) {
        double sr[8];
        const double tau = rxTime + T - (txPred + (x1[3] / kC)) + sp[3];
        rotate_state(sp, tau, sr);
        const double bcRc = back_calc_rc(c, sr, x1, rxTime + T, nullptr);
        c.cpElaStart = c.cpElaEnd;
        c.rcStart = c.rcEnd;
        c.cpElaEnd += floor(bcRc / kLCA);
        c.rcEnd = wrap_pos(bcRc, (double)kLCA);
        c.riStart = c.riEnd;
        c.riEnd = wrap_pos(c.fi * T + c.riEnd, 1.0);
        c.txTime = tx_of(c, c.cpElaEnd, c.rcEnd);
        const double dt = c.txTime - txPred;
        for (int i = 0; i < 8; ++i) c.sat[i] = fma((sS1[k][i] - sp[i]) / kChmH, dt, sp[i]);
        st->ch[k] = c;
        st->warmE[k] = wE; st->warmM[k] = wM; st->warmOk[k] = wOk;
        // ports (cuchanmgr.cu:1136-1171)
        a.p.txTime[k] = c.txTime;
        a.p.rcStart[k] = c.rcStart; a.p.riStart[k] = c.riStart;
        a.p.rcEnd[k] = c.rcEnd;     a.p.riEnd[k] = c.riEnd;
        a.p.fc[k] = c.fc;           a.p.fi[k] = c.fi;
        a.p.cpRef[k] = c.cpRef;     a.p.cpElaStart[k] = c.cpElaStart;
        a.p.cpElaEnd[k] = c.cpElaEnd; a.p.cpRefTOW[k] = c.cpRefTOW;
        a.p.prn[k] = (unsigned char)c.prn;
        // CHM_GridPrep :892-916 at the new receive time: the mid-time rotation here, the K x dimT entries by all threads below
        const double tau0 = rxTime + T - (c.txTime + ((a.p.timeGrid[dimT / 2] + sXk[3]) / kC)) + c.sat[3];
        double ct0, st0;
        sincos(-kOEDot * tau0, &st0, &ct0);
        sCt[k] = ct0; sSt[k] = st0; sTau0[k] = tau0;
        for (int i = 0; i < 8; ++i) sSat[k][i] = c.sat[i];
        if (a.svPos) {
            double mid[8];
            rotate_state_cs(c.sat, ct0, st0, mid);
            BcmSvDev ap, av;
            bcm_prep_one(sXk, sR, mid, c.rcEnd, c.fc, c.fi, c.cpRefTOW, c.cpElaEnd, c.cpRef, ds, rxTime + T, a.fs, a.Cf, a.S, a.L, a.B, a.C, ap, av);
            a.svPos[k] = ap;
            a.svVel[k] = av;
        }
    }
    __syncthreads();
    // ---- 4. batch satellite states, entry (channel, time-grid index) per thread (see batch_states: the mid entry takes the
    //         reference's own evaluation, the others its first-order neighbourhood)
    for (int e = tid; e < K * dimT; e += nThreads) {
        const int kk = e / dimT, t = e - kk * dimT;
        double *o = a.p.sat + (size_t)e * 8;
        const double ct0 = sCt[kk], st0 = sSt[kk];
        if (t == dimT / 2) { rotate_state_cs(sSat[kk], ct0, st0, o); continue; }
        const double dTau = -(a.p.timeGrid[t] - a.p.timeGrid[dimT / 2]) / kC;   // tau - tau0
        const double d = -kOEDot * dTau;
        if (fabs(d) < 1e-8) rotate_state_cs(sSat[kk], ct0 - d * st0, st0 + d * ct0, o);
        else rotate_state(sSat[kk], sTau0[kk] + dTau, o);
    }
    if (tid == 0) {
        st->rxTime = rxTime + T;   // :1121, :1249
        if (a.mode == 1) st->window += 1;
        if (sFlags) st->status |= sFlags;
    }
    if (ringRec) {   // the record is complete once its fields have arrived: sequence word last
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(&ringRec->seq, ringSeq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// chm_k3 (two waves, beside chm_k2 in the stage-1 launch): the satellite states the NEXT time update will ask for.  That update's
// transmit time follows from the channel as chm_k2 is leaving it right now and from the next fix; predicted from chm_k1's snapshot
// -- two windows of code-phase advance at the present code frequency -- it is off by the next fix's correction, ~1e-7 s.
__device__ __forceinline__ static void chm_k3(const ChmKArgs &a)
{
    ChmDevState *st = a.st;
    const int tid = threadIdx.x, wave = tid >> 6, k = tid & 63, K = st->K;
    const bool active = wave < 2 && k < K;
    const int wb = (a.specPar & 1) ^ 1;
    int bad = 0;
    if (active) {
        const double adv2 = 2.0 * (st->snapFc[k] * st->T) + st->snapRcEnd[k];
        const double cp2 = st->snapCpElaEnd[k] + floor(adv2 / kLCA), rc2 = wrap_pos(adv2, (double)kLCA);
        const double tx0 = st->snapCpRefTOW[k] + ((cp2 - st->snapCpRef[k]) * kTCA) + (rc2 / kFCA);
        double wE = st->specWE[wave][k], wM = st->specWM[wave][k];
        int wOk = st->specWOk[wave][k];
        double out[8];
        bad = sat_state_warm(st->ephC[k], tx0 + (wave == 1 ? kChmH : 0.0), out, wE, wM, wOk);
        for (int i = 0; i < 8; ++i) st->specSat[wb][wave][k][i] = out[i];
        st->specWE[wave][k] = wE; st->specWM[wave][k] = wM; st->specWOk[wave][k] = wOk;
        if (wave == 0) { st->specTx[wb][k] = tx0; st->specOk[wb][k] = bad ? 0 : 1; }
    }
    __syncthreads();
    if (active && wave == 1 && bad) st->specOk[wb][k] = 0;   // (behind wave 0's store: both waves of a channel run in this block)
}

__global__ __launch_bounds__(256) static void chm_k2_kernel(ChmKArgs a) { chm_k2(a); }

}  // namespace dpe
#endif  // __HIPCC__
