// dpe_chm_dev.h -- the device-resident channel manager's measurement kernel chm_k1 (cudarecv/modules/src/cuchanmgr.cu:380-447 with
// BCM_MakePosMeas / MakeVelMeas and cuEKF inside it), on top of the pieces it shares: the orbit arithmetic (dpe_sat.h), the channel
// manager's arithmetic, which the host form dpe_chm_* uses too (dpe_chm_arith.h), the filter's device form (dpe_ekf_dev.h) and the
// loop's state, ports, arguments and time update chm_k2 / chm_k3 (dpe_chm_k2.h), which the stage-1 kernels of dpe_bcs.hip carry as
// extra blocks of their launch.  dpe_chanmgr.hip includes this header and so has all of it.
#pragma once
#include "dpe_common.h"
#include "dpe_prep.h"
#include "dpe_bcm_moments_cov.h"
#include "dpe_sat.h"
#include "dpe_chm_arith.h"
#include "dpe_ekf_dev.h"
#include "dpe_chm_k2.h"

#ifdef __HIPCC__
namespace dpe {

// Point `index` (global) of a tensor grid given by its axes (x [dim0], y [dim1], z [dim2], t [dim3] back to back)
__device__ inline const double *axes_point(const double *ax, const int dim[4], long long index, double out[4])
{
    const double *a[4] = {ax, ax + dim[0], ax + dim[0] + dim[1], ax + dim[0] + dim[1] + dim[2]};
    for (int c = 3; c >= 0; --c) {
        out[c] = a[c][index % dim[c]];
        index /= dim[c];
    }
    return out;
}

// The same point into `out` whichever form the grid has: axes (ax set; index local + off) or a point list (row `local` of grid)
__device__ __forceinline__ void chm_point(const double *ax, const int (&dim)[4], const double *grid, long long local, long long off, double (&out)[4])
{
    if (ax) {
        long long index = local + off;
        const double *a3 = ax + dim[0] + dim[1] + dim[2], *a2 = ax + dim[0] + dim[1], *a1 = ax + dim[0];
        out[3] = a3[index % dim[3]]; index /= dim[3];
        out[2] = a2[index % dim[2]]; index /= dim[2];
        out[1] = a1[index % dim[1]]; index /= dim[1];
        out[0] = ax[index % dim[0]];
    } else {
        out[0] = grid[4 * local]; out[1] = grid[4 * local + 1]; out[2] = grid[4 * local + 2]; out[3] = grid[4 * local + 3];
    }
}

// The manifold moments' share of the measurement kernel (dpe_chm_dev_set_measurement_cov): where the partial sums of
// the moments launch behind the scan lie, the grid's quantisation floor, and the ring of R records (device memory)
struct ChmCovArgs {
    const double *partial;          // [2][nBlk][kMomSlots]: the blocks of a row are added here, in block order (bcm_moments_finish_kernel's)
    int nBlk, split[2];
    float rho[2];
    const double *sums;             // the two-launch form: bcm_moments_finish_kernel ran in front and left the sums [2][15] and the
    const long long *nAbove;        //   counts [2] here; nullptr: this kernel adds the partials itself (the fold, the form in use)
    double floorVar[2][4];          // (E, N, U, t) quantisation variance of the position and the velocity grid
    dpe_rval_record *ring;          // device memory, ringDepth records (the fix ring's depth)
    int ringDepth;
};
constexpr int kMomFold = 32;     // block partials a lane of chm_k1_cov_kernel has in flight while it adds a row's blocks in order
struct ChmCovLds {
    double mom[32];                 // the 2 x 15 sums, then the two counts as integers
    double R[64];
    int fall;                       // bit m: block m of R fell back to the identity
};

// COV (chm_k1_cov_kernel): the filter runs on the R of the window's manifold moments; cv and lds are read in that form only
template <bool COV>
__device__ static inline void chm_k1(const ChmKArgs &a, const ChmCovArgs &cv, ChmCovLds *lds)
{
    __shared__ double sX1[8], sXk[8], sZ[8];   // x_k|k, x_k+1|k, the measurement
    __shared__ double sEkf[kEkfDevScratch];
    __shared__ int sPiv[8];
    __shared__ int sFlags;
    ChmDevState *st = a.st;
    const int k = threadIdx.x, K = st->K;
    const double rxTime = st->rxTime, T = st->T;
    const int ds = st->dopplerSign;
    if (k == 0) sFlags = 0;
    DPE_EKF_STAMP(0);
    EkfPre ekfPre{};
    if (a.meas && a.ekf) ekfPre = ekf_dev_prefetch(a.ekf);
    double momV = 0.0;   // COV, lanes 0 .. 29: sum (manifold k / 15, slot k % 15); lanes 30 / 31: the count of manifold 0 / 1, as an integer
    if constexpr (COV) {
        // requested here, beside the keys and the filter's operands: the row's block partials in block order -- the order and the
        // operations of bcm_moments_finish_kernel, so sums and counts carry the bits dpe_bcm_moments gives
        if (k < 32) {
            const int m = k < 30 ? k / kMomSums : k - 30, j = k < 30 ? k - m * kMomSums : kMomSums;
            if (cv.sums) {
                momV = k < 30 ? cv.sums[k] : __longlong_as_double(cv.nAbove[m]);
            } else {
                // (bcm_moments_finish_kernel's a = p[0]; a += p[b] and n += count[b], with the loads of kMomFold blocks in flight at a time:
                //  one block per round trip to device memory made this loop the kernel -- 128 blocks per row at 25^4)
                const double *p = cv.partial + (size_t)m * cv.nBlk * kMomSlots + j;
                const int split = m ? cv.split[1] : cv.split[0];   // (selects: no indexed kernel argument)
                double v = 0.0;
                long long n = 0;
                for (int b0 = 0; b0 < split; b0 += kMomFold) {
                    double t[kMomFold];
#pragma unroll
                    for (int i = 0; i < kMomFold; ++i) t[i] = b0 + i < split ? p[(size_t)(b0 + i) * kMomSlots] : 0.0;
#pragma unroll
                    for (int i = 0; i < kMomFold; ++i) {
                        if (b0 + i < split) {
                            v = b0 + i == 0 ? t[i] : v + t[i];
                            n += __double_as_longlong(t[i]);
                        }
                    }
                }
                momV = k < 30 ? v : __longlong_as_double(n);
            }
            lds->mom[k] = momV;
        }
        lds->R[k] = 0.0;
        if (k == 0) lds->fall = 0;
    }
    Chan c;
    if (k < K) c = st->ch[k];
    double z[8];
    unsigned long long kp = 0ull, kv = 0ull;
    long long ip = 0, iv = 0;
    int measBad = 0;
    if (k == 63) {
        if (a.meas) {
            // ML grid points -> ECEF measurement about the grid centre and with the ENU matrix the scan of this window used
            // = the ports as the previous window's chm_k2 left them
            kp = a.keys[0]; kv = a.keys[1];
            ip = (long long)(0xFFFFFFFFu - (unsigned)(kp & 0xFFFFFFFFull)) - a.posOff;
            iv = (long long)(0xFFFFFFFFu - (unsigned)(kv & 0xFFFFFFFFull)) - a.velOff;
            if (kp == 0ull || ip < 0 || ip >= a.posG) { measBad = 4; ip = 0; }
            if (kv == 0ull || iv < 0 || iv >= a.velG) { measBad = 4; iv = 0; }
            double gAx[4], vAx[4];   // (grid axes: the point decoded from its global index)
            const double *g, *v;
            if constexpr (COV) {   // (the same doubles, by value: a pointer that is either the list's row or a local array keeps the array in scratch)
                chm_point(a.posAx, a.posDim, a.posGrid, ip, a.posOff, gAx);
                chm_point(a.velAx, a.velDim, a.velGrid, iv, a.velOff, vAx);
                g = gAx; v = vAx;
            } else {
                g = a.posAx ? axes_point(a.posAx, a.posDim, ip + a.posOff, gAx) : a.posGrid + 4 * ip;
                v = a.velAx ? axes_point(a.velAx, a.velDim, iv + a.velOff, vAx) : a.velGrid + 4 * iv;
            }
            const double *R = a.p.enu2ecef, *cc = a.p.xkk1;
            {
#pragma clang fp contract(off)   // (the host form's BCM_MakePosMeas / MakeVelMeas run without fused multiply-adds: the same doubles here)
                z[0] = R[0] * g[0] + R[1] * g[1] + R[2] * g[2] + cc[0];   // :1990-1999
                z[1] = R[3] * g[0] + R[4] * g[1] + R[5] * g[2] + cc[1];
                z[2] = R[6] * g[0] + R[7] * g[1] + R[8] * g[2] + cc[2];
                z[3] = g[3] + cc[3];
                z[4] = R[0] * v[0] + R[1] * v[1] + R[2] * v[2] + cc[4];   // :2042-2051
                z[5] = R[3] * v[0] + R[4] * v[1] + R[5] * v[2] + cc[5];
                z[6] = R[6] * v[0] + R[7] * v[1] + R[8] * v[2] + cc[6];
                z[7] = v[3] + cc[7];
            }
            if (measBad) {   // no valid score this window: hold the state (and say so)
                for (int i = 0; i < 8; ++i) z[i] = cc[i];
                atomicOr(&sFlags, measBad);
            }
            for (int i = 0; i < 8; ++i) { sX1[i] = z[i]; sXk[i] = z[i]; sZ[i] = z[i]; a.p.zVal[i] = z[i]; }   // EKF_PassMeas: z to both state ports (below)
        }
    }
    if (a.meas && a.ekf) {   // EnableEKF = true: StepUpdate + StepPredict on the measurement (block-uniform branch; all 64 lanes work)
        __syncthreads();
        DPE_EKF_STAMP(1);
        bool ok;
        if constexpr (COV) {
            // R from the sums, in the frame the measurement was formed in (the ports as the previous window's chm_k2 left them): one
            // lane per manifold, dpe_bcm_moments_rval's own function.  No measurement: the state is held and the moments are not used
            // (the record then carries the sums and an R of zeros).
            if (sFlags == 0 && k < 2) {
                double blk[16], fv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) fv[i] = k ? cv.floorVar[1][i] : cv.floorVar[0][i];
                if (mom_rval_block(lds->mom + kMomSums * k, a.p.enu2ecef, fv, blk)) atomicOr(&lds->fall, 1 << k);
#pragma unroll
                for (int i = 0; i < 16; ++i) lds->R[(4 * k + (i >> 2)) * 8 + 4 * k + (i & 3)] = blk[i];
            }
            __syncthreads();
            ok = sFlags == 0 && ekf_dev_step<true>(a.ekf, ekfPre, sZ, sEkf, sPiv, lds->R);
        } else {
            ok = sFlags == 0 && ekf_dev_step<false>(a.ekf, ekfPre, sZ, sEkf, sPiv, nullptr);
        }
        __syncthreads();
        if constexpr (COV) {
            // the window's record: plain stores to device memory (dpe_chm_dev_rval copies it out behind the stream)
            const unsigned long long seq = (unsigned long long)(st->window + 1);
            dpe_rval_record *rr = cv.ring + (long long)(seq - 1ull) % cv.ringDepth;
            rr->R[k] = lds->R[k];
            if (k < 30) {
                rr->sums[k / kMomSums][k % kMomSums] = momV;
            } else if (k < 32) {
                const int m = k - 30;
                rr->nAbove[m] = __double_as_longlong(momV);
                rr->threshold[m] = __fmul_rn(m ? cv.rho[1] : cv.rho[0], __uint_as_float((unsigned int)(a.keys[m] >> 32)));   // (mom_tau's multiply)
            } else if (k == 32) {
                rr->fallback = lds->fall;
                rr->reserved = 0;
                rr->seq = seq;
            }
        }
        if (k < 8) {
            if (ok) { sX1[k] = sEkf[kEkfDevX1 + k]; sXk[k] = sEkf[kEkfDevXk + k]; }
            else { sX1[k] = a.p.xkk1[k]; sXk[k] = a.p.xkk1[k]; }   // (no measurement, or S singular: hold the predicted state)
        }
        if (!ok && k == 0 && sFlags == 0) { atomicOr(&sFlags, 32); a.ekf->failed = 1; }
        if constexpr (COV) {
            if (k == 0 && lds->fall) atomicOr(&sFlags, 128);       // (behind the test above: bit 128 does not hold the state)
        }
        DPE_EKF_STAMP(8);
        __syncthreads();
    }
    if (k == 63) {
        if (a.meas) {
            for (int i = 0; i < 8; ++i) { z[i] = sX1[i]; a.p.xk1k1[i] = sX1[i]; a.p.xkk1[i] = sXk[i]; }   // the state ports (cuekf.cu:277-279)
            // the fix for the host: staged in device memory; the chm_k2 behind this kernel (which has time to spare) sends it over
            // the host link -- stores to the pinned ring and the wait for them cost this kernel, which the next window's
            // correlator waits for, ~2 us
            dpe_fix_record *r = a.stage;
            for (int i = 0; i < 8; ++i) r->zVal[i] = z[i];
            r->rxTime = rxTime;
            r->posIndex = (long long)(ip + a.posOff);
            r->velIndex = (long long)(iv + a.velOff);
            r->posOutOfWindow = (long long)a.keys[2];
            r->velOutOfWindow = (long long)a.keys[3];
#if defined(DPE_EXPERIMENTS) && defined(DPE_EKF_STAMPS)
            {   // eight phase lengths in units of 4 shader clocks, 16 bits each
                unsigned long long lo = 0ull, hi = 0ull;
                for (int i = 0; i < 4; ++i) lo |= (((dpe_ekf_stamps[i + 1] - dpe_ekf_stamps[i]) >> 2) & 0xFFFFull) << (16 * i);
                for (int i = 0; i < 4; ++i) hi |= (((dpe_ekf_stamps[i + 5] - dpe_ekf_stamps[i + 4]) >> 2) & 0xFFFFull) << (16 * i);
                r->posOutOfWindow = (long long)lo;
                r->velOutOfWindow = (long long)hi;
            }
#endif
            r->posScore = __uint_as_float((unsigned)(kp >> 32));
            r->velScore = __uint_as_float((unsigned)(kv >> 32));
            r->status = st->status | measBad | (sFlags & (COV ? 32 | 128 : 32));
            r->seq = (unsigned long long)(st->window + 1);
        } else {
            for (int i = 0; i < 8; ++i) {
                const double x1 = a.xk1k1[i], xk = a.xkk1[i];
                sX1[i] = x1; a.p.xk1k1[i] = x1; a.p.xkk1[i] = xk;
            }
        }
    }
    __syncthreads();
    if (k < K && a.mode == 1) {   // measurement update (CHM_PropagateChannels :380-447)
        double bcFi, bcFc;
        meas_update(c, sX1, rxTime, T, ds, bcFi, bcFc);
        c.fi = bcFi;
        c.fc = bcFc;
        st->ch[k].fi = bcFi;
        st->ch[k].fc = bcFc;
    }
    if (k < K) {   // what chm_k3 needs of the channel (it runs beside chm_k2, which rewrites ch[])
        st->snapFc[k] = c.fc; st->snapRcEnd[k] = c.rcEnd;
        st->snapCpElaEnd[k] = c.cpElaEnd; st->snapCpRef[k] = c.cpRef; st->snapCpRefTOW[k] = c.cpRefTOW;
    }
    if (k < K && a.bcsChan) {   // the next window starts where this one ended: rcEnd, riEnd, cpElaEnd with the new frequencies
        int bad;
        const BcsChanDev d = bcs_prep_one(c.rcEnd, c.riEnd, c.fc, c.fi, c.cpElaEnd, c.cpRef, c.prn, a.fs, a.S, bad);
        a.bcsChan[k] = d;
        if (a.hintL1 > 0 && hint_broken(d, a.hintL1, a.hintStepMax)) {   // (the prepared form launches no prep kernel: the promise is checked here)
            bad |= 8;
            __hip_atomic_store(a.hintViol, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        if (bad) atomicOr(&sFlags, bad << 3);
    }
    __syncthreads();
    if (k == 0) {
        if (sFlags) st->status |= sFlags;
        if (a.bcsStatus) {   // BatchCorrScores' input flags: bits 0, 1 and 3 replaced; bit 2 (the batch kernels' own) and the sticky bit 4 kept, as bcs_prep_kernel does
            const int v = (int)((sFlags >> 3) & 11u);
            const int old = *a.bcsStatus;          // (one thread, stream order: nothing else writes the word while this kernel runs)
            if ((old & ~11) != old || v) *a.bcsStatus = (old & ~11) | v;
        }
    }
}

__global__ __launch_bounds__(64) static void chm_k1_kernel(ChmKArgs a) { chm_k1<false>(a, ChmCovArgs{}, nullptr); }
// the measurement kernel of a loop with dpe_chm_dev_set_measurement_cov: behind bcm_moments_kernel (the fold), or behind that and
// bcm_moments_finish_kernel (cv.sums set)
__global__ __launch_bounds__(64) static void chm_k1_cov_kernel(ChmKArgs a, ChmCovArgs cv)
{
    __shared__ ChmCovLds lds;
    chm_k1<true>(a, cv, &lds);
}

}  // namespace dpe
#endif  // __HIPCC__
