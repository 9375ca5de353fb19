// dpe_bcs.hip -- BatchCorrScores for MI355X (gfx950): int16 I/Q -> windowed code-lag bank +
// windowed Doppler-bin bank per SV, for a batch of windows.
//
// Replaces the reference chain  BCS_Load -> thrust::reduce(mean) -> BCS_ComputeDopplerWipeoff
// -> BCS_ComputeCodeReplica -> 5x cufftExecZ2Z(S) -> BCS_ChooseCodeCorr -> fftshift ->
// BCS_SubtractDCOffset -> BCS_ChoosyBatchMultiplyAndPad -> cufftExecZ2Z(C) -> fftshift
// (cudarecv/modules/src/batchcorrscores.cu:1043-1180) by ONE streaming pass over the samples:
//
//   code bank   corr[l] = sum_n b[n] r[(n-l) mod S]         (== ifft(conj(fft r) fft b), :1099-1144)
//               for the lags l in [-L,+L] the manifold grid can reach, split at the nav-bit
//               boundary (X: replica index < idxNext, Y: >=) so that no-flip = X+Y, flip = X-Y;
//   carr bank   F[b] = sum_n c[n] exp(-j 2 pi n b / C)      (== zero-padded FFT bin b, :1179)
//               for bins b in [-B,+B], from per-256-sample power moments M_p = sum x^p c[n]
//               (x = n - block centre) and a degree-5 Taylor factor per block -- exact to
//               (2 pi 127.5 B / C)^6 / 720 (checked at create), ~15x fewer flops than direct.
//
// Data layout (HBM): samples int16 I,Q interleaved, read once per SV with 16-byte lane loads;
// chip table int8 [37][1024] -> LDS per block; replica +/-1 (nav-bit side masked) per wave
// sub-tile in LDS; per-block partial lag sums and per-sub-tile moments in global scratch,
// reduced in fixed order (no float atomics: bit-reproducible run to run).
#include <type_traits>

#include "dpe_common.h"
#include "dpe_bcs_plan.h"   // the launch plan and its constants (kSub, kSumSlots, kPass, ...): plain C++
#include "dpe_prep.h"
#include "dpe_chm_k2.h"    // chm_k2 / chm_k3: the device-resident channel manager's time update, carried as extra blocks (FUSE form)
#include "dpe_bcs_pieces.h"   // what the forms of stage 1 share: cmul, wipe_seed, phases, BcsParamBlock, window_mean, replica / store pieces

namespace dpe {

// ------------------------------------------------------------------------------------------
// DC sum (thrust::reduce at batchcorrscores.cu:1065): exact int64 sums.  Each block writes its own slot
// sums[w][blockIdx.x][2] (no atomics, nothing to zero beforehand -- the whole Update stays free of memset
// nodes, which matters for the hipGraph replay); consumers add the <= kSumSlots slots (window_mean).
__device__ __forceinline__ void sum_body(const int16_t *__restrict__ iq, long long winStride, int S, long long *__restrict__ sums)
{
    const int w = blockIdx.y;
    const int *x = reinterpret_cast<const int *>(iq + (size_t)w * winStride * 2);
    int sI = 0, sQ = 0;  // each thread sums < 64k samples: no int32 overflow
    const int gtid = blockIdx.x * blockDim.x + threadIdx.x, gsz = gridDim.x * blockDim.x;
    if (((reinterpret_cast<uintptr_t>(x)) & 15) == 0) {
        const int4 *x4 = reinterpret_cast<const int4 *>(x);
        const int n4 = S >> 2;
        for (int n = gtid; n < n4; n += gsz) iq_add4(sI, sQ, x4[n]);
        for (int n = (n4 << 2) + gtid; n < S; n += gsz) iq_add(sI, sQ, x[n]);
    } else {
        for (int n = gtid; n < S; n += gsz) iq_add(sI, sQ, x[n]);
    }
    long long tI = sI, tQ = sQ;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        tI += __shfl_xor(tI, off, 64);
        tQ += __shfl_xor(tQ, off, 64);
    }
    __shared__ long long sW[4][2];
    if ((threadIdx.x & 63) == 0) { sW[threadIdx.x >> 6][0] = tI; sW[threadIdx.x >> 6][1] = tQ; }
    __syncthreads();
    if (threadIdx.x < 2) {
        long long *o = sums + ((size_t)w * kSumSlots + blockIdx.x) * 2;
        o[threadIdx.x] = sW[0][threadIdx.x] + sW[1][threadIdx.x] + sW[2][threadIdx.x] + sW[3][threadIdx.x];
    }
}

// (upDst / upSrc / upN16: the batch's channel parameters ride along -- the blocks copy the pinned staging block to the device,
//  one launch boundary less than a separate upload kernel; upN16 = 0: nothing to copy)
__global__ __launch_bounds__(256) void bcs_sum_kernel(const int16_t *__restrict__ iq, long long winStride, int S,
                                                      long long *__restrict__ sums, uint4 *__restrict__ upDst,
                                                      const uint4 *__restrict__ upSrc, int upN16)
{
    const int nThreads = gridDim.x * gridDim.y * 256;
    for (int i = (blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x; i < upN16; i += nThreads) upDst[i] = upSrc[i];
    sum_body(iq, winStride, S, sums);
}

}  // namespace dpe

#include "dpe_bcs_bank.h"   // the per-sample forms: dense, batch (16 samples per lane) and wide
#include "dpe_bcs_chip.h"   // chip-boundary form of stage 1 (high sampling rates)
#include "dpe_bcs_chip2.h"  // second form: lanes <-> chips in the prefix stage too (16 .. 25 samples per chip)
#include "dpe_bcs_fft.h"    // full-length FFT form (fallback for very wide lag / bin windows)

namespace dpe {

// ------------------------------------------------------------------------------------------
// blockIdx.x == 0: code bank (+ replica choice); blockIdx.x >= 1: 64 Doppler bins each.
// momLen = samples per moment block (kSub for the per-sample kernels, kPass for the chip kernel); nValid = entries of a
// block partial that hold lags (65, or 64 for the chip kernel whose lanes cover lagShift - 32 .. lagShift + 31).
// (batch form with 4 moments: held to 128 registers = four blocks per CU -- the kernel is a chain of latencies, 0.033 -> 0.030 ms at R)
// (NG = bin groups a block walks: 1 for the split shape, the handle's group count for the fat one -- the per-group registers of
//  unused groups made the 4-moment batch form spill 28 bytes under its 128-register bound)
template <int kNMom, bool FUSE, int NG>
__global__ __launch_bounds__(256, (kNMom == 4 && !FUSE) ? 4 : 1) void bcs_finalize_kernel(BcsParamBlock pb, int inl, int S, int K, int nSub, int nBlk, int LH, int L, int B, int wide, int lagShift,
                                                           int momLen, int nValid, long long C, const BcsChanDev *__restrict__ chan,
                                                           const float2 *__restrict__ part,
                                                           const float2 *__restrict__ mom,
                                                           float2 *__restrict__ codeBank, float2 *__restrict__ carrBank,
                                                           int *__restrict__ info, int maxK,
                                                           const float2 *__restrict__ momRep,     // fuse: moments of wipe x replica
                                                           const long long *__restrict__ sums, int nSumBlk)
{
    const int k = blockIdx.y, w = blockIdx.z, tid = threadIdx.x;
    const int NL = 2 * LH + 1;
    if (rerun_not_wanted(pb)) return;
    const BcsChanDev ch = params_ptr(chan, inl)[w * K + k];
    const float2 *pp = part + ((size_t)w * K + k) * nBlk * 2 * NL;
    constexpr int kChunk = 256;         // sub-tiles staged in LDS at a time
    __shared__ float2 sXY[2 * 65];      // [side][lag] totals of the per-block partials (NL <= 65)
    __shared__ float2 sTmp[256];
    __shared__ float2 sRed[16][16];
    __shared__ float2 sMom[kChunk * kNMom];   // flip-combined moments of the current chunk
    // A single window keeps only a few of these blocks in flight, so the kernel is a chain of memory
    // latencies: every stage issues ALL of its loads before consuming any.  Doppler blocks fetch their
    // first chunk of moments up front, under the partial-sum stage.
    // Two launch shapes: gridDim.x = 1 + nBinBlk (block 0: code bank, block 1+g: Doppler bins 16g..16g+15) for a few
    // windows, where more blocks mean a shorter latency chain; gridDim.x = 1 ("fat": one block per (window, SV)
    // does the code bank and then ALL bin groups from one staging of the moments) for batches, where the
    // redundant partial sums / moment reads of the split shape cost more than they hide.
    // lagShift != 0: a further chunk of a lag window wider than +-32 (one block per (window, SV): partial sums and
    // code-bank entries only; the replica choice was made by the lagShift == 0 launch and is read back from info[])
    const bool fat = gridDim.x == 1 && lagShift == 0;
    const bool carrBlk = lagShift == 0 && (fat || blockIdx.x != 0);
    const float2 *m0 = mom + (((size_t)w * K + k) * 2) * nSub * kNMom;
    const float2 *m1 = m0 + (size_t)nSub * kNMom;
    // fuse (single windows): the stage-1 kernel stored M_p[raw w r] in mom and M_p[w r] in momRep; the DC mean comes
    // from the per-block sample sums it left in `sums`:  M_p[(raw - mean) w r] = M_p[raw w r] - mean * M_p[w r]
    const float2 *q0 = momRep + (((size_t)w * K + k) * 2) * nSub * kNMom;
    const float2 *q1 = q0 + (size_t)nSub * kNMom;
    float mRe = 0.f, mIm = 0.f;
    if (FUSE) window_mean(sums, w, nSumBlk, S, mRe, mIm);
    float2 r0[kNMom], r1[kNMom], s0[FUSE ? kNMom : 1], s1[FUSE ? kNMom : 1];
    auto load_chunk = [&](int c0) {
        const int n = (nSub - c0 < kChunk ? nSub - c0 : kChunk) * kNMom;
#pragma unroll
        for (int i = 0; i < kNMom; ++i) {
            const int idx = tid + 256 * i;
            const bool ok = idx < n;
            r0[i] = ok ? m0[(size_t)c0 * kNMom + idx] : make_float2(0.f, 0.f);
            r1[i] = ok ? m1[(size_t)c0 * kNMom + idx] : make_float2(0.f, 0.f);
            if (FUSE) {
                s0[i] = ok ? q0[(size_t)c0 * kNMom + idx] : make_float2(0.f, 0.f);
                s1[i] = ok ? q1[(size_t)c0 * kNMom + idx] : make_float2(0.f, 0.f);
            }
        }
    };
    if (carrBlk) load_chunk(0);
    {
        // fixed-order two-level sum (bit-reproducible, identical in every block): T threads per
        // (side, lag) pair each add a strided subset of the blocks, then one thread adds the T partials
        const int pairs = 2 * NL;
        int np2 = 1;
        while (np2 < pairs) np2 <<= 1;
        const int T = 256 / np2;                     // pairs <= 130 -> T >= 1
        const int pair = tid / T, sub = tid - pair * T;
        // (compensated: a window's lag sums reach ~1e7 while a block partial is ~1e5 -- added plainly, a few hundred partials cost
        //  the total 4e-7 of its value; the third chip form writes one partial per group of tiles)
        float2 acc = make_float2(0.f, 0.f), comp = make_float2(0.f, 0.f);
        if (pair < pairs) {
            const int side = pair / NL, lag = pair - side * NL;
            for (int b0 = sub; b0 < nBlk; b0 += 8 * T) {
                float2 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int bq = b0 + u * T;
                    v[u] = bq < nBlk ? pp[(size_t)(bq * 2 + side) * NL + lag] : make_float2(0.f, 0.f);
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {   // Kahan steps (no fast-math in this build: the compiler keeps them)
                    const float yx = v[u].x - comp.x, yy = v[u].y - comp.y;
                    const float tx = acc.x + yx, ty = acc.y + yy;
                    comp.x = (tx - acc.x) - yx; comp.y = (ty - acc.y) - yy;
                    acc.x = tx; acc.y = ty;
                }
            }
        }
        sTmp[tid] = acc;
        __syncthreads();
        if (pair < pairs && sub == 0) {
            float2 t = sTmp[tid];
            for (int q = 1; q < T; ++q) { t.x += sTmp[tid + q].x; t.y += sTmp[tid + q].y; }
            sXY[pair] = t;
        }
        __syncthreads();
    }
    if (wide) {   // wide-lag layout: [0] = corr[-LH], [1+i] = step D[-LH+i]  ->  corr[j] by prefix sum
        if (tid < 2) {
            float2 run = sXY[tid * NL];
            for (int j = 1; j < NL; ++j) {
                run.x += sXY[tid * NL + j].x; run.y += sXY[tid * NL + j].y;
                sXY[tid * NL + j] = run;
            }
        }
        __syncthreads();
    }
    // BCS_ChooseCodeCorr :512-516 -- decision at lag 0 only
    const float2 X0 = sXY[LH], Y0 = sXY[NL + LH];
    const float nr0 = X0.x + Y0.x, ni0 = X0.y + Y0.y, fr0 = X0.x - Y0.x, fi0 = X0.y - Y0.y;
    const int noFlip = lagShift == 0 ? ((!ch.hasFlip) || (nr0 * nr0 + ni0 * ni0 > fr0 * fr0 + fi0 * fi0)) : info[w * K + k];
    const float sgn = noFlip ? 1.f : -1.f;

    if (blockIdx.x == 0) {
        if (tid == 0 && lagShift == 0) info[w * K + k] = noFlip;
        for (int jj = tid; jj < NL; jj += 256) {
            const int lag = lagShift + jj - LH;        // this chunk holds the lags lagShift - LH .. lagShift + LH
            if (lag < -L || lag > L || jj >= nValid) continue;
            const float2 X = sXY[jj], Y = sXY[NL + jj];
            codeBank[((size_t)w * maxK + k) * (2 * L + 1) + lag + L] = make_float2(X.x + sgn * Y.x, X.y + sgn * Y.y);
        }
        if (!fat) return;
    }
    // ---- Doppler bins: F[b] = sum_sub tw(sub,b) * sum_p (-j theta)^p / p! * M_p[sub]
    // 16 bins per group, 16 thread groups striding the sub-tiles; a fat block walks all bin groups per chunk
    constexpr int kMaxFatGroups = NG;
    const int nGroups = (2 * B + 1 + 15) / 16;
    const int gFirst = fat ? 0 : (int)blockIdx.x - 1, gCount = fat ? nGroups : 1;   // host: fat only if nGroups <= kMaxFatGroups
    const int grp = tid >> 4;
    const float invC = 1.0f / (float)C;  // C is a power of two: exact
    const double twoPiOverC = 6.283185307179586476925286766559 / (double)C;   // exact scaling of 2 pi (power of two)
    float2 F[kMaxFatGroups];
    float theta[kMaxFatGroups], stepS[kMaxFatGroups], stepC[kMaxFatGroups], sn[kMaxFatGroups], cs[kMaxFatGroups];
    bool live[kMaxFatGroups];
    int bb[kMaxFatGroups];
#pragma unroll
    for (int g = 0; g < kMaxFatGroups; ++g) {
        const int bi = (gFirst + g) * 16 + (tid & 15);  // bank entry
        bb[g] = bi - B;
        live[g] = g < gCount && bi < 2 * B + 1;
        F[g] = make_float2(0.f, 0.f);
        theta[g] = (float)((double)bb[g] * twoPiOverC);
        // centre twiddle exp(-j 2 pi n_c b / C), n_c = momLen sub + (momLen - 1) / 2: exact (integer-reduced phase +
        // sincospif) every 8th step of this thread, one complex rotation by exp(-j 2 pi 16 momLen b / C) between
        stepS[g] = 0.f; stepC[g] = 1.f; sn[g] = 0.f; cs[g] = 1.f;
        if (live[g]) {
            // (C = 8 next_pow2(S) is a power of two: the reduction mod 2C is a mask -- a 64-bit `%` by a run-time value costs
            // some 300 instructions per call and was 60 % of this kernel)
            const long long ts = ((long long)(32 * momLen) * (long long)bb[g]) & (2 * C - 1);   // 2 * (16 * momLen) b  (phase unit: pi / C)
            sincospif((float)ts * invC, &stepS[g], &stepC[g]);
        }
    }
    int it = 0;
    for (int c0 = 0; c0 < nSub; c0 += kChunk) {
        if (c0) {
            __syncthreads();   // the previous chunk is fully consumed
            load_chunk(c0);
        }
#pragma unroll
        for (int i = 0; i < kNMom; ++i) {
            float ax = fmaf(sgn, r1[i].x, r0[i].x), ay = fmaf(sgn, r1[i].y, r0[i].y);
            if (FUSE) {
                const float qx = fmaf(sgn, s1[i].x, s0[i].x), qy = fmaf(sgn, s1[i].y, s0[i].y);
                ax = fmaf(-mRe, qx, fmaf(mIm, qy, ax));
                ay = fmaf(-mRe, qy, fmaf(-mIm, qx, ay));
            }
            sMom[tid + 256 * i] = make_float2(ax, ay);
        }
        __syncthreads();
        const int cEnd = nSub - c0 < kChunk ? nSub - c0 : kChunk;
        for (int sl = grp; sl < cEnd; sl += 16, ++it) {   // kChunk is a multiple of 16: the stride continues across chunks
            const int sub = c0 + sl;
            const float2 *a = sMom + sl * kNMom;
#pragma unroll
            for (int g = 0; g < kMaxFatGroups; ++g) {
                if (!live[g]) continue;
                float ar = a[kNMom - 1].x, ai = a[kNMom - 1].y;
#pragma unroll
                for (int p = kNMom - 1; p >= 1; --p) {
                    const float sc = theta[g] * (1.0f / (float)p);   // (constant reciprocals: no division sequence in the loop set-up)
                    const float mr = a[p - 1].x, mi = a[p - 1].y;
                    const float nr = fmaf(sc, ai, mr);
                    ai = fmaf(-sc, ar, mi);
                    ar = nr;
                }
                if ((it & 7) == 0) {
                    const long long tt = (((long long)(2 * momLen) * sub + (momLen - 1)) * (long long)bb[g]) & (2 * C - 1);
                    sincospif((float)tt * invC, &sn[g], &cs[g]);  // angle = pi * tt / C
                } else {
                    // (explicit FMAs, here and below: the two launch shapes are different instantiations (NG), and left to the
                    // compiler's contraction their sums would round differently -- the shapes are bit-identical by test)
                    const float nc = fmaf(cs[g], stepC[g], -(sn[g] * stepS[g]));
                    sn[g] = fmaf(sn[g], stepC[g], cs[g] * stepS[g]);
                    cs[g] = nc;
                }
                // (cs - j sn) * (ar + j ai)
                F[g].x = fmaf(cs[g], ar, fmaf(sn[g], ai, F[g].x));
                F[g].y = fmaf(cs[g], ai, fmaf(-sn[g], ar, F[g].y));
            }
        }
    }
#pragma unroll
    for (int g = 0; g < kMaxFatGroups; ++g) {
        if (g >= gCount) break;   // block-uniform
        if (g) __syncthreads();
        sRed[grp][tid & 15] = F[g];
        __syncthreads();
        if (grp == 0 && live[g]) {
            float2 t = sRed[0][tid];
            for (int q = 1; q < 16; ++q) { t.x += sRed[q][tid].x; t.y += sRed[q][tid].y; }
            carrBank[((size_t)w * maxK + k) * (2 * B + 1) + (gFirst + g) * 16 + tid] = t;
        }
    }
}

// Device-resident channel parameters (dpe_bcs_update_dev): what the host loop of dpe_bcs_update computes per channel, from
// the reference's own port arrays on the device (cuChanMgr's outputs, dpeflow.cpp:169-176; captured once by the reference at
// batchcorrscores.cu:991-1004).  One block; fp64 throughout, expression for expression the host form (bcs_prep_one, dpe_prep.h).
// status: bit 0 = a PRN outside 1..37 (clamped so that the kernels stay inside the chip table), bit 1 = a non-positive code
// frequency / negative code phase (nominal values substituted: the kernels index the chip table with them).
struct BcsPortsDev {
    const double *rc, *ri, *fc, *fi;
    const int *cpEla, *cpRef;
    const unsigned char *prn;
};
// hintL1 > 0 (dpe_bcs_set_dev_hint): the host has chosen the chip kernels from NOMINAL channel values without reading this block back;
// the conditions it could not check are checked here, bit 3 of the status = one of them does not hold (chips of hintL1 or hintL1 + 1
// samples, code step within the assumed bound, 2 pi |fi| <= 0.25 fc, the nav-bit boundary on a chip boundary of the replica).
__global__ void bcs_prep_kernel(BcsPortsDev p, int K, double fs, int S, BcsChanDev *__restrict__ out, int *__restrict__ status, int hintL1,
                                double hintStepMax, int *__restrict__ hintViol)
{
    const int k = threadIdx.x;
    if (k == 0) atomicAnd(status, ~15);   // (bits 0 .. 3 are this kernel's; bits 2 and 4 belong to the batches whose DC sums ride in the stage-1 launch)
    __syncthreads();
    if (k >= K) return;
    int bad;
    const BcsChanDev d = bcs_prep_one(p.rc[k], p.ri[k], p.fc[k], p.fi[k], p.cpEla[k], p.cpRef[k], (int)p.prn[k], fs, S, bad);
    out[k] = d;
    if (hintL1 > 0 && hint_broken(d, hintL1, hintStepMax)) {
        bad |= 8;
        __hip_atomic_store(hintViol, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // (pinned: the host drops the hint at its next call)
    }
    if (bad) atomicOr(status, bad);
}

// Dense export in the reference layout (complex128, fft-shifted rows), zero outside the banks.
__global__ void bcs_export_kernel(const float2 *__restrict__ bank, int n, long long rowLen, long long centre, int K,
                                  int maxK, int half, double2 *__restrict__ dense)
{
    const int k = blockIdx.y;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        const float2 v = bank[(size_t)k * n + j];
        dense[(size_t)k * rowLen + centre - half + j] = make_double2((double)v.x, (double)v.y);
    }
    (void)K; (void)maxK;
}

}  // namespace dpe

// ============================================================================================
struct dpe_bcs {
    dpe_bcs_config cfg;
    dpe::BcsShape sh;   // everything create derives from cfg, the device and the switches (dpe_bcs_plan.h)
    bool havePlans = false;   // full-length FFT fallback (dpe_bcs_fft.h, sh.fftMode)
    dpe::FftPlan planS3, planS2, planC;   // rocFFT: length S, batch 3 chunk K (forward) / 2 chunk K (inverse); length C, batch chunk K
    int planK = 0;        // channels per window the plans are made for (the Update's nChan: re-planned when it changes)
    int fftChunkW = 1;
    float2 *fftWork_d = nullptr;
    int chipDbg = 0;                   // -DDPE_EXPERIMENTS builds only, DPE_BCS_CHIP_DBG: skips parts of the chip kernel (timing; wrong results)
    int8_t *chipTable_d = nullptr;
    uint32_t *chipBits_d = nullptr;   // the same chips as sign bits, periodically extended (bcs_bank_chip2_kernel: scalar loads)
    double *tTable_d = nullptr;   // ns-rounded sample times (always allocated; used only when sh.useTable)
    long long *sums_d = nullptr;
    unsigned long long *rideWord_d = nullptr;   // [maxWindows][kSumSlots] {epoch, I, Q} words of the sums computed inside the chip2 launch
    unsigned rideEpoch = 0;                     // cycles 1 .. 3
    int rideW = 0, rideSlots = 0;               // the slot set the last such launch wrote
    int rideSpin = dpe::kRideSpinDefault;       // polls after which a correlator block sums its window itself (DPE_BCS_RIDE_SPIN; tests force 1)
    dpe::BcsChanDev *chan_d = nullptr;
    // pinned parameter staging: a ring of kStaging blocks, each guarded by an event recorded once its H2D copy (or the
    // graph that contains it) has been enqueued -- Updates may be issued kStaging - 1 deep without waiting
    static constexpr int kStaging = 4;
    dpe::BcsChanDev *chanBase_h = nullptr, *chan_h = nullptr, *chanBase_hd = nullptr;   // _hd: the pinned block's device address
    hipEvent_t stagingFree[kStaging] = {};
    int slot = 0;
    float2 *part_d = nullptr, *mom_d = nullptr, *momRep_d = nullptr, *codeBank_d = nullptr, *carrBank_d = nullptr;
    int *info_d = nullptr;
    int lastW = 0, lastK = 0, lastSumBlocks = 1;
    bool lastDev = false;              // the last Update took its channel parameters from device arrays (dpe_bcs_update_dev)
    int *status_d = nullptr;           // that form's input check, written by bcs_prep_kernel
    const char *lastKernel = "";   // stage-1 kernel of the last Update (dpe_bcs_stage1_kernel)
    dpe::ChmKArgs co{};            // a task of the device-resident channel manager for the next stage-1 launch (dpe_bcs_cotask_set)
    bool coPending = false;
    dpe_owner_detach_fn ownerDetach = nullptr;   // an attached device-resident channel manager: told first when this handle is destroyed
    void *owner = nullptr;
    int devHint = 0;               // dpe_bcs_set_dev_hint: bit 0 = the caller promises the chip kernels' conditions for the device-parameter form
    int *hintViol_h = nullptr, *hintViol_hd = nullptr;   // pinned word a device-side check raises when the promise did not hold: the hint is then dropped
    std::vector<int32_t> idxNext_h;
    dpe::KernelProfiler prof;  // slots: 0 sum, 1 bank, 2 finalize
    dpe::GraphCache graphs;
};

// The environment switches of dpe_hip.h, read once per create.
static dpe::BcsSwitches bcs_read_switches()
{
    dpe::BcsSwitches sw;
    const auto num = [](const char *name) { const char *e = getenv(name); return e ? atoi(e) : 0; };
    sw.forceFft = getenv("DPE_BCS_FORCE_FFT") != nullptr;
    sw.noBank16 = getenv("DPE_BCS_NO_BANK16") != nullptr;
    sw.noFuse = getenv("DPE_BCS_NO_FUSE") != nullptr;
    sw.noChip = getenv("DPE_BCS_NO_CHIP") != nullptr;
    sw.noChip2 = getenv("DPE_BCS_NO_CHIP2") != nullptr;
    sw.noSumRide = num("DPE_BCS_NO_SUMRIDE") != 0;
    sw.sumRideMin = num("DPE_BCS_SUMRIDE_MIN");
    sw.chip2P = num("DPE_BCS_CHIP2_P");
    sw.chipTpb = num("DPE_BCS_CHIP_TPB");
    sw.tpb16 = num("DPE_BCS_TPB16");
#ifdef DPE_EXPERIMENTS   // ablation switches: never in the product library
    sw.noWide = getenv("DPE_BCS_NO_WIDE") != nullptr;
    sw.rideLA = num("DPE_BCS_RIDE_LA");
    if (const char *e = getenv("DPE_BCS_FAT")) sw.fat = e[0] == '1' ? 1 : 0;
#endif
    return sw;
}

extern "C" {

int dpe_bcs_create(const dpe_bcs_config *cfg, dpe_bcs **out)
{
    using namespace dpe;
    DPE_REQUIRE(cfg && out, "[BatchCorrScores] create: null argument");
    DPE_REQUIRE(cfg->samplesPerWindow >= 1024, "[BatchCorrScores] create: samplesPerWindow %d < 1024", cfg->samplesPerWindow);
    DPE_REQUIRE(cfg->samplingFrequency > 0, "[BatchCorrScores] create: bad samplingFrequency");
    DPE_REQUIRE(cfg->maxWindows >= 1 && cfg->maxChannels >= 1 && cfg->maxChannels <= DPE_MAX_CHAN,
                "[BatchCorrScores] create: maxWindows/maxChannels out of range");
    DPE_REQUIRE(cfg->lagHalfWidth >= 1 && 2 * (long long)cfg->lagHalfWidth + 1 < cfg->samplesPerWindow,
                "[BatchCorrScores] create: lagHalfWidth %d not in [1, S/2)", cfg->lagHalfWidth);
    DPE_REQUIRE(cfg->binHalfWidth >= 1, "[BatchCorrScores] create: binHalfWidth < 1");
    int dev = 0, cus = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    BcsShape sh = bcs_shape(*cfg, bcs_read_switches(), cus);
    DPE_REQUIRE(2 * (long long)cfg->binHalfWidth + 1 < sh.C, "[BatchCorrScores] create: binHalfWidth %d not below C/2 = %lld",
                cfg->binHalfWidth, sh.C / 2);
    if (sh.chipOK) {
        int nbChip = 0, nbChip2 = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nbChip, (const void *)bcs_bank_chip_kernel<6>, 64, 0) != hipSuccess) nbChip = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nbChip2, (const void *)bcs_bank_chip2_kernel<6, 24>, 64, 0) != hipSuccess) nbChip2 = 0;
        bcs_shape_residency(sh, nbChip, nbChip2);
    }
    const int S = sh.S;
    const long long C = sh.C;
    const double fs = sh.fs;
    dpe_bcs *h = new dpe_bcs();
    h->cfg = *cfg;
    h->sh = sh;
    const size_t W = cfg->maxWindows, K = cfg->maxChannels;
    std::vector<int8_t> table(37 * 1024, 0);
    for (int prn = 1; prn <= 37; ++prn) gen_ca_code_host(prn, table.data() + (prn - 1) * 1024);
    h->chipTable_d = dev_alloc<int8_t>(table.size());
    std::vector<uint32_t> bitTable((size_t)37 * k2BitWords, 0u);
    for (int prn = 1; prn <= 37; ++prn)
        for (int b = 0; b < 32 * k2BitWords; ++b)
            if (table[(size_t)(prn - 1) * 1024 + b % kLCA] > 0) bitTable[(size_t)(prn - 1) * k2BitWords + (b >> 5)] |= 1u << (b & 31);
    h->chipBits_d = dev_alloc<uint32_t>(bitTable.size());
    {
        std::vector<double> tt(S);
        for (int n = 0; n < S; ++n) tt[n] = std::round(((double)n / fs) * 1.0e9) / 1.0e9;
        h->tTable_d = dev_alloc<double>(S);
        if (h->tTable_d) (void)hipMemcpy(h->tTable_d, tt.data(), sizeof(double) * S, hipMemcpyHostToDevice);
    }
    h->sums_d = dev_alloc<long long>(2 * W * kSumSlots);
    h->rideWord_d = dev_alloc<unsigned long long>(W * kSumSlots);
    if (h->rideWord_d) (void)hipMemset(h->rideWord_d, 0, sizeof(unsigned long long) * W * kSumSlots);
    if (getenv("DPE_BCS_RIDE_SPIN") && atoi(getenv("DPE_BCS_RIDE_SPIN")) >= -1) h->rideSpin = atoi(getenv("DPE_BCS_RIDE_SPIN"));
    h->chan_d = dev_alloc<BcsChanDev>(W * K);
    h->part_d = dev_alloc<float2>(W * K * sh.nBlkAlloc * 2 * (2 * sh.LH + 1));
    h->mom_d = dev_alloc<float2>(W * K * 2 * sh.nSub * kNMomMax);
    h->momRep_d = dev_alloc<float2>(W * K * 2 * sh.nSub * kNMomMax);
    h->codeBank_d = dev_alloc<float2>(W * K * (2 * cfg->lagHalfWidth + 1));
    h->carrBank_d = dev_alloc<float2>(W * K * (2 * cfg->binHalfWidth + 1));
    h->info_d = dev_alloc<int>(W * K);
    h->status_d = dev_alloc<int>(1);
    if (h->status_d) (void)hipMemset(h->status_d, 0, sizeof(int));
    if (hipHostMalloc((void **)&h->hintViol_h, sizeof(int), hipHostMallocDefault) == hipSuccess) {
        *h->hintViol_h = 0;
        (void)hipHostGetDevicePointer((void **)&h->hintViol_hd, h->hintViol_h, 0);
    }
    if (!h->status_d || !h->hintViol_hd || !h->rideWord_d || !h->tTable_d || !h->chipTable_d || !h->chipBits_d || !h->sums_d || !h->chan_d || !h->part_d || !h->mom_d || !h->momRep_d || !h->codeBank_d || !h->carrBank_d ||
        !h->info_d || hipHostMalloc((void **)&h->chanBase_h, dpe_bcs::kStaging * W * K * sizeof(BcsChanDev), hipHostMallocDefault) != hipSuccess) {
        set_error("[BatchCorrScores] create: device allocation failed");
        dpe_bcs_destroy(h);
        return -1;
    }
    const auto finish = [&]() -> int {   // a failure from here on must not leak the handle
        DPE_CHECK_HIP(hipMemcpy(h->chipTable_d, table.data(), table.size(), hipMemcpyHostToDevice));
        DPE_CHECK_HIP(hipMemcpy(h->chipBits_d, bitTable.data(), bitTable.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        DPE_CHECK_HIP(hipMemset(h->codeBank_d, 0, W * K * (2 * cfg->lagHalfWidth + 1) * sizeof(float2)));
        DPE_CHECK_HIP(hipMemset(h->carrBank_d, 0, W * K * (2 * cfg->binHalfWidth + 1) * sizeof(float2)));
        for (hipEvent_t &e : h->stagingFree) DPE_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        DPE_CHECK_HIP(hipHostGetDevicePointer((void **)&h->chanBase_hd, h->chanBase_h, 0));
        if (sh.fftMode) {
            // windows per chunk: at most 2^27 complex work elements (1 GB); planes b, rX, rY of [chunk][K][S], reused as [chunk][K][C]
            const size_t perW = K * (size_t)(3 * (size_t)S > (size_t)C ? 3 * (size_t)S : (size_t)C);
            size_t chunk = ((size_t)1 << 27) / perW;
            if (chunk < 1) chunk = 1;
            if (chunk > W) chunk = W;
            h->fftChunkW = (int)chunk;
            h->fftWork_d = dev_alloc<float2>(chunk * perW);
            DPE_REQUIRE(h->fftWork_d, "[BatchCorrScores] create: FFT work buffer (%zu MB) allocation failed", chunk * perW * 8 >> 20);
            DPE_REQUIRE(C < (1ll << 31), "[BatchCorrScores] create: carrier transform length %lld too long for the FFT path", C);
            // (rows of a short last chunk / of unused channels are transformed but never read: keep them finite)
            DPE_CHECK_HIP(hipMemset(h->fftWork_d, 0, chunk * perW * sizeof(float2)));
            // the batched plans are made at the first Update, for the channel count actually used (and again when it changes)
        }
        return 0;
    };
    if (finish()) {
        dpe_bcs_destroy(h);
        return -1;
    }
    h->idxNext_h.assign(W * K, 0);
    h->chan_h = h->chanBase_h;
#ifdef DPE_EXPERIMENTS   // ablation switch: never in the product library (it makes the banks wrong)
    if (const char *e = getenv("DPE_BCS_CHIP_DBG")) h->chipDbg = atoi(e);
#endif
    *out = h;
    return 0;
}

int dpe_bcs_destroy(dpe_bcs *h)
{
    if (!h) return 0;
    if (h->ownerDetach) h->ownerDetach(h->owner, 0);   // (runs the parked time update, forgets this handle)
    void *bufs[] = {h->tTable_d, h->chipTable_d, h->chipBits_d, h->sums_d, h->rideWord_d, h->chan_d, h->part_d, h->mom_d, h->momRep_d, h->codeBank_d, h->carrBank_d, h->info_d, h->status_d};
    for (void *b : bufs) (void)hipFree(b);
    if (h->chanBase_h) (void)hipHostFree(h->chanBase_h);
    if (h->hintViol_h) (void)hipHostFree(h->hintViol_h);
    h->planS3.destroy(); h->planS2.destroy(); h->planC.destroy();
    (void)hipFree(h->fftWork_d);
    for (hipEvent_t e : h->stagingFree)
        if (e) (void)hipEventDestroy(e);
    h->graphs.clear();
    delete h;
    return 0;
}

}  // extern "C"

// ---- Update: staging, channel facts, plan (dpe_bcs_plan.h), launch -----------------------------------------------------------

// Run-time value -> template argument: pick<4, 8, 16, 32>(LH, f) calls f(std::integral_constant<int, 4>{}) when LH == 4, ...; a value
// outside the list calls nothing (the callers' values are in their lists by construction of the plan).
template <int V, int... Vs, class F>
static inline void pick(int v, F &&f)
{
    if (v == V) f(std::integral_constant<int, V>{});
    else if constexpr (sizeof...(Vs) > 0) pick<Vs...>(v, f);
}
template <class F>
static inline void pick_bool(bool b, F &&f)
{
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// The dpe_chan_start -> BcsChanDev loop of the host-parameter form, into the staging block.
static int bcs_stage_host_params(dpe_bcs *h, const dpe_chan_start *chan_host, int n)
{
    using namespace dpe;
    const int S = h->cfg.samplesPerWindow;
    const double fs = h->cfg.samplingFrequency;
    for (int i = 0; i < n; ++i) {
        const dpe_chan_start &c = chan_host[i];
        DPE_REQUIRE(c.prn >= 1 && c.prn <= kPrnMax, "[BatchCorrScores] Update: PRN %d out of range", c.prn);
        DPE_REQUIRE(c.codeFrequency > 0 && c.codePhaseStart >= 0, "[BatchCorrScores] Update: bad code phase/frequency");
        BcsChanDev &d = h->chan_h[i];
        d.rc = c.codePhaseStart;
        d.codeStep = c.codeFrequency / fs;
        d.ri = c.carrierPhaseStart;
        d.carrStep = c.carrierFrequency / fs;
        d.fc = c.codeFrequency;
        d.fi = c.carrierFrequency;
        d.invStep = fs / c.codeFrequency;
        const double ang = -6.283185307179586476925286766559 * d.carrStep;
        d.rotRe = (float)std::cos(ang);
        d.rotIm = (float)std::sin(ang);
        // BCS_NavBitBoundary, batchcorrscores.cu:247-253
        const int since = (((c.cpElapsedStart - c.cpReference) % 20) + 20) % 20;
        d.idxNext = (int)(std::floor((kLCA * (20 - since) - c.codePhaseStart) * (fs / c.codeFrequency)) + 1);
        d.hasFlip = (d.idxNext > 0 && d.idxNext < S) ? 1 : 0;
        d.prn = c.prn;
        d.pad = 0;
        h->idxNext_h[i] = d.idxNext;
    }
    return 0;
}

// The caller's promise for the device-parameter form (dpe_bcs_set_dev_hint): the chip kernels are chosen from NOMINAL channel
// values -- code frequency F_CA within 1e-5 (ten times the largest code Doppler), carrier offset inside the closed-form DC term's
// range -- and bcs_prep_kernel / chm_k1 check what was promised (hintL1, hintStepMax; status bit 3, the pinned violation word).
// A raised violation word withdraws the hint for the life of the handle.
struct BcsHint {
    bool hinted;
    int l1;           // hintL1 of the device-side check, 0: no hint
    double stepMax;
};
static BcsHint bcs_hint_state(dpe_bcs *h)
{
    if ((h->devHint & 1) && __atomic_load_n(h->hintViol_h, __ATOMIC_RELAXED)) h->devHint &= ~1;
    const bool hinted = (h->devHint & 1) && h->sh.chipOK && h->sh.chipAllowed;
    const double nomStep = dpe::kFCA / h->cfg.samplingFrequency;
    return {hinted, hinted ? (int)(1.0 / nomStep) : 0, nomStep * (1.0 + 1e-5)};
}

// What this Update knows of the channel values (BcsChanFacts).  The host form has them in the staging block.  The device-parameter
// form has them only on the device: under the hint nominal values stand in and nothing is read back (the host does not wait for the
// stream); without it, at sampling rates where the chip kernels exist at all (>= 16 samples per chip), the block bcs_prep_kernel has
// just derived is read back -- <= 3 KB and one stream wait per window, against a 4-5 x slower stage 1; at lower rates nothing is
// fetched and nothing the host decides depends on the values.
static int bcs_channel_facts(dpe_bcs *h, bool dev, bool hinted, int n, hipStream_t stream, dpe::BcsChanFacts &facts)
{
    using namespace dpe;
    if (dev && hinted) {
        const double fs = h->cfg.samplingFrequency;
        for (int i = 0; i < n; ++i) {
            BcsChanDev &d = h->chan_h[i];
            d = BcsChanDev{};
            d.fc = kFCA; d.fi = 0.0;
            d.codeStep = kFCA / fs * (1.0 + 1e-5);
            d.invStep = fs / kFCA;
            d.hasFlip = 0;
        }
    } else if (dev) {
        DPE_CHECK_HIP(hipMemcpyAsync(h->chan_h, h->chan_d, sizeof(BcsChanDev) * n, hipMemcpyDeviceToHost, stream));
        DPE_CHECK_HIP(hipStreamSynchronize(stream));
    }
    facts = bcs_chan_facts(h->chan_h, n, h->sh.chip2Allowed);
    return 0;
}

// What every launch of one Update shares.
struct BcsLaunchArgs {
    const int16_t *samples;
    long long winStride;
    int nWindows, nChan;
    hipStream_t stream;
};

// Full-length FFT form (dpe_bcs_fft.h): DC sum, then per chunk of windows the reference's own sequence.
static int bcs_launch_fft(dpe_bcs *h, const dpe::BcsPlan &plan, const BcsLaunchArgs &a, bool dev)
{
    using namespace dpe;
    const hipStream_t stream = a.stream;
    const int S = h->cfg.samplesPerWindow, nWindows = a.nWindows, nChan = a.nChan;
    if (h->coPending) {   // (a pending task of the device-resident channel manager: a kernel of its own in front)
        hipLaunchKernelGGL(chm_k2_kernel, dim3(1), dim3(256), 0, stream, h->co);
        h->coPending = false;
    }
    const long long C = h->sh.C;
    const int L = h->cfg.lagHalfWidth, B = h->cfg.binHalfWidth, maxK = h->cfg.maxChannels;
    const int sumBlocks = plan.sumBlocks;
    h->lastSumBlocks = plan.sumSlotsUsed;
    h->lastKernel = plan.kernel;
    if (dev) {}
    else if (h->graphs.capturing) DPE_CHECK_HIP(hipMemcpyAsync(h->chan_d, h->chan_h, sizeof(BcsChanDev) * nWindows * nChan, hipMemcpyHostToDevice, stream));
    else upload_params(h->chan_d, h->chanBase_hd + (h->chan_h - h->chanBase_h), sizeof(BcsChanDev) * nWindows * nChan, stream);
    DPE_CHECK_HIP(hipEventRecord(h->stagingFree[h->slot], stream));
    h->prof.begin(0, stream);
    hipLaunchKernelGGL(bcs_sum_kernel, dim3(sumBlocks, nWindows), dim3(256), 0, stream, a.samples, a.winStride, S, h->sums_d,
                       (uint4 *)nullptr, (const uint4 *)nullptr, 0);
    h->prof.end(0, stream);
    const int chunk = h->fftChunkW;
    if (!h->havePlans || h->planK != nChan) {   // batched over the channels this host really tracks, not over maxChannels
        h->havePlans = false;
        const size_t b3 = (size_t)3 * chunk * nChan, b2 = (size_t)2 * chunk * nChan, b1 = (size_t)chunk * nChan;
        if (h->planS3.create((size_t)S, b3, false) || h->planS2.create((size_t)S, b2, true) || h->planC.create((size_t)C, b1, false)) {
            h->planS3.destroy(); h->planS2.destroy(); h->planC.destroy();
            return -1;   // (the message is rocFFT's, from dpe_fft.h)
        }
        h->havePlans = true;
        h->planK = nChan;
    }
    h->prof.begin(1, stream);
    const size_t plane = (size_t)chunk * nChan * S;
    const int gxS = S / 256 < 64 ? (S / 256 > 0 ? S / 256 : 1) : 64;
    const auto exec = [&](FftPlan &p, float2 *ptr) {   // a failed transform closes the profiler slot on its way out
        if (p.exec(stream, (void *)ptr) == 0) return true;
        h->prof.end(1, stream);
        return false;
    };
    for (int w0 = 0; w0 < nWindows; w0 += chunk) {
        const int nw = nWindows - w0 < chunk ? nWindows - w0 : chunk;
        // the plans transform `chunk` windows of rows; a short last chunk carries stale (finite) rows that nobody reads
        if (h->sh.useTable)
            hipLaunchKernelGGL((bcs_fft_prep_code_kernel<true>), dim3(gxS, nChan, nw), dim3(256), 0, stream, a.samples, a.winStride,
                               S, nChan, chunk, w0, h->chan_d, h->chipTable_d, h->tTable_d, h->fftWork_d);
        else
            hipLaunchKernelGGL((bcs_fft_prep_code_kernel<false>), dim3(gxS, nChan, nw), dim3(256), 0, stream, a.samples, a.winStride,
                               S, nChan, chunk, w0, h->chan_d, h->chipTable_d, h->tTable_d, h->fftWork_d);
        if (!exec(h->planS3, h->fftWork_d)) return -1;
        hipLaunchKernelGGL(bcs_fft_mul_kernel, dim3(2048), dim3(256), 0, stream, h->fftWork_d, plane);
        if (!exec(h->planS2, h->fftWork_d + plane)) return -1;
        hipLaunchKernelGGL(bcs_fft_extract_code_kernel, dim3(nChan, nw), dim3(256), 0, stream, h->fftWork_d, plane, S, nChan, L, w0, maxK,
                           h->chan_d, h->codeBank_d, h->info_d);
        const int gxC = 256;
        if (h->sh.useTable)
            hipLaunchKernelGGL((bcs_fft_prep_carr_kernel<true>), dim3(gxC, nChan, nw), dim3(256), 0, stream, a.samples, a.winStride,
                               S, C, nChan, w0, sumBlocks, h->chan_d, h->sums_d, h->chipTable_d, h->tTable_d, h->info_d, h->fftWork_d);
        else
            hipLaunchKernelGGL((bcs_fft_prep_carr_kernel<false>), dim3(gxC, nChan, nw), dim3(256), 0, stream, a.samples, a.winStride,
                               S, C, nChan, w0, sumBlocks, h->chan_d, h->sums_d, h->chipTable_d, h->tTable_d, h->info_d, h->fftWork_d);
        if (!exec(h->planC, h->fftWork_d)) return -1;
        hipLaunchKernelGGL(bcs_fft_extract_carr_kernel, dim3(nChan, nw), dim3(256), 0, stream, h->fftWork_d, C, nChan, B, w0, maxK, h->carrBank_d);
    }
    h->prof.end(1, stream);
    DPE_CHECK_HIP(hipGetLastError());
    return 0;
}

// One chunk's stage-1 launch: the form's kernel with the plan's run-time choices as template arguments.
static void bcs_launch_bank(dpe_bcs *h, const dpe::BcsPlan &p, const dpe::BcsChunk &c, const dpe::BcsParamBlock &pb, const BcsLaunchArgs &a)
{
    using namespace dpe;
    const hipStream_t stream = a.stream;
    const int S = h->cfg.samplesPerWindow, nWindows = a.nWindows, nChan = a.nChan;
    const BcsShape &sh = h->sh;
    const int inl = p.inl ? 1 : 0, vecOK = p.vecOK ? 1 : 0;
    const dim3 grid(p.nBlk, nChan, nWindows), block(256);
    if (c.c2) {
        const int c2Groups = (p.c2nBlk * nWindows + 7) / 8;
        // one block per (tile, SV), tiles dealt to the XCDs (see the kernel)
        const dim3 cgrid(p.ride ? p.rideF + ((c2Groups + p.rideGS - 1) / p.rideGS) * (p.rideSB + p.rideGS * 8 * nChan) : c2Groups * 8 * nChan);
        pick<16, 17, 18, 19, 20, 21, 22, 23, 24>(p.c2L1, [&](auto l1) {
            pick_bool(p.ride, [&](auto rd) {
                pick<4, 6>(p.c2NMom, [&](auto nm) {
                    hipLaunchKernelGGL((bcs_bank_chip2_kernel<nm(), l1(), rd()>), cgrid, dim3(64), 0, stream, pb, inl, a.samples, a.winStride, S,
                                       nChan, nWindows, p.c2Lt, p.c2nBlk, p.sumBlocks, h->chan_d, h->sums_d, h->chipTable_d, h->chipBits_d, h->part_d,
                                       h->mom_d, h->rideWord_d, h->rideEpoch, p.rideF, p.rideSB, p.rideGS, h->rideSpin, h->status_d);
                });
            });
        });
    } else if (p.chip) {
        const dim3 cgrid(((p.nBlk * nWindows + 7) / 8) * 8 * nChan);   // one block per (tile, SV), tiles dealt to the XCDs (see the kernel)
        pick<4, 6>(p.chipNMom, [&](auto nm) {
            hipLaunchKernelGGL((bcs_bank_chip_kernel<nm()>), cgrid, dim3(64), 0, stream, pb, inl, a.samples, a.winStride, S, nChan, nWindows,
                               sh.nPassChip, p.tpb, p.nBlk, p.sumBlocks, c.lagShift, h->chipDbg, h->chan_d, h->sums_d, h->chipTable_d, h->part_d, h->mom_d);
        });
    } else if (p.form == BcsForm::Bank16) {
        pick<4, 8>(sh.LH, [&](auto lh) {
            pick<4, 6>(sh.nMom, [&](auto nm) {
                pick_bool(sh.useTable, [&](auto tb) {
                    hipLaunchKernelGGL((bcs_bank16_kernel<lh(), nm(), tb()>), dim3(((p.nBlk * nWindows + 7) / 8) * 8 * nChan), block, 0, stream, pb, inl,
                                       a.samples, a.winStride, S, nChan, nWindows, sh.nSub, p.tpb, p.nBlk, vecOK, p.sumBlocks, h->chan_d, h->sums_d,
                                       h->chipTable_d, h->tTable_d, h->part_d, h->mom_d);
                });
            });
        });
    } else if (p.form == BcsForm::Wide) {
        pick<4, 6>(sh.nMom, [&](auto nm) {
            pick_bool(sh.useTable, [&](auto tb) {
                hipLaunchKernelGGL((bcs_bank_wide_kernel<nm(), tb()>), grid, block, 0, stream, pb, inl, a.samples, a.winStride, S, nChan, sh.nSub, p.tpb,
                                   p.nBlk, vecOK, p.sumBlocks, c.lagShift, h->chan_d, h->sums_d, h->chipTable_d, h->tTable_d, h->part_d, h->mom_d);
            });
        });
    } else {
        // dense: FUSE (the DC sums ride along) only for LH <= 16, the co-task form only without the time table
        const auto dense = [&](auto lh, auto nm, auto tb, auto fs, auto co, dim3 g) {
            hipLaunchKernelGGL((bcs_bank_kernel<lh(), nm(), tb(), fs(), co()>), g, block, 0, stream, pb, inl, a.samples, a.winStride, S, nChan,
                               sh.nSub, p.tpb, p.nBlk, vecOK, p.sumBlocks, c.lagShift, h->chan_d, h->sums_d, h->chipTable_d, h->tTable_d, h->part_d,
                               h->mom_d, h->momRep_d, h->sums_d, co() ? h->co : ChmKArgs{});
        };
        pick<4, 8, 16, 32>(sh.LH, [&](auto lh) {
            pick<4, 6>(sh.nMom, [&](auto nm) {
                pick_bool(sh.useTable, [&](auto tb) {
                    if constexpr (lh() <= 16) {
                        if (p.fuse && p.coRide) return dense(lh, nm, std::false_type{}, std::true_type{}, std::true_type{}, dim3(p.nBlk + 1, nChan, nWindows));
                        if (p.fuse) return dense(lh, nm, tb, std::true_type{}, std::false_type{}, grid);
                    }
                    dense(lh, nm, tb, std::false_type{}, std::false_type{}, grid);
                });
            });
        });
    }
}

// One chunk's finalize launch.
static void bcs_launch_finalize(dpe_bcs *h, const dpe::BcsPlan &p, const dpe::BcsChunk &c, const dpe::BcsParamBlock &pb, const BcsLaunchArgs &a)
{
    using namespace dpe;
    const int inl = p.inl ? 1 : 0;
    const bool fat = p.fatFinalize && c.lagShift == 0;
    const dim3 fgrid((p.fatFinalize || c.lagShift != 0) ? 1 : 1 + p.nBinBlk, a.nChan, a.nWindows);
    const int ng = fat ? p.nBinBlk : 1;   // (fat: nBinBlk <= 4)
    pick<4, 6>(c.nMomUse, [&](auto nm) {
        pick_bool(p.fuse && c.lagShift == 0, [&](auto fs) {
            pick<1, 2, 3, 4>(ng <= 1 ? 1 : ng >= 4 ? 4 : ng, [&](auto g) {
                hipLaunchKernelGGL((bcs_finalize_kernel<nm(), fs(), g()>), fgrid, dim3(256), 0, a.stream, pb, inl, h->cfg.samplesPerWindow, a.nChan,
                                   p.chip ? c.nBlkUse : h->sh.nSub, c.nBlkUse, h->sh.LH, h->cfg.lagHalfWidth, h->cfg.binHalfWidth,
                                   p.form == BcsForm::Wide ? 1 : 0, c.lagShift, c.momLenUse, p.chip ? 64 : 65, h->sh.C, h->chan_d, h->part_d, h->mom_d,
                                   h->codeBank_d, h->carrBank_d, h->info_d, h->cfg.maxChannels, h->momRep_d, h->sums_d, p.sumSlotsUsed);
            });
        });
    });
}

// Everything a plan enqueues: the riding sums' prelude, the channel manager's task, the DC sums, then per chunk of lags the stage-1
// kernel and the finalize kernel.  guard: the device status word for the re-run behind a hinted chip launch, else nullptr.
static int bcs_launch(dpe_bcs *h, const dpe::BcsPlan &p, const BcsLaunchArgs &a, const int *guard)
{
    using namespace dpe;
    const hipStream_t stream = a.stream;
    const int nWindows = a.nWindows, nChan = a.nChan;
    const size_t chanBytes = sizeof(BcsChanDev) * nWindows * nChan;
    const BcsChanDev *staged_hd = h->chanBase_hd + (h->chan_h - h->chanBase_h);   // the staging block's device address
    BcsParamBlock pb{};
    pb.guard = guard;
    if (p.inl) memcpy(pb.c, h->chan_h, chanBytes);
    // (batches: the DC-sum kernel below carries the parameter upload; a captured graph keeps a copy node)
    else if (h->graphs.capturing) DPE_CHECK_HIP(hipMemcpyAsync(h->chan_d, h->chan_h, chanBytes, hipMemcpyHostToDevice, stream));
    if (p.ride) {
        if (nWindows > h->rideW || p.sumBlocks > h->rideSlots)   // slots this launch reads that the last one did not write: clear the words
            DPE_CHECK_HIP(hipMemsetAsync(h->rideWord_d, 0, sizeof(unsigned long long) * (size_t)h->cfg.maxWindows * kSumSlots, stream));
        h->rideW = nWindows;
        h->rideSlots = p.sumBlocks;
        h->rideEpoch = h->rideEpoch % 3 + 1;
        if (p.upInSum) {
            h->prof.begin(0, stream);
            // (the same kernel clears the status word's "a block of this launch gave up waiting" bit: a block behind such a block skips its own wait)
            upload_params(h->chan_d, staged_hd, chanBytes, stream, h->status_d, 4);
            h->prof.end(0, stream);
            DPE_CHECK_HIP(hipEventRecord(h->stagingFree[h->slot], stream));
        }
    }
    if (h->coPending && !p.coRide) hipLaunchKernelGGL(chm_k2_kernel, dim3(1), dim3(256), 0, stream, h->co);
    h->coPending = false;
    h->lastSumBlocks = p.sumSlotsUsed;
    h->lastKernel = p.kernel;
    if (p.sumLaunch) {
        h->prof.begin(0, stream);
        hipLaunchKernelGGL(bcs_sum_kernel, dim3(p.sumBlocks, nWindows), dim3(256), 0, stream, a.samples, a.winStride, h->cfg.samplesPerWindow,
                           h->sums_d, (uint4 *)h->chan_d, (const uint4 *)staged_hd, p.upInSum ? (int)(chanBytes / 16) : 0);
        h->prof.end(0, stream);
        if (p.upInSum) DPE_CHECK_HIP(hipEventRecord(h->stagingFree[h->slot], stream));   // the staging block is free again
    }
    for (int i = 0; i < p.nChunks; ++i) {
        h->prof.begin(1, stream);
        bcs_launch_bank(h, p, p.chunk[i], pb, a);
        h->prof.end(1, stream);
        h->prof.begin(2, stream);
        bcs_launch_finalize(h, p, p.chunk[i], pb, a);
        h->prof.end(2, stream);
    }
    return 0;
}

// chan_host == nullptr: the channel parameters of this (single-window) call are already in h->chan_d, written by
// bcs_prep_kernel earlier on `stream` (dpe_bcs_update_dev) -- nothing the host decides may then depend on their values,
// except the choice of a chip-boundary kernel at high sampling rates (bcs_channel_facts).
static int bcs_update_impl(dpe_bcs *h, const int16_t *samples_dev, int64_t windowStrideSamples, int32_t nWindows,
                           int32_t nChan, const dpe_chan_start *chan_host, dpe_stream_t stream_)
{
    using namespace dpe;
    const bool dev = chan_host == nullptr;
    DPE_REQUIRE(h && samples_dev, "[BatchCorrScores] Update: null argument");
    DPE_REQUIRE(nWindows >= 1 && nWindows <= h->cfg.maxWindows, "[BatchCorrScores] Update: nWindows %d out of range", nWindows);
    DPE_REQUIRE(nChan >= 1 && nChan <= h->cfg.maxChannels, "[BatchCorrScores] Update: nChan %d out of range", nChan);
    const int S = h->cfg.samplesPerWindow;
    DPE_REQUIRE(nWindows == 1 || windowStrideSamples >= S, "[BatchCorrScores] Update: window stride < S");
    const hipStream_t stream = (hipStream_t)stream_;
    const BcsLaunchArgs args{samples_dev, (long long)windowStrideSamples, nWindows, nChan, stream};
    // next staging block of the ring; an Update issued kStaging calls ago may still be copying it (no-op otherwise)
    h->slot = (h->slot + 1) % dpe_bcs::kStaging;
    DPE_CHECK_HIP(hipEventSynchronize(h->stagingFree[h->slot]));
    h->chan_h = h->chanBase_h + (size_t)h->slot * h->cfg.maxWindows * h->cfg.maxChannels;
    h->lastDev = dev;
    if (!dev && bcs_stage_host_params(h, chan_host, nWindows * nChan)) return -1;
    BcsCall call;
    call.dev = dev;
    call.graphEnabled = h->graphs.enabled;
    call.profiler = h->prof.enabled;
    call.vecOK = ((uintptr_t)samples_dev & 15) == 0 && (windowStrideSamples % 4) == 0;
    const bool hintedCall = dev && bcs_hint_state(h).hinted;   // the chip kernels on the caller's promise: the guarded re-run follows
    BcsChanFacts facts;
    if (bcs_wants_chip(h->sh, false) && bcs_channel_facts(h, dev, hintedCall, nWindows * nChan, stream, facts)) return -1;
    h->lastW = nWindows;
    h->lastK = nChan;
    if (h->sh.fftMode) {
        call.capturing = h->graphs.capturing;
        call.coPending = h->coPending;
        return bcs_launch_fft(h, bcs_plan(h->sh, facts, nWindows, nChan, call), args, dev);
    }
    GraphCache::Guard graphGuard{h->graphs, stream};
    if (bcs_use_graph(call)) {
        const int rc = h->graphs.begin({samples_dev, nullptr, (long long)windowStrideSamples, nWindows, nChan,
                                        (h->sh.wideAllowed ? 1 : 0) | (h->sh.bank16Allowed ? 2 : 0) | (h->slot << 8), stream}, stream);
        DPE_REQUIRE(rc >= 0, "[BatchCorrScores] Update: hipGraph capture/replay failed");
        if (rc == 1) {
            DPE_CHECK_HIP(hipEventRecord(h->stagingFree[h->slot], stream));   // the replayed graph reads this slot
            return 0;
        }
    }
    call.capturing = h->graphs.capturing;
    call.coPending = h->coPending;
    const BcsPlan plan = bcs_plan(h->sh, facts, nWindows, nChan, call);
    if (bcs_launch(h, plan, args, nullptr)) return -1;
    const bool captured = h->graphs.capturing;
    DPE_REQUIRE(h->graphs.end(stream) == 0, "[BatchCorrScores] Update: hipGraph instantiate/launch failed");
    if (captured) DPE_CHECK_HIP(hipEventRecord(h->stagingFree[h->slot], stream));
    DPE_CHECK_HIP(hipGetLastError());
    if (hintedCall && plan.chip) {
        // the chip kernels ran on a promise nobody has checked yet on the host: the general kernels follow, guarded by the device
        // status word -- two launches whose blocks exit at once in all but the flagged windows (~1e-10 of them with honest callers).
        // The re-run's plan never takes a chip form, so it reads no channel value on the host.
        call.rerun = true;
        call.coPending = false;
        const BcsPlan again = bcs_plan(h->sh, BcsChanFacts{}, nWindows, nChan, call);
        DPE_REQUIRE(again.form == BcsForm::Dense || again.form == BcsForm::Wide, "[BatchCorrScores] Update: the guarded re-run chose %s", again.kernel);
        if (bcs_launch(h, again, args, h->status_d)) return -1;
        h->lastKernel = plan.kernel;
        DPE_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

static int bcs_check_dev_call(dpe_bcs *h, const int16_t *samples_dev, int32_t nChan)
{
    DPE_REQUIRE(h && samples_dev, "[BatchCorrScores] Update: null argument");
    DPE_REQUIRE(nChan >= 1 && nChan <= h->cfg.maxChannels, "[BatchCorrScores] Update: nChan %d out of range", nChan);
    return 0;
}

extern "C" {

int dpe_bcs_update(dpe_bcs *h, const int16_t *samples_dev, int64_t windowStrideSamples, int32_t nWindows,
                   int32_t nChan, const dpe_chan_start *chan_host, dpe_stream_t stream)
{
    DPE_REQUIRE(chan_host, "[BatchCorrScores] Update: null argument");
    return bcs_update_impl(h, samples_dev, windowStrideSamples, nWindows, nChan, chan_host, stream);
}

int dpe_bcs_update_dev(dpe_bcs *h, const int16_t *samples_dev, int32_t nChan, const dpe_bcs_ports_dev *ports, dpe_stream_t stream)
{
    using namespace dpe;
    DPE_REQUIRE(ports, "[BatchCorrScores] Update: null argument");
    if (bcs_check_dev_call(h, samples_dev, nChan)) return -1;
    DPE_REQUIRE(ports->codePhaseStart && ports->carrierPhaseStart && ports->codeFrequency && ports->carrierFrequency &&
                ports->cpElapsedStart && ports->cpReference && ports->validPRNs, "[BatchCorrScores] Update: a device port pointer is null");
    const BcsPortsDev p = {ports->codePhaseStart, ports->carrierPhaseStart, ports->codeFrequency, ports->carrierFrequency,
                           ports->cpElapsedStart, ports->cpReference, ports->validPRNs};
    const BcsHint hint = bcs_hint_state(h);
    hipLaunchKernelGGL(bcs_prep_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, p, (int)nChan, h->cfg.samplingFrequency,
                       h->cfg.samplesPerWindow, h->chan_d, h->status_d, hint.l1, hint.stepMax, h->hintViol_hd);
    return bcs_update_impl(h, samples_dev, h->cfg.samplesPerWindow, 1, nChan, nullptr, stream);
}

int dpe_bcs_set_dev_hint(dpe_bcs *h, int32_t flags)
{
    DPE_REQUIRE(h, "[BatchCorrScores] set_dev_hint: null handle");
    h->devHint = flags;
    return 0;
}

int dpe_bcs_update_prepared(dpe_bcs *h, const int16_t *samples_dev, int32_t nChan, dpe_stream_t stream)
{
    if (bcs_check_dev_call(h, samples_dev, nChan)) return -1;
    return bcs_update_impl(h, samples_dev, h->cfg.samplesPerWindow, 1, nChan, nullptr, stream);
}

int dpe_bcs_cotask_set(dpe_bcs *h, const void *args, size_t bytes)
{
    DPE_REQUIRE(h && args && bytes == sizeof(dpe::ChmKArgs), "[BatchCorrScores] cotask: bad arguments");
    DPE_REQUIRE(!h->coPending, "[BatchCorrScores] cotask: the previous task was never launched");
    memcpy(&h->co, args, bytes);
    h->coPending = true;
    return 0;
}

int dpe_bcs_cotask_flush(dpe_bcs *h, void *stream)
{
    DPE_REQUIRE(h, "[BatchCorrScores] cotask: null handle");
    if (!h->coPending) return 0;
    hipLaunchKernelGGL(dpe::chm_k2_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, h->co);
    h->coPending = false;
    DPE_CHECK_HIP(hipGetLastError());
    return 0;
}

int dpe_bcs_hook_set_owner(dpe_bcs *h, dpe_owner_detach_fn detach, void *owner)
{
    DPE_REQUIRE(h, "[BatchCorrScores] hook: null handle");
    DPE_REQUIRE(!owner || !h->owner || h->owner == owner, "[BatchCorrScores] hook: the handle is attached to another channel manager");
    h->ownerDetach = owner ? detach : nullptr;
    h->owner = owner;
    if (!owner) h->coPending = false;   // (the manager is going away: whatever it parked points into its buffers)
    return 0;
}

int dpe_bcs_hook_get(dpe_bcs *h, dpe_bcs_hook *out)
{
    DPE_REQUIRE(h && out, "[BatchCorrScores] hook: null argument");
    out->chan_d = h->chan_d;
    out->status_d = h->status_d;
    out->fs = h->cfg.samplingFrequency;
    out->S = h->cfg.samplesPerWindow;
    out->maxChannels = h->cfg.maxChannels;
    const BcsHint hint = bcs_hint_state(h);
    out->hintL1 = hint.l1;
    out->hintStepMax = hint.stepMax;
    out->hintViol = h->hintViol_hd;
    return 0;
}

int dpe_bcs_dev_status(dpe_bcs *h, int32_t *status, dpe_stream_t stream)
{
    DPE_REQUIRE(h && status && (h->lastDev || h->rideEpoch != 0), "[BatchCorrScores] dev_status: no device-parameter Update (and no batch whose DC sums ride in the chip2 launch) yet");
    DPE_CHECK_HIP(hipMemcpyAsync(status, h->status_d, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    DPE_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

int dpe_bcs_set_graph(dpe_bcs *h, int32_t enable)
{
    DPE_REQUIRE(h, "[BatchCorrScores] set_graph: null handle");
    DPE_REQUIRE(!(enable && h->sh.fftMode), "[BatchCorrScores] set_graph: the full-length FFT form (this handle's lag / bin windows) is not captured as a hipGraph");
    h->graphs.enabled = enable != 0;
    if (!enable) h->graphs.clear();
    return 0;
}

int dpe_bcs_outputs(dpe_bcs *h, const float **codeBank_dev, const float **carrBank_dev, int32_t *nLag, int32_t *nBin,
                    int64_t *numFFTPoints)
{
    DPE_REQUIRE(h, "[BatchCorrScores] outputs: null handle");
    if (codeBank_dev) *codeBank_dev = reinterpret_cast<const float *>(h->codeBank_d);
    if (carrBank_dev) *carrBank_dev = reinterpret_cast<const float *>(h->carrBank_d);
    if (nLag) *nLag = 2 * h->cfg.lagHalfWidth + 1;
    if (nBin) *nBin = 2 * h->cfg.binHalfWidth + 1;
    if (numFFTPoints) *numFFTPoints = h->sh.C;
    return 0;
}

int dpe_bcs_allgather_banks(dpe_bcs *h, dpe_comm *c, float *codeAll_dev, float *carrAll_dev, dpe_stream_t stream)
{
    DPE_REQUIRE(h && c && codeAll_dev && carrAll_dev && h->lastW > 0, "[BatchCorrScores] allgather_banks: no update yet / null argument");
    const size_t K = h->cfg.maxChannels, nLag = 2 * (size_t)h->cfg.lagHalfWidth + 1, nBin = 2 * (size_t)h->cfg.binHalfWidth + 1;
    if (dpe_comm_allgather(c, h->codeBank_d, codeAll_dev, (int64_t)(h->lastW * K * nLag * sizeof(float2)), stream)) return -1;
    return dpe_comm_allgather(c, h->carrBank_d, carrAll_dev, (int64_t)(h->lastW * K * nBin * sizeof(float2)), stream);
}

int dpe_bcs_profile(dpe_bcs *h, int32_t enable, float *ms, int32_t *count)
{
    DPE_REQUIRE(h, "[BatchCorrScores] profile: null handle");
    float m[dpe::KernelProfiler::kSlots];
    int c[dpe::KernelProfiler::kSlots];
    h->prof.collect(m, c);
    for (int i = 0; i < 3; ++i) {
        if (ms) ms[i] = m[i];
        if (count) count[i] = c[i];
    }
    h->prof.enabled = enable != 0;
    h->prof.mask = enable <= 1 ? ~0u : (unsigned)(enable >> 1);   // enable = 1: every kernel; 2 * m: the slots of bit mask m
    return 0;
}

const char *dpe_bcs_stage1_kernel(dpe_bcs *h)
{
    return h ? h->lastKernel : "";
}

int dpe_bcs_read_info(dpe_bcs *h, int32_t *idxNext, int32_t *noFlipLarger, double *mean, dpe_stream_t stream)
{
    DPE_REQUIRE(h && h->lastW > 0, "[BatchCorrScores] read_info: no update yet");
    DPE_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    const int n = h->lastW * h->lastK;
    if (idxNext && h->lastDev) {   // the parameters never were on the host: fetch what bcs_prep_kernel derived
        std::vector<dpe::BcsChanDev> c((size_t)n);
        DPE_CHECK_HIP(hipMemcpy(c.data(), h->chan_d, sizeof(dpe::BcsChanDev) * n, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) idxNext[i] = c[i].idxNext;
    } else if (idxNext) memcpy(idxNext, h->idxNext_h.data(), sizeof(int32_t) * n);
    if (noFlipLarger) DPE_CHECK_HIP(hipMemcpy(noFlipLarger, h->info_d, sizeof(int) * n, hipMemcpyDeviceToHost));
    if (mean) {
        using dpe::kSumSlots;
        const int S = h->cfg.samplesPerWindow;
        const int sumBlocks = h->lastSumBlocks;
        std::vector<long long> s((size_t)2 * kSumSlots * h->lastW);
        DPE_CHECK_HIP(hipMemcpy(s.data(), h->sums_d, sizeof(long long) * s.size(), hipMemcpyDeviceToHost));
        for (int i = 0; i < 2 * h->lastW; ++i) {
            long long t = 0;
            for (int b = 0; b < sumBlocks; ++b) t += s[((size_t)(i / 2) * kSumSlots + b) * 2 + (i & 1)];
            mean[i] = (double)t / (double)(float)S;
        }
    }
    return 0;
}

int dpe_bcs_export_dense(dpe_bcs *h, int32_t window, double *codeScores_dev, double *carrScores_dev, dpe_stream_t stream_)
{
    using namespace dpe;
    DPE_REQUIRE(h && window >= 0 && window < h->lastW, "[BatchCorrScores] export_dense: bad window");
    hipStream_t stream = (hipStream_t)stream_;
    const int K = h->lastK, maxK = h->cfg.maxChannels, S = h->cfg.samplesPerWindow;
    const int nLag = 2 * h->cfg.lagHalfWidth + 1, nBin = 2 * h->cfg.binHalfWidth + 1;
    if (codeScores_dev) {
        DPE_CHECK_HIP(hipMemsetAsync(codeScores_dev, 0, sizeof(double2) * (size_t)K * S, stream));
        hipLaunchKernelGGL(bcs_export_kernel, dim3(1, K), dim3(256), 0, stream,
                           h->codeBank_d + (size_t)window * maxK * nLag, nLag, (long long)S, (long long)(S / 2), K, maxK,
                           h->cfg.lagHalfWidth, reinterpret_cast<double2 *>(codeScores_dev));
    }
    if (carrScores_dev) {
        DPE_CHECK_HIP(hipMemsetAsync(carrScores_dev, 0, sizeof(double2) * (size_t)K * h->sh.C, stream));
        hipLaunchKernelGGL(bcs_export_kernel, dim3(1, K), dim3(256), 0, stream,
                           h->carrBank_d + (size_t)window * maxK * nBin, nBin, h->sh.C, h->sh.C / 2, K, maxK,
                           h->cfg.binHalfWidth, reinterpret_cast<double2 *>(carrScores_dev));
    }
    DPE_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
