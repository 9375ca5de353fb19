// dpe_trk_dev.h -- the scalar tracker's device pieces that other kernels reuse: the sample phase, the fixed-order fp64 reduction, the
// window's boundary cases and scalar_correlate's combination of the segment sums (see dpe_trk.hip for what they restate), with the
// loop state of one channel.  dpe_trk.hip (trk_scalar_kernel, trk_correlate_kernel) and dpe_vt.hip (vt_correlate_kernel) include it.
#pragma once
#include "dpe_common.h"

namespace dpe {

constexpr int kTrkThreads = 256;
constexpr int kTrkTile = 4 * kTrkThreads;   // samples per block tile (4 consecutive samples per lane)
constexpr int kTrkNQ = 18;                  // 3 segments x 3 taps x (re, im)
constexpr int kTrkRow = kTrkThreads + 8;    // padded LDS row of per-lane partials (conflict-free column sums)
constexpr int kTrkLogDoubles = DPE_TRK_LOG_DOUBLES;
constexpr int kTrkSnrN = 20;

// Loop state of one channel; 8-byte members only (copied as words between global memory and LDS).
struct TrkState {
    double rc, ri, fc, fi;           // parameters of the NEXT window
    double fc_bias, fi_bias;
    double paRe, paIm;               // Correlator.p_a
    double cIntH, iIntH;             // BilinearIntegrator.h of the code / carrier loop filter
    double lockI, lockQ;             // LockDetector low-pass states
    double snrMean, snrVar;          // RunningAverageFilter.average (mean power, power variance)
    double snrQm[kTrkSnrN], snrQv[kTrkSnrN];
    double dc, di, efc, efi, dpc, dpi;   // last measurement update (logged with the next window, as the twin's arrays are indexed)
    long long cpcount;               // Channel._cpcount
    long long lossCount, lockCount, lock;
    long long snrPos;
    long long nWindows;              // windows tracked since set_params
    long long nSigns;                // cp_sign entries written since set_params
    long long frozen;
};
static_assert(sizeof(TrkState) % 8 == 0, "TrkState is copied as 8-byte words");

struct TrkLoopCfg {
    double fs, T, fcaid;
    double cKvp, cKpp, iKvp, iKpp;   // loopfilter.py:37-40
    double lockK, lockAlpha;         // lockdetector.py:36-40
    double snrAvgTime;               // snrmeter.py:25
    int lossThreshold, lockThreshold;
};

// ---------------------------------------------------------------------------------------------------------------
// Sample phase of one window.  Block-uniform inputs; every lane returns its 18 partial sums.
// i1 / i2: the window's boundaries clamped to [0, S] (sample n belongs to segment 0 if n < i1, 1 if n < i2, else 2).
__device__ __forceinline__ void trk_sample_phase(const int16_t *__restrict__ x, int S, double fs, double rc, double ri, double fc,
                                                 double fi, int i1, int i2, const int8_t *sTab, float (&acc)[kTrkNQ])
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < kTrkNQ; ++q) acc[q] = 0.f;
    // fp64 seeds of this lane's first sample (n = 4 tid), once per window
    const double codeStep = fc / fs, carrStep = fi / fs;
    const double kTwo52 = 4503599627370496.0, kTwo64 = 18446744073709551616.0;
    // code phase + 1 chip (the late tap reaches half a chip back), chips x 2^52: 12 integer bits, always a valid table index
    const double cph = fma((double)(4 * tid), codeStep, rc) + 1.0;
    unsigned long long code = (unsigned long long)(cph * kTwo52);
    const unsigned long long codeInc = (unsigned long long)(long long)rint(codeStep * kTwo52);
    const unsigned long long codeTile = (unsigned long long)(long long)rint(codeStep * (double)kTrkTile * kTwo52);
    double ph = fma((double)(4 * tid), carrStep, ri);
    ph -= rint(ph);                                       // cycles in [-0.5, 0.5] -> two's-complement fraction x 2^64
    unsigned long long carr = (unsigned long long)(long long)(ph * kTwo64);
    const double cs1 = carrStep - rint(carrStep), csT = carrStep * (double)kTrkTile - rint(carrStep * (double)kTrkTile);
    const unsigned long long carrInc = (unsigned long long)(long long)(cs1 * kTwo64), carrTile = (unsigned long long)(long long)(csT * kTwo64);
    const unsigned long long kHalf = 1ull << 51;
    const bool vecOK = (reinterpret_cast<uintptr_t>(x) & 15) == 0;

    for (int base = 0; base < S; base += kTrkTile) {     // the sample loop: integer phase, fp32 arithmetic
        const int n0 = base + 4 * tid;
        int raw[4];
        if (vecOK && n0 + 3 < S) {
            const int4 v = *reinterpret_cast<const int4 *>(x + 2 * (size_t)n0);
            raw[0] = v.x; raw[1] = v.y; raw[2] = v.z; raw[3] = v.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) raw[i] = (n0 + i < S) ? *reinterpret_cast<const int *>(x + 2 * (size_t)(n0 + i)) : 0;
        }
        unsigned long long c = code, p = carr;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = n0 + i;
            const float re = (float)(short)(raw[i] & 0xFFFF), im = (float)(raw[i] >> 16);
            // wipe-off exp(-j 2 pi phase): top 24 bits of the cycle fraction through sincospi, the next 8 as a first-order turn
            const int a = (int)(unsigned)(p >> 32);
            const float hi = (float)(a >> 8) * 0x1p-23f;                     // half-cycles in [-1, 1): exact
            const float dl = (float)(a & 255) * (6.283185307179586f * 0x1p-32f);   // radians, < 3.8e-7
            float sn, cs;
            sincospif(hi, &sn, &cs);
            const float c2 = fmaf(-dl, sn, cs), s2 = fmaf(dl, cs, sn);
            const float br = fmaf(im, s2, re * c2), bi = fmaf(-re, s2, im * c2);
            // early / prompt / late chips: floor(t fc + rc + 0.5 | 0 | -0.5) mod 1023 (correlator.py:145-147), table extended periodically
            const float ce = (float)sTab[(unsigned)((c + kHalf) >> 52)];
            const float cp = (float)sTab[(unsigned)(c >> 52)];
            const float cl = (float)sTab[(unsigned)((c - kHalf) >> 52)];
            const float f0 = n < i1 ? 1.f : 0.f, f2 = n >= i2 ? 1.f : 0.f, f1 = 1.f - f0 - f2;
            const float er = ce * br, ei = ce * bi, pr = cp * br, pi = cp * bi, lr = cl * br, li = cl * bi;
            acc[0] = fmaf(f0, er, acc[0]);   acc[1] = fmaf(f0, ei, acc[1]);
            acc[2] = fmaf(f0, pr, acc[2]);   acc[3] = fmaf(f0, pi, acc[3]);
            acc[4] = fmaf(f0, lr, acc[4]);   acc[5] = fmaf(f0, li, acc[5]);
            acc[6] = fmaf(f1, er, acc[6]);   acc[7] = fmaf(f1, ei, acc[7]);
            acc[8] = fmaf(f1, pr, acc[8]);   acc[9] = fmaf(f1, pi, acc[9]);
            acc[10] = fmaf(f1, lr, acc[10]); acc[11] = fmaf(f1, li, acc[11]);
            acc[12] = fmaf(f2, er, acc[12]); acc[13] = fmaf(f2, ei, acc[13]);
            acc[14] = fmaf(f2, pr, acc[14]); acc[15] = fmaf(f2, pi, acc[15]);
            acc[16] = fmaf(f2, lr, acc[16]); acc[17] = fmaf(f2, li, acc[17]);
            c += codeInc;
            p += carrInc;
        }
        code += codeTile;
        carr += carrTile;
    }
}

// Block sum of the 18 partials in fp64, fixed order: sSum[q] holds the totals after the call (ends with a barrier).
__device__ __forceinline__ void trk_reduce(const float (&acc)[kTrkNQ], float *sPart, double *sRed, double *sSum)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < kTrkNQ; ++q) sPart[q * kTrkRow + tid] = acc[q];
    __syncthreads();
    if (tid < kTrkNQ * 8) {
        const int q = tid >> 3, c = tid & 7;
        double s = 0.0;
        for (int i = 0; i < kTrkThreads / 8; ++i) s += (double)sPart[q * kTrkRow + i * 8 + c];
        sRed[tid] = s;
    }
    __syncthreads();
    if (tid < kTrkNQ) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 8; ++c) s += sRed[tid * 8 + c];
        sSum[tid] = s;
    }
    __syncthreads();
}

// The window's boundaries (correlator.py:157-158) and which of the twin's branches it takes:
// 1 normal (one boundary inside), 2 (two inside), 0 (none), -1 the twin's "EXTREME ERROR" (also: parameters not finite).
__device__ __forceinline__ int trk_boundaries(double rc, double fc, double fs, int S, int &i1, int &i2, double &d1, double &d2)
{
    d1 = floor(((double)kLCA - rc) * (fs / fc)) + 1.0;
    d2 = floor((2.0 * (double)kLCA - rc) * (fs / fc)) + 1.0;
    int kase = -1;
    // (also what the fixed-point code phase of the sample phase assumes: rc in [0, 1023], less than 2 000 chips per window)
    const bool ok = fabs(d1) < 1e9 && fabs(d2) < 1e9 && fc > 0.0 && rc >= 0.0 && rc <= (double)kLCA && (double)S * (fc / fs) < 2000.0;   // false for NaN
    if (ok) {
        if (d1 <= (double)S && (double)S < d2) kase = 1;
        else if (d1 < d2 && d2 <= (double)S) kase = 2;
        else if ((double)S < d1) kase = 0;
    }
    i1 = i2 = S;
    if (kase >= 0) {
        i1 = d1 < 0.0 ? 0 : (d1 > (double)S ? S : (int)d1);
        i2 = d2 < 0.0 ? 0 : (d2 > (double)S ? S : (int)d2);
        if (i2 < i1) i2 = i1;
    }
    return kase;
}

#pragma clang fp contract(off)
// scalar_correlate's combination of the segment sums (correlator.py:162-279).  v = sSum (E, P, L per segment).
// out: e_r, p_r, l_r (re, im); returns the number of completed code periods; sg[] the prompt signs -sign(Re p_s).
__device__ __forceinline__ int trk_combine(int kase, const double *v, double &paRe, double &paIm, double (&out)[6], double (&sg)[2])
{
    const double ebR = v[0], ebI = v[1], pbR = v[2], pbI = v[3], lbR = v[4], lbI = v[5];
    const double e1R = v[6], e1I = v[7], p1R = v[8], p1I = v[9], l1R = v[10], l1I = v[11];
    const double e2R = v[12], e2I = v[13], p2R = v[14], p2I = v[15], l2R = v[16], l2I = v[17];
    auto sgn = [](double a) { return a > 0.0 ? -1.0 : (a < 0.0 ? 1.0 : 0.0); };   // -np.sign
    if (kase == 0) {
        paRe = paRe + pbR; paIm = paIm + pbI;
        out[0] = ebR; out[1] = ebI; out[2] = pbR; out[3] = pbI; out[4] = lbR; out[5] = lbI;
        return 0;
    }
    const double ps1R = paRe + pbR;
    sg[0] = sgn(ps1R);
    // sum of the three taps of segment B and of the segment after it, in the twin's order of additions
    const double bR = (ebR + pbR) + lbR, bI = (ebI + pbI) + lbI;
    const double posR = ((bR + e1R) + p1R) + l1R, posI = ((bI + e1I) + p1I) + l1I;
    const double negR = ((bR - e1R) - p1R) - l1R, negI = ((bI - e1I) - p1I) - l1I;
    const bool same1 = hypot(posR, posI) > hypot(negR, negI);
    if (kase == 1) {
        paRe = p1R; paIm = p1I;
        const double s = same1 ? 1.0 : -1.0;
        out[0] = ebR + s * e1R; out[1] = ebI + s * e1I; out[2] = pbR + s * p1R; out[3] = pbI + s * p1I;
        out[4] = lbR + s * l1R; out[5] = lbI + s * l1I;
        return 1;
    }
    sg[1] = sgn(p1R);
    paRe = p2R; paIm = p2I;
    if (same1) {
        const double sR = (e1R + p1R) + l1R, sI = (e1I + p1I) + l1I;
        const double qR = ((sR + e2R) + p2R) + l2R, qI = ((sI + e2I) + p2I) + l2I;
        const double mR = ((sR - e2R) - p2R) - l2R, mI = ((sI - e2I) - p2I) - l2I;
        const double s = hypot(qR, qI) > hypot(mR, mI) ? 1.0 : -1.0;
        out[0] = (ebR + e1R) + s * e2R; out[1] = (ebI + e1I) + s * e2I; out[2] = (pbR + p1R) + s * p2R; out[3] = (pbI + p1I) + s * p2I;
        out[4] = (lbR + l1R) + s * l2R; out[5] = (lbI + l1I) + s * l2I;
    } else {
        out[0] = (ebR - e1R) - e2R; out[1] = (ebI - e1I) - e2I; out[2] = (pbR - p1R) - p2R; out[3] = (pbI - p1I) - p2I;
        out[4] = (lbR - l1R) - l2R; out[5] = (lbI - l1I) - l2I;
    }
    return 2;
}

__device__ __forceinline__ double trk_mod(double a, double b)   // numpy.mod for b > 0
{
    double m = fmod(a, b);
    if (m != 0.0 && m < 0.0) m += b;
    return m;
}
#pragma clang fp contract(fast)

__device__ __forceinline__ void trk_fill_table(int8_t *sTab, const int8_t *__restrict__ chipTable, int prn)
{
    // sTab[i] = chip[(i - 1) mod 1023], i in [0, 4096): the sample phase indexes it with floor(code phase + 1 +- 0.5)
    for (int i = threadIdx.x; i < 4096; i += kTrkThreads) sTab[i] = chipTable[(prn - 1) * 1024 + (i + kLCA - 1) % kLCA];
}

// the tracker's device-resident loop state as another translation unit may read it (dpe_vt_init_from_trk).  Defined in dpe_trk.hip.
struct TrkStateView { const TrkState *state; int K; bool haveParams; const int *prn; double fs, T; };
int trk_state_view(dpe_trk *h, TrkStateView *out);

}  // namespace dpe
