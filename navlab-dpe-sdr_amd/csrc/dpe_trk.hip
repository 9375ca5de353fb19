// dpe_trk.hip -- scalar tracking for MI355X (gfx950): every channel's early / prompt / late loop over a whole record in
// ONE launch.  The stage between acquisition (dpe_acq_*) and the DPE loop; only the reference's Python twin has it:
// Receiver.scalar_track (pygnss/pythonreceiver/receiver.py:522-542) = per 1 ms window and channel
//   Correlator.scalar_correlate          scalar/correlator.py:135-283
//   Channel.scalar_correlation           scalar/channel.py:104-122   (lock detector, SNR meter, cp_sign stream)
//   Channel.scalar_time_update           scalar/channel.py:173-191
//   Channel.scalar_measurement_update    scalar/channel.py:247-273   (DLL / PLL discriminators, two 2nd-order loop filters)
//
// The loops are channel-local, so trk_scalar_kernel runs one block per channel and walks the windows in order:
//   sample phase (256 lanes, fp32 + integer): carrier wipe-off and the three code taps, accumulated per SEGMENT of the
//     window (cut at the code-period boundaries idxs1, idxs2 of correlator.py:157-158) -- 3 segments x 3 taps x (re, im)
//     per lane.  Carrier and code phase advance as 64-bit FIXED-POINT integers from one fp64 seed per lane and window
//     (carrier: cycles x 2^64; code: chips x 2^52), so the chip a sample is assigned to and the phase it is wiped with
//     are exact to 2^-52 chip / 2^-32 cycle whatever the window length -- no fp64 in the sample loop, no fp32 phase run;
//   reduction in fp64 through LDS in a fixed order (bit-reproducible);
//   loop phase (one lane, fp64): the three boundary cases with their polarity decisions, carried p_a, cp_sign, lock
//     detector, SNR meter, time update, discriminators, loop filters, frequency corrections -- the twin's operations
//     in the twin's order (contraction off).  The next window's parameters reach the other lanes through LDS.
// All K blocks read the same samples (L2 after the first reader); nothing else is shared.  Every write to memory is a
// plain vector store; a state the twin would report as "EXTREME ERROR" sets a status bit and freezes the channel.
#include <algorithm>

#include "dpe_common.h"
#include "dpe_trk_log.h"
#include "dpe_trk_dev.h"

namespace dpe {

#pragma clang fp contract(off)
// One window of the loop, one lane: everything after the correlations.  rec: the window's log record; signs: this channel's ring.
__device__ __noinline__ void trk_loop_window(TrkState &st, const TrkLoopCfg &cfg, int kase, const double *sums, double *rec, int8_t *signs, long long signCap)
{
    double o[6], sg[2] = {0.0, 0.0};
    const double cpNow = (double)st.cpcount;   // Channel.cp[mc]: _cpcount as the previous time update left it
    const int compl_ = trk_combine(kase, sums, st.paRe, st.paIm, o, sg);
    const double iE = o[0], qE = o[1], iP = o[2], qP = o[3], iL = o[4], qL = o[5];
    // LockDetector.update (lockdetector.py:82-101)
    st.lockI = cfg.lockAlpha * fabs(iP) + (1.0 - cfg.lockAlpha) * st.lockI;
    st.lockQ = cfg.lockAlpha * fabs(qP) + (1.0 - cfg.lockAlpha) * st.lockQ;
    const double li = st.lockI / cfg.lockK, lq = st.lockQ;
    if (li > lq) {
        st.lossCount = 0;
        if (st.lockCount > cfg.lockThreshold) st.lock = 1; else st.lockCount += 1;
    } else {
        st.lockCount = 0;
        if (st.lossCount > cfg.lossThreshold) st.lock = 0; else st.lossCount += 1;
    }
    // SignalNoiseMeter.update (snrmeter.py:52-61), running averages of filters.py:54-57
    const double z = iP * iP + qP * qP;
    const int sp = (int)st.snrPos;
    st.snrMean = st.snrMean + (z - st.snrQm[sp]) / (double)kTrkSnrN;
    st.snrQm[sp] = z;
    const double dz = z - st.snrMean, zv = dz * dz;
    st.snrVar = st.snrVar + (zv - st.snrQv[sp]) / (double)kTrkSnrN;
    st.snrQv[sp] = zv;
    st.snrPos = (sp + 1) % kTrkSnrN;
    double sq = st.snrMean * st.snrMean - st.snrVar;
    sq = sq > 0.0 ? sq : 0.0;
    const double cm = sqrt(sq), nv = (st.snrMean - cm) / 2.0;
    double la = cm / (2.0 * cfg.snrAvgTime * nv);
    la = la > 1.0 ? la : 1.0;            // (NaN -> 1, as Python's conditional expression)
    const double snr = 10.0 * log10(fabs(la));
    // cp_sign stream
    for (int j = 0; j < compl_; ++j) {
        signs[st.nSigns % signCap] = (int8_t)sg[j];
        st.nSigns += 1;
    }
    st.cpcount += compl_;
    rec[0] = cpNow; rec[1] = st.rc; rec[2] = st.ri; rec[3] = st.fc; rec[4] = st.fi;
    rec[5] = iE; rec[6] = qE; rec[7] = iP; rec[8] = qP; rec[9] = iL; rec[10] = qL;
    rec[11] = st.dc; rec[12] = st.di; rec[13] = st.efc; rec[14] = st.efi; rec[15] = st.dpc; rec[16] = st.dpi;
    rec[17] = st.fc_bias; rec[18] = st.fi_bias; rec[19] = (double)st.lock; rec[20] = li - lq; rec[21] = snr;
    rec[22] = (double)kase; rec[23] = (double)compl_;
    // scalar_time_update (channel.py:179-180)
    const double rcN = trk_mod(st.rc + st.fc * cfg.T, (double)kLCA), riN = trk_mod(st.ri + st.fi * cfg.T, 1.0);
    // scalar_measurement_update (channel.py:253-271), discriminator.py:25-54, loopfilter.py:102, filters.py:113-115
    double dpi = 0.0, dpc = 0.0;
    if (iP != 0.0) dpi = atan(qP / iP) / (2.0 * kPi);
    const double E = sqrt(iE * iE + qE * qE), L = sqrt(iL * iL + qL * qL);
    if (E + L != 0.0) dpc = (E - L) / (2.0 * (E + L));
    double h0 = st.iIntH;
    st.iIntH = st.iIntH + cfg.T * (dpi * cfg.iKvp + 0.0);
    const double di = (st.iIntH + h0) / 2.0 + dpi * cfg.iKpp;
    h0 = st.cIntH;
    st.cIntH = st.cIntH + cfg.T * (dpc * cfg.cKvp + 0.0);
    const double dc = (st.cIntH + h0) / 2.0 + dpc * cfg.cKpp;
    const double efi = (st.fi_bias + di) - st.fi;
    const double efc = ((kFCA + st.fc_bias + dc) + cfg.fcaid * (st.fi_bias + di)) - st.fc;
    st.fi = st.fi + efi;
    st.fc = st.fc + efc;
    st.rc = rcN; st.ri = riN;
    st.dc = dc; st.di = di; st.efc = efc; st.efi = efi; st.dpc = dpc; st.dpi = dpi;
}
#pragma clang fp contract(fast)

struct TrkWinParams { double rc, ri, fc, fi; int kase, i1, i2, pad; };

__global__ __launch_bounds__(kTrkThreads) void trk_scalar_kernel(const int16_t *__restrict__ iq, int S, int nWin, TrkLoopCfg cfg,
                                                                const int *__restrict__ prn, const int8_t *__restrict__ chipTable,
                                                                TrkState *__restrict__ state, double *__restrict__ log, long long logCap,
                                                                int nChan, int8_t *__restrict__ signs, long long signCap, int *__restrict__ status)
{
    __shared__ int8_t sTab[4096];
    __shared__ float sPart[kTrkNQ * kTrkRow];
    __shared__ double sRed[kTrkNQ * 8], sSum[kTrkNQ], sRec[kTrkLogDoubles];
    __shared__ TrkState sSt;
    __shared__ TrkWinParams sWin;
    __shared__ TrkLoopCfg sCfg;   // read by the one lane of the loop phase: from LDS, not held in scalar registers across the sample phase
    const int k = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) sCfg = cfg;
    constexpr int kWords = (int)(sizeof(TrkState) / 8);
    for (int i = tid; i < kWords; i += kTrkThreads) reinterpret_cast<long long *>(&sSt)[i] = reinterpret_cast<const long long *>(state + k)[i];
    trk_fill_table(sTab, chipTable, prn[k]);
    __syncthreads();
    if (tid == 0) {
        double d1, d2;
        sWin.rc = sSt.rc; sWin.ri = sSt.ri; sWin.fc = sSt.fc; sWin.fi = sSt.fi;
        sWin.kase = sSt.frozen ? -1 : trk_boundaries(sSt.rc, sSt.fc, cfg.fs, S, sWin.i1, sWin.i2, d1, d2);
    }
    __syncthreads();
    for (int m = 0; m < nWin; ++m) {
        const TrkWinParams w = sWin;
        float acc[kTrkNQ];
        if (w.kase >= 0) {
            trk_sample_phase(iq + 2 * (size_t)m * S, S, cfg.fs, w.rc, w.ri, w.fc, w.fi, w.i1, w.i2, sTab, acc);
        } else {
#pragma unroll
            for (int q = 0; q < kTrkNQ; ++q) acc[q] = 0.f;
        }
        trk_reduce(acc, sPart, sRed, sSum);
        if (tid == 0) {
            if (w.kase >= 0) {
                trk_loop_window(sSt, sCfg, w.kase, sSum, sRec, signs + (size_t)k * signCap, signCap);
            } else {
                // the twin's fourth branch: flag it, freeze the channel, log the parameters it stopped at
                if (!sSt.frozen) atomicOr(status, 1);
                sSt.frozen = 1;
                const double nan = __builtin_nan("");
                for (int i = 0; i < kTrkLogDoubles; ++i) sRec[i] = nan;
                sRec[0] = (double)sSt.cpcount; sRec[1] = sSt.rc; sRec[2] = sSt.ri; sRec[3] = sSt.fc; sRec[4] = sSt.fi;
                sRec[17] = sSt.fc_bias; sRec[18] = sSt.fi_bias; sRec[19] = (double)sSt.lock; sRec[22] = -1.0; sRec[23] = 0.0;
            }
            double d1, d2;
            sWin.rc = sSt.rc; sWin.ri = sSt.ri; sWin.fc = sSt.fc; sWin.fi = sSt.fi;
            sWin.kase = sSt.frozen ? -1 : trk_boundaries(sSt.rc, sSt.fc, cfg.fs, S, sWin.i1, sWin.i2, d1, d2);
        }
        __syncthreads();
        if (tid < kTrkLogDoubles) {
            const long long slot = (sSt.nWindows + m) % logCap;
            log[((size_t)slot * nChan + k) * kTrkLogDoubles + tid] = sRec[tid];
        }
        // (sRec / sWin are next written after the barriers of the next window's reduction)
    }
    __syncthreads();
    if (tid == 0) sSt.nWindows += nWin;
    __syncthreads();
    for (int i = tid; i < kWords; i += kTrkThreads) reinterpret_cast<long long *>(state + k)[i] = reinterpret_cast<const long long *>(&sSt)[i];
}

// Teacher-forced correlator: block (m, k) correlates window m with the given parameters and a carried p_a of zero.
// out[m][k][32]: 18 segment sums, e_r p_r l_r (6), case, completed code periods, idxs1, idxs2, sign 1, sign 2, 2 spare.
__global__ __launch_bounds__(kTrkThreads) void trk_correlate_kernel(const int16_t *__restrict__ iq, int S, double fs, const int *__restrict__ prn,
                                                                   const int8_t *__restrict__ chipTable, const double *__restrict__ params,
                                                                   double *__restrict__ out, int nChan, int *__restrict__ status)
{
    __shared__ int8_t sTab[4096];
    __shared__ float sPart[kTrkNQ * kTrkRow];
    __shared__ double sRed[kTrkNQ * 8], sSum[kTrkNQ];
    const int m = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    trk_fill_table(sTab, chipTable, prn[k]);
    const double *p = params + ((size_t)m * nChan + k) * 4;
    const double rc = p[0], ri = p[1], fc = p[2], fi = p[3];
    int i1, i2;
    double d1, d2;
    const int kase = trk_boundaries(rc, fc, fs, S, i1, i2, d1, d2);
    __syncthreads();
    float acc[kTrkNQ];
    if (kase >= 0) {
        trk_sample_phase(iq + 2 * (size_t)m * S, S, fs, rc, ri, fc, fi, i1, i2, sTab, acc);
    } else {
#pragma unroll
        for (int q = 0; q < kTrkNQ; ++q) acc[q] = 0.f;
    }
    trk_reduce(acc, sPart, sRed, sSum);
    double *o = out + ((size_t)m * nChan + k) * 32;
    if (tid < kTrkNQ) o[tid] = sSum[tid];
    if (tid == 0) {
        double r[6] = {0, 0, 0, 0, 0, 0}, sg[2] = {0.0, 0.0}, paRe = 0.0, paIm = 0.0;
        int compl_ = 0;
        if (kase >= 0) compl_ = trk_combine(kase, sSum, paRe, paIm, r, sg);
        else atomicOr(status, 1);
        for (int i = 0; i < 6; ++i) o[18 + i] = r[i];
        o[24] = (double)kase; o[25] = (double)compl_; o[26] = d1; o[27] = d2; o[28] = sg[0]; o[29] = sg[1]; o[30] = 0.0; o[31] = 0.0;
    }
}

}  // namespace dpe

struct dpe_trk {
    dpe_trk_config cfg;
    dpe::TrkLoopCfg loop;
    int S = 0, K = 0;
    long long logCap = 0, signCap = 0;
    long long nWindows = 0;            // host mirror of the windows enqueued since set_params
    bool haveParams = false;
    int *prn_d = nullptr, *status_d = nullptr;
    int8_t *chips_d = nullptr, *signs_d = nullptr;
    dpe::TrkState *state_d = nullptr;
    double *log_d = nullptr;
    double *corrParams_d = nullptr, *corrOut_d = nullptr;
    long long corrCap = 0;
};

namespace dpe {
int trk_log_view(dpe_trk *h, TrkLogView *out)   // dpe_trk_log.h
{
    DPE_REQUIRE(h && out, "[ScalarTracker] log view: null argument");
    *out = TrkLogView{h->log_d, h->logCap, h->nWindows, h->K, h->cfg.prn};
    return 0;
}
int trk_state_view(dpe_trk *h, TrkStateView *out)   // dpe_trk_dev.h
{
    DPE_REQUIRE(h && out, "[ScalarTracker] state view: null argument");
    *out = TrkStateView{h->state_d, h->K, h->haveParams, h->cfg.prn, h->loop.fs, h->loop.T};
    return 0;
}
int trk_log_load(dpe_trk *h, int nWindows, const double *rows, hipStream_t st)
{
    DPE_REQUIRE(h && rows, "[ScalarTracker] load_log: null argument");
    DPE_REQUIRE(nWindows >= 1 && nWindows <= h->logCap, "[ScalarTracker] load_log: %d windows do not fit the log (capacity %lld)", nWindows, h->logCap);
    DPE_CHECK_HIP(hipStreamSynchronize(st));
    DPE_CHECK_HIP(hipMemcpy(h->log_d, rows, (size_t)nWindows * h->K * kTrkLogDoubles * sizeof(double), hipMemcpyHostToDevice));
    h->nWindows = nWindows;
    h->haveParams = false;   // the loop state is not part of a log: tracking starts again from dpe_trk_set_params
    return 0;
}
}  // namespace dpe

extern "C" {

int dpe_trk_destroy(dpe_trk *h)
{
    if (!h) return 0;
    void *bufs[] = {h->prn_d, h->status_d, h->chips_d, h->signs_d, h->state_d, h->log_d, h->corrParams_d, h->corrOut_d};
    for (void *b : bufs) (void)hipFree(b);
    delete h;
    return 0;
}

int dpe_trk_create(const dpe_trk_config *cfg, dpe_trk **out)
{
    using namespace dpe;
    DPE_REQUIRE(cfg && out, "[ScalarTracker] create: null argument");
    DPE_REQUIRE(cfg->samplingFrequency > 0 && cfg->T > 0 && cfg->T <= 1.5e-3,
                "[ScalarTracker] create: the window must be positive and at most 1.5 ms (the twin's boundary cases cover one code period)");
    DPE_REQUIRE(cfg->nChan >= 1 && cfg->nChan <= DPE_MAX_CHAN, "[ScalarTracker] create: nChan out of range");
    DPE_REQUIRE(cfg->order == 0 || cfg->order == 2, "[ScalarTracker] create: only second-order loops (the twin constructs no other)");
    DPE_REQUIRE(cfg->logCapacityWindows >= 1, "[ScalarTracker] create: logCapacityWindows must be positive");
    for (int i = 0; i < cfg->nChan; ++i)
        DPE_REQUIRE(cfg->prn[i] >= 1 && cfg->prn[i] <= kPrnMax, "[ScalarTracker] create: PRN %d out of range", cfg->prn[i]);
    dpe_trk *h = new dpe_trk();
    h->cfg = *cfg;
    h->S = (int)llround(cfg->T * cfg->samplingFrequency);   // rawfile.py:164
    h->K = cfg->nChan;
    h->logCap = cfg->logCapacityWindows;
    h->signCap = 2 * h->logCap + 2;
    const double ds = cfg->dopplerSign != 0.0 ? cfg->dopplerSign : 1.0;
    const double cB = cfg->codeBnp > 0 ? cfg->codeBnp : 3.0, iB = cfg->carrBnp > 0 ? cfg->carrBnp : 40.0;   // channel.py:57-58
    TrkLoopCfg &L = h->loop;
    L.fs = cfg->samplingFrequency; L.T = cfg->T; L.fcaid = ds * kFCA / kFL1;                                 // rawfile.py:98
    L.cKvp = std::pow(cB / 0.53, 2.0); L.cKpp = 1.414 * (cB / 0.53);
    L.iKvp = std::pow(iB / 0.53, 2.0); L.iKpp = 1.414 * (iB / 0.53);
    L.lockK = 1.5; L.lockAlpha = 0.0247; L.lossThreshold = 50; L.lockThreshold = 240;                        // channel.py:61
    L.snrAvgTime = (double)kTrkSnrN * cfg->T;
    h->prn_d = dev_alloc<int>(DPE_MAX_CHAN);
    h->status_d = dev_alloc<int>(1);
    h->chips_d = dev_alloc<int8_t>((size_t)kPrnMax * 1024);
    h->signs_d = dev_alloc<int8_t>((size_t)h->K * h->signCap);
    h->state_d = dev_alloc<TrkState>(h->K);
    h->log_d = dev_alloc<double>((size_t)h->logCap * h->K * kTrkLogDoubles);
    if (!h->prn_d || !h->status_d || !h->chips_d || !h->signs_d || !h->state_d || !h->log_d) {
        set_error("[ScalarTracker] create: device allocation failed");
        dpe_trk_destroy(h);
        return -1;
    }
    std::vector<int8_t> chips((size_t)kPrnMax * 1024, 0);
    for (int p = 1; p <= kPrnMax; ++p) gen_ca_code_host(p, chips.data() + (size_t)(p - 1) * 1024);
    if (hipMemcpy(h->chips_d, chips.data(), chips.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->prn_d, cfg->prn, sizeof(int) * h->K, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(h->status_d, 0, sizeof(int)) != hipSuccess || hipMemset(h->signs_d, 0, (size_t)h->K * h->signCap) != hipSuccess ||
        hipMemset(h->state_d, 0, sizeof(TrkState) * h->K) != hipSuccess) {
        set_error("[ScalarTracker] create: device initialisation failed");
        dpe_trk_destroy(h);
        return -1;
    }
    *out = h;
    return 0;
}

int dpe_trk_set_params(dpe_trk *h, const dpe_acq_track_init *init, dpe_stream_t stream_)
{
    using namespace dpe;
    DPE_REQUIRE(h && init, "[ScalarTracker] set_params: null argument");
    hipStream_t st = (hipStream_t)stream_;
    std::vector<TrkState> s(h->K);
    const double nan = std::nan("");
    for (int k = 0; k < h->K; ++k) {
        DPE_REQUIRE(init[k].prn == h->cfg.prn[k], "[ScalarTracker] set_params: entry %d is PRN %d, the tracker's channel is PRN %d", k,
                    init[k].prn, h->cfg.prn[k]);
        TrkState &t = s[k];
        std::memset(&t, 0, sizeof(t));
        // Channel.set_scalar_params (channel.py:82-102): biases from the start values, both loop filters reset
        t.rc = init[k].rc; t.ri = init[k].ri; t.fc = init[k].fc; t.fi = init[k].fi;
        t.fi_bias = init[k].fi;
        t.fc_bias = init[k].fc - kFCA - h->loop.fcaid * t.fi_bias;
        t.dc = t.di = t.efc = t.efi = t.dpc = t.dpi = nan;   // the twin's logs hold NaN until the first measurement update
    }
    DPE_CHECK_HIP(hipStreamSynchronize(st));
    DPE_CHECK_HIP(hipMemcpy(h->state_d, s.data(), sizeof(TrkState) * h->K, hipMemcpyHostToDevice));
    DPE_CHECK_HIP(hipMemset(h->status_d, 0, sizeof(int)));
    h->nWindows = 0;
    h->haveParams = true;
    return 0;
}

int dpe_trk_track(dpe_trk *h, const int16_t *samples_dev, int32_t nWindows, dpe_stream_t stream_)
{
    using namespace dpe;
    DPE_REQUIRE(h && samples_dev, "[ScalarTracker] track: null argument");
    DPE_REQUIRE(h->haveParams, "[ScalarTracker] track: set_params has not been called");
    DPE_REQUIRE(nWindows >= 1, "[ScalarTracker] track: nWindows must be positive");
    hipStream_t st = (hipStream_t)stream_;
    hipLaunchKernelGGL(trk_scalar_kernel, dim3(h->K), dim3(kTrkThreads), 0, st, samples_dev, h->S, (int)nWindows, h->loop, h->prn_d,
                       h->chips_d, h->state_d, h->log_d, h->logCap, h->K, h->signs_d, h->signCap, h->status_d);
    DPE_CHECK_HIP(hipGetLastError());
    h->nWindows += nWindows;
    return 0;
}

int dpe_trk_correlate(dpe_trk *h, const int16_t *samples_dev, int32_t nWindows, const double *params, double *out, dpe_stream_t stream_)
{
    using namespace dpe;
    DPE_REQUIRE(h && samples_dev && params && out, "[ScalarTracker] correlate: null argument");
    DPE_REQUIRE(nWindows >= 1 && nWindows <= 65535 * 32, "[ScalarTracker] correlate: nWindows out of range");
    hipStream_t st = (hipStream_t)stream_;
    const size_t n = (size_t)nWindows * h->K;
    if (h->corrCap < (long long)n) {
        DPE_CHECK_HIP(hipStreamSynchronize(st));
        (void)hipFree(h->corrParams_d); (void)hipFree(h->corrOut_d);
        h->corrCap = 0;
        h->corrParams_d = dev_alloc<double>(n * 4);
        h->corrOut_d = dev_alloc<double>(n * 32);
        DPE_REQUIRE(h->corrParams_d && h->corrOut_d, "[ScalarTracker] correlate: device allocation failed");
        h->corrCap = (long long)n;
    }
    DPE_CHECK_HIP(hipMemcpyAsync(h->corrParams_d, params, n * 4 * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(trk_correlate_kernel, dim3(nWindows, h->K), dim3(kTrkThreads), 0, st, samples_dev, h->S, h->loop.fs, h->prn_d,
                       h->chips_d, h->corrParams_d, h->corrOut_d, h->K, h->status_d);
    DPE_CHECK_HIP(hipGetLastError());
    DPE_CHECK_HIP(hipMemcpyAsync(out, h->corrOut_d, n * 32 * sizeof(double), hipMemcpyDeviceToHost, st));
    DPE_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

int dpe_trk_read_log(dpe_trk *h, int64_t firstWindow, int32_t nWindows, double *out, dpe_stream_t stream_)
{
    using namespace dpe;
    DPE_REQUIRE(h && out, "[ScalarTracker] read_log: null argument");
    DPE_REQUIRE(firstWindow >= 0 && nWindows >= 0 && firstWindow + nWindows <= h->nWindows, "[ScalarTracker] read_log: windows [%lld, %lld) have not been tracked",
                (long long)firstWindow, (long long)(firstWindow + nWindows));
    DPE_REQUIRE(firstWindow >= h->nWindows - h->logCap, "[ScalarTracker] read_log: window %lld has left the log (capacity %lld)",
                (long long)firstWindow, h->logCap);
    hipStream_t st = (hipStream_t)stream_;
    DPE_CHECK_HIP(hipStreamSynchronize(st));
    const size_t rowBytes = (size_t)h->K * dpe::kTrkLogDoubles * sizeof(double);
    for (long long m = firstWindow; m < firstWindow + nWindows;) {        // the log is a ring: at most two pieces
        const long long slot = m % h->logCap, run = std::min<long long>(firstWindow + nWindows - m, h->logCap - slot);
        DPE_CHECK_HIP(hipMemcpy((char *)out + (size_t)(m - firstWindow) * rowBytes, (const char *)h->log_d + (size_t)slot * rowBytes, (size_t)run * rowBytes,
                                hipMemcpyDeviceToHost));
        m += run;
    }
    return 0;
}

int dpe_trk_state(dpe_trk *h, dpe_trk_chan_state *out, dpe_stream_t stream_)
{
    using namespace dpe;
    DPE_REQUIRE(h && out, "[ScalarTracker] state: null argument");
    hipStream_t st = (hipStream_t)stream_;
    DPE_CHECK_HIP(hipStreamSynchronize(st));
    std::vector<TrkState> s(h->K);
    DPE_CHECK_HIP(hipMemcpy(s.data(), h->state_d, sizeof(TrkState) * h->K, hipMemcpyDeviceToHost));
    for (int k = 0; k < h->K; ++k) {
        dpe_trk_chan_state &o = out[k];
        o.prn = h->cfg.prn[k]; o.lock = (int32_t)s[k].lock; o.frozen = (int32_t)s[k].frozen; o.reserved = 0;
        o.cp = s[k].cpcount; o.nWindows = s[k].nWindows; o.nSigns = s[k].nSigns;
        o.rc = s[k].rc; o.ri = s[k].ri; o.fc = s[k].fc; o.fi = s[k].fi; o.fc_bias = s[k].fc_bias; o.fi_bias = s[k].fi_bias;
        o.paRe = s[k].paRe; o.paIm = s[k].paIm;
    }
    return 0;
}

int dpe_trk_read_cp_signs(dpe_trk *h, int32_t chan, int64_t first, int32_t n, int8_t *out, dpe_stream_t stream_)
{
    using namespace dpe;
    DPE_REQUIRE(h && out && chan >= 0 && chan < h->K, "[ScalarTracker] read_cp_signs: bad argument");
    hipStream_t st = (hipStream_t)stream_;
    DPE_CHECK_HIP(hipStreamSynchronize(st));
    TrkState s;
    DPE_CHECK_HIP(hipMemcpy(&s, h->state_d + chan, sizeof(TrkState), hipMemcpyDeviceToHost));
    DPE_REQUIRE(first >= 0 && n >= 0 && first + n <= s.nSigns, "[ScalarTracker] read_cp_signs: signs [%lld, %lld) of %lld", (long long)first,
                (long long)(first + n), s.nSigns);
    DPE_REQUIRE(first >= s.nSigns - h->signCap, "[ScalarTracker] read_cp_signs: sign %lld has left the stream's buffer", (long long)first);
    for (long long i = first; i < first + n;) {
        const long long slot = i % h->signCap, run = std::min<long long>(first + n - i, h->signCap - slot);
        DPE_CHECK_HIP(hipMemcpy(out + (i - first), h->signs_d + (size_t)chan * h->signCap + slot, (size_t)run, hipMemcpyDeviceToHost));
        i += run;
    }
    return 0;
}

int dpe_trk_dev_status(dpe_trk *h, int32_t *status, dpe_stream_t stream_)
{
    DPE_REQUIRE(h && status, "[ScalarTracker] dev_status: null argument");
    hipStream_t st = (hipStream_t)stream_;
    DPE_CHECK_HIP(hipStreamSynchronize(st));
    int v = 0;
    DPE_CHECK_HIP(hipMemcpy(&v, h->status_d, sizeof(int), hipMemcpyDeviceToHost));
    *status = v;
    return 0;
}

}  // extern "C"
