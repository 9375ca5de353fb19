// dpe_vt.hip -- vector tracking for MI355X (gfx950): all channels steered by one 8-state navigation filter, on the device.  The
// twin names the loop (Receiver.vt_init / vt_track / vt_measurement_update / vt_time_update, pygnss/pythonreceiver/receiver.py:545-720)
// but cannot run it; the algorithm is DESIGN.md 7e.  One epoch = N consecutive windows during which the NCOs run open loop, so the
// N x K windows of an epoch are independent:
//   vt_correlate_kernel   grid (N, K), 256 lanes: block (j, k) correlates window j of channel k with rc_j = mod(rc + j fc T, 1023),
//                         ri_j = mod(ri + j fi T, 1) and the epoch's fc, fi, read from the device-resident state -- the scalar tracker's
//                         sample phase, fixed-order fp64 reduction, boundary cases and polarity-resolved combination (dpe_trk_dev.h)
//                         with a carried p_a of zero -- and writes iE qE iP qP iL qL, the case and the completed periods to its slot;
//   vt_filter_kernel      one 64-lane block: dpe_vt_dev.h's epoch on those N x K x 8 doubles -- it writes the next epoch's parameters.
// dpe_vt_track enqueues the 2 nEpochs launches on the caller's stream; the host never waits.  No block waits for another inside a
// kernel: the order correlate -> filter -> correlate is the stream's.  Every write to memory is a plain vector store.
#include <cmath>
#include <cstring>
#include <vector>

#include "dpe_common.h"
#include "dpe_trk_dev.h"
#include "dpe_vt_dev.h"

namespace dpe {

#pragma clang fp contract(off)
__device__ __forceinline__ void vt_window_params(const dpe_vt_chan &c, int j, double T, double &rc, double &ri)
{
    rc = trk_mod(c.rc + (double)j * c.fc * T, (double)kLCA);   // Channel.scalar_time_update (channel.py:179-180), j windows on
    ri = trk_mod(c.ri + (double)j * c.fi * T, 1.0);
}
#pragma clang fp contract(fast)

__global__ __launch_bounds__(kTrkThreads) void vt_correlate_kernel(const int16_t *__restrict__ iq, int S, double fs, double T, const int *__restrict__ prn,
                                                                  const int8_t *__restrict__ chipTable, const dpe_vt_state_rec *__restrict__ st,
                                                                  double *__restrict__ out, int nChan)
{
    __shared__ int8_t sTab[4096];
    __shared__ float sPart[kTrkNQ * kTrkRow];
    __shared__ double sRed[kTrkNQ * 8], sSum[kTrkNQ];
    const int j = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    trk_fill_table(sTab, chipTable, prn[k]);
    const dpe_vt_chan &c = st->chan[k];
    const double fc = c.fc, fi = c.fi;
    double rc, ri;
    vt_window_params(c, j, T, rc, ri);
    int i1, i2;
    double d1, d2;
    const int kase = (fi == fi && ri == ri) ? trk_boundaries(rc, fc, fs, S, i1, i2, d1, d2) : -1;
    __syncthreads();
    float acc[kTrkNQ];
    if (kase >= 0) {
        trk_sample_phase(iq + 2 * (size_t)j * S, S, fs, rc, ri, fc, fi, i1, i2, sTab, acc);
    } else {
#pragma unroll
        for (int q = 0; q < kTrkNQ; ++q) acc[q] = 0.f;
    }
    trk_reduce(acc, sPart, sRed, sSum);
    if (tid == 0) {
        double r[6] = {0, 0, 0, 0, 0, 0}, sg[2] = {0.0, 0.0}, paRe = 0.0, paIm = 0.0;
        int compl_ = 0;
        if (kase >= 0) compl_ = trk_combine(kase, sSum, paRe, paIm, r, sg);
        double *o = out + ((size_t)j * nChan + k) * DPE_VT_CORR_DOUBLES;
        o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; o[3] = r[3]; o[4] = r[4]; o[5] = r[5];
        o[6] = (double)kase; o[7] = (double)compl_;
    }
}

__global__ __launch_bounds__(kVtLanes) void vt_filter_kernel(VtCfg cfg, const VtEph *__restrict__ eph, dpe_vt_state_rec *st, const double *sums,
                                                            double *log, long long logCap)
{
    __shared__ VtWork w;
    double *rec = log + (size_t)(st->epochs % logCap) * DPE_VT_LOG_DOUBLES;
    vt_filter_epoch(cfg, eph, st, sums, rec, w);
}

// the vt_init hand-over: the scalar tracker's parameters of its next window become the channels' state
__global__ __launch_bounds__(kVtLanes) void vt_adopt_kernel(const TrkState *__restrict__ ts, dpe_vt_state_rec *st, int K)
{
    const int k = threadIdx.x;
    if (k >= K) return;
    dpe_vt_chan &c = st->chan[k];
    c.rc = ts[k].rc; c.ri = ts[k].ri; c.fc = ts[k].fc; c.fi = ts[k].fi;
    c.cp = (double)ts[k].cpcount;
    c.histN = 0; c.histPos = 0;
}

static int vt_make_cfg(const dpe_vt_config *cfg, VtCfg &v, int &S)
{
    DPE_REQUIRE(cfg->samplingFrequency > 0 && cfg->T > 0, "[VectorTracker] create: sampling frequency and window length must be positive");
    DPE_REQUIRE(cfg->nChan >= 1, "[VectorTracker] create: nChan must be positive");
    DPE_REQUIRE(cfg->nChan <= DPE_VT_MAX_CHAN, "[VectorTracker] create: at most %d channels (S = H Sigma H^T + W is factored at order 2 K <= 32), got %d",
                DPE_VT_MAX_CHAN, cfg->nChan);
    const int N = cfg->N ? cfg->N : 20;
    DPE_REQUIRE(N >= 2 && N <= DPE_VT_MAX_WINDOWS && N % 2 == 0, "[VectorTracker] create: N must be even and in 2 .. %d (the FLL rule pairs the windows), got %d",
                DPE_VT_MAX_WINDOWS, N);
    DPE_REQUIRE(cfg->T <= 1.5e-3, "[VectorTracker] create: the window must be at most 1.5 ms (the tracker's boundary cases cover one code period)");
    S = (int)llround(cfg->T * cfg->samplingFrequency);
    DPE_REQUIRE(S >= 2 && S % 2 == 0, "[VectorTracker] create: round(T fs) = %d samples per window must be even", S);
    const int numPrev = cfg->numPrev ? cfg->numPrev : 20;
    DPE_REQUIRE(numPrev >= 2 && numPrev <= DPE_VT_MAX_PREV, "[VectorTracker] create: numPrev must be in 2 .. %d", DPE_VT_MAX_PREV);
    for (int i = 0; i < cfg->nChan; ++i)
        DPE_REQUIRE(cfg->prn[i] >= 1 && cfg->prn[i] <= kPrnMax, "[VectorTracker] create: PRN %d out of range", cfg->prn[i]);
    v.fs = cfg->samplingFrequency; v.T = cfg->T;
    v.ds = cfg->dopplerSign != 0.0 ? cfg->dopplerSign : 1.0;
    v.NT = (double)N * cfg->T;
    v.fcaid = v.ds * kFCA / kFL1;
    v.N = N; v.K = cfg->nChan; v.numPrev = numPrev;
    v.roundMs = std::fabs(v.NT * 1000.0 - std::round(v.NT * 1000.0)) < 1e-9 ? 1 : 0;
    v.initVarR = cfg->initVarRange > 0 ? cfg->initVarRange : 225.0;
    v.initVarV = cfg->initVarRate > 0 ? cfg->initVarRate : 1.0;
    v.minVarR = cfg->minVarRange > 0 ? cfg->minVarRange : (cfg->minVarRange < 0 ? 0.0 : 1.0);
    v.minVarV = cfg->minVarRate > 0 ? cfg->minVarRate : (cfg->minVarRate < 0 ? 0.0 : 0.01);
    bool anyQ = false;
    for (int i = 0; i < 8; ++i) anyQ = anyQ || cfg->qDiag[i] != 0.0;
    // ekf.py:58-70 at v clamped to 50: 1 + 250 / 50 on the velocities, ((2.5e-10) c)^2 on the clock drift
    const double qDef[8] = {0.0, 0.0, 0.0, 0.0, 6.0, 6.0, 6.0, (2.5e-10 * kC) * (2.5e-10 * kC)};
    for (int i = 0; i < 8; ++i) v.q[i] = anyQ ? cfg->qDiag[i] : qDef[i];
    v.lockThr = cfg->lockThreshold > 0 ? cfg->lockThreshold : 4.0;
    return 0;
}

static void vt_fill_eph(VtEph *e, int K, const double *eph, const int32_t *tow, const int64_t *cp)
{
    for (int k = 0; k < K; ++k) {
        std::memcpy(&e[k].eph, eph + (size_t)k * DPE_NAV_EPH_DOUBLES, sizeof(double) * DPE_NAV_EPH_DOUBLES);
        e[k].tow = (double)tow[k];
        e[k].cps = (double)cp[k];
    }
}

}  // namespace dpe

static_assert(sizeof(dpe::Eph) == sizeof(double) * DPE_NAV_EPH_DOUBLES, "Eph is the 21 ephemeris doubles");

struct dpe_vt {
    dpe_vt_config cfg;
    dpe::VtCfg v;
    int S = 0, K = 0;
    long long logCap = 0, epochs = 0;
    bool haveEph = false, haveInit = false;
    int *prn_d = nullptr;
    int8_t *chips_d = nullptr;
    dpe::VtEph *eph_d = nullptr;
    dpe_vt_state_rec *state_d = nullptr;
    double *corr_d = nullptr, *log_d = nullptr;
};

extern "C" {

int dpe_vt_destroy(dpe_vt *h)
{
    if (!h) return 0;
    void *bufs[] = {h->prn_d, h->chips_d, h->eph_d, h->state_d, h->corr_d, h->log_d};
    for (void *b : bufs) (void)hipFree(b);
    delete h;
    return 0;
}

int dpe_vt_create(const dpe_vt_config *cfg, dpe_vt **out)
{
    using namespace dpe;
    DPE_REQUIRE(cfg && out, "[VectorTracker] create: null argument");
    VtCfg v;
    int S = 0;
    if (vt_make_cfg(cfg, v, S)) return -1;
    DPE_REQUIRE(cfg->logCapacityEpochs >= 1, "[VectorTracker] create: logCapacityEpochs must be positive");
    dpe_vt *h = new dpe_vt();
    h->cfg = *cfg;
    h->v = v;
    h->S = S;
    h->K = cfg->nChan;
    h->logCap = cfg->logCapacityEpochs;
    h->prn_d = dev_alloc<int>(DPE_VT_MAX_CHAN);
    h->chips_d = dev_alloc<int8_t>((size_t)kPrnMax * 1024);
    h->eph_d = dev_alloc<VtEph>(DPE_VT_MAX_CHAN);
    h->state_d = dev_alloc<dpe_vt_state_rec>(1);
    h->corr_d = dev_alloc<double>((size_t)DPE_VT_MAX_WINDOWS * DPE_VT_MAX_CHAN * DPE_VT_CORR_DOUBLES);
    h->log_d = dev_alloc<double>((size_t)h->logCap * DPE_VT_LOG_DOUBLES);
    if (!h->prn_d || !h->chips_d || !h->eph_d || !h->state_d || !h->corr_d || !h->log_d) {
        set_error("[VectorTracker] create: device allocation failed");
        dpe_vt_destroy(h);
        return -1;
    }
    std::vector<int8_t> chips((size_t)kPrnMax * 1024, 0);
    for (int p = 1; p <= kPrnMax; ++p) gen_ca_code_host(p, chips.data() + (size_t)(p - 1) * 1024);
    if (hipMemcpy(h->chips_d, chips.data(), chips.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->prn_d, cfg->prn, sizeof(int) * h->K, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(h->state_d, 0, sizeof(dpe_vt_state_rec)) != hipSuccess ||
        hipMemset(h->corr_d, 0, sizeof(double) * DPE_VT_MAX_WINDOWS * DPE_VT_MAX_CHAN * DPE_VT_CORR_DOUBLES) != hipSuccess) {
        set_error("[VectorTracker] create: device initialisation failed");
        dpe_vt_destroy(h);
        return -1;
    }
    *out = h;
    return 0;
}

int dpe_vt_set_ephemerides(dpe_vt *h, const double *eph, const int32_t *tow, const int64_t *cp)
{
    using namespace dpe;
    DPE_REQUIRE(h && eph && tow && cp, "[VectorTracker] set_ephemerides: ephemerides, TOW and cp stamps are all required");
    std::vector<VtEph> e(h->K);
    vt_fill_eph(e.data(), h->K, eph, tow, cp);
    DPE_CHECK_HIP(hipDeviceSynchronize());
    DPE_CHECK_HIP(hipMemcpy(h->eph_d, e.data(), sizeof(VtEph) * h->K, hipMemcpyHostToDevice));
    h->haveEph = true;
    return 0;
}

static int vt_upload_head(dpe_vt *h, const double *X, const double *Sigma, double rxTime0, const double *chan, hipStream_t st)
{
    std::vector<dpe_vt_state_rec> buf(1);
    dpe_vt_state_rec &s = buf[0];
    std::memset(&s, 0, sizeof(s));
    for (int i = 0; i < 8; ++i) s.X[i] = X[i];
    for (int i = 0; i < 64; ++i) s.Sigma[i] = Sigma[i];
    s.rxTime0 = s.rxBase = rxTime0;
    if (chan)
        for (int k = 0; k < h->K; ++k) {
            dpe_vt_chan &c = s.chan[k];
            c.rc = chan[5 * k]; c.ri = chan[5 * k + 1]; c.fc = chan[5 * k + 2]; c.fi = chan[5 * k + 3]; c.cp = chan[5 * k + 4];
        }
    DPE_CHECK_HIP(hipStreamSynchronize(st));
    DPE_CHECK_HIP(hipMemcpy(h->state_d, &s, sizeof(s), hipMemcpyHostToDevice));
    h->epochs = 0;
    h->haveInit = true;
    return 0;
}

int dpe_vt_init(dpe_vt *h, const double *X, const double *Sigma, double rxTime0, const double *chan, dpe_stream_t stream_)
{
    DPE_REQUIRE(h && X && Sigma && chan, "[VectorTracker] init: null argument");
    return vt_upload_head(h, X, Sigma, rxTime0, chan, (hipStream_t)stream_);
}

int dpe_vt_init_from_trk(dpe_vt *h, dpe_trk *trk, const dpe_nav_fix *fix, dpe_stream_t stream_)
{
    using namespace dpe;
    DPE_REQUIRE(h && trk && fix, "[VectorTracker] init_from_trk: null argument");
    TrkStateView v;
    if (trk_state_view(trk, &v)) return -1;
    DPE_REQUIRE(v.K == h->K, "[VectorTracker] init_from_trk: the tracker has %d channels, the vector tracker %d", v.K, h->K);
    DPE_REQUIRE(v.haveParams, "[VectorTracker] init_from_trk: the tracker holds no loop state (set_params has not been called)");
    DPE_REQUIRE(v.fs == h->v.fs, "[VectorTracker] init_from_trk: the tracker's sampling frequency differs");
    for (int k = 0; k < h->K; ++k)
        DPE_REQUIRE(v.prn[k] == h->cfg.prn[k], "[VectorTracker] init_from_trk: channel %d is PRN %d in the tracker, PRN %d here", k, v.prn[k], h->cfg.prn[k]);
    double Sigma[64];
    for (int i = 0; i < 64; ++i) Sigma[i] = 0.0;
    for (int i = 0; i < 8; ++i) {
        const double d = h->cfg.initSigmaDiag[i];
        Sigma[i * 9] = d > 0 ? d : ((i & 4) ? 1.0 : 1.0e4);
    }
    // the fix belongs to the start of the tracker's last window, the loop state to its end: one window of the constant-velocity model
    double X[8];
    for (int i = 0; i < 8; ++i) X[i] = i < 4 ? fix->X_ECEF[i] + v.T * fix->X_ECEF[i + 4] : fix->X_ECEF[i];
    hipStream_t st = (hipStream_t)stream_;
    if (vt_upload_head(h, X, Sigma, fix->rxTime + v.T, nullptr, st)) return -1;
    hipLaunchKernelGGL(vt_adopt_kernel, dim3(1), dim3(kVtLanes), 0, st, v.state, h->state_d, h->K);
    DPE_CHECK_HIP(hipGetLastError());
    return 0;
}

int dpe_vt_track(dpe_vt *h, const int16_t *samples_dev, int32_t nEpochs, dpe_stream_t stream_)
{
    using namespace dpe;
    DPE_REQUIRE(h && samples_dev, "[VectorTracker] track: null argument");
    DPE_REQUIRE(h->haveEph, "[VectorTracker] track: set_ephemerides has not been called");
    DPE_REQUIRE(h->haveInit, "[VectorTracker] track: init has not been called");
    DPE_REQUIRE(nEpochs >= 1, "[VectorTracker] track: nEpochs must be positive");
    hipStream_t st = (hipStream_t)stream_;
    const size_t epochSamples = (size_t)h->v.N * h->S;
    for (int e = 0; e < nEpochs; ++e) {
        hipLaunchKernelGGL(vt_correlate_kernel, dim3(h->v.N, h->K), dim3(kTrkThreads), 0, st, samples_dev + 2 * (size_t)e * epochSamples, h->S, h->v.fs,
                           h->v.T, h->prn_d, h->chips_d, h->state_d, h->corr_d, h->K);
        hipLaunchKernelGGL(vt_filter_kernel, dim3(1), dim3(kVtLanes), 0, st, h->v, h->eph_d, h->state_d, h->corr_d, h->log_d, h->logCap);
    }
    DPE_CHECK_HIP(hipGetLastError());
    h->epochs += nEpochs;
    return 0;
}

int dpe_vt_read_log(dpe_vt *h, int64_t firstEpoch, int32_t nEpochs, double *out, dpe_stream_t stream_)
{
    DPE_REQUIRE(h && out, "[VectorTracker] read_log: null argument");
    DPE_REQUIRE(firstEpoch >= 0 && nEpochs >= 0 && firstEpoch + nEpochs <= h->epochs, "[VectorTracker] read_log: epochs [%lld, %lld) have not been tracked",
                (long long)firstEpoch, (long long)(firstEpoch + nEpochs));
    DPE_REQUIRE(firstEpoch >= h->epochs - h->logCap, "[VectorTracker] read_log: epoch %lld has left the log (capacity %lld)", (long long)firstEpoch, h->logCap);
    hipStream_t st = (hipStream_t)stream_;
    DPE_CHECK_HIP(hipStreamSynchronize(st));
    const size_t rowBytes = (size_t)DPE_VT_LOG_DOUBLES * sizeof(double);
    for (long long m = firstEpoch; m < firstEpoch + nEpochs;) {   // the log is a ring: at most two pieces
        const long long slot = m % h->logCap, run = std::min<long long>(firstEpoch + nEpochs - m, h->logCap - slot);
        DPE_CHECK_HIP(hipMemcpy((char *)out + (size_t)(m - firstEpoch) * rowBytes, (const char *)h->log_d + (size_t)slot * rowBytes, (size_t)run * rowBytes,
                                hipMemcpyDeviceToHost));
        m += run;
    }
    return 0;
}

int dpe_vt_read_corr(dpe_vt *h, double *out, dpe_stream_t stream_)
{
    DPE_REQUIRE(h && out, "[VectorTracker] read_corr: null argument");
    hipStream_t st = (hipStream_t)stream_;
    DPE_CHECK_HIP(hipStreamSynchronize(st));
    DPE_CHECK_HIP(hipMemcpy(out, h->corr_d, sizeof(double) * (size_t)h->v.N * h->K * DPE_VT_CORR_DOUBLES, hipMemcpyDeviceToHost));
    return 0;
}

int dpe_vt_state(dpe_vt *h, dpe_vt_state_rec *out, dpe_stream_t stream_)
{
    DPE_REQUIRE(h && out, "[VectorTracker] state: null argument");
    hipStream_t st = (hipStream_t)stream_;
    DPE_CHECK_HIP(hipStreamSynchronize(st));
    DPE_CHECK_HIP(hipMemcpy(out, h->state_d, sizeof(dpe_vt_state_rec), hipMemcpyDeviceToHost));
    return 0;
}

int dpe_vt_dev_status(dpe_vt *h, int32_t *status, dpe_stream_t stream_)
{
    DPE_REQUIRE(h && status, "[VectorTracker] dev_status: null argument");
    hipStream_t st = (hipStream_t)stream_;
    DPE_CHECK_HIP(hipStreamSynchronize(st));
    int v = 0;
    DPE_CHECK_HIP(hipMemcpy(&v, (const char *)h->state_d + offsetof(dpe_vt_state_rec, status), sizeof(int), hipMemcpyDeviceToHost));
    *status = v;
    return 0;
}

int dpe_vt_filter_step_host(const dpe_vt_config *cfg, const double *eph, const int32_t *tow, const int64_t *cp, dpe_vt_state_rec *st,
                            const double *sums, double *rec)
{
    using namespace dpe;
    DPE_REQUIRE(cfg && eph && tow && cp && st && sums && rec, "[VectorTracker] filter_step_host: null argument");
    VtCfg v;
    int S = 0;
    if (vt_make_cfg(cfg, v, S)) return -1;
    for (int k = 0; k < v.K; ++k)
        DPE_REQUIRE(st->chan[k].histN >= 0 && st->chan[k].histN <= v.numPrev && st->chan[k].histPos >= 0 && st->chan[k].histPos < v.numPrev,
                    "[VectorTracker] filter_step_host: channel %d's residual history (histN %d, histPos %d) does not fit numPrev %d", k,
                    st->chan[k].histN, st->chan[k].histPos, v.numPrev);
    std::vector<VtEph> e(v.K);
    vt_fill_eph(e.data(), v.K, eph, tow, cp);
    std::vector<VtWork> w(1);
    vt_filter_epoch(v, e.data(), st, sums, rec, w[0]);
    return 0;
}

}  // extern "C"
