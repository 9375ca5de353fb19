// dpe_syn.hip -- the dpe_syn_ family: seeded interleaved int16 I/Q written straight into a device buffer from channel parameters.
//
// The signal model is synth.py's (gen_iq for windows, gen_iq_record for a continuous record; correlator.py:367-465 and
// rawfile.py:140-158 on the reference's side): per channel a C/A chip, a nav-bit sign and a carrier, summed, plus white Gaussian noise
// and a DC offset, rounded to nearest even and clipped to int16.  What decides WHICH chip and WHICH sign a sample gets -- the sample
// time, floor(t fc + rc), its quotient and remainder by 1023, the nav-bit index -- is IEEE fp64 with multiply and add unfused, numpy's
// values in every bit (dpe_syn_plan.h); the carrier's cycle fraction is fp64 too.  Sine, cosine, logarithm and the sums are fp32.
// The noise is counter-based (Philox4x32-10 on {sample index, stream id} under the seed), so a sample depends on nothing but its
// triple (seed, stream, index): not on launch geometry, chunking or batch position.  DESIGN.md 7f.
#include "dpe_common.h"
#include "dpe_syn_plan.h"

namespace dpe {

struct SynArgs {
    long long strideSamples;       // I/Q pairs between the first samples of consecutive segments
    long long firstSample;         // record form: absolute index of the segment's sample 0
    unsigned long long stream0;    // stream id of segment 0; segment w uses stream0 + w
    double fs;
    int S, K, blocksPerSeg, maxNavBits;
    float sigma, dcI, dcQ;
    unsigned seedLo, seedHi;
};

// Philox4x32-10 (Salmon et al., SC'11): counter {c0..c3}, key {k0, k1}; the first two output words.
__device__ __forceinline__ void philox2(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned &w0, unsigned &w1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w0 = c0;
    w1 = c1;
}

// One block: samples [i0, i1) of one segment (syn_block_range).  RECORD: t = n / fs with the absolute index n, nav bits from the
// handle's bit arrays, noise counter n.  Window form: t = rint(i / fs 1e9) / 1e9, one sign change at flipAt, noise counter i.
template <bool RECORD>
__global__ __launch_bounds__(kSynThreads) void syn_kernel(int16_t *__restrict__ out, const SynChan *__restrict__ chan,
                                                          const int8_t *__restrict__ chipsAll, const int8_t *__restrict__ bits, SynArgs a)
{
    extern __shared__ int8_t sChips[];   // [K][kSynChipPitch]
    const int seg = blockIdx.x / a.blocksPerSeg, j = blockIdx.x - seg * a.blocksPerSeg;
    const int tid = threadIdx.x;
    int *__restrict__ o = reinterpret_cast<int *>(out) + (long long)seg * a.strideSamples;
    const int align = (int)((reinterpret_cast<uintptr_t>(o) >> 2) & 3);
    int i0, i1;
    syn_block_range(a.S, align, j, i0, i1);
    if (i0 >= i1) return;
    const SynChan *__restrict__ ch = chan + (long long)seg * a.K;
    for (int k = 0; k < a.K; ++k)   // a row is 256 dwords: one per lane
        reinterpret_cast<int *>(sChips)[k * (kSynChipPitch / 4) + tid] = reinterpret_cast<const int *>(chipsAll)[ch[k].prnRow * (kSynChipPitch / 4) + tid];
    __syncthreads();
    const unsigned long long stream = a.stream0 + (unsigned long long)seg;

    for (int it = 0; it < kSynBlockGroups / kSynThreads; ++it) {
        const int is = (j * kSynBlockGroups + it * kSynThreads + tid) * kSynLaneSamples - align;   // the group's first sample (may be < 0)
        if (is >= a.S || is + kSynLaneSamples <= 0) continue;
        double t[kSynLaneSamples];
        float accI[kSynLaneSamples], accQ[kSynLaneSamples];
#pragma unroll
        for (int m = 0; m < kSynLaneSamples; ++m) {
            const int i = min(max(is + m, 0), a.S - 1);   // samples outside the segment are computed at its edge and not stored
            t[m] = RECORD ? syn_time_record(a.firstSample + i, a.fs) : syn_time_window(i, a.fs);
            accI[m] = accQ[m] = 0.f;
        }
        for (int k = 0; k < a.K; ++k) {
            const SynChan c = ch[k];
            const int8_t *__restrict__ row = sChips + k * kSynChipPitch;
#pragma unroll
            for (int m = 0; m < kSynLaneSamples; ++m) {
                double period;
                const int chip = min(max(syn_chip(t[m], c.fc, c.rc, period), 0), kLCA - 1);
                float sc = (float)row[chip];
                if (RECORD) {
                    const int b = min(max((int)syn_bit_index(period, c.firstEdge), 0), a.maxNavBits - 1);   // (the host refused what would clamp)
                    sc *= (float)bits[(long long)k * a.maxNavBits + b];
                } else if (is + m >= c.flipAt) {
                    sc = -sc;
                }
                double fr;
                {
                    DPE_SYN_FP
                    const double prod = c.fi * t[m];
                    const double ph = prod + c.ri;
                    fr = ph - floor(ph);          // [0, 1]
                }
                if (fr > 0.5) fr -= 1.0;          // exact; the same angle, and the fp32 value below keeps one more bit
                float sn, cs;
                sincospif(2.f * (float)fr, &sn, &cs);
                const float av = c.amp * sc;
                accI[m] = fmaf(av, cs, accI[m]);
                accQ[m] = fmaf(av, sn, accQ[m]);
            }
        }
        int v[kSynLaneSamples];
#pragma unroll
        for (int m = 0; m < kSynLaneSamples; ++m) {
            float xI = accI[m], xQ = accQ[m];
            if (a.sigma != 0.f) {
                const unsigned long long n = RECORD ? (unsigned long long)(a.firstSample + min(max(is + m, 0), a.S - 1))
                                                    : (unsigned long long)min(max(is + m, 0), a.S - 1);
                unsigned w0, w1;
                philox2((unsigned)n, (unsigned)(n >> 32), (unsigned)stream, (unsigned)(stream >> 32), a.seedLo, a.seedHi, w0, w1);
                const float u1 = (float)((w0 >> 8) + 1u) * 0x1p-24f;   // (0, 1]: exact
                const float u2 = (float)(w1 >> 8) * 0x1p-24f;          // [0, 1): exact
                const float r = sqrtf(-2.f * logf(u1));                // at most sqrt(48 ln 2) = 5.77
                float sn, cs;
                sincospif(2.f * u2, &sn, &cs);
                xI = fmaf(a.sigma, r * cs, xI);
                xQ = fmaf(a.sigma, r * sn, xQ);
            }
            xI += a.dcI;
            xQ += a.dcQ;
            const int qi = (int)fminf(fmaxf(rintf(xI), -32768.f), 32767.f);
            const int qq = (int)fminf(fmaxf(rintf(xQ), -32768.f), 32767.f);
            v[m] = (qi & 0xFFFF) | (qq << 16);
        }
        if (is >= 0 && is + kSynLaneSamples <= a.S) {
            *reinterpret_cast<int4 *>(o + is) = make_int4(v[0], v[1], v[2], v[3]);   // 16-byte aligned by the choice of `is`
        } else {
#pragma unroll
            for (int m = 0; m < kSynLaneSamples; ++m)
                if (is + m >= 0 && is + m < a.S) o[is + m] = v[m];
        }
    }
}

}  // namespace dpe

using namespace dpe;

struct dpe_syn {
    dpe_syn_config cfg{};
    int8_t *chips_d = nullptr;    // [37][kSynChipPitch]
    int8_t *bits_d = nullptr;     // [maxChannels][maxNavBits]
    std::vector<int32_t> nBits;   // per channel slot, as last set
    // pinned parameter staging and its device copies: a ring of kStaging blocks, each guarded by an event recorded behind the launch
    // that reads it -- calls may be issued kStaging - 1 deep before one waits for an earlier one
    static constexpr int kStaging = 4;
    SynChan *stage_h = nullptr, *stage_hd = nullptr, *chan_d = nullptr;
    hipEvent_t stagingFree[kStaging] = {};
    int slot = 0;
    size_t slotLen() const { return (size_t)cfg.maxSegments * cfg.maxChannels; }
};

namespace {

int syn_check_common(const char *who, dpe_syn *h, const int16_t *out_dev, int nChan, const dpe_chan_start *chan, const double *amp,
                     const dpe_syn_signal *sig)
{
    DPE_REQUIRE(h != nullptr, "[Synthesizer] %s: null handle", who);
    DPE_REQUIRE(out_dev != nullptr, "[Synthesizer] %s: null output", who);
    DPE_REQUIRE((reinterpret_cast<uintptr_t>(out_dev) & 3) == 0, "[Synthesizer] %s: the output is not aligned to an I/Q pair (4 bytes)", who);
    DPE_REQUIRE(nChan >= 1 && nChan <= h->cfg.maxChannels, "[Synthesizer] %s: nChan %d outside 1..%d (the handle's maximum)", who, nChan,
                h->cfg.maxChannels);
    DPE_REQUIRE(chan && amp && sig, "[Synthesizer] %s: null channel parameters, amplitudes or signal block", who);
    DPE_REQUIRE(std::isfinite(sig->sigma) && sig->sigma >= 0.0 && std::isfinite(sig->dcI) && std::isfinite(sig->dcQ),
                "[Synthesizer] %s: sigma negative or not finite, or a DC offset not finite", who);
    return 0;
}

// stages `n` parameter blocks (already written to the slot) and launches; records the slot's event behind the launch
template <bool RECORD>
int syn_launch(dpe_syn *h, int16_t *out_dev, const SynArgs &a, int nSeg, hipStream_t stream)
{
    const SynGeom g = syn_geom(a.S, nSeg, a.K);
    DPE_REQUIRE(g.nBlocks <= 0x7fffffffLL, "[Synthesizer] %lld blocks in one launch: split the call", g.nBlocks);
    SynChan *dst = h->chan_d + (size_t)h->slot * h->slotLen();
    upload_params(dst, h->stage_hd + (size_t)h->slot * h->slotLen(), sizeof(SynChan) * (size_t)nSeg * a.K, stream);
    syn_kernel<RECORD><<<dim3((unsigned)g.nBlocks), dim3(kSynThreads), g.ldsBytes, stream>>>(out_dev, dst, h->chips_d, h->bits_d, a);
    DPE_CHECK_HIP(hipGetLastError());
    DPE_CHECK_HIP(hipEventRecord(h->stagingFree[h->slot], stream));
    return 0;
}

SynChan *syn_next_slot(dpe_syn *h)
{
    h->slot = (h->slot + 1) % dpe_syn::kStaging;
    if (hipEventSynchronize(h->stagingFree[h->slot]) != hipSuccess) return nullptr;   // returns at once unless kStaging calls are in flight
    return h->stage_h + (size_t)h->slot * h->slotLen();
}

SynArgs syn_args(const dpe_syn *h, const dpe_syn_signal *sig, int S, int K)
{
    SynArgs a{};
    a.fs = h->cfg.samplingFrequency;
    a.S = S;
    a.K = K;
    a.blocksPerSeg = syn_geom(S, 1, K).blocksPerSeg;
    a.maxNavBits = h->cfg.maxNavBits > 0 ? h->cfg.maxNavBits : 1;
    a.sigma = (float)sig->sigma;
    a.dcI = (float)sig->dcI;
    a.dcQ = (float)sig->dcQ;
    a.seedLo = (unsigned)(sig->seed & 0xFFFFFFFFull);
    a.seedHi = (unsigned)(sig->seed >> 32);
    return a;
}

}  // namespace

extern "C" {

int dpe_syn_create(const dpe_syn_config *cfg, dpe_syn **out)
{
    DPE_REQUIRE(cfg && out, "[Synthesizer] create: null argument");
    DPE_REQUIRE(std::isfinite(cfg->samplingFrequency) && cfg->samplingFrequency > 0.0, "[Synthesizer] create: sampling frequency not positive");
    DPE_REQUIRE(cfg->maxSegments >= 1 && cfg->maxSegments <= 65536, "[Synthesizer] create: maxSegments %d outside 1..65536", cfg->maxSegments);
    DPE_REQUIRE(cfg->maxChannels >= 1 && cfg->maxChannels <= DPE_MAX_CHAN, "[Synthesizer] create: maxChannels %d outside 1..%d", cfg->maxChannels,
                DPE_MAX_CHAN);
    DPE_REQUIRE(cfg->maxNavBits >= 0 && cfg->maxNavBits <= (1 << 24), "[Synthesizer] create: maxNavBits %d outside 0..2^24", cfg->maxNavBits);
    dpe_syn *h = new dpe_syn;
    h->cfg = *cfg;
    h->nBits.assign(cfg->maxChannels, 0);
    const size_t bitBytes = (size_t)cfg->maxChannels * (cfg->maxNavBits > 0 ? cfg->maxNavBits : 1);
    const size_t ringBytes = dpe_syn::kStaging * h->slotLen() * sizeof(SynChan);
    bool ok = hipMalloc((void **)&h->chips_d, (size_t)kPrnMax * kSynChipPitch) == hipSuccess && hipMalloc((void **)&h->bits_d, bitBytes) == hipSuccess &&
              hipMalloc((void **)&h->chan_d, ringBytes) == hipSuccess && hipHostMalloc((void **)&h->stage_h, ringBytes, hipHostMallocDefault) == hipSuccess &&
              hipHostGetDevicePointer((void **)&h->stage_hd, h->stage_h, 0) == hipSuccess;
    for (int i = 0; ok && i < dpe_syn::kStaging; ++i) ok = hipEventCreateWithFlags(&h->stagingFree[i], hipEventDisableTiming) == hipSuccess;
    if (ok) {
        std::vector<int8_t> chips((size_t)kPrnMax * kSynChipPitch, 0);
        for (int prn = 1; prn <= kPrnMax; ++prn) gen_ca_code_host(prn, chips.data() + (size_t)(prn - 1) * kSynChipPitch);
        ok = hipMemcpy(h->chips_d, chips.data(), chips.size(), hipMemcpyHostToDevice) == hipSuccess && hipMemset(h->bits_d, 1, bitBytes) == hipSuccess;
    }
    if (!ok) {
        const hipError_t e = hipGetLastError();
        dpe_syn_destroy(h);
        set_error("[Synthesizer] create: no device memory, pinned memory or events (%s)", hipGetErrorString(e));
        return -1;
    }
    *out = h;
    return 0;
}

int dpe_syn_destroy(dpe_syn *h)
{
    if (!h) return 0;
    for (hipEvent_t e : h->stagingFree)
        if (e) {
            (void)hipEventSynchronize(e);
            (void)hipEventDestroy(e);
        }
    if (h->chips_d) (void)hipFree(h->chips_d);
    if (h->bits_d) (void)hipFree(h->bits_d);
    if (h->chan_d) (void)hipFree(h->chan_d);
    if (h->stage_h) (void)hipHostFree(h->stage_h);
    delete h;
    return 0;
}

int dpe_syn_set_nav_bits(dpe_syn *h, int32_t chan, const int8_t *bits, int32_t nBits, dpe_stream_t stream_)
{
    DPE_REQUIRE(h && bits, "[Synthesizer] set_nav_bits: null argument");
    DPE_REQUIRE(chan >= 0 && chan < h->cfg.maxChannels, "[Synthesizer] set_nav_bits: channel %d outside 0..%d", chan, h->cfg.maxChannels - 1);
    DPE_REQUIRE(nBits >= 1 && nBits <= h->cfg.maxNavBits, "[Synthesizer] set_nav_bits: %d bits outside 1..%d (the handle's maximum)", nBits,
                h->cfg.maxNavBits);
    for (int i = 0; i < nBits; ++i) DPE_REQUIRE(bits[i] == 1 || bits[i] == -1, "[Synthesizer] set_nav_bits: bit %d of channel %d is not +-1", i, chan);
    const hipStream_t stream = (hipStream_t)stream_;
    DPE_CHECK_HIP(hipMemcpyAsync(h->bits_d + (size_t)chan * h->cfg.maxNavBits, bits, (size_t)nBits, hipMemcpyHostToDevice, stream));
    DPE_CHECK_HIP(hipStreamSynchronize(stream));   // `bits` is the caller's, and pageable
    h->nBits[chan] = nBits;
    return 0;
}

int dpe_syn_windows(dpe_syn *h, int16_t *out_dev, int64_t strideInt16, int32_t nWindows, int32_t S, int32_t nChan, const dpe_chan_start *chan_host,
                    const double *amp, const dpe_syn_signal *sig, const uint8_t *flip, uint64_t firstStream, dpe_stream_t stream_)
{
    if (syn_check_common("windows", h, out_dev, nChan, chan_host, amp, sig)) return -1;
    DPE_REQUIRE(nWindows >= 1 && nWindows <= h->cfg.maxSegments, "[Synthesizer] windows: nWindows %d outside 1..%d (the handle's maximum)", nWindows,
                h->cfg.maxSegments);
    DPE_REQUIRE(S >= 1 && S <= (1 << 30), "[Synthesizer] windows: S %d outside 1..2^30", S);
    DPE_REQUIRE((strideInt16 & 1) == 0, "[Synthesizer] windows: odd stride %lld (int16 values: an I/Q pair is two)", (long long)strideInt16);
    DPE_REQUIRE(nWindows == 1 || strideInt16 >= 2 * (int64_t)S, "[Synthesizer] windows: stride %lld below 2 S = %lld", (long long)strideInt16,
                2 * (long long)S);
    const double fs = h->cfg.samplingFrequency, tLast = syn_time_window(S - 1, fs);
    for (int i = 0; i < nWindows * nChan; ++i) {
        const dpe_chan_start &c = chan_host[i];
        const char *why = syn_chan_problem(c, amp[i % nChan]);
        if (why) {
            char fmt[160];
            snprintf(fmt, sizeof(fmt), "[Synthesizer] windows: window %d, %s", i / nChan, why);
            set_error(fmt, i % nChan);
            return -1;
        }
        DPE_REQUIRE(std::fabs(c.codePhaseStart) < kSynMaxChips && std::fabs(tLast * c.codeFrequency + c.codePhaseStart) < kSynMaxChips,
                    "[Synthesizer] windows: window %d, channel %d: code phase beyond 2^51 chips", i / nChan, i % nChan);
    }
    SynChan *st = syn_next_slot(h);
    DPE_REQUIRE(st != nullptr, "[Synthesizer] windows: waiting for a staging block failed");
    for (int i = 0; i < nWindows * nChan; ++i) {
        const dpe_chan_start &c = chan_host[i];
        const int64_t at = (flip && flip[i]) ? syn_flip_at(c.cpElapsedStart, c.cpReference, c.codePhaseStart, c.codeFrequency, fs) : 0;
        st[i] = syn_chan(c, amp[i % nChan], at, S);
    }
    SynArgs a = syn_args(h, sig, S, nChan);
    a.strideSamples = strideInt16 / 2;
    a.stream0 = firstStream;
    return syn_launch<false>(h, out_dev, a, nWindows, (hipStream_t)stream_);
}

int dpe_syn_record(dpe_syn *h, int16_t *out_dev, int64_t firstSample, int64_t nSamples, int32_t nChan, const dpe_chan_start *chan_host,
                   const double *amp, const dpe_syn_signal *sig, uint64_t streamId, dpe_stream_t stream_)
{
    if (syn_check_common("record", h, out_dev, nChan, chan_host, amp, sig)) return -1;
    DPE_REQUIRE(nSamples >= 1 && nSamples <= (1 << 30), "[Synthesizer] record: %lld samples outside 1..2^30 per call", (long long)nSamples);
    DPE_REQUIRE(firstSample >= 0 && firstSample <= (INT64_C(1) << 52), "[Synthesizer] record: first sample %lld outside 0..2^52", (long long)firstSample);
    const double fs = h->cfg.samplingFrequency;
    for (int k = 0; k < nChan; ++k) {
        const char *why = syn_chan_problem(chan_host[k], amp[k]);
        if (why) {
            char fmt[160];
            snprintf(fmt, sizeof(fmt), "[Synthesizer] record: %s", why);
            set_error(fmt, k);
            return -1;
        }
        int64_t b0 = 0, b1 = 0;
        DPE_REQUIRE(syn_bit_span(firstSample, nSamples, fs, chan_host[k], b0, b1), "[Synthesizer] record: channel %d: code phase beyond 2^51 chips", k);
        DPE_REQUIRE(b0 >= 0, "[Synthesizer] record: channel %d: the first sample lies before nav bit 0 (negative code phase)", k);
        DPE_REQUIRE(b1 < h->nBits[k], "[Synthesizer] record: channel %d needs %lld nav bits for its last sample, has %d (dpe_syn_set_nav_bits)", k,
                    (long long)(b1 + 1), h->nBits[k]);
    }
    SynChan *st = syn_next_slot(h);
    DPE_REQUIRE(st != nullptr, "[Synthesizer] record: waiting for a staging block failed");
    for (int k = 0; k < nChan; ++k) st[k] = syn_chan(chan_host[k], amp[k], 0, 0);
    SynArgs a = syn_args(h, sig, (int)nSamples, nChan);
    a.firstSample = firstSample;
    a.stream0 = streamId;
    return syn_launch<true>(h, out_dev, a, 1, (hipStream_t)stream_);
}

}  // extern "C"
