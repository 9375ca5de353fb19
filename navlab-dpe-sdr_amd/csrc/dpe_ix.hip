// dpe_ix.hip -- the dpe_ix_ family: interference excision on complex baseband samples in a device buffer, written at the same rate
// into a device buffer.  Pulse blanker, windowed half-overlapped transform, detection against the frame's lower median power,
// zeroing, inverse transform and overlap-add in one kernel; a frame lives in the LDS from its load to its store.  DESIGN.md 7i.
//
// A block owns kIxHopsPerBlock consecutive hops (dpe_ix_plan.h) and computes the frames they need one after the other: stage
// (blanked, windowed), transform forwards in place (radix 2, decimation in frequency, two stages per pass; the spectrum stays in
// bit-reversed order), select the lower median of the powers exactly by a radix select over their bit patterns, mark the detected
// bins in natural order, zero the excised ones, transform backwards (decimation in time, bit-reversed in, natural out), window,
// add the half the lanes carry in registers from the frame before, store.  Element i of a frame is always handled by lane i mod 256
// in the same order of operations, whichever block, launch or call computes the frame: its values depend on the frame's index, the
// handle and the input alone.  dpe_ix_analyse runs the same kernel up to the mask and writes P, m and e instead of going on.
#include "dpe_common.h"
#include "dpe_ix_plan.h"

namespace dpe {

typedef float ix2 __attribute__((ext_vector_type(2)));

struct IxArgs {
    const void *x;              // input sample xFirst begins at byte 0
    void *out;                  // output outFirst at element 0
    const ix2 *tw;              // [N / 2] (ix_twiddles)
    const float *win;           // [N] (ix_window)
    const uint8_t *stat;        // [N] or null
    unsigned long long *counters;   // frames, excised bins, blanked, clipped, then per bin [N]
    float *power, *median;      // analyse: [frames][N], [frames], [frames][N]; each may be null
    uint8_t *mask;
    long long xFirst;
    int64_t lo, hi;             // the input samples that exist and lie in the buffer: [0, recordLength) cut to the buffer's range
    long long outFirst, outEnd;
    long long h0, h1;           // the call's first and last hop (analyse: its first and last frame)
    int N, H, logN, guard, inF32, outF32, analyse;
    unsigned blankWord;
    float blankPower, kappa, gain, invN;
    IxLds lds;
};

__device__ __forceinline__ ix2 ix_add(ix2 a, ix2 b) { return ix2{__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y)}; }
__device__ __forceinline__ ix2 ix_sub(ix2 a, ix2 b) { return ix2{__fsub_rn(a.x, b.x), __fsub_rn(a.y, b.y)}; }
// d w and d conj(w): one multiply and one FMA per part
__device__ __forceinline__ ix2 ix_mul(ix2 d, ix2 w) { return ix2{__fmaf_rn(-d.y, w.y, __fmul_rn(d.x, w.x)), __fmaf_rn(d.x, w.y, __fmul_rn(d.y, w.x))}; }
__device__ __forceinline__ ix2 ix_mulc(ix2 d, ix2 w) { return ix2{__fmaf_rn(d.y, w.y, __fmul_rn(d.x, w.x)), __fmaf_rn(-d.x, w.y, __fmul_rn(d.y, w.x))}; }
__device__ __forceinline__ float ix_power(ix2 v) { return __fmaf_rn(v.y, v.y, __fmul_rn(v.x, v.x)); }

// natural order in, bit-reversed order out; ends behind a barrier
__device__ __forceinline__ void ix_forward(ix2 *__restrict__ s, const ix2 *__restrict__ tw, int N, int tid)
{
    int hf = N >> 1;
    for (; hf >= 2; hf >>= 2) {                 // the stages of half-size hf = 2 q and q
        const int q = hf >> 1, mA = N / (2 * hf), mB = N / hf;
        for (int u = tid; u < (N >> 2); u += kIxThreads) {
            int base, j;
            ix_pair_index(u, q, base, j);
            const ix2 e0 = s[base], e1 = s[base + q], e2 = s[base + 2 * q], e3 = s[base + 3 * q];
            const ix2 wA0 = tw[j * mA], wA1 = tw[(j + q) * mA], wB = tw[j * mB];
            const ix2 a0 = ix_add(e0, e2), a2 = ix_mul(ix_sub(e0, e2), wA0), a1 = ix_add(e1, e3), a3 = ix_mul(ix_sub(e1, e3), wA1);
            s[base] = ix_add(a0, a1);
            s[base + q] = ix_mul(ix_sub(a0, a1), wB);
            s[base + 2 * q] = ix_add(a2, a3);
            s[base + 3 * q] = ix_mul(ix_sub(a2, a3), wB);
        }
        __syncthreads();
    }
    if (hf == 1) {                              // an odd number of stages: the last one alone
        for (int t = tid; t < (N >> 1); t += kIxThreads) {
            int i0, j;
            ix_single_index(t, 1, i0, j);
            const ix2 a = s[i0], b = s[i0 + 1];
            s[i0] = ix_add(a, b);
            s[i0 + 1] = ix_mul(ix_sub(a, b), tw[j * (N >> 1)]);
        }
        __syncthreads();
    }
}

// bit-reversed order in, natural order out, N times the inverse transform; ends behind a barrier
__device__ __forceinline__ void ix_inverse(ix2 *__restrict__ s, const ix2 *__restrict__ tw, int N, int logN, int tid)
{
    int q = 1;
    if (logN & 1) {
        for (int t = tid; t < (N >> 1); t += kIxThreads) {
            int i0, j;
            ix_single_index(t, 1, i0, j);
            const ix2 a = s[i0], b = ix_mulc(s[i0 + 1], tw[j * (N >> 1)]);
            s[i0] = ix_add(a, b);
            s[i0 + 1] = ix_sub(a, b);
        }
        __syncthreads();
        q = 2;
    }
    for (; 4 * q <= N; q <<= 2) {               // the stages of half-size q and 2 q
        const int mA = N / (4 * q), mB = N / (2 * q);
        for (int u = tid; u < (N >> 2); u += kIxThreads) {
            int base, j;
            ix_pair_index(u, q, base, j);
            const ix2 e0 = s[base], e1 = s[base + q], e2 = s[base + 2 * q], e3 = s[base + 3 * q];
            const ix2 wA0 = tw[j * mA], wA1 = tw[(j + q) * mA], wB = tw[j * mB];
            const ix2 b1 = ix_mulc(e1, wB), b3 = ix_mulc(e3, wB);
            const ix2 a0 = ix_add(e0, b1), a1 = ix_sub(e0, b1), a2 = ix_add(e2, b3), a3 = ix_sub(e2, b3);
            const ix2 c2 = ix_mulc(a2, wA0), c3 = ix_mulc(a3, wA1);
            s[base] = ix_add(a0, c2);
            s[base + 2 * q] = ix_sub(a0, c2);
            s[base + q] = ix_add(a1, c3);
            s[base + 3 * q] = ix_sub(a1, c3);
        }
        __syncthreads();
    }
}

// The lower median of the N powers (element N / 2 - 1 of their ascending sort), exactly: non-negative floats order as their bit
// patterns, and four passes fix eight bits each from a 256-bin histogram of the values that share the prefix found so far.
// Called behind a barrier; every lane returns the value.
__device__ __forceinline__ float ix_median(const ix2 *__restrict__ s, unsigned *__restrict__ hist, unsigned *__restrict__ sel, int N, int tid)
{
    if (tid == 0) {
        sel[0] = 0u;
        sel[1] = (unsigned)(N / 2 - 1);
    }
    __syncthreads();
    for (int shift = 24; shift >= 0; shift -= 8) {
        const unsigned prefix = sel[0], rank = sel[1];
        hist[tid] = 0u;
        __syncthreads();
        for (int p = tid; p < N; p += kIxThreads) {
            const unsigned bits = __float_as_uint(ix_power(s[p]));
            if (shift == 24 || (bits >> (shift + 8)) == prefix) atomicAdd(&hist[(bits >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 64) {                         // one wave: four bins per lane, a scan over the lanes, the bin that holds the rank
            const unsigned c0 = hist[4 * tid], c1 = hist[4 * tid + 1], c2 = hist[4 * tid + 2], c3 = hist[4 * tid + 3];
            const unsigned sum = c0 + c1 + c2 + c3;
            unsigned incl = sum;
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned t = __shfl_up(incl, off, 64);
                if (tid >= off) incl += t;
            }
            const unsigned excl = incl - sum;
            if (rank >= excl && rank < incl) {
                unsigned r = rank - excl, d = 0u;
                if (r >= c0) {
                    r -= c0; d = 1u;
                    if (r >= c1) {
                        r -= c1; d = 2u;
                        if (r >= c2) { r -= c2; d = 3u; }
                    }
                }
                sel[0] = (prefix << 8) | (4u * tid + d);
                sel[1] = r;
            }
        }
        __syncthreads();
    }
    return __uint_as_float(sel[0]);
}

__global__ __launch_bounds__(kIxThreads) void ix_kernel(IxArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sRaw[];
    ix2 *__restrict__ s = reinterpret_cast<ix2 *>(sRaw + a.lds.frame);
    unsigned *__restrict__ sPerBin = reinterpret_cast<unsigned *>(sRaw + a.lds.perBin);
    uint8_t *__restrict__ sDet = sRaw + a.lds.detected;
    unsigned *__restrict__ sHist = reinterpret_cast<unsigned *>(sRaw + a.lds.hist);
    unsigned *__restrict__ sSel = reinterpret_cast<unsigned *>(sRaw + a.lds.select);
    unsigned *__restrict__ sCnt = reinterpret_cast<unsigned *>(sRaw + a.lds.counts);
    const int tid = threadIdx.x, N = a.N, H = a.H;
    int64_t ha, hb;
    ix_block_hops(a.h0, a.h1, blockIdx.x, ha, hb);
    const int64_t kLast = a.analyse ? hb : hb + 1;

    for (int f = tid; f < N; f += kIxThreads) sPerBin[f] = 0u;
    if (tid < 4) sCnt[tid] = 0u;                // (the first use lies behind the barriers of the first frame)
    ix2 carry[kIxCarry];
#pragma unroll
    for (int m = 0; m < kIxCarry; ++m) carry[m] = ix2{0.f, 0.f};
    unsigned nFrames = 0, nExcised = 0, nBlanked = 0, nClipped = 0;

    for (int64_t k = ha; k <= kLast; ++k) {
        // ---- stage: frame element i is input (k - 1) H + i, blanked and windowed; zero outside the record
        const long long n0 = (k - 1) * H;
        const bool countBlanked = !a.analyse && k > ha;            // the first half of frame k is hop k - 1, which this block owns
        for (int i = tid; i < N; i += kIxThreads) {
            const long long n = n0 + i;
            ix2 v{0.f, 0.f};
            if (n >= a.lo && n < a.hi) {
                bool blank;
                if (a.inF32) {
                    v = reinterpret_cast<const ix2 *>(a.x)[n - a.xFirst];
                    blank = a.blankPower > 0.f && ix_power(v) > a.blankPower;
                } else {
                    int vi, vq;
                    stream_unpack(reinterpret_cast<const int *>(a.x)[n - a.xFirst], vi, vq);
                    v = ix2{(float)vi, (float)vq};
                    blank = a.blankWord != 0u && (unsigned)(vi * vi) + (unsigned)(vq * vq) > a.blankWord;
                }
                if (blank) {
                    v = ix2{0.f, 0.f};
                    nBlanked += countBlanked && i < H && n >= a.outFirst && n < a.outEnd;
                }
            }
            const float w = a.win[i];
            s[i] = ix2{__fmul_rn(v.x, w), __fmul_rn(v.y, w)};
        }
        __syncthreads();

        ix_forward(s, a.tw, N, tid);

        // ---- detect: position p of the spectrum holds bin f = bitrev(p)
        const float med = ix_median(s, sHist, sSel, N, tid);
        const float thr = __fmul_rn(a.kappa, med);
        for (int p = tid; p < N; p += kIxThreads) sDet[__brev((unsigned)p) >> (32 - a.logN)] = ix_power(s[p]) > thr;
        __syncthreads();
        const bool counted = !a.analyse && k <= hb && ix_counted(k, H, a.outFirst, a.outEnd - a.outFirst);
        nFrames += counted && tid == 0;
        for (int p = tid; p < N; p += kIxThreads) {
            const int f = (int)(__brev((unsigned)p) >> (32 - a.logN));
            bool e = a.stat != nullptr && a.stat[f] != 0;
            for (int d = -a.guard; d <= a.guard && !e; ++d) e = sDet[(f + d) & (N - 1)] != 0;
            if (a.analyse) {
                const long long at = (k - a.h0) * N + f;
                if (a.power) a.power[at] = ix_power(s[p]);
                if (a.mask) a.mask[at] = e;
            }
            if (e) {
                s[p] = ix2{0.f, 0.f};
                if (counted) {
                    ++nExcised;
                    atomicAdd(&sPerBin[f], 1u);
                }
            }
        }
        if (a.analyse) {
            if (tid == 0 && a.median) a.median[k - a.h0] = med;
            __syncthreads();
            continue;
        }
        __syncthreads();

        ix_inverse(s, a.tw, N, a.logN, tid);

        // ---- window, add the carried half of frame k - 1, store hop k - 1; carry this frame's second half
#pragma unroll
        for (int m = 0; m < kIxCarry; ++m) {
            const int r = tid + m * kIxThreads;
            if (r < H) {
                const long long n = n0 + r;
                if (k > ha && n >= a.outFirst && n < a.outEnd) {
                    const float w = a.win[r];
                    const ix2 y = s[r];
                    const ix2 t = ix2{__fmul_rn(w, __fmul_rn(y.x, a.invN)), __fmul_rn(w, __fmul_rn(y.y, a.invN))};
                    const ix2 o = ix2{__fmul_rn(a.gain, __fadd_rn(carry[m].x, t.x)), __fmul_rn(a.gain, __fadd_rn(carry[m].y, t.y))};
                    stream_store(a.out, n - a.outFirst, o.x, o.y, a.outF32, nClipped);
                }
                const float w2 = a.win[r + H];
                const ix2 y2 = s[r + H];
                carry[m] = ix2{__fmul_rn(w2, __fmul_rn(y2.x, a.invN)), __fmul_rn(w2, __fmul_rn(y2.y, a.invN))};
            }
        }
        __syncthreads();
    }
    if (a.analyse) return;

    // ---- the block's counters: one atomic per counter and per excised bin
    if (nFrames) atomicAdd(&sCnt[0], nFrames);
    if (nExcised) atomicAdd(&sCnt[1], nExcised);
    if (nBlanked) atomicAdd(&sCnt[2], nBlanked);
    if (nClipped) atomicAdd(&sCnt[3], nClipped);
    __syncthreads();
    if (tid < 4 && sCnt[tid]) atomicAdd(a.counters + tid, (unsigned long long)sCnt[tid]);
    for (int f = tid; f < N; f += kIxThreads)
        if (sPerBin[f]) atomicAdd(a.counters + 4 + f, (unsigned long long)sPerBin[f]);
}

}  // namespace dpe

using namespace dpe;

struct dpe_ix {
    dpe_ix_config cfg{};
    IxLds lds{};
    int N = 0;
    bool hasStatic = false;
    float *tables_d = nullptr;              // twiddles [N], window [N]
    uint8_t *static_d = nullptr;
    unsigned long long *counters_d = nullptr;   // [4 + N]
    hipStream_t last = nullptr;
};

static IxArgs ix_args(const dpe_ix *h, const void *x_dev, int64_t xFirst, int64_t xCount, int64_t recordLength)
{
    IxArgs a{};
    a.x = x_dev;
    a.tw = reinterpret_cast<const ix2 *>(h->tables_d);
    a.win = h->tables_d + h->N;
    a.stat = h->hasStatic ? h->static_d : nullptr;
    a.counters = h->counters_d;
    a.xFirst = xFirst;
    a.lo = xFirst;
    a.hi = xFirst + xCount;
    stream_cut(recordLength, a.lo, a.hi);
    a.N = h->N;
    a.H = h->N / 2;
    a.logN = ix_log2(h->N);
    a.guard = h->cfg.guard;
    a.inF32 = h->cfg.inputFormat == DPE_IX_IN_F32;
    a.outF32 = h->cfg.outputFormat == DPE_FE_OUT_F32;
    a.blankWord = ix_blank_word(h->cfg.blankPower);
    a.blankPower = (float)h->cfg.blankPower;
    a.kappa = (float)h->cfg.threshold;
    a.gain = (float)h->cfg.gain;
    a.invN = 1.0f / (float)h->N;
    a.lds = h->lds;
    return a;
}

extern "C" {

int dpe_ix_create(const dpe_ix_config *cfg, const uint8_t *staticMask, dpe_ix **out)
{
    char msg[256];
    if (ix_config_problem(cfg, msg, sizeof(msg))) {
        set_error("%s", msg);
        return -1;
    }
    DPE_REQUIRE(out != nullptr, "[Excisor] create: null argument");
    dpe_ix *h = new dpe_ix;
    h->cfg = *cfg;
    h->N = cfg->frameLength;
    h->lds = ix_lds(h->N);
    std::vector<float> tab = ix_twiddles(h->N);
    const std::vector<float> win = ix_window(h->N);
    tab.insert(tab.end(), win.begin(), win.end());
    std::vector<uint8_t> stat((size_t)h->N, 0);
    for (int f = 0; staticMask && f < h->N; ++f) {
        stat[(size_t)f] = staticMask[f] != 0;
        h->hasStatic = h->hasStatic || staticMask[f] != 0;
    }
    const size_t cBytes = (size_t)(4 + h->N) * sizeof(unsigned long long);
    const bool ok = hipMalloc((void **)&h->tables_d, tab.size() * sizeof(float)) == hipSuccess &&
                    hipMalloc((void **)&h->static_d, stat.size()) == hipSuccess && hipMalloc((void **)&h->counters_d, cBytes) == hipSuccess &&
                    hipMemcpy(h->tables_d, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
                    hipMemcpy(h->static_d, stat.data(), stat.size(), hipMemcpyHostToDevice) == hipSuccess &&
                    hipMemset(h->counters_d, 0, cBytes) == hipSuccess;
    if (!ok) {
        const hipError_t e = hipGetLastError();
        dpe_ix_destroy(h);
        set_error("[Excisor] create: no device memory (%s)", hipGetErrorString(e));
        return -1;
    }
    *out = h;
    return 0;
}

int dpe_ix_destroy(dpe_ix *h)
{
    if (!h) return 0;
    if (h->tables_d) (void)hipFree(h->tables_d);
    if (h->static_d) (void)hipFree(h->static_d);
    if (h->counters_d) (void)hipFree(h->counters_d);
    delete h;
    return 0;
}

int dpe_ix_info(const dpe_ix *h, dpe_ix_info_t *info)
{
    DPE_REQUIRE(h && info, "[Excisor] info: null argument");
    *info = dpe_ix_info_t{};
    info->hop = h->N / 2;
    info->hopsPerBlock = kIxHopsPerBlock;
    info->ldsBytes = h->lds.bytes;
    info->leadHops = kIxLeadHops;
    info->tailHops = kIxTailHops;
    return 0;
}

int dpe_ix_process(dpe_ix *h, const void *x_dev, int64_t xFirst, int64_t xCount, int64_t recordLength, void *out_dev, int64_t outFirst,
                   int64_t outCount, dpe_stream_t stream_)
{
    DPE_REQUIRE(h != nullptr, "[Excisor] process: null handle");
    char msg[320];
    if (ix_process_problem(h->cfg, x_dev == nullptr, out_dev == nullptr, (unsigned)(reinterpret_cast<uintptr_t>(x_dev) & 15),
                           (unsigned)(reinterpret_cast<uintptr_t>(out_dev) & 15), xFirst, xCount, recordLength, outFirst, outCount, msg, sizeof(msg))) {
        set_error("%s", msg);
        return -1;
    }
    const hipStream_t stream = (hipStream_t)stream_;
    IxArgs a = ix_args(h, x_dev, xFirst, xCount, recordLength);
    const IxLaunch l = ix_launch(outFirst, outCount, h->N);
    a.out = out_dev;
    a.outFirst = outFirst;
    a.outEnd = outFirst + outCount;
    a.h0 = l.h0;
    a.h1 = l.h1;
    DPE_CHECK_HIP(hipMemsetAsync(h->counters_d, 0, (size_t)(4 + h->N) * sizeof(unsigned long long), stream));
    ix_kernel<<<dim3((unsigned)l.blocks), dim3(kIxThreads), h->lds.bytes, stream>>>(a);
    DPE_CHECK_HIP(hipGetLastError());
    h->last = stream;
    return 0;
}

int dpe_ix_stats(dpe_ix *h, dpe_ix_stats_t *stats, int64_t *perBin)
{
    DPE_REQUIRE(h && stats, "[Excisor] stats: null argument");
    std::vector<unsigned long long> v((size_t)(4 + h->N));
    if (read_counters(v.data(), h->counters_d, v.size(), h->last)) return -1;
    stats->frames = (int64_t)v[0];
    stats->excisedBins = (int64_t)v[1];
    stats->blanked = (int64_t)v[2];
    stats->clipped = (int64_t)v[3];
    for (int f = 0; perBin && f < h->N; ++f) perBin[f] = (int64_t)v[(size_t)(4 + f)];
    return 0;
}

int dpe_ix_analyse(dpe_ix *h, const void *x_dev, int64_t xFirst, int64_t xCount, int64_t recordLength, int64_t frameFirst,
                   int64_t frameCount, float *power_dev, float *median_dev, uint8_t *mask_dev, dpe_stream_t stream_)
{
    DPE_REQUIRE(h != nullptr, "[Excisor] analyse: null handle");
    char msg[320];
    if (ix_analyse_problem(h->cfg, x_dev == nullptr, (unsigned)(reinterpret_cast<uintptr_t>(x_dev) & 15), xFirst, xCount, recordLength, frameFirst,
                           frameCount, (unsigned)(reinterpret_cast<uintptr_t>(power_dev) & 15), (unsigned)(reinterpret_cast<uintptr_t>(median_dev) & 15),
                           msg, sizeof(msg))) {
        set_error("%s", msg);
        return -1;
    }
    IxArgs a = ix_args(h, x_dev, xFirst, xCount, recordLength);
    a.analyse = 1;
    a.power = power_dev;
    a.median = median_dev;
    a.mask = mask_dev;
    a.h0 = frameFirst;
    a.h1 = frameFirst + frameCount - 1;
    const unsigned blocks = (unsigned)((frameCount + kIxHopsPerBlock - 1) / kIxHopsPerBlock);
    ix_kernel<<<dim3(blocks), dim3(kIxThreads), h->lds.bytes, (hipStream_t)stream_>>>(a);
    DPE_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
