// dpe_fe.hip -- the dpe_fe_ family: raw record bytes in a device buffer to interleaved int16 (or fp32) I/Q at zero IF and at
// fs_in / D, written straight into a device buffer.  Unpack, mix, low-pass and decimate in one kernel.  DESIGN.md 7h.
//
// A block owns tileOut consecutive outputs (dpe_fe_plan.h).  It decodes the inputs they read on the way into the LDS, ordered by
// decimation phase, so that each phase is a stride-one filter; a lane owns kFeRun consecutive outputs and slides one window of
// kFeRun elements per phase through registers: one LDS read and one scalar tap load per kFeRun packed FMAs.  The mixer is in the
// taps (gain h[t] exp(-j phase(t)), wave-uniform) and in one rotation per output by exp(-j phase(m D - T0)), whose angle comes
// from the 32-bit phase word split into 24 + 8 bits.  An output's arithmetic -- phase order, tap order, rotation -- depends on its
// index alone, never on its lane, tile or call.
#include "dpe_common.h"
#include "dpe_fe_plan.h"

namespace dpe {

typedef float fe2 __attribute__((ext_vector_type(2)));
constexpr int kFeBatch = 8;   // loads a lane has in flight while it stages a tile

struct FeArgs {
    const uint8_t *raw;         // input sample rawFirst begins at byte 0
    void *out;                  // output outFirst at element 0
    const float4 *taps;         // [D][qPitch] (fe_taps)
    unsigned long long *clipped;
    unsigned long long magic;
    long long rawFirst;
    int64_t lo, hi;             // the input samples that exist and lie in the buffer: [0, recordLength) cut to the buffer's range
    long long outFirst;
    int outCount, D, T0, Q, rem, tileOut, rowLen, pitch, qPitch;
    int format, outF32;
    unsigned delta;
    float levels[4];
};

__device__ __forceinline__ float fe_level(const FeArgs &a, unsigned code)   // selects, not an indexed read of the argument block
{
    const float lo = (code & 1u) ? a.levels[1] : a.levels[0], hi = (code & 1u) ? a.levels[3] : a.levels[2];
    return (code & 2u) ? hi : lo;
}

// x[rawFirst + rel] of the buffer (0 <= rel < rawCount: the caller's bounds).  Real formats return (x, 0).
template <int FMT>
__device__ __forceinline__ fe2 fe_load(const FeArgs &a, long long rel)
{
    if constexpr (FMT == DPE_FE_I16C) {
        float i, q;
        stream_unpack(reinterpret_cast<const int *>(a.raw)[rel], i, q);
        return fe2{i, q};
    } else if constexpr (FMT == DPE_FE_I8C) {
        const int v = reinterpret_cast<const unsigned short *>(a.raw)[rel];
        return fe2{(float)(signed char)(v & 0xFF), (float)(signed char)(v >> 8)};
    } else if constexpr (FMT == DPE_FE_I16R) {
        return fe2{(float)reinterpret_cast<const short *>(a.raw)[rel], 0.f};
    } else if constexpr (FMT == DPE_FE_I8R) {
        return fe2{(float)reinterpret_cast<const signed char *>(a.raw)[rel], 0.f};
    } else if constexpr (FMT == DPE_FE_ARGPI4) {
        const unsigned k = a.raw[rel] & 7u;                       // exp(j pi k / 4)
        const float r = 0.70710678118654752f;
        const unsigned kc = k, ks = (k + 6u) & 7u;                // sin(pi k / 4) = cos(pi (k - 2) / 4)
        const float c = (kc & 3u) == 2u ? 0.f : ((kc & 1u) ? r : 1.f), s = (ks & 3u) == 2u ? 0.f : ((ks & 1u) ? r : 1.f);
        return fe2{(kc >= 3u && kc <= 5u) ? -c : c, (ks >= 3u && ks <= 5u) ? -s : s};
    } else if constexpr (FMT == DPE_FE_P2R) {
        const unsigned b = a.raw[rel >> 2];
        return fe2{fe_level(a, (b >> (2u * ((unsigned)rel & 3u))) & 3u), 0.f};
    } else {   // DPE_FE_P2C
        const unsigned b = a.raw[rel >> 1] >> (4u * ((unsigned)rel & 1u));
        return fe2{fe_level(a, b & 3u), fe_level(a, (b >> 2) & 3u)};
    }
}

template <int MODE> struct FeElem { typedef fe2 type; };
template <> struct FeElem<kFeRealIn> { typedef float type; };

// acc += x c for one tap (the table entry c as fe_taps lays it out)
template <int MODE>
__device__ __forceinline__ fe2 fe_mac(typename FeElem<MODE>::type x, const float4 c, fe2 acc)
{
    if constexpr (MODE == kFeRealIn) {
        return __builtin_elementwise_fma(fe2{x, x}, fe2{c.x, c.y}, acc);
    } else if constexpr (MODE == kFeComplex) {
        return __builtin_elementwise_fma(x, fe2{c.x, c.y}, acc);
    } else {
        acc = __builtin_elementwise_fma(fe2{x.x, x.x}, fe2{c.x, c.y}, acc);
        return __builtin_elementwise_fma(fe2{x.y, x.y}, fe2{c.z, c.w}, acc);
    }
}

// Decodes the tile's inputs into the LDS.  Staged index i holds input n0 + i; [iLo, iHi) of the tile exists in the record and lies
// in the buffer, the rest is zero.  Inside a tile that holds any input every lane loads from a clamped, valid index and the value
// is dropped where the index was moved: the loads are unconditional, and kFeBatch of them go out before the first is waited for.
template <int MODE, int FMT>
__device__ __forceinline__ void fe_stage(const FeArgs &a, typename FeElem<MODE>::type *__restrict__ sTile, int tid, long long n0)
{
    if constexpr ((MODE == kFeRealIn) != (FMT == DPE_FE_I16R || FMT == DPE_FE_I8R || FMT == DPE_FE_P2R)) {
        return;   // (the host launches a real format in the real form only, and the others never in it)
    } else {
        const int nElem = a.rowLen * a.D;
        const int iLo = (int)min(max(a.lo - n0, 0LL), (long long)nElem), iHi = (int)min(max(a.hi - n0, 0LL), (long long)nElem);
        const long long relBase = n0 - a.rawFirst;
        const int kStep = kFeThreads / a.D, pStep = kFeThreads - kStep * a.D;
        int k, p;
        fe_split((unsigned)tid, a.D, a.magic, k, p);
        if (iLo >= iHi) {                                          // a tile beyond the record: zeros
            for (int i = tid; i < nElem; i += kFeThreads) {
                if constexpr (MODE == kFeRealIn) sTile[p * a.pitch + k] = 0.f;
                else sTile[p * a.pitch + k] = fe2{0.f, 0.f};
                fe_advance(k, p, a.D, kStep, pStep);
            }
            return;
        }
        for (int i = tid; i < nElem; i += kFeBatch * kFeThreads) {
            fe2 x[kFeBatch];
#pragma unroll
            for (int u = 0; u < kFeBatch; ++u) {                   // (an index past the tile's end loads a valid sample too, and stores nothing)
                const int iu = i + u * kFeThreads, ic = min(max(iu, iLo), iHi - 1);
                x[u] = fe_load<FMT>(a, relBase + ic);
                if (ic != iu) x[u] = fe2{0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < kFeBatch; ++u) {
                if (i + u * kFeThreads < nElem) {
                    if constexpr (MODE == kFeRealIn) sTile[p * a.pitch + k] = x[u].x;
                    else sTile[p * a.pitch + k] = x[u];
                }
                fe_advance(k, p, a.D, kStep, pStep);
            }
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(kFeThreads) void fe_kernel(FeArgs a)
{
    typedef typename FeElem<MODE>::type elem;
    extern __shared__ __attribute__((aligned(16))) unsigned char sRaw[];
    elem *__restrict__ sTile = reinterpret_cast<elem *>(sRaw);   // [D][pitch]
    const int tid = threadIdx.x;
    const long long i0 = (long long)blockIdx.x * a.tileOut;      // the tile's first output, counted from outFirst
    const int nOut = (int)min((long long)a.tileOut, (long long)a.outCount - i0);
    const long long n0 = (a.outFirst + i0) * a.D - a.T0;          // the input sample at staged index 0 (below zero at the record's start)

    switch (a.format) {     // one staging loop per format, so that a loop's loads carry no branch and go out together
    case DPE_FE_I16C: fe_stage<MODE, DPE_FE_I16C>(a, sTile, tid, n0); break;
    case DPE_FE_I8C: fe_stage<MODE, DPE_FE_I8C>(a, sTile, tid, n0); break;
    case DPE_FE_I16R: fe_stage<MODE, DPE_FE_I16R>(a, sTile, tid, n0); break;
    case DPE_FE_I8R: fe_stage<MODE, DPE_FE_I8R>(a, sTile, tid, n0); break;
    case DPE_FE_ARGPI4: fe_stage<MODE, DPE_FE_ARGPI4>(a, sTile, tid, n0); break;
    case DPE_FE_P2R: fe_stage<MODE, DPE_FE_P2R>(a, sTile, tid, n0); break;
    default: fe_stage<MODE, DPE_FE_P2C>(a, sTile, tid, n0); break;
    }
    __syncthreads();

    const int k0 = tid * kFeRun;
    if (k0 >= nOut) return;
    fe2 acc[kFeRun];
#pragma unroll
    for (int r = 0; r < kFeRun; ++r) acc[r] = fe2{0.f, 0.f};
    for (int p = 0; p < a.D; ++p) {
        const int nq = fe_phase_taps(p, a.Q, a.rem);
        const elem *__restrict__ row = sTile + p * a.pitch + k0;
        const float4 *__restrict__ tp = a.taps + p * a.qPitch;
        elem w[kFeRun];
#pragma unroll
        for (int r = 0; r < kFeRun; ++r) w[r] = row[r];
        // tap q of the phase, q = q0 + j: slot (r + j) mod kFeRun of the window holds what output r reads; then slot j takes the
        // element the next tap's last output reads.  Whole groups of kFeRun taps run unguarded, so their tap loads go out together.
        int q0 = 0;
        for (; q0 + kFeRun <= nq; q0 += kFeRun) {
#pragma unroll
            for (int j = 0; j < kFeRun; ++j) {
                const float4 c = tp[q0 + j];
#pragma unroll
                for (int r = 0; r < kFeRun; ++r) acc[r] = fe_mac<MODE>(w[(r + j) % kFeRun], c, acc[r]);
                w[j] = row[q0 + j + kFeRun];
            }
        }
#pragma unroll
        for (int j = 0; j < kFeRun - 1; ++j) {
            if (q0 + j < nq) {                                     // wave-uniform
                const float4 c = tp[q0 + j];
#pragma unroll
                for (int r = 0; r < kFeRun; ++r) acc[r] = fe_mac<MODE>(w[(r + j) % kFeRun], c, acc[r]);
                w[j] = row[q0 + j + kFeRun];
            }
        }
    }

    unsigned nClip = 0;
#pragma unroll
    for (int r = 0; r < kFeRun; ++r) {
        if (k0 + r >= nOut) break;
        fe2 y = acc[r];
        if constexpr (MODE != kFeComplex) {
            // exp(-j theta), theta = 2 pi w / 2^32 = pi (hi 2^-23 + lo 2^-31) with w = hi 2^8 + lo taken as a signed word: hi is exact
            // in fp32, and lo turns the pair by less than 2^-21 rad (first order: the second is below 2^-43)
            const long long nc = (a.outFirst + i0 + k0 + r) * a.D - a.T0;
            const int ws = (int)fe_phase(nc, a.delta);
            float s0, c0;
            sincospif((float)(ws >> 8) * 0x1p-23f, &s0, &c0);
            const float b = (float)(ws & 0xFF) * (3.14159265358979323846f * 0x1p-31f);
            const float c = fmaf(-s0, b, c0), s = fmaf(c0, b, s0);
            y = fe2{fmaf(acc[r].y, s, acc[r].x * c), fmaf(-acc[r].x, s, acc[r].y * c)};
        }
        stream_store(a.out, i0 + k0 + r, y.x, y.y, a.outF32, nClip);
    }
    if (nClip) atomicAdd(a.clipped, (unsigned long long)nClip);
}

}  // namespace dpe

using namespace dpe;

struct dpe_fe {
    dpe_fe_config cfg{};
    FeGeom g{};
    FeMode mode = kFeRealIn;
    uint32_t delta = 0;
    int bytesNum = 1, bytesDen = 1;
    float4 *taps_d = nullptr;
    unsigned long long *clipped_d = nullptr;
    hipStream_t last = nullptr;
};

extern "C" {

int dpe_fe_create(const dpe_fe_config *cfg, const double *taps, dpe_fe **out)
{
    char msg[256];
    if (fe_config_problem(cfg, taps, msg, sizeof(msg))) {
        set_error("%s", msg);
        return -1;
    }
    DPE_REQUIRE(out != nullptr, "[FrontEnd] create: null argument");
    dpe_fe *h = new dpe_fe;
    h->cfg = *cfg;
    bool realIn = false;
    (void)fe_format(cfg->format, h->bytesNum, h->bytesDen, realIn);
    h->delta = fe_delta(cfg->intermediateFrequency, cfg->samplingFrequency);
    h->mode = fe_mode(realIn, h->delta);
    h->g = fe_geom(cfg->decimation, cfg->nTaps, realIn);
    const std::vector<float> tab = fe_taps(h->g, h->mode, h->delta, cfg->gain, taps);
    const bool ok = hipMalloc((void **)&h->taps_d, tab.size() * sizeof(float)) == hipSuccess &&
                    hipMalloc((void **)&h->clipped_d, sizeof(unsigned long long)) == hipSuccess &&
                    hipMemcpy(h->taps_d, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
                    hipMemset(h->clipped_d, 0, sizeof(unsigned long long)) == hipSuccess;
    if (!ok) {
        const hipError_t e = hipGetLastError();
        dpe_fe_destroy(h);
        set_error("[FrontEnd] create: no device memory (%s)", hipGetErrorString(e));
        return -1;
    }
    *out = h;
    return 0;
}

int dpe_fe_destroy(dpe_fe *h)
{
    if (!h) return 0;
    if (h->taps_d) (void)hipFree(h->taps_d);
    if (h->clipped_d) (void)hipFree(h->clipped_d);
    delete h;
    return 0;
}

int dpe_fe_info(const dpe_fe *h, dpe_fe_info_t *info)
{
    DPE_REQUIRE(h && info, "[FrontEnd] info: null argument");
    *info = dpe_fe_info_t{};
    info->realisedIF = fe_realised_if(h->delta, h->cfg.samplingFrequency);
    info->outputFrequency = h->cfg.samplingFrequency / h->cfg.decimation;
    info->delta = (int64_t)h->delta;
    info->groupDelay = h->g.T0;
    info->bytesNum = h->bytesNum;
    info->bytesDen = h->bytesDen;
    info->tileOutputs = h->g.tileOut;
    info->ldsBytes = h->g.ldsBytes;
    return 0;
}

int dpe_fe_convert(dpe_fe *h, const void *raw_dev, int64_t rawFirstSample, int64_t rawCount, int64_t recordLength, void *out_dev,
                   int64_t outFirst, int64_t outCount, dpe_stream_t stream_)
{
    DPE_REQUIRE(h != nullptr, "[FrontEnd] convert: null handle");
    char msg[320];
    if (fe_convert_problem(h->cfg, raw_dev == nullptr, out_dev == nullptr, (unsigned)(reinterpret_cast<uintptr_t>(raw_dev) & 15),
                           (unsigned)(reinterpret_cast<uintptr_t>(out_dev) & 15), rawFirstSample, rawCount, recordLength, outFirst, outCount, msg,
                           sizeof(msg))) {
        set_error("%s", msg);
        return -1;
    }
    const hipStream_t stream = (hipStream_t)stream_;
    const FeGeom &g = h->g;
    FeArgs a{};
    a.raw = static_cast<const uint8_t *>(raw_dev);
    a.out = out_dev;
    a.taps = h->taps_d;
    a.clipped = h->clipped_d;
    a.magic = g.magic;
    a.rawFirst = rawFirstSample;
    a.lo = rawFirstSample;
    a.hi = rawFirstSample + rawCount;
    stream_cut(recordLength, a.lo, a.hi);
    a.outFirst = outFirst;
    a.outCount = (int)outCount;
    a.D = g.D;
    a.T0 = g.T0;
    a.Q = g.Q;
    a.rem = g.rem;
    a.tileOut = g.tileOut;
    a.rowLen = g.rowLen;
    a.pitch = g.pitch;
    a.qPitch = g.qPitch;
    a.format = h->cfg.format;
    a.outF32 = h->cfg.outputFormat == DPE_FE_OUT_F32;
    a.delta = h->delta;
    for (int i = 0; i < 4; ++i) a.levels[i] = (float)h->cfg.levels[i];
    const dim3 grid((unsigned)fe_blocks(g, outCount)), block(kFeThreads);
    DPE_CHECK_HIP(hipMemsetAsync(h->clipped_d, 0, sizeof(unsigned long long), stream));
    switch (h->mode) {
    case kFeRealIn: fe_kernel<kFeRealIn><<<grid, block, g.ldsBytes, stream>>>(a); break;
    case kFeComplex: fe_kernel<kFeComplex><<<grid, block, g.ldsBytes, stream>>>(a); break;
    default: fe_kernel<kFeComplexMix><<<grid, block, g.ldsBytes, stream>>>(a); break;
    }
    DPE_CHECK_HIP(hipGetLastError());
    h->last = stream;
    return 0;
}

int dpe_fe_clipped(dpe_fe *h, int64_t *count)
{
    DPE_REQUIRE(h && count, "[FrontEnd] clipped: null argument");
    unsigned long long v = 0;
    if (read_counters(&v, h->clipped_d, 1, h->last)) return -1;
    *count = (int64_t)v;
    return 0;
}

}  // extern "C"
