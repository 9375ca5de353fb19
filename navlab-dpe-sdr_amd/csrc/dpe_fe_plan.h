// dpe_fe_plan.h -- the front end's host-side planning as plain C++: the phase word of the mixer, the input range a range of outputs
// needs, the tile geometry (which block, lane and slot owns an output, where a staged input sample lies in the LDS, how many bytes
// that takes), the modulated tap table the kernel reads, and every refusal with its message.  Nothing of HIP is included:
// dpe_fe.hip passes sizes and alignments in, the kernel calls the same index functions (DPE_STREAM_HD), and host/test_fe_plan.cpp
// holds them to their properties with a plain C++ compiler.  The index limits, the record cut and the refusals every stream stage
// makes are dpe_stream_plan.h's.  DESIGN.md 7h.
//
// The stage:  y[m] = gain sum_t h[t] z[m D + t - T0],  z[n] = x[n] exp(-2 pi j ((n delta) mod 2^32) / 2^32),  T0 = (T - 1) / 2.
// The phase word is additive modulo 2^32, so  z-phase(m D + t - T0) = phase(m D - T0) + phase(t)  exactly: the kernel sums
// x[...] c[t] with the modulated taps c[t] = gain h[t] exp(-j phase(t)) (fp64 here, held as fp32) and rotates each output once.
#pragma once
#include <vector>

#include "dpe_stream_plan.h"

namespace dpe {

constexpr int kFeThreads = 256;             // lanes per block
constexpr int kFeRun = 5;                   // consecutive outputs per lane; odd, so that the lanes' LDS reads (stride kFeRun elements) spread over all banks
constexpr int kFeMaxD = 64;
constexpr int kFeMaxT = 1023;
constexpr int kFeLdsBytes = 32 * 1024;      // the staged tile's upper limit: five blocks per CU keep enough loads in flight

enum FeMode { kFeRealIn = 0, kFeComplex = 1, kFeComplexMix = 2 };   // what the tap loop multiplies (fe_taps)

// bytes per input sample as the ratio num / den; false: no such format
inline bool fe_format(int fmt, int &num, int &den, bool &realIn)
{
    switch (fmt) {
    case DPE_FE_I16C: num = 4; den = 1; realIn = false; return true;
    case DPE_FE_I8C: num = 2; den = 1; realIn = false; return true;
    case DPE_FE_I16R: num = 2; den = 1; realIn = true; return true;
    case DPE_FE_I8R: num = 1; den = 1; realIn = true; return true;
    case DPE_FE_ARGPI4: num = 1; den = 1; realIn = false; return true;
    case DPE_FE_P2R: num = 1; den = 4; realIn = true; return true;
    case DPE_FE_P2C: num = 1; den = 2; realIn = false; return true;
    }
    return false;
}

// delta = rint(f_IF / fs_in 2^32) mod 2^32 (round half to even; a negative f_IF wraps).  |f_IF| <= fs_in is the caller's check.
inline uint32_t fe_delta(double fIF, double fsIn)
{
    double r = std::fmod(std::rint(fIF / fsIn * 4294967296.0), 4294967296.0);
    if (r < 0.0) r += 4294967296.0;
    return (uint32_t)(uint64_t)r;
}
// the mixer's phase word of input sample n: (n delta) mod 2^32, exact for any n (two's complement below zero)
DPE_STREAM_HD uint32_t fe_phase(int64_t n, uint32_t delta) { return (uint32_t)((uint64_t)n * (uint64_t)delta); }
// the frequency delta realises, in (-fs/2, fs/2]
inline double fe_realised_if(uint32_t delta, double fsIn)
{
    const double f = (double)delta * fsIn / 4294967296.0;
    return delta > 0x80000000u ? f - fsIn : f;
}
// cos and sin of 2 pi w / 2^32, exact on the axes: the quadrant is taken off the word before the angle is formed
inline void fe_cos_sin(uint32_t w, double &c, double &s)
{
    const double a = (double)(w & 0x3fffffffu) * (1.5707963267948966 / 1073741824.0);
    const double c0 = std::cos(a), s0 = std::sin(a);
    switch (w >> 30) {
    case 0: c = c0; s = s0; break;
    case 1: c = -s0; s = c0; break;
    case 2: c = -c0; s = -s0; break;
    default: c = s0; s = -c0; break;
    }
}

// ---- the input range the outputs [outFirst, outFirst + outCount) read: [outFirst D - T0, (outFirst + outCount - 1) D + T - T0),
// cut to the record [0, recordLength) (recordLength < 0: no end).  lo >= hi: they read nothing but zeros.
inline void fe_needed(int64_t outFirst, int64_t outCount, int D, int T, int64_t recordLength, int64_t &lo, int64_t &hi)
{
    const int T0 = (T - 1) / 2;
    lo = outFirst * D - T0;
    hi = (outFirst + outCount - 1) * D + T - T0;
    stream_cut(recordLength, lo, hi);
}

// ---- tile geometry.  A block owns tileOut consecutive outputs of the call, lane l of it the outputs l kFeRun .. l kFeRun +
// kFeRun - 1 of the tile (slots).  The block stages the inputs n0 .. n0 + rowLen D - 1, n0 = (first output of the tile) D - T0, into
// the LDS by decimation phase: input n0 + i lies at element (i mod D) pitch + i / D.  Output j of the tile reads, for the tap
// t = q D + p, element p pitch + j + q: a stride-one filter per phase, so a lane slides one window of kFeRun elements per phase.
struct FeGeom {
    int D, T, T0;
    int Q;            // ceil(T / D): taps of the longest phase
    int rem;          // phases p < rem have Q taps, the others Q - 1 (T = (Q - 1) D + rem, 1 <= rem <= D)
    int elemBytes;    // 4: a real sample as one float, 8: a complex one as two
    int tileOut;      // outputs per block, a multiple of kFeRun
    int rowLen;       // elements staged per phase: tileOut + Q - 1
    int pitch;        // elements between phases: rowLen + 1 (the window's last refill reads one element past the row; never used)
    int ldsBytes;
    int qPitch;       // tap-table entries per phase
    uint64_t magic;   // 2^32 / D + 1: i / D == (i magic) >> 32 for every staged i (fe_split)
};
inline FeGeom fe_geom(int D, int T, bool realIn)
{
    FeGeom g{};
    g.D = D;
    g.T = T;
    g.T0 = (T - 1) / 2;
    g.Q = (T + D - 1) / D;
    g.rem = T - (g.Q - 1) * D;
    g.elemBytes = realIn ? 4 : 8;
    const int pitchMax = kFeLdsBytes / g.elemBytes / D;
    int tile = pitchMax - g.Q;                                   // rowLen + 1 <= pitchMax
    if (tile > kFeThreads * kFeRun) tile = kFeThreads * kFeRun;
    g.tileOut = tile / kFeRun * kFeRun;
    g.rowLen = g.tileOut + g.Q - 1;
    g.pitch = g.rowLen + 1;
    g.ldsBytes = g.pitch * D * g.elemBytes;
    g.qPitch = g.Q;
    g.magic = 4294967296ULL / (uint64_t)D + 1ULL;
    return g;
}
DPE_STREAM_HD int fe_phase_taps(int p, int Q, int rem) { return p < rem ? Q : Q - 1; }
// staged input i of a tile -> its row position k = i / D and phase p = i mod D
DPE_STREAM_HD void fe_split(uint32_t i, int D, uint64_t magic, int &k, int &p)
{
    k = (int)(((uint64_t)i * magic) >> 32);
    p = (int)i - k * D;
}
// the same for staged input i + kFeThreads, from (k, p) of input i: kStep = kFeThreads / D, pStep = kFeThreads mod D
DPE_STREAM_HD void fe_advance(int &k, int &p, int D, int kStep, int pStep)
{
    k += kStep;
    p += pStep;
    if (p >= D) { p -= D; ++k; }
}
// output i of a call (counted from outFirst) -> its owner
inline void fe_owner(const FeGeom &g, int64_t i, int64_t &block, int &lane, int &slot)
{
    block = i / g.tileOut;
    const int j = (int)(i - block * g.tileOut);
    lane = j / kFeRun;
    slot = j - lane * kFeRun;
}
inline int64_t fe_blocks(const FeGeom &g, int64_t outCount) { return (outCount + g.tileOut - 1) / g.tileOut; }

// ---- the tap table: [D][qPitch] entries of four floats; entry (p, q) belongs to the tap t = q D + p.
//   kFeRealIn      (cr, ci, 0, 0)      acc += (x, x) (cr, ci)
//   kFeComplex     (g, g, 0, 0)        acc += (xI, xQ) (g, g)                        delta = 0: real taps
//   kFeComplexMix  (cr, ci, -ci, cr)   acc += (xI, xI) (cr, ci) + (xQ, xQ) (-ci, cr)
// with cr + j ci = gain h[t] exp(-2 pi j ((t delta) mod 2^32) / 2^32) and g = gain h[t], formed in fp64 and rounded to fp32 once.
inline FeMode fe_mode(bool realIn, uint32_t delta) { return realIn ? kFeRealIn : (delta == 0 ? kFeComplex : kFeComplexMix); }
inline std::vector<float> fe_taps(const FeGeom &g, FeMode mode, uint32_t delta, double gain, const double *h)
{
    std::vector<float> tab((size_t)g.D * g.qPitch * 4, 0.f);
    for (int t = 0; t < g.T; ++t) {
        double c, s;
        fe_cos_sin(fe_phase(t, delta), c, s);
        const float cr = (float)(gain * h[t] * c), ci = (float)(-(gain * h[t] * s));
        float *e = tab.data() + ((size_t)(t % g.D) * g.qPitch + t / g.D) * 4;
        if (mode == kFeComplex) {
            e[0] = e[1] = (float)(gain * h[t]);
        } else {
            e[0] = cr;
            e[1] = ci;
            if (mode == kFeComplexMix) { e[2] = -ci; e[3] = cr; }
        }
    }
    return tab;
}

// ---- what is refused before anything is allocated or launched.  true: refused, `msg` holds the reason.
inline bool fe_config_problem(const dpe_fe_config *cfg, const double *taps, char *msg, size_t len)
{
    DPE_STREAM_REFUSE(!cfg || !taps, "[FrontEnd] create: null argument");
    int num, den;
    bool realIn;
    DPE_STREAM_REFUSE(!fe_format(cfg->format, num, den, realIn), "[FrontEnd] create: input format %d is none of DPE_FE_I16C .. DPE_FE_P2C", cfg->format);
    if (stream_format_problem("[FrontEnd]", "create", cfg->outputFormat, msg, len)) return true;
    DPE_STREAM_REFUSE(cfg->decimation < 1 || cfg->decimation > kFeMaxD, "[FrontEnd] create: decimation D = %d outside 1..%d", cfg->decimation, kFeMaxD);
    DPE_STREAM_REFUSE(cfg->nTaps < 1 || cfg->nTaps > kFeMaxT, "[FrontEnd] create: T = %d taps outside 1..%d", cfg->nTaps, kFeMaxT);
    DPE_STREAM_REFUSE(cfg->nTaps % 2 == 0, "[FrontEnd] create: T = %d taps is even (the group delay (T - 1) / 2 has to be whole samples)", cfg->nTaps);
    DPE_STREAM_REFUSE(!(std::isfinite(cfg->samplingFrequency) && cfg->samplingFrequency > 0.0), "[FrontEnd] create: sampling frequency not positive");
    DPE_STREAM_REFUSE(!(std::isfinite(cfg->intermediateFrequency) && std::fabs(cfg->intermediateFrequency) <= cfg->samplingFrequency),
                      "[FrontEnd] create: intermediate frequency not finite or beyond the sampling frequency");
    if (stream_gain_problem("[FrontEnd]", "create", cfg->gain, msg, len)) return true;
    for (int i = 0; i < 4; ++i) DPE_STREAM_REFUSE(!std::isfinite(cfg->levels[i]), "[FrontEnd] create: level %d not finite", i);
    for (int t = 0; t < cfg->nTaps; ++t) DPE_STREAM_REFUSE(!std::isfinite(taps[t]), "[FrontEnd] create: tap %d not finite", t);
    return false;
}

// rawAlign / outAlign: the two device addresses modulo 16
inline bool fe_convert_problem(const dpe_fe_config &cfg, bool rawNull, bool outNull, unsigned rawAlign, unsigned outAlign, int64_t rawFirst,
                               int64_t rawCount, int64_t recordLength, int64_t outFirst, int64_t outCount, char *msg, size_t len)
{
    DPE_STREAM_REFUSE(rawNull || outNull, "[FrontEnd] convert: null %s buffer", rawNull ? "input" : "output");
    int num = 1, den = 1;
    bool realIn = false;
    (void)fe_format(cfg.format, num, den, realIn);
    const unsigned outBytes = cfg.outputFormat == DPE_FE_OUT_F32 ? 8u : 4u;
    DPE_STREAM_REFUSE(outAlign % outBytes != 0, "[FrontEnd] convert: the output is not aligned to an I/Q pair (%u bytes)", outBytes);
    DPE_STREAM_REFUSE(den == 1 && rawAlign % (unsigned)num != 0, "[FrontEnd] convert: the input is not aligned to a sample (%d bytes)", num);
    if (stream_outputs_problem("[FrontEnd]", "convert", outFirst, outCount, msg, len)) return true;
    if (stream_held_problem("[FrontEnd]", "convert", rawFirst, rawCount, recordLength, msg, len)) return true;
    DPE_STREAM_REFUSE(rawFirst % den != 0, "[FrontEnd] convert: the buffer's first sample %lld is not on a byte boundary (%d samples per byte)",
                      (long long)rawFirst, den);
    int64_t lo, hi;
    fe_needed(outFirst, outCount, cfg.decimation, cfg.nTaps, recordLength, lo, hi);
    return stream_coverage_problem("[FrontEnd]", "convert", "outputs", "the buffer holds", outFirst, outCount, lo, hi, rawFirst, rawCount, msg, len);
}

}  // namespace dpe
