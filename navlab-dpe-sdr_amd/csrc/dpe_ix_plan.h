// dpe_ix_plan.h -- the excisor's host-side planning as plain C++: the input range a range of outputs needs, which block computes
// which frames for which hops, the set of frames a call counts in its statistics, the LDS layout, the transform's index functions,
// the twiddle and window tables, and every refusal with its message.  Nothing of HIP is included: dpe_ix.hip passes sizes and
// alignments in, the kernel calls the same index functions (DPE_STREAM_HD), and host/test_ix_plan.cpp holds them to their
// properties with a plain C++ compiler.  The index limits, the record cut and the refusals every stream stage makes are
// dpe_stream_plan.h's.  DESIGN.md 7i.
//
// The stage, for the frame length N and the hop H = N / 2:  frame k >= 0 covers the samples (k - 1) H + i, i < N, windowed by
// w[i] = sin(pi (i + 1/2) / N); its spectrum loses the bins above kappa times its lower median power (widened by the guard) and the
// static mask; output n = h H + r is  gain (w[r + H] y_h[r + H] + w[r] y_{h+1}[r]).  So hop h needs the frames h and h + 1, and a
// block that owns the hops [ha, hb] computes the frames ha .. hb + 1 in order, carrying each frame's second half to the next.
#pragma once
#include <vector>

#include "dpe_stream_plan.h"

namespace dpe {

constexpr int kIxThreads = 256;             // lanes per block
constexpr int kIxMinN = 64, kIxMaxN = 4096;
constexpr int kIxHopsPerBlock = 16;         // hops a block owns: it computes one frame more than that, 1/16 of the work twice
constexpr int kIxCarry = kIxMaxN / 2 / kIxThreads;   // elements of a frame's second half a lane carries in registers
constexpr int kIxLeadHops = 1, kIxTailHops = 2;      // the needed range: [(a div H - 1) H, ((a + c - 1) div H + 2) H)
constexpr int64_t kIxMaxFrames = INT64_C(1) << 24;   // frames per analyse call

DPE_STREAM_HD int ix_log2(int N)
{
    int l = 0;
    while ((1 << l) < N) ++l;
    return l;
}

// ---- the input range the outputs [outFirst, outFirst + outCount) read, cut to the record [0, recordLength) (recordLength < 0: no
// end).  lo >= hi: they read nothing but zeros.
inline void ix_needed(int64_t outFirst, int64_t outCount, int N, int64_t recordLength, int64_t &lo, int64_t &hi)
{
    const int64_t H = N / 2;
    lo = (outFirst / H - kIxLeadHops) * H;
    hi = ((outFirst + outCount - 1) / H + kIxTailHops) * H;
    stream_cut(recordLength, lo, hi);
}
// the same for the frames [frameFirst, frameFirst + frameCount) of an analyse call
inline void ix_needed_frames(int64_t frameFirst, int64_t frameCount, int N, int64_t recordLength, int64_t &lo, int64_t &hi)
{
    const int64_t H = N / 2;
    lo = (frameFirst - 1) * H;
    hi = (frameFirst + frameCount) * H;
    stream_cut(recordLength, lo, hi);
}

// ---- ownership.  A call's hops are h0 = outFirst div H .. h1 = (outFirst + outCount - 1) div H; block b owns the hops
// h0 + b kIxHopsPerBlock .. and computes the frames from its first hop to its last hop + 1.  An analyse call's block b computes
// the frames frameFirst + b kIxHopsPerBlock .. and nothing more.
struct IxLaunch {
    int64_t h0, h1;     // first and last hop of the call
    int64_t blocks;
};
inline IxLaunch ix_launch(int64_t outFirst, int64_t outCount, int N)
{
    const int64_t H = N / 2;
    IxLaunch l{};
    l.h0 = outFirst / H;
    l.h1 = (outFirst + outCount - 1) / H;
    l.blocks = (l.h1 - l.h0 + kIxHopsPerBlock) / kIxHopsPerBlock;
    return l;
}
// the hops [ha, hb] of block b, for the call's hops [h0, h1]
DPE_STREAM_HD void ix_block_hops(int64_t h0, int64_t h1, int64_t b, int64_t &ha, int64_t &hb)
{
    ha = h0 + b * kIxHopsPerBlock;
    hb = ha + kIxHopsPerBlock - 1;
    if (hb > h1) hb = h1;
}
// the owner of output n (a sample index of the record) in a call whose first hop is h0
inline int64_t ix_owner(int64_t n, int64_t h0, int N) { return (n / (N / 2) - h0) / kIxHopsPerBlock; }
// frame k is counted by the block that owns hop k, when its centre k H is one of the call's outputs
DPE_STREAM_HD bool ix_counted(int64_t k, int64_t H, int64_t outFirst, int64_t outCount) { return k * H >= outFirst && k * H < outFirst + outCount; }
inline int64_t ix_counted_frames(int64_t outFirst, int64_t outCount, int N)
{
    return stream_multiples(outFirst, outFirst + outCount, N / 2);
}

// ---- LDS layout of a block (bytes from the allocation's start)
struct IxLds {
    int frame;      // float2 [N]: the frame, its spectrum (bit-reversed order) and the synthesised frame in turn
    int perBin;     // uint32 [N]: the block's excisions per bin, flushed to the counters at its end
    int detected;   // uint8 [N]: the frame's detected bins, natural order
    int hist;       // uint32 [256]: the radix select's histogram
    int select;     // uint32 [2]: the select's prefix and remaining rank
    int counts;     // uint32 [4]: frames, excised bins, blanked, clipped of the block
    int bytes;
};
inline IxLds ix_lds(int N)
{
    IxLds l{};
    l.frame = 0;
    l.perBin = l.frame + 8 * N;
    l.detected = l.perBin + 4 * N;
    l.hist = l.detected + N;
    l.select = l.hist + 4 * 256;
    l.counts = l.select + 8;
    l.bytes = l.counts + 16;
    return l;
}

// ---- the transform: radix-2 butterflies on the frame in place, decimation in frequency forwards (natural order in, bit-reversed
// out) and decimation in time backwards (bit-reversed in, natural out), two stages per pass where two remain.  Pass element u < N / 4
// of the stage pair (2 q, q) works on base, base + q, base + 2 q, base + 3 q; stage element t < N / 2 of a single stage of half-size
// s on i0, i0 + s.  j is the butterfly's position in its group: the twiddle is tw[j N / (2 s)], tw[m] = exp(-2 pi j m / N).
DPE_STREAM_HD void ix_pair_index(int u, int q, int &base, int &j)
{
    j = u & (q - 1);
    base = ((u - j) << 2) + j;
}
DPE_STREAM_HD void ix_single_index(int t, int s, int &i0, int &j)
{
    j = t & (s - 1);
    i0 = ((t - j) << 1) + j;
}
DPE_STREAM_HD int ix_bitrev(int p, int log2N)
{
    unsigned v = (unsigned)p, r = 0;
    for (int b = 0; b < log2N; ++b) {
        r = (r << 1) | (v & 1u);
        v >>= 1;
    }
    return (int)r;
}
// tw[m] = exp(-2 pi j m / N), m < N / 2, and the window w[i], i < N: fp64 here, held as fp32.  The eighth-turn symmetries are
// taken before the angle is formed, so that tw[N / 4] = (0, -1) and tw[N / 8] has equal parts.
inline std::vector<float> ix_twiddles(int N)
{
    std::vector<float> t((size_t)N, 0.f);
    const double step = 6.283185307179586476925 / N;
    for (int m = 0; m < N / 2; ++m) {
        double c, s;
        if (m <= N / 8) { c = std::cos(step * m); s = std::sin(step * m); }
        else if (m <= N / 4) { c = std::sin(step * (N / 4 - m)); s = std::cos(step * (N / 4 - m)); }
        else if (m <= 3 * N / 8) { c = -std::sin(step * (m - N / 4)); s = std::cos(step * (m - N / 4)); }
        else { c = -std::cos(step * (N / 2 - m)); s = std::sin(step * (N / 2 - m)); }
        t[2 * (size_t)m] = (float)c;
        t[2 * (size_t)m + 1] = (float)-s;
    }
    return t;
}
inline std::vector<float> ix_window(int N)
{
    std::vector<float> w((size_t)N);
    for (int i = 0; i < N / 2; ++i) w[(size_t)i] = w[(size_t)(N - 1 - i)] = (float)std::sin(3.14159265358979323846 * (i + 0.5) / N);
    return w;
}
// floor(blankPower) as the 32-bit word an int16 sample's I^2 + Q^2 (at most 2^31) is compared with; 0: the blanker is off
inline uint32_t ix_blank_word(double blankPower) { return blankPower >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)std::floor(blankPower); }

// ---- what is refused before anything is allocated or launched.  true: refused, `msg` holds the reason.
inline bool ix_config_problem(const dpe_ix_config *cfg, char *msg, size_t len)
{
    DPE_STREAM_REFUSE(!cfg, "[Excisor] create: null argument");
    const int N = cfg->frameLength;
    DPE_STREAM_REFUSE(N < kIxMinN || N > kIxMaxN || (N & (N - 1)) != 0, "[Excisor] create: frame length N = %d is no power of two in %d..%d", N, kIxMinN, kIxMaxN);
    DPE_STREAM_REFUSE(!(std::isfinite(cfg->threshold) && cfg->threshold > 0.0), "[Excisor] create: threshold not finite or not positive");
    DPE_STREAM_REFUSE(cfg->guard < 0 || 2 * (int64_t)cfg->guard + 1 >= N, "[Excisor] create: guard %d outside 0..%d (2 guard + 1 < N)", cfg->guard, (N - 2) / 2);
    DPE_STREAM_REFUSE(!(std::isfinite(cfg->blankPower) && cfg->blankPower >= 0.0), "[Excisor] create: blanking power not finite or negative");
    if (stream_gain_problem("[Excisor]", "create", cfg->gain, msg, len)) return true;
    DPE_STREAM_REFUSE(cfg->inputFormat != DPE_IX_IN_I16 && cfg->inputFormat != DPE_IX_IN_F32,
                      "[Excisor] create: input format %d is neither DPE_IX_IN_I16 nor DPE_IX_IN_F32", cfg->inputFormat);
    return stream_format_problem("[Excisor]", "create", cfg->outputFormat, msg, len);
}

// the checks process and analyse share: the buffer and the record
inline bool ix_input_problem(const char *call, const dpe_ix_config &cfg, bool xNull, unsigned xAlign, int64_t xFirst, int64_t xCount, int64_t recordLength,
                             char *msg, size_t len)
{
    DPE_STREAM_REFUSE(xNull, "[Excisor] %s: null input buffer", call);
    const unsigned inBytes = cfg.inputFormat == DPE_IX_IN_F32 ? 8u : 4u;
    DPE_STREAM_REFUSE(xAlign % inBytes != 0, "[Excisor] %s: the input is not aligned to an I/Q pair (%u bytes)", call, inBytes);
    return stream_held_problem("[Excisor]", call, xFirst, xCount, recordLength, msg, len);
}

// xAlign / outAlign: the two device addresses modulo 16
inline bool ix_process_problem(const dpe_ix_config &cfg, bool xNull, bool outNull, unsigned xAlign, unsigned outAlign, int64_t xFirst, int64_t xCount,
                               int64_t recordLength, int64_t outFirst, int64_t outCount, char *msg, size_t len)
{
    DPE_STREAM_REFUSE(outNull, "[Excisor] process: null output buffer");
    if (ix_input_problem("process", cfg, xNull, xAlign, xFirst, xCount, recordLength, msg, len)) return true;
    const unsigned outBytes = cfg.outputFormat == DPE_FE_OUT_F32 ? 8u : 4u;
    DPE_STREAM_REFUSE(outAlign % outBytes != 0, "[Excisor] process: the output is not aligned to an I/Q pair (%u bytes)", outBytes);
    if (stream_outputs_problem("[Excisor]", "process", outFirst, outCount, msg, len)) return true;
    int64_t lo, hi;
    ix_needed(outFirst, outCount, cfg.frameLength, recordLength, lo, hi);
    return stream_coverage_problem("[Excisor]", "process", "outputs", "the buffer holds", outFirst, outCount, lo, hi, xFirst, xCount, msg, len);
}

inline bool ix_analyse_problem(const dpe_ix_config &cfg, bool xNull, unsigned xAlign, int64_t xFirst, int64_t xCount, int64_t recordLength,
                               int64_t frameFirst, int64_t frameCount, unsigned powerAlign, unsigned medianAlign, char *msg, size_t len)
{
    if (ix_input_problem("analyse", cfg, xNull, xAlign, xFirst, xCount, recordLength, msg, len)) return true;
    DPE_STREAM_REFUSE(powerAlign % 4u != 0 || medianAlign % 4u != 0, "[Excisor] analyse: an fp32 result buffer is not aligned to 4 bytes");
    DPE_STREAM_REFUSE(frameCount < 1 || frameCount > kIxMaxFrames, "[Excisor] analyse: %lld frames outside 1..2^24 per call", (long long)frameCount);
    // (the last output, 2^55 - 1, reads frame (2^55 - 1) div H + 1 = 2^55 / H)
    DPE_STREAM_REFUSE(frameFirst < 0 || frameFirst > kStreamMaxIndex / (cfg.frameLength / 2) + 1 - frameCount,
                      "[Excisor] analyse: first frame %lld with %lld frames outside the frames 0..2^55 / H the outputs read", (long long)frameFirst,
                      (long long)frameCount);
    int64_t lo, hi;
    ix_needed_frames(frameFirst, frameCount, cfg.frameLength, recordLength, lo, hi);
    return stream_coverage_problem("[Excisor]", "analyse", "frames", "the buffer holds", frameFirst, frameCount, lo, hi, xFirst, xCount, msg, len);
}

}  // namespace dpe
