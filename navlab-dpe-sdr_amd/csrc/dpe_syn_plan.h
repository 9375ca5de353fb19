// dpe_syn_plan.h -- the synthesiser's host-side planning as plain C++: the launch geometry (blocks per segment and each block's
// sample range), the per-channel parameter block the kernel reads, the nav-bit boundary of the window form and the nav-bit index of
// the record form with the check that a channel's bit array reaches its last sample.  Nothing of HIP is included: dpe_syn.hip passes
// pointers' alignments and sizes in, the kernel calls the same range and index functions (DPE_SYN_HD), and host/test_syn_plan.cpp
// holds them to their properties with a plain C++ compiler.  DESIGN.md 7f.
//
// The sample-to-chip and sample-to-bit mappings are fp64 expressions whose operand order and rounding are numpy's (synth.py):
// every function runs under fp contract(off), and the one fused multiply-add that appears is asked for by name because its single
// rounding is what makes the remainder exact.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/dpe_hip.h"
#include "dpe_consts.h"

#if defined(__clang__)
#define DPE_SYN_FP _Pragma("clang fp contract(off)")
#else
#define DPE_SYN_FP
#endif
#if defined(__HIPCC__)
#define DPE_SYN_HD __host__ __device__ inline
#else
#define DPE_SYN_HD inline
#endif

namespace dpe {

constexpr int kSynThreads = 256;            // lanes per block
constexpr int kSynLaneSamples = 4;          // consecutive samples per lane: one 16-byte store
constexpr int kSynBlockGroups = 1024;       // 16-byte groups per block: every lane walks four of them
constexpr int kSynChipPitch = 1024;         // bytes per PRN row of the chip tables (1023 chips and one spare)
constexpr int kSynNoFlip = 0x7fffffff;      // SynChan::flipAt of a channel without a sign change inside its window
constexpr double kSynMaxChips = 2251799813685248.0;   // 2^51: code phases below this keep floor, quotient and remainder exact in fp64

// One channel of one segment as the kernel reads it (block-uniform: scalar loads).
struct SynChan {
    double fc, rc, fi, ri;   // chips/s, chips at t = 0, Hz, cycles at t = 0
    float amp;
    int32_t flipAt;          // window form: the sign is -1 from this in-window sample on (kSynNoFlip: never)
    int32_t firstEdge;       // record form: cpReference % 20, code periods from the one sample 0 lies in to the first bit edge
    int32_t prnRow;          // prn - 1
    int32_t pad[4];
};
static_assert(sizeof(SynChan) == 64, "the parameter upload copies 16-byte words");

// floor(m / d) and the floor remainder for integer-valued m, d in fp64 (|m| < 2^51, 0 < d < 2^20, invD = 1 / d rounded): the
// estimate floor(m invD) is off by at most one, the fused remainder m - q d is an integer below 2^53 and therefore exact, and one
// correction step puts it into [0, d).
DPE_SYN_HD double syn_floor_div(double m, double d, double invD, double &rem)
{
    double q = std::floor(m * invD);
    double r = std::fma(-q, d, m);
    if (r < 0.0) { r += d; q -= 1.0; }
    else if (r >= d) { r -= d; q += 1.0; }
    rem = r;
    return q;
}

// Sample time: n / fs of a record, rint(i / fs 1e9) / 1e9 of a window (synth.time_idx).
DPE_SYN_HD double syn_time_record(int64_t n, double fs)
{
    DPE_SYN_FP
    return (double)n / fs;
}
DPE_SYN_HD double syn_time_window(int32_t i, double fs)
{
    DPE_SYN_FP
    const double ns = (double)i / fs * 1.0e9;
    return std::rint(ns) / 1.0e9;
}

// floor(t fc + rc): the chip count since the code period sample 0 lies in.  period = its floor quotient by 1023, return = the chip.
DPE_SYN_HD int syn_chip(double t, double fc, double rc, double &period)
{
    DPE_SYN_FP
    const double prod = t * fc;
    const double cph = prod + rc;
    double r;
    period = syn_floor_div(std::floor(cph), 1023.0, 1.0 / 1023.0, r);
    return (int)r;
}

// bits[(period - firstEdge + 20) // 20] of gen_iq_record: the index (negative: before the array).
DPE_SYN_HD double syn_bit_index(double period, int firstEdge)
{
    DPE_SYN_FP
    double r;
    return syn_floor_div(period - (double)firstEdge + 20.0, 20.0, 0.05, r);
}

// synth.nav_bit_boundary / BCS_NavBitBoundary: the first sample of the next nav bit.
inline int64_t syn_flip_at(int32_t cpEla, int32_t cpRef, double rc, double fc, double fs)
{
    DPE_SYN_FP
    const int since = (int)((((int64_t)cpEla - (int64_t)cpRef) % 20 + 20) % 20);
    const double chips = (double)(kLCA * (20 - since)) - rc;
    const double ratio = fs / fc;
    const double v = std::floor(chips * ratio);
    if (!(v > -9.0e18 && v < 9.0e18)) return INT64_MAX;
    return (int64_t)v + 1;
}

// ---- launch geometry.  A lane's four samples are the ones a 16-byte aligned address holds, so the groups of a segment start
// `align` samples (0..3, the segment's first byte address / 4 mod 4) before its sample 0; head and tail groups are partial.
struct SynGeom {
    int blocksPerSeg;        // the same for every segment of a call (a segment with fewer groups leaves its last block empty)
    long long nBlocks;
    size_t ldsBytes;         // the K x 1023 chip table
};
DPE_SYN_HD int syn_groups(int S, int align) { return (S + align + kSynLaneSamples - 1) / kSynLaneSamples; }
inline SynGeom syn_geom(int S, int nSeg, int K)
{
    SynGeom g;
    g.blocksPerSeg = (syn_groups(S, 3) + kSynBlockGroups - 1) / kSynBlockGroups;
    g.nBlocks = (long long)g.blocksPerSeg * nSeg;
    g.ldsBytes = (size_t)K * kSynChipPitch;
    return g;
}
// samples [i0, i1) of block j of a segment of S samples; empty (i0 >= i1) past the segment's last group
DPE_SYN_HD void syn_block_range(int S, int align, int j, int &i0, int &i1)
{
    const long long g0 = (long long)j * kSynBlockGroups, g1 = g0 + kSynBlockGroups;
    const long long a = g0 * kSynLaneSamples - align, b = g1 * kSynLaneSamples - align;
    i0 = (int)(a < 0 ? 0 : (a > S ? S : a));
    i1 = (int)(b < 0 ? 0 : (b > S ? S : b));
}

// ---- what a call is refused for before anything is staged.  Returns nullptr or the reason (a printf format taking `chan`).
inline const char *syn_chan_problem(const dpe_chan_start &c, double amp)
{
    if (c.prn < 1 || c.prn > 37) return "channel %d: PRN outside 1..37";
    if (!std::isfinite(c.codePhaseStart) || !std::isfinite(c.carrierPhaseStart) || !std::isfinite(c.codeFrequency) ||
        !std::isfinite(c.carrierFrequency) || !std::isfinite(amp))
        return "channel %d: a parameter is not finite";
    if (!(c.codeFrequency > 0.0)) return "channel %d: code frequency not positive";
    return nullptr;
}

// The last-bit check of the record form: the nav-bit indices of the first and the last sample of [first, first + n) -- the code
// phase grows with n (fc > 0), so every index between lies between these.  false: the code phase leaves the exact range.
inline bool syn_bit_span(int64_t first, int64_t n, double fs, const dpe_chan_start &c, int64_t &bitFirst, int64_t &bitLast)
{
    DPE_SYN_FP
    const int fe = ((c.cpReference % 20) + 20) % 20;
    const double tl = syn_time_record(first + n - 1, fs), tf = syn_time_record(first, fs);
    const double lo = tf * c.codeFrequency + c.codePhaseStart, hi = tl * c.codeFrequency + c.codePhaseStart;
    if (!(std::fabs(lo) < kSynMaxChips && std::fabs(hi) < kSynMaxChips)) return false;
    double p;
    (void)syn_chip(tf, c.codeFrequency, c.codePhaseStart, p);
    bitFirst = (int64_t)syn_bit_index(p, fe);
    (void)syn_chip(tl, c.codeFrequency, c.codePhaseStart, p);
    bitLast = (int64_t)syn_bit_index(p, fe);
    return true;
}

// One channel's parameter block.  flipAt: the in-window sample of the sign change, or anything outside (0, S) for none.
inline SynChan syn_chan(const dpe_chan_start &c, double amp, int64_t flipAt, int S)
{
    SynChan d{};
    d.fc = c.codeFrequency;
    d.rc = c.codePhaseStart;
    d.fi = c.carrierFrequency;
    d.ri = c.carrierPhaseStart;
    d.amp = (float)amp;
    d.flipAt = (flipAt > 0 && flipAt < S) ? (int32_t)flipAt : kSynNoFlip;
    d.firstEdge = ((c.cpReference % 20) + 20) % 20;
    d.prnRow = c.prn - 1;
    return d;
}

}  // namespace dpe
