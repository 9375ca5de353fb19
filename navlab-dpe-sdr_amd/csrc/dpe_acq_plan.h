// dpe_acq_plan.h -- the acquisition search's plan as plain C++: what dpe_acq_create derives from its configuration, the DPE_ACQ_*
// switches and the device's answers (AcqShape, acq_shape), and the launches of one search in order, as records (AcqLaunch, acq_plan,
// acq_chunk_launches).  Nothing of HIP is included: dpe_acq.hip asks the runtime and the environment and passes the answers in, and
// host/test_acq_plan.cpp holds the same functions to a recorded table with a plain C++ compiler.  DESIGN.md 7b.1.
//
// The 1 GiB rule of the chunk, the rounding of the persistent block count, the 40 KB row limit of the statistics and the percentile
// positions are tie-sensitive: the expressions keep their operand order and types, and every function runs under fp contract(off).
#pragma once
#include <cmath>
#include <cstddef>

#include "../../include/dpe_hip.h"
#include "dpe_consts.h"

#if defined(__clang__)
#define DPE_PLAN_FP _Pragma("clang fp contract(off)")
#else
#define DPE_PLAN_FP
#endif

namespace dpe {

constexpr int kAcqFusedLen = 2500;   // delays per code period of acq_corr2500_kernel / acq_wipe_fft2500_kernel / the packed form
constexpr int kAcqFusedBins = 6;     // bins per block: 21 x 32 blocks are resident at once (three per CU) on 256 CUs
constexpr int kAcqBinGroup = 25;     // acq_fold_kernel: bins a block walks
constexpr int kAcqStatsR = 10;       // acq_stats_small_kernel: delays per thread, rows up to 2 560
constexpr size_t kAcqCplxBytes = 2 * sizeof(float);   // sizeof(float2)
// dynamic LDS of the kernels that opt in (dpe_acq.hip asserts them against kPkLdsBytes and AcqMixedShape<...>::ldsBytes)
constexpr size_t kAcqPackLds = 128000, kAcqMixedLds4000 = 51520, kAcqMixedLds5000 = 64400;

// The DPE_ACQ_* switches as dpe_acq_create reads them (false: not set).
struct AcqSwitches {
    bool noFused = false;      // DPE_ACQ_NO_FUSED (set at all): every search keeps the rocFFT chain
    bool noPack = false;       // DPE_ACQ_NO_PACK: non-coherent 10 x 2 500 search through acq_radix10_kernel + four-pass transforms
    bool noFwdPack = false;    // DPE_ACQ_NO_FWD_PACK: packed form with wipe kernel + rocFFT + decimation in front
    bool noFusedFwd = false;   // DPE_ACQ_NO_FUSED_FWD (-DDPE_EXPERIMENTS builds): textbook 2 500 search keeps wipe kernel + rocFFT
    bool statsLds = false;     // DPE_ACQ_STATS_LDS (-DDPE_EXPERIMENTS builds): rows of up to 2 560 delays through acq_stats_kernel
};

// What the runtime answered.
struct AcqDevice {
    int cus = 0;            // multiProcessorCount (< 1: the query failed)
    bool packLds = true;    // the 128 000 B opt-in of acq_corr25k_pack_kernel and acq_fwd25k_pack_kernel was granted (asked only when acq_wants_pack)
    bool mixedLds = true;   // the opt-ins of the four acq_corr_mixed_kernel instances were granted (asked only for a shape with mixedOptIn)
};

enum class AcqCorr { RocfftChain, Fused2500, FusedMixed, AliasPacked, AliasRadix10, AliasRadix10Mixed };
enum class AcqFwd { WipeRocfft, WipeFoldRocfft, WipeFft2500, FwdPack };

inline const char *acq_corr_name(AcqCorr c)
{
    switch (c) {
        case AcqCorr::Fused2500: return "fused-2500";
        case AcqCorr::FusedMixed: return "fused-mixed";
        case AcqCorr::AliasPacked: return "alias-packed";
        case AcqCorr::AliasRadix10: return "alias-radix10-2500";
        case AcqCorr::AliasRadix10Mixed: return "alias-radix10-mixed";
        default: return "rocfft-chain";
    }
}
inline const char *acq_fwd_name(AcqFwd f)
{
    switch (f) {
        case AcqFwd::WipeFoldRocfft: return "wipe-fold+rocfft";
        case AcqFwd::WipeFft2500: return "acq_wipe_fft2500_kernel";
        case AcqFwd::FwdPack: return "acq_fwd25k_pack_kernel";
        default: return "wipe+rocfft";
    }
}

struct AcqShape {
    int mode = 0;
    int S = 0, N = 0, M = 0, B = 0, P = 0;
    int len = 0;     // FFT length (S in mode 1; M in modes 0 and 2)
    int SX = 0;      // samples per Doppler row after the wipe-off (M in mode 0: time-folded)
    int chunk = 0;   // PRNs per chunked launch group
    AcqCorr corr = AcqCorr::RocfftChain;
    AcqFwd fwd = AcqFwd::WipeRocfft;
    // element counts of the buffers and tables (0: none)
    size_t nX = 0, nRc = 0, nY = 0, nSurf = 0, nMp = 0, nRcq = 0;
    size_t nTw = 0;       // exp(+j 2 pi n / M): the fused transforms
    size_t nTw25k = 0;    // exp(+j 2 pi n / 10 M): the radix-10 stage and the packed form
    size_t nTw2 = 0;      // W2500^(a c) as [c][a]: the packed form
    // rocFFT plans (batch 0: none).  The forward plan exists for every shape, also where no search executes it.
    int fwdLen = 0, fwdBatch = 0, invLen = 0, invBatch = 0;
    bool mixedOptIn = false;   // create obtains the LDS opt-in of the four acq_corr_mixed_kernel instances; a refusal fails it
    int cus = 256;             // packed form: persistent blocks at most (the device's CUs, rounded down to whole eights from eight on)
    // statistics: percentile positions of _trim_mean(max_percode, 10), the mask about the peak, the kernel
    int iLo = 0, iHi = 0, maskS = 0, rowInLds = 0;
    double fLo = 0.0, fHi = 0.0;
    bool statsSmall = false;   // acq_stats_small_kernel (row in registers), else acq_stats_kernel (row walked in LDS or memory)
};

inline bool acq_fused_len(int M) { return M == kAcqFusedLen || M == 4000 || M == 5000; }
// coherent / textbook search at 2 500 / 4 000 / 5 000 delays per code period: the fused kernels, which need neither the product buffer
// nor the inverse plan
inline bool acq_wants_fused(const dpe_acq_config &cfg, const AcqSwitches &sw)
{
    return (cfg.mode == 0 || cfg.mode == 2) && acq_fused_len(cfg.samplesPerWindow / cfg.nCodePeriods) && !sw.noFused;
}
// the reference's non-coherent search at 10 code periods of such a length: radix-10 stage + ten fused transforms per (PRN, bin), or the
// packed form; the product buffer holds the stage's output, no inverse plan
inline bool acq_wants_alias(const dpe_acq_config &cfg, const AcqSwitches &sw)
{
    return cfg.mode == 1 && acq_fused_len(cfg.samplesPerWindow / cfg.nCodePeriods) && cfg.nCodePeriods == 10 && !sw.noFused;
}
// Does create ask the runtime for the packed kernels' LDS at all?
inline bool acq_wants_pack(const dpe_acq_config &cfg, const AcqSwitches &sw)
{
    return acq_wants_alias(cfg, sw) && cfg.samplesPerWindow / cfg.nCodePeriods == kAcqFusedLen && !sw.noPack;
}

// Everything create derives by arithmetic; cfg has passed create's range checks.
inline AcqShape acq_shape(const dpe_acq_config &cfg, const AcqSwitches &sw, const AcqDevice &dev)
{
    DPE_PLAN_FP
    AcqShape s;
    s.mode = cfg.mode;
    s.S = cfg.samplesPerWindow; s.N = cfg.nCodePeriods; s.M = s.S / s.N; s.B = cfg.nBins; s.P = cfg.nPrn;
    s.len = (cfg.mode == 1) ? s.S : s.M;
    s.SX = (cfg.mode == 0) ? s.M : s.S;
    s.chunk = cfg.prnChunk > 0 ? (cfg.prnChunk < s.P ? cfg.prnChunk : s.P) : (8 < s.P ? 8 : s.P);
    // (the fused non-coherent form wants every PRN in one launch pair -- 32 PRNs x 25 bins: 0.19 ms at one chunk, 0.24 at chunks of
    //  8, 1.16 at chunks of 1 -- while its stage buffer stays modest: 160 MB at the reference's raster)
    if (cfg.prnChunk <= 0 && cfg.mode == 1 && s.M == 2500 && s.N == 10 && (size_t)s.P * s.B * s.S * kAcqCplxBytes <= ((size_t)1 << 30)) s.chunk = s.P;
    const size_t S = s.SX, B = s.B, P = s.P;
    const bool fused = acq_wants_fused(cfg, sw), alias = acq_wants_alias(cfg, sw);
    // the packed form keeps ten transforms of a (PRN, bin) in 128 000 B of dynamic LDS: a device (or partition) that does not grant
    // that much per work group runs the radix-10 kernel + four-pass transforms instead
    const bool pack = acq_wants_pack(cfg, sw) && dev.packLds;
    s.corr = fused ? (s.M == kAcqFusedLen ? AcqCorr::Fused2500 : AcqCorr::FusedMixed)
                   : alias ? (pack ? AcqCorr::AliasPacked : s.M == kAcqFusedLen ? AcqCorr::AliasRadix10 : AcqCorr::AliasRadix10Mixed)
                           : AcqCorr::RocfftChain;
    // textbook mode at 2 500 (N rows per bin): wipe-off and the forward transform in one launch, 0.271 -> 0.260 ms per 32-PRN window.
    // (Coherent mode keeps the two launches: one block per bin would have to fold ten periods -- a hundred sin / cos pairs per
    // thread on 125 blocks -- and measured 0.066 against 0.060 ms.)
    s.fwd = (pack && !sw.noFwdPack) ? AcqFwd::FwdPack
            : (s.corr == AcqCorr::Fused2500 && !sw.noFusedFwd && cfg.mode != 0) ? AcqFwd::WipeFft2500
            : cfg.mode == 0 ? AcqFwd::WipeFoldRocfft : AcqFwd::WipeRocfft;
    s.nX = B * S;
    s.nRc = P * (size_t)s.len;
    s.nY = fused ? 1 : pack ? B * S : (size_t)s.chunk * B * S;   // (packed form: the bins' decimated spectra)
    s.nSurf = P * B * (size_t)s.M;
    s.nMp = P * (size_t)s.M;
    s.fwdLen = s.len; s.fwdBatch = (int)(B * (S / s.len));
    if (!fused && !alias) { s.invLen = s.len; s.invBatch = (int)(s.chunk * B * (S / s.len)); }
    if (alias) s.nTw25k = (size_t)10 * s.M;
    if (pack) {
        s.nTw2 = 2500;
        s.nRcq = P * (size_t)s.len;
        if (dev.cus >= 1) s.cus = dev.cus >= 8 ? dev.cus / 8 * 8 : dev.cus;
    }
    if (fused || alias) {
        s.nTw = (size_t)s.M;
        s.mixedOptIn = s.M != kAcqFusedLen;
    }
    // percentile positions of _trim_mean(max_percode, 10): pos = (M - 1) q / 100, q = 5 and 95 (numpy.percentile)
    const int M = s.M;
    const double posLo = (double)(M - 1) * 5.0 / 100.0, posHi = (double)(M - 1) * 95.0 / 100.0;
    s.iLo = (int)std::floor(posLo); s.iHi = (int)std::floor(posHi);
    s.fLo = posLo - (double)s.iLo; s.fHi = posHi - (double)s.iHi;
    s.maskS = (int)std::ceil(cfg.samplingFrequency / kFCA);   // correlator.py:96-99
    // (the statistics kernel's static LDS is ~17 KB: the row joins it only while the sum stays below the 64 KB a launch gets without
    //  an opt-in -- M <= 10 240 -- and is read from memory beyond)
    s.rowInLds = (size_t)M * sizeof(float) <= 40 * 1024 ? 1 : 0;
    s.statsSmall = M <= 256 * kAcqStatsR && !sw.statsLds;
    return s;
}

// create succeeds only with the opt-ins its shape cannot do without
inline bool acq_create_ok(const AcqShape &s, const AcqDevice &dev) { return !s.mixedOptIn || dev.mixedLds; }

// ---- search: the launches ---------------------------------------------------------------------------------------------------
enum class AcqKernel {
    Wipe, WipeFold, WipeFft2500, FwdPack, FftFwd,                                    // forward
    Corr2500, Mixed4000, Mixed5000,                                                  // fused: one launch per search
    Decimate10, CorrPack, Radix10, Corr2500Alias, Mixed4000Alias, Mixed5000Alias,    // alias forms, per PRN chunk
    Mul, FftInv, Fold,                                                               // rocFFT chain, per PRN chunk
    StatsSmall, Stats,
    Count
};

inline const char *acq_kernel_name(AcqKernel k)
{
    switch (k) {
        case AcqKernel::Wipe: return "acq_wipe_kernel";
        case AcqKernel::WipeFold: return "acq_wipe_fold_kernel";
        case AcqKernel::WipeFft2500: return "acq_wipe_fft2500_kernel";
        case AcqKernel::FwdPack: return "acq_fwd25k_pack_kernel";
        case AcqKernel::FftFwd: return "rocfft forward";
        case AcqKernel::Corr2500: return "acq_corr2500_kernel<false>";
        case AcqKernel::Mixed4000: return "acq_corr_mixed_kernel<4000, 10, 8, 5, false>";
        case AcqKernel::Mixed5000: return "acq_corr_mixed_kernel<5000, 10, 10, 5, false>";
        case AcqKernel::Decimate10: return "acq_decimate10_kernel";
        case AcqKernel::CorrPack: return "acq_corr25k_pack_kernel";
        case AcqKernel::Radix10: return "acq_radix10_kernel";
        case AcqKernel::Corr2500Alias: return "acq_corr2500_kernel<true>";
        case AcqKernel::Mixed4000Alias: return "acq_corr_mixed_kernel<4000, 10, 8, 5, true>";
        case AcqKernel::Mixed5000Alias: return "acq_corr_mixed_kernel<5000, 10, 10, 5, true>";
        case AcqKernel::Mul: return "acq_mul_kernel";
        case AcqKernel::FftInv: return "rocfft inverse";
        case AcqKernel::Fold: return "acq_fold_kernel";
        case AcqKernel::StatsSmall: return "acq_stats_small_kernel";
        case AcqKernel::Stats: return "acq_stats_kernel";
        default: return "";
    }
}

// One launch.  The rocFFT records carry no grid: the plan (AcqShape::fwdLen / invLen and batch) is the launch.
struct AcqLaunch {
    AcqKernel kernel = AcqKernel::Count;
    unsigned int gx = 0, gy = 1, gz = 1, block = 0;
    size_t lds = 0;     // dynamic LDS bytes
    int bpb = 0;        // fused kernels: bins per block
    int nSeg = 0;       // fused kernels: transforms per (PRN, bin); acq_wipe_fft2500_kernel: periods folded into a row; acq_fold_kernel: terms
    int p0 = 0, pc = 0; // chunked launches: first PRN and PRNs of the chunk
    int order = 0;      // acq_corr25k_pack_kernel: XCD-aware item order (whole eights of PRNs on whole eights of blocks)
    int coherent = 0;   // acq_fold_kernel: |sum| instead of the sum of magnitudes
};

inline AcqLaunch acq_launch(AcqKernel k, unsigned int gx, unsigned int gy, unsigned int gz, unsigned int block, size_t lds = 0)
{
    AcqLaunch l;
    l.kernel = k; l.gx = gx; l.gy = gy; l.gz = gz; l.block = block; l.lds = lds;
    return l;
}

struct AcqPlan {
    int nHead = 0;
    AcqLaunch head[3];      // the forward launches and the fused forms' one correlation launch
    bool chunked = false;   // acq_chunk_launches for p0 = 0, chunk, 2 chunk, ... < P follow
    AcqLaunch stats;
};
constexpr int kAcqChunkLaunches = 3;

inline AcqPlan acq_plan(const AcqShape &s)
{
    AcqPlan p;
    const int S = s.SX, B = s.B, P = s.P, M = s.M;
    const bool coh = s.mode == 0;
    switch (s.fwd) {
        case AcqFwd::FwdPack:
            p.head[p.nHead++] = acq_launch(AcqKernel::FwdPack, B, 1, 1, 512, kAcqPackLds);
            break;
        case AcqFwd::WipeFft2500:
            p.head[p.nHead] = acq_launch(AcqKernel::WipeFft2500, B, coh ? 1 : s.N, 1, 512);
            p.head[p.nHead++].nSeg = coh ? s.N : 1;
            break;
        case AcqFwd::WipeFoldRocfft:
            p.head[p.nHead++] = acq_launch(AcqKernel::WipeFold, (M + 255) / 256, B, 1, 256);
            p.head[p.nHead++] = acq_launch(AcqKernel::FftFwd, 0, 1, 1, 0);
            break;
        case AcqFwd::WipeRocfft:
            p.head[p.nHead++] = acq_launch(AcqKernel::Wipe, (S + 1023) / 1024, B, 1, 256);
            p.head[p.nHead++] = acq_launch(AcqKernel::FftFwd, 0, 1, 1, 0);
            break;
    }
    if (s.corr == AcqCorr::FusedMixed) {
        // 4 / 5 Msps: the generic four-pass transform (dpe_acq_mixed.h), two blocks resident per CU; bins per block measured over 1 .. 8
        // (profiles/r5_ab_acq_rates.txt): 16 x 32 = 512 blocks = one round at two per CU / 32 x 32 = two rounds of ten transforms per bin
        const int bpb = coh ? 8 : 4;
        AcqLaunch &l = p.head[p.nHead++];
        l = M == 4000 ? acq_launch(AcqKernel::Mixed4000, (B + bpb - 1) / bpb, P, 1, 400, kAcqMixedLds4000)
                      : acq_launch(AcqKernel::Mixed5000, (B + bpb - 1) / bpb, P, 1, 500, kAcqMixedLds5000);
        l.bpb = bpb; l.nSeg = coh ? 1 : s.N;
    } else if (s.corr == AcqCorr::Fused2500) {
        // bins per block: six in the coherent mode (672 blocks = one round of the 768 resident ones); ONE in the textbook mode, whose blocks
        // already run ten transforms per bin -- 4 000 short blocks balance the tail (0.229 -> 0.206 ms per 32 x 125 search; five bins per
        // block, 800 blocks = one round plus 32 stragglers, measured 0.265)
        const int bpb = coh ? kAcqFusedBins : 1;
        AcqLaunch &l = p.head[p.nHead++];
        l = acq_launch(AcqKernel::Corr2500, (B + bpb - 1) / bpb, P, 1, 256);
        l.bpb = bpb; l.nSeg = coh ? 1 : s.N;
    } else p.chunked = true;
    p.stats = s.statsSmall ? acq_launch(AcqKernel::StatsSmall, P, 1, 1, 256)
                           : acq_launch(AcqKernel::Stats, P, 1, 1, 256, s.rowInLds ? (size_t)M * sizeof(float) : 0);
    return p;
}

// The launches of the PRN chunk that starts at p0 (shapes whose plan is chunked) -> their count.
inline int acq_chunk_launches(const AcqShape &s, int p0, AcqLaunch (&out)[kAcqChunkLaunches])
{
    const int S = s.SX, B = s.B, P = s.P, M = s.M;
    const int pc = s.chunk < P - p0 ? s.chunk : P - p0;
    int n = 0;
    if (s.corr == AcqCorr::AliasPacked) {
        if (p0 == 0 && s.fwd != AcqFwd::FwdPack) out[n++] = acq_launch(AcqKernel::Decimate10, 40, (unsigned int)B, 1, 640);
        const int items = pc * B, want = pc % 8 == 0 ? (items + 7) / 8 * 8 : items, nBlk = s.cus < want ? s.cus : want;
        out[n] = acq_launch(AcqKernel::CorrPack, nBlk, 1, 1, 512, kAcqPackLds);
        out[n++].order = (pc % 8 == 0 && nBlk % 8 == 0) ? 1 : 0;
    } else if (s.corr == AcqCorr::AliasRadix10 || s.corr == AcqCorr::AliasRadix10Mixed) {
        out[n++] = acq_launch(AcqKernel::Radix10, (M + 255) / 256, B, pc, 256);
        // one bin per block: 10 transforms each, B x pc blocks (25 x 32 = 800 at the reference's raster: one round of the chip)
        out[n] = M == 4000 ? acq_launch(AcqKernel::Mixed4000Alias, B, pc, 1, 400, kAcqMixedLds4000)
                 : M == 5000 ? acq_launch(AcqKernel::Mixed5000Alias, B, pc, 1, 500, kAcqMixedLds5000)
                             : acq_launch(AcqKernel::Corr2500Alias, B, pc, 1, 256);
        out[n].bpb = 1; out[n++].nSeg = s.N;
    } else {
        out[n++] = acq_launch(AcqKernel::Mul, (S + 1023) / 1024, B, pc, 256);
        // a short last chunk still runs the full-batch plan over stale rows; they are never read
        out[n++] = acq_launch(AcqKernel::FftInv, 0, 1, 1, 0);
        // mode 0 arrives already folded: one term, |.|
        out[n] = acq_launch(AcqKernel::Fold, (M + 255) / 256, (B + kAcqBinGroup - 1) / kAcqBinGroup, pc, 256);
        out[n].nSeg = s.mode == 0 ? 1 : s.N; out[n++].coherent = s.mode == 0 ? 1 : 0;
    }
    for (int i = 0; i < n; ++i) { out[i].p0 = p0; out[i].pc = pc; }
    return n;
}

// Every launch of one search, in order, while f says to go on (f returns false: stop) -> all were handed out.
template <class F>
inline bool acq_for_each_launch(const AcqShape &s, F &&f)
{
    const AcqPlan p = acq_plan(s);
    for (int i = 0; i < p.nHead; ++i)
        if (!f(p.head[i])) return false;
    for (int p0 = 0; p.chunked && p0 < s.P; p0 += s.chunk) {
        AcqLaunch c[kAcqChunkLaunches];
        const int n = acq_chunk_launches(s, p0, c);
        for (int i = 0; i < n; ++i)
            if (!f(c[i])) return false;
    }
    return f(p.stats);
}

}  // namespace dpe

#undef DPE_PLAN_FP
