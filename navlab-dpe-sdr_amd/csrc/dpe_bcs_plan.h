// dpe_bcs_plan.h -- stage 1's launch plan as plain C++: what dpe_bcs_create derives from its configuration (BcsShape), what an Update
// learns from the channel values (BcsChanFacts), and the choice among the stage-1 forms with every tile, block and chunk count the
// launches need (BcsPlan, bcs_plan).  Nothing of HIP is included: dpe_bcs.hip asks the runtime and the environment and passes the
// answers in, and host/test_bcs_plan.cpp holds the same functions to a recorded table with a plain C++ compiler.  DESIGN.md 2.3a.
//
// Several choices are an arg-min over a cost in doubles or long longs: a tie broken differently is a different launch.  The
// expressions keep their operand order and types, and every function runs under fp contract(off).
#pragma once
#include <cmath>

#include "../../include/dpe_hip.h"
#include "dpe_consts.h"

#if defined(__clang__)
#define DPE_PLAN_FP _Pragma("clang fp contract(off)")
#else
#define DPE_PLAN_FP
#endif

namespace dpe {

constexpr int kSub = 256;        // samples per wave sub-tile (4 per lane) == moment block
constexpr int kSumSlots = 64;    // DC-sum slots per window (bcs_sum_kernel, window_mean)
constexpr int kB16Blocks = 4;    // blocks per CU the narrow, table-free form is held to (128 registers; five -> 96 with spills measured 1 % slower)
#ifndef DPE_CHIP_SPL
#define DPE_CHIP_SPL 17
#endif
constexpr int kSPL = DPE_CHIP_SPL;   // chip kernel: samples per lane (odd: the chunk stride in LDS entries must be odd for conflict-free writes)
constexpr int kPass = 64 * kSPL;     // chip kernel: samples per wave pass
#ifndef DPE_C2_OWN
#define DPE_C2_OWN 58
#endif
constexpr int k2Own = DPE_C2_OWN;   // chip2: owner lanes per pass: lanes 3 .. 60 (measured at H: 58 owners at 11 blocks per CU 0.593 ms per 128 windows,
                                    // 57 at 12 blocks 0.604, 50 at 13 blocks 0.635 -- lanes that own samples matter more than resident waves)
constexpr int k2MaxL1 = 24;    // chip2: L1 = floor(fs / fc) <= 24: chips of at most 25 samples
constexpr int k2MinL1 = 16;    // chip2: the margins reach +-32 samples: two regular chips must cover them
// widest supported lag window: the centre chunk (+-32) plus 4 chunks of 65 lags on each side
constexpr int kMaxLagHalfWidth = DPE_MAX_LAG_HALF_WIDTH;
static_assert(kMaxLagHalfWidth == 32 + 4 * 65, "centre chunk plus four 65-lag chunks per side");
constexpr int kMaxChunks = 1 + 2 * ((kMaxLagHalfWidth - 31 + 63) / 64);   // the chip form's chunks of 64 lags are the most

// ---- create ---------------------------------------------------------------------------------------------------------------
// The environment switches of dpe_hip.h as dpe_bcs_create read them (0 / false: not set).
struct BcsSwitches {
    bool forceFft = false;                   // DPE_BCS_FORCE_FFT
    bool noWide = false;                     // DPE_BCS_NO_WIDE (-DDPE_EXPERIMENTS builds)
    bool noBank16 = false, noFuse = false, noChip = false, noChip2 = false, noSumRide = false;   // DPE_BCS_NO_*
    int sumRideMin = 0;                      // DPE_BCS_SUMRIDE_MIN (>= 1)
    int rideLA = 0;                          // DPE_BCS_RIDE_LA (-DDPE_EXPERIMENTS builds, >= 1)
    int chip2P = 0, chipTpb = 0, tpb16 = 0;  // DPE_BCS_CHIP2_P, DPE_BCS_CHIP_TPB, DPE_BCS_TPB16
    int fat = -1;                            // DPE_BCS_FAT (-DDPE_EXPERIMENTS builds): finalize block shape (0 split, 1 fat)
};

struct BcsShape {
    int S = 0, L = 0, B = 0, maxWindows = 0, maxChannels = 0;   // the configuration: samples per window, lag / bin half widths
    double fs = 0.0;
    long long C = 0;             // carrier transform length, 8 * next_pow2(S) (batchcorrscores.cu:761)
    int nMom = 6;                // Taylor order of the moment expansion: power moments 0..5, 4 when the bin window is narrow
    bool fftMode = false;        // full-length FFT fallback (dpe_bcs_fft.h): lag windows beyond DPE_MAX_LAG_HALF_WIDTH, bin windows beyond the
                                 // moment expansion, or DPE_BCS_FORCE_FFT=1
    bool useTable = false;       // the sampling period is no whole number of ns: the kernels read the reference's rounded time table
    int LH = 32;                 // internal lag half width (4, 8, 16, 32)
    int nSub = 0;                // sub-tiles of kSub samples
    int tilesPerBlock = 1;       // fewest tiles per block ever used -> sizes the partial buffer
    int nBlk = 0;                // blocks per (window, SV) at that
    int nPassChip = 0;           // chip kernel: passes of kPass samples
    int chipTpbMax = 1;          // longest tile (passes) whose 6-moment block still meets the Taylor bound
    bool chipOK = false;         // create-time eligibility of the chip-boundary kernel (dpe_bcs_chip.h)
    int nBlkAlloc = 0;           // partial sums per (window, SV) the buffers hold
    int cus = 256;
    int resident16 = 1024;       // co-resident blocks of the 16-samples-per-lane kernel on the whole device
    int chipResident = 0;        // co-resident waves of the chip kernel on the whole device
    int chip2Resident = 0;       // and of its second form
    bool wideAllowed = true, bank16Allowed = true, fuseAllowed = true, chipAllowed = true, chip2Allowed = true, rideAllowed = true;
    int rideMinW = 48;           // smallest batch that takes the riding form (measured at H: 8 / 16 windows slower, 32 equal, 64 -1.2 %, 128 -2.6 %)
    int rideLA = 4;              // look-ahead of the sum blocks in windows
    int chip2PForce = 0, chipTpbForce = 0, tpb16Force = 0, fatForce = -1;
};

inline long long next_pow2(long long x)
{
    long long p = 1;
    while (p < x) p <<= 1;
    return p;
}

// Everything create derives by arithmetic; cfg has passed create's range checks.  chipResident / chip2Resident: bcs_shape_residency.
inline BcsShape bcs_shape(const dpe_bcs_config &cfg, const BcsSwitches &sw, int cus)
{
    DPE_PLAN_FP
    BcsShape s;
    s.S = cfg.samplesPerWindow; s.L = cfg.lagHalfWidth; s.B = cfg.binHalfWidth;
    s.maxWindows = cfg.maxWindows; s.maxChannels = cfg.maxChannels;
    s.fs = cfg.samplingFrequency;
    const int S = s.S;
    const double fs = s.fs;
    s.fftMode = sw.forceFft;   // full-length FFT form instead of the streaming kernels
    if (cfg.lagHalfWidth > kMaxLagHalfWidth || cfg.lagHalfWidth + 32 + kSub >= cfg.samplesPerWindow) s.fftMode = true;
    s.C = 8 * next_pow2(S);  // batchcorrscores.cu:761
    // Taylor remainder of the moment expansion must stay below fp32 rounding (dpe_bcs.hip, file header)
    const double th = 6.283185307179586 * 127.5 * cfg.binHalfWidth / (double)s.C;
    s.nMom = (std::pow(th, 4) / 24.0 < 1e-7) ? 4 : 6;   // Taylor order of the moment expansion
    if (!(std::pow(th, 6) / 720.0 < 2e-7)) s.fftMode = true;   // bin window too wide for the moment expansion at this C
    // The reference rounds the sample times to 1 ns (BCS_GenTimeIdcs :191-193).  For integer-ns sampling
    // periods (all usual SDR rates) that is a no-op and the kernels use n/fs; otherwise they read the
    // reference's own table.
    bool needTable = false;
    for (int n = 0; n < S && !needTable; ++n) {
        const double t = (double)n / fs, tr = std::round(t * 1.0e9) / 1.0e9;
        if (std::fabs(t - tr) > 4e-16 * (t + 1e-9)) needTable = true;
    }
    s.useTable = needTable;
    s.LH = cfg.lagHalfWidth <= 4 ? 4 : cfg.lagHalfWidth <= 8 ? 8 : cfg.lagHalfWidth <= 16 ? 16 : 32;
    s.nSub = (S + kSub - 1) / kSub;
    const int nTiles = (s.nSub + 3) / 4;
    s.tilesPerBlock = (nTiles + 63) / 64;
    s.nBlk = (nTiles + s.tilesPerBlock - 1) / s.tilesPerBlock;
    // chip-boundary kernel (dpe_bcs_chip.h): lag windows of 17..31 samples (wider: chunks of 64 lags) at sampling rates where a
    // sub-tile holds few chips, plain n/fs sample times; its moment block is one pass of kPass samples, and a chip's
    // second-order term (theta len)^2 / 24 must stay below fp32 rounding
    s.nPassChip = (S + kPass - 1) / kPass;
    {
        const double thetaB = 6.283185307179586 * cfg.binHalfWidth / (double)s.C;   // phase step per sample of the outermost bin
        const double chipLen = fs / kFCA * 1.001;
        // the moment block is the wave's tile of tpb passes, 6 moments: (thetaB tpb kPass / 2)^6 / 720 < 2e-7
        const double halfMax = std::pow(2e-7 * 720.0, 1.0 / 6.0) / thetaB;
        s.chipTpbMax = (int)(2.0 * halfMax / kPass);
        if (s.chipTpbMax > 32) s.chipTpbMax = 32;
        s.chipOK = s.LH == 32 && !needTable && (kFCA / fs) * 128.0 < 40.0 && s.chipTpbMax >= 1 && chipLen < 31.0 &&
                   (thetaB * chipLen) * (thetaB * chipLen) / 24.0 < 5e-7 && S >= 2 * kPass;
    }
    s.nBlkAlloc = s.nBlk;
    s.cus = cus;
    s.resident16 = ((s.LH <= 4 && !needTable) ? kB16Blocks : 3) * cus;   // the kernel's launch bounds
    if (s.chipOK) {
        // partial sums of up to 128 blocks per (window, SV); a handle for a few windows gets one block per pass
        int want = 2048 / cfg.maxWindows > 128 ? 2048 / cfg.maxWindows : 128;
        if (want > s.nPassChip) want = s.nPassChip;
        if (want < (s.nPassChip + s.chipTpbMax - 1) / s.chipTpbMax) want = (s.nPassChip + s.chipTpbMax - 1) / s.chipTpbMax;
        if (s.nBlkAlloc < want) s.nBlkAlloc = want;
    }
    s.wideAllowed = !sw.noWide;
    s.bank16Allowed = !sw.noBank16;
    s.fuseAllowed = !sw.noFuse;
    s.chipAllowed = !sw.noChip;
    s.chip2Allowed = !sw.noChip2;
    s.rideAllowed = !sw.noSumRide;
    if (sw.sumRideMin >= 1) s.rideMinW = sw.sumRideMin;
    if (sw.rideLA >= 1) s.rideLA = sw.rideLA;
    s.chip2PForce = sw.chip2P;
    s.chipTpbForce = sw.chipTpb;
    s.tpb16Force = sw.tpb16;
    s.fatForce = sw.fat;
    return s;
}

// The runtime's occupancy answers (blocks per CU, <= 0: none) for bcs_bank_chip_kernel<6> and bcs_bank_chip2_kernel<6, 24>; create
// asks only for a shape with chipOK.
inline void bcs_shape_residency(BcsShape &s, int chipBlocksPerCU, int chip2BlocksPerCU)
{
    s.chipResident = (chipBlocksPerCU > 0 ? chipBlocksPerCU : 12) * s.cus;
    s.chip2Resident = (chip2BlocksPerCU > 0 ? chip2BlocksPerCU : 11) * s.cus;
}

// ---- Update: the channel values -------------------------------------------------------------------------------------------
// The chip kernels' eligibility is a property of the channel VALUES (all false: not asked, see bcs_wants_chip).
struct BcsChanFacts {
    bool chip = false;      // every channel: 2 pi |fi| <= 0.25 fc, the range of the closed-form DC term of a chip
    bool chip2 = false;     // and: a common l1 in k2MinL1 .. k2MaxL1, the nav-bit boundary on a chip boundary of the replica
    int l1 = 0;             // floor(fs / fc) of the first channel: chips of l1 or l1 + 1 samples
    double stepMax = 0.0;   // largest code step (chips per sample)
};

// Chan: BcsChanDev (dpe_prep.h) or any struct with its fields rc, codeStep, fc, fi, invStep, idxNext, hasFlip.
template <class Chan>
inline BcsChanFacts bcs_chan_facts(const Chan *chan, int n, bool chip2Allowed)
{
    DPE_PLAN_FP
    BcsChanFacts f;
    // chip-boundary kernel: the closed-form DC term of a chip needs 2 pi |fi| / fc <= 0.25 (|fi| below ~40 kHz)
    f.chip = true;
    for (int i = 0; f.chip && i < n; ++i)
        if (6.283185307179586 * std::fabs(chan[i].fi) > 0.25 * chan[i].fc) f.chip = false;
    // second form of the chip kernel (dpe_bcs_chip2.h): every chip 16 .. 25 samples long, and the nav-bit boundary
    // (BCS_NavBitBoundary :247-253) on a chip boundary of the replica (:347-349) -- it is, unless fp64 rounding separates them
    f.chip2 = f.chip && chip2Allowed;
    for (int i = 0; f.chip2 && i < n; ++i) {
        const Chan &d = chan[i];
        const int l1 = (int)d.invStep;   // chips of l1 or l1 + 1 samples; instantiated for every l1 in 16 .. 24 (16.4 .. 25.6 Msps)
        if (i == 0) f.l1 = l1;
        if (l1 != f.l1 || l1 < k2MinL1 || l1 > k2MaxL1) f.chip2 = false;
        if (d.hasFlip && (int)std::fma((double)d.idxNext, d.codeStep, d.rc) == (int)std::fma((double)(d.idxNext - 1), d.codeStep, d.rc)) f.chip2 = false;
        if (d.codeStep > f.stepMax) f.stepMax = d.codeStep;
    }
    return f;
}

// ---- Update: the plan -----------------------------------------------------------------------------------------------------
struct BcsCall {
    bool dev = false;            // the channel parameters are on the device already (dpe_bcs_update_dev / _prepared)
    bool graphEnabled = false;   // dpe_bcs_set_graph
    bool capturing = false;      // the stream is being captured into a hipGraph
    bool vecOK = false;          // 16-byte aligned samples, window stride a multiple of 4
    bool rerun = false;          // the guarded general kernels behind a hinted chip-kernel launch (BcsParamBlock::guard)
    bool coPending = false;      // a task of the device-resident channel manager waits for the next stage-1 launch
    bool profiler = false;       // per-kernel event timing
};

enum class BcsForm { Dense, Wide, Bank16, Chip, Chip2, Fft };

inline const char *bcs_form_kernel(BcsForm f)
{
    switch (f) {
        case BcsForm::Chip2: return "bcs_bank_chip2_kernel";
        case BcsForm::Chip: return "bcs_bank_chip_kernel";
        case BcsForm::Bank16: return "bcs_bank16_kernel";
        case BcsForm::Wide: return "bcs_bank_wide_kernel";
        case BcsForm::Fft: return "rocfft full-lag path (bcs_fft_*_kernel)";
        default: return "bcs_bank_kernel";
    }
}

// One chunk of lags: the centre chunk first (it makes the replica choice and the Doppler bank), then the side chunks of a window
// wider than +-32 -- the same kernels against the replica delayed by lagShift samples.
struct BcsChunk {
    int lagShift = 0;
    bool c2 = false;     // the second chip form produces this chunk (the centre chunk; side chunks use the first form)
    int nMomUse = 6, nBlkUse = 0, momLenUse = 0;
};

struct BcsPlan {
    BcsForm form = BcsForm::Dense;   // the centre chunk's stage-1 kernel
    const char *kernel = "";
    bool chip = false;       // form is Chip or Chip2 (side chunks of either: the first chip form)
    int nTiles = 0;          // tiles per (window, SV) of the dense / wide / bank16 forms
    int tpb = 0;             // tiles (chip: passes) per block
    int nBlk = 0;            // blocks per (window, SV)
    int chipNMom = 6;
    int c2Lt = 0, c2nBlk = 0, c2NMom = 6, c2L1 = 0;   // second chip form: tile length (samples), tiles, moment order, samples per chip
    bool fuse = false;       // dense: the DC sums ride in the bank kernel, the finalize kernel applies the mean
    bool coRide = false;     // the channel manager's task rides as an extra block of the fused launch
    bool inl = false;        // the channel parameters travel as kernel arguments
    bool upInSum = false;    // the DC-sum kernel (riding sums: a kernel of its own) carries the parameter upload
    bool useGraph = false;   // the Update is captured / replayed as a hipGraph
    bool vecOK = false;      // 16-byte lane loads of the samples (BcsCall::vecOK)
    bool ride = false;       // chip2 batches: the DC sums ride in the chip2 launch
    int rideF = 0, rideSB = 0, rideGS = 1;
    int sumBlocks = 1;       // blocks per window of the DC sums
    int sumSlotsUsed = 1;    // slots the finalize kernel (and read_info) adds
    bool sumLaunch = false;  // a DC-sum kernel of its own in front
    int chunkLags = 65, nSideChunks = 0;
    int nBinBlk = 1;
    bool fatFinalize = false;
    int nChunks = 0;
    BcsChunk chunk[kMaxChunks];
};

// Blocks per window of the DC-sum kernel: ~8192 samples per block for batches; few windows get up to
// one int4 load per thread (a lone window is latency-bound, not bandwidth-bound).
inline int sum_blocks(int S, int nWindows)
{
    const int base = S / 8192 > 0 ? S / 8192 : 1;
    const int fine = (S / 4 + 255) / 256;
    int want = 512 / nWindows < fine ? 512 / nWindows : fine;
    if (want < base) want = base;
    return want > kSumSlots ? kSumSlots : want;
}

// Does this call ask the channel values about the chip kernels at all?
inline bool bcs_wants_chip(const BcsShape &s, bool rerun) { return s.chipOK && s.chipAllowed && !rerun; }
// the per-kernel event timing and the graph replay exclude each other
inline bool bcs_use_graph(const BcsCall &call) { return call.graphEnabled && !call.profiler && !call.dev; }

inline BcsPlan bcs_plan(const BcsShape &s, const BcsChanFacts &facts, int nWindows, int nChan, const BcsCall &call)
{
    DPE_PLAN_FP
    BcsPlan p;
    const int S = s.S;
    const double fs = s.fs;
    p.sumBlocks = sum_blocks(S, nWindows);
    if (s.fftMode) {
        p.form = BcsForm::Fft;
        p.kernel = bcs_form_kernel(p.form);
        p.sumSlotsUsed = p.sumBlocks;
        p.sumLaunch = true;
        return p;
    }
    const bool chip = bcs_wants_chip(s, call.rerun) && facts.chip;
    bool chip2 = chip && facts.chip2;
    const double stepMax = facts.stepMax;
    p.c2L1 = facts.l1;
    p.useGraph = bcs_use_graph(call);
    p.vecOK = call.vecOK;
    // few channels (the per-window call of a running receiver): parameters travel as kernel arguments of
    // the bank / finalize kernels; batches go through one H2D copy from the pinned staging block.  A
    // captured graph would freeze by-value arguments, so the graph path always copies.
    p.inl = !call.dev && !call.capturing && nWindows * nChan <= DPE_MAX_CHAN;
    // (batches: the DC-sum kernel carries the parameter upload; a captured graph keeps a copy node)
    p.upInSum = !call.dev && !p.inl && !call.capturing;
    // |lag| <= 32 windows: boundary-difference kernel when a sub-tile holds few chip boundaries
    // (~128 codeStep per lag step against 4 x 65 dense FMAs per lane), else a dense kernel
    const bool wide = !chip && s.LH == 32 && s.wideAllowed && (kFCA / fs) * 128.0 < 40.0;
    // narrow lag windows in batches: the 16-samples-per-lane kernel (tiles of 16 sub-tiles) once the batch
    // offers >= 2048 of its tiles; fewer (a single window in particular) keep the short 4-sub-tile tiles
    const int nTiles16 = (s.nSub + 15) / 16;
    const bool use16 = !wide && s.LH <= 8 && s.bank16Allowed && (long long)nTiles16 * nChan * nWindows >= 2048;
    const int nTiles = use16 ? nTiles16 : (s.nSub + 3) / 4;
    int tpb;   // tiles per block: amortise the end-of-block lag reduction while keeping >= ~4096 blocks in flight
    if (use16) {
        // the choice that minimises rounds x (tiles + fixed cost): a block's start-up (chip table into LDS, parameters, the
        // end-of-side lag reductions) measures ~0.4 tile times, and a launch whose blocks are all resident in two rounds beats
        // eight rounds of short ones (config R: 4 tiles per block 0.237 ms, all 13 in one block 0.181 ms)
        const int least = (nTiles + s.nBlk - 1) / s.nBlk;   // the partial buffer holds s.nBlk blocks per (window, SV)
        double best = -1.0;
        tpb = least < 1 ? 1 : least;
        for (int c = tpb; c <= nTiles; ++c) {
            const long long blocks = (long long)((nTiles + c - 1) / c) * nChan * nWindows;
            const double cost = (double)((blocks + s.resident16 - 1) / s.resident16) * ((double)c + 0.4);
            if (best < 0.0 || cost < best) { best = cost; tpb = c; }
        }
        if (s.tpb16Force >= least && s.tpb16Force >= 1) tpb = s.tpb16Force;
    } else {
        tpb = (int)(((long long)nTiles * nChan * nWindows) / 4096);
        if (tpb < s.tilesPerBlock) tpb = s.tilesPerBlock;
        if (tpb > 16) tpb = 16;
    }
    // chip-boundary kernel: one wave per block walks tpb passes of one (window, SV)
    int chipNMom = 6;
    if (chip) {
        // passes per wave: the choice that leaves the smallest tail -- ceil(waves / resident waves) rounds of tpb passes each
        const int least = (s.nPassChip + s.nBlkAlloc - 1) / s.nBlkAlloc;
        long long best = -1;
        tpb = least;
        for (int c = least; c <= s.chipTpbMax; ++c) {
            const long long waves = (long long)((s.nPassChip + c - 1) / c) * nChan * nWindows;
            // + the finalize kernel's share: its time grows by ~0.06 pass-rounds per partial block (measured, config H)
            const long long cost = 100 * ((waves + s.chipResident - 1) / s.chipResident) * c + 6 * ((s.nPassChip + c - 1) / c);
            if (best < 0 || cost < best) { best = cost; tpb = c; }
        }
        if (s.chipTpbForce >= least && s.chipTpbForce <= s.chipTpbMax) tpb = s.chipTpbForce;
        const double thc = 6.283185307179586 * s.B / (double)s.C * 0.5 * ((double)tpb * kPass - 1.0);
        chipNMom = (std::pow(thc, 4) / 24.0 < 1e-7) ? 4 : 6;
    }
    const int nBlk = chip ? (s.nPassChip + tpb - 1) / tpb : (nTiles + tpb - 1) / tpb;
    // second form: a tile = the chips that start inside a nominal range of Lt samples, at most P passes of k2Own chips
    int c2Lt = 0, c2nBlk = 0, c2NMom = 6;
    if (chip2) {
        const double thetaB = 6.283185307179586 * s.B / (double)s.C;
        const double halfMax = std::pow(2e-7 * 720.0, 1.0 / 6.0) / thetaB;   // 6-moment Taylor radius (samples)
        long long best = -1;
        for (int P = 1; P <= 64; ++P) {
            const int Lt = (int)std::floor((double)(k2Own * P - 2) / stepMax);
            if (Lt < 64 || 0.5 * Lt + 26.0 > halfMax) continue;
            const int nb = (S + Lt - 1) / Lt;
            if (nb > s.nBlkAlloc) continue;
            if (s.chip2PForce > 0 && P != s.chip2PForce) continue;
            const long long waves = (long long)nb * nChan * nWindows;
            const long long cost = 100 * ((waves + s.chip2Resident - 1) / s.chip2Resident) * P + 6 * nb;
            if (best < 0 || cost < best) { best = cost; c2Lt = Lt; c2nBlk = nb; }
        }
        if (c2Lt == 0) chip2 = false;
        else {
            const double thc = thetaB * (0.5 * c2Lt + 26.0);
            c2NMom = (std::pow(thc, 4) / 24.0 < 1e-7) ? 4 : 6;
        }
    }
    p.form = chip2 ? BcsForm::Chip2 : chip ? BcsForm::Chip : use16 ? BcsForm::Bank16 : wide ? BcsForm::Wide : BcsForm::Dense;
    p.kernel = bcs_form_kernel(p.form);
    p.chip = chip;
    // single windows (<= 37 (window, channel) pairs) with a dense stage-1 kernel: no separate DC-sum launch, the
    // sums ride along in the bank kernel (FUSE) and the finalize kernel applies the mean
    const bool fuse = nWindows * nChan <= DPE_MAX_CHAN && !use16 && !wide && !chip && s.LH <= 16 && s.L <= 32 && s.fuseAllowed;
    // chip2 batches: the DC sums ride in the chip2 launch (sum blocks interleaved ahead of the correlator blocks, dpe_bcs_chip2.h);
    // the parameter upload keeps a small kernel of its own (riding as well, every correlator block had to poll for it first thing:
    // 0.7035 against 0.696 ms per step)
    bool ride = chip2 && !call.dev && !call.capturing && call.vecOK && s.rideAllowed && nWindows >= s.rideMinW;
    int sumBlocks = p.sumBlocks;
    int rideF = 0, rideSB = 0, rideGS = 1;
    if (ride) {   // one sum slot per correlator tile (the sum block then shares its tile's XCD): <= 64 slots, 31-bit sum fields
        if (c2nBlk > kSumSlots || c2Lt + 8 >= 32768) ride = false;
        else sumBlocks = c2nBlk;
    }
    if (ride) {
        const long long totalSum = (long long)nWindows * sumBlocks, NG = ((long long)c2nBlk * nWindows + 7) / 8;
        const int lookAhead = s.rideLA;   // windows between a sum block and the correlator blocks of its tile
        rideF = (int)(((long long)lookAhead * sumBlocks + 7) / 8 * 8);
        const long long groupsAvail = NG - ((long long)lookAhead * c2nBlk + 7) / 8 - 1;
        if (rideF >= totalSum || groupsAvail < 1) rideF = (int)((totalSum + 7) / 8 * 8);
        else {
            // sum blocks per group of 8 K correlator blocks at a STEADY lead (a lead that grows puts the samples a sum block fetched
            // out of its XCD's L2 before the correlator blocks of the same tile read them): whole eights per group, or one eight
            // every rideGS groups; what does not fit behind the look-ahead joins the blocks in front
            const long long rest = totalSum - rideF;
            if (rest >= 8 * groupsAvail) { rideSB = (int)(rest / (8 * groupsAvail)) * 8; rideGS = 1; }
            else { rideSB = 8; rideGS = (int)((8 * groupsAvail) / rest); }
            const long long cap = (long long)rideSB * (groupsAvail / rideGS);
            if (totalSum - cap > rideF) rideF = (int)((totalSum - cap + 7) / 8 * 8);
        }
    }
    p.nTiles = nTiles; p.tpb = tpb; p.nBlk = nBlk; p.chipNMom = chipNMom;
    p.c2Lt = c2Lt; p.c2nBlk = c2nBlk; p.c2NMom = c2NMom;
    p.fuse = fuse;
    p.ride = ride; p.rideF = rideF; p.rideSB = rideSB; p.rideGS = rideGS;
    p.sumBlocks = sumBlocks;
    p.sumSlotsUsed = fuse ? nBlk : sumBlocks;
    // a pending task of the device-resident channel manager: an extra block of the FUSE form's launch, a kernel of its own in
    // front of every other form
    p.coRide = call.coPending && fuse && !s.useTable && !call.capturing;
    p.sumLaunch = !fuse && !ride && !call.rerun;   // (a re-run uses the sums of the launch it follows: same window, same slots)
    // Lag windows wider than +-32: further chunks of 65 lags, centred 65 samples apart.  One chunk when L <= 32.
    // (the chip kernel's lanes cover lagShift - 32 .. lagShift + 31: chunks of 64 lags, 64 apart)
    p.chunkLags = chip ? 64 : 65;
    p.nSideChunks = chip ? (s.L > 31 ? (s.L - 31 + 63) / 64 : 0) : (s.L > 32 ? (s.L - 32 + 64) / 65 : 0);
    p.nBinBlk = (2 * s.B + 1 + 15) / 16;
    // batches: one fat block per (window, SV); few windows: 1 + nBinBlk short blocks (see the kernel);
    // side chunks of a wide lag window: one block per (window, SV), code-bank entries only
    // (crossover measured in round 2: 96 / 128 (window, SV) pairs are faster split, 192 / 256 / 384 fat -- H at 32 windows 0.0205 -> 0.0113 ms)
    p.fatFinalize = p.nBinBlk <= 4 && (long long)nChan * nWindows >= 192;
    if (s.fatForce >= 0) p.fatFinalize = p.nBinBlk <= 4 && s.fatForce == 1;   // (experiment builds)
    p.nChunks = 2 * p.nSideChunks + 1;
    for (int chunk = 0; chunk < p.nChunks; ++chunk) {
        BcsChunk &c = p.chunk[chunk];
        c.lagShift = chunk == 0 ? 0 : ((chunk + 1) / 2) * p.chunkLags * ((chunk & 1) ? 1 : -1);
        c.c2 = chip2 && c.lagShift == 0;
        c.nMomUse = c.c2 ? c2NMom : chip ? chipNMom : s.nMom;
        c.nBlkUse = c.c2 ? c2nBlk : nBlk;
        c.momLenUse = c.c2 ? c2Lt : chip ? tpb * kPass : kSub;
    }
    return p;
}

}  // namespace dpe

#undef DPE_PLAN_FP
