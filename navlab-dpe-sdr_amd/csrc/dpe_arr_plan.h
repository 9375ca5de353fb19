// dpe_arr_plan.h -- the array combiner's host-side planning as plain C++: the input range a range of outputs needs, which workgroup
// computes which covariance blocks, the set of blocks a call counts in its statistics, the packing of a Hermitian covariance into
// M^2 integers, the LDS layout, the order of the FMA chain that applies the weights, and every refusal with its message.  Nothing
// of HIP is included: dpe_arr.hip passes sizes and addresses in, the kernel calls the same functions (DPE_STREAM_HD), and
// host/test_arr_plan.cpp holds them to their properties with a plain C++ compiler.  The index limits, the record cut and the
// refusals every stream stage makes are dpe_stream_plan.h's.  DESIGN.md 7j.
//
// The stage, for M elements and the block length L:  block k >= 0 covers the samples [k L, (k + 1) L) cut to the record; its
// covariance S_k (exact integers), loaded with lambda tr S_k / M, gives per constraint c the weights w = R^-1 c / (c^H R^-1 c);
// output n = k L + r of constraint b is  sum_a fp32(gain conj(w_{b,a})) x_a[n].  So output n needs the whole block n div L of every
// element, and a workgroup that owns the blocks [ka, kb] reads exactly their samples.
#pragma once
#include "dpe_stream_plan.h"

namespace dpe {

constexpr int kArrThreads = 256;            // lanes per workgroup
constexpr int kArrWaves = kArrThreads / 64;
constexpr int kArrMinM = 2, kArrMaxM = 8;   // elements
constexpr int kArrMaxB = 4;                 // constraints = outputs
constexpr int kArrMinL = 256, kArrMaxL = 65536;
constexpr int kArrUnitSamples = 4096;       // a workgroup (the launch unit) owns max(1, 4096 / L) consecutive blocks
constexpr int kArrMaxUnitBlocks = kArrUnitSamples / kArrMinL;
constexpr int64_t kArrMaxBlocks = INT64_C(1) << 24;  // blocks per analyse call

DPE_STREAM_HD int arr_unit_blocks(int L) { return L >= kArrUnitSamples ? 1 : kArrUnitSamples / L; }

// ---- the input range the outputs [outFirst, outFirst + outCount) read, cut to the record [0, recordLength) (recordLength < 0: no
// end).  lo >= hi: they read nothing but zeros.
inline void arr_needed(int64_t outFirst, int64_t outCount, int L, int64_t recordLength, int64_t &lo, int64_t &hi)
{
    lo = outFirst / L * L;
    hi = ((outFirst + outCount - 1) / L + 1) * L;
    stream_cut(recordLength, lo, hi);
}
// the same for the blocks [blockFirst, blockFirst + blockCount) of an analyse call
inline void arr_needed_blocks(int64_t blockFirst, int64_t blockCount, int L, int64_t recordLength, int64_t &lo, int64_t &hi)
{
    lo = blockFirst * L;
    hi = (blockFirst + blockCount) * L;
    stream_cut(recordLength, lo, hi);
}

// ---- ownership.  A call's blocks are k0 = outFirst div L .. k1 = (outFirst + outCount - 1) div L; unit u owns the blocks
// k0 + u arr_unit_blocks(L) .. cut to k1.  An analyse call's units are laid over its blocks the same way.
struct ArrLaunch {
    int64_t k0, k1;     // first and last block of the call
    int64_t units;
};
inline ArrLaunch arr_launch(int64_t outFirst, int64_t outCount, int L)
{
    ArrLaunch l{};
    l.k0 = outFirst / L;
    l.k1 = (outFirst + outCount - 1) / L;
    l.units = (l.k1 - l.k0) / arr_unit_blocks(L) + 1;
    return l;
}
// the blocks [ka, kb] of unit u, for the call's blocks [k0, k1]
DPE_STREAM_HD void arr_unit_range(int64_t k0, int64_t k1, int64_t u, int L, int64_t &ka, int64_t &kb)
{
    ka = k0 + u * arr_unit_blocks(L);
    kb = ka + arr_unit_blocks(L) - 1;
    if (kb > k1) kb = k1;
}
// the owner of output n (a sample index of the record) in a call whose first block is k0
inline int64_t arr_owner(int64_t n, int64_t k0, int L) { return (n / L - k0) / arr_unit_blocks(L); }
// the samples of block k inside the record
DPE_STREAM_HD int64_t arr_block_samples(int64_t k, int L, int64_t recordLength)
{
    if (recordLength < 0) return L;
    const int64_t c = recordLength - k * L;
    return c < 0 ? 0 : (c > L ? L : c);
}
// block k is counted by the call that holds its first sample k L among its outputs, when that sample lies inside the record
DPE_STREAM_HD bool arr_counted(int64_t k, int L, int64_t outFirst, int64_t outCount, int64_t recordLength)
{
    return k * L >= outFirst && k * L < outFirst + outCount && (recordLength < 0 || k * L < recordLength);
}
inline int64_t arr_counted_blocks(int64_t outFirst, int64_t outCount, int L, int64_t recordLength)
{
    int64_t end = outFirst + outCount;
    if (recordLength >= 0 && end > recordLength) end = recordLength;
    return stream_multiples(outFirst, end, L);
}

// ---- the covariance of a block as M^2 integers: entry (a, a) is S[a][a]; for a > b entry (a, b) is Re S[a][b] and entry (b, a) is
// Im S[a][b], with S[a][b] = sum x_a conj(x_b).  A wave reduces arr_padded(M) >= M^2 values, a power of two.
DPE_STREAM_HD constexpr int arr_padded(int M)
{
    int v = 4;
    while (v < M * M) v <<= 1;
    return v;
}
// (Re, Im) of S[a][b] from the packed entries
DPE_STREAM_HD void arr_cov_entry(const int64_t *p, int M, int a, int b, int64_t &re, int64_t &im)
{
    if (a == b) { re = p[a * M + a]; im = 0; }
    else if (a > b) { re = p[a * M + b]; im = p[b * M + a]; }
    else { re = p[b * M + a]; im = -p[a * M + b]; }
}

// ---- LDS layout of a workgroup (bytes from the allocation's start), for B = kArrMaxB
struct ArrLds {
    int cov;        // int64 [unit blocks][M^2]: the packed covariances
    int part;       // int64 [2][kArrWaves][arr_padded(M)]: the waves' partial sums of one block, two buffers taken in turn
    int applied;    // float2 [unit blocks][kArrMaxB][M]: v = fp32(gain conj(w))
    int fallback;   // uint32 [unit blocks]: nonzero where a constraint of the block took the fallback
    int counts;     // uint32 [4]: blocks, fallback blocks, clipped components of the workgroup
    int bytes;
};
inline ArrLds arr_lds(int M, int L)
{
    const int ub = arr_unit_blocks(L);
    ArrLds l{};
    l.cov = 0;
    l.part = l.cov + 8 * ub * M * M;
    l.applied = l.part + 8 * 2 * kArrWaves * arr_padded(M);
    l.fallback = l.applied + 8 * ub * kArrMaxB * M;
    l.counts = l.fallback + 4 * ub;
    l.bytes = l.counts + 16;
    return l;
}

// ---- the apply: y = sum_a v[a] x[a] with v = (vr, vi) and x = (xi, xq), each component one chain of FMAs from +0 with the
// elements in ascending order.  Every code path that forms an output calls this.
DPE_STREAM_HD void arr_apply(int M, const float *vr, const float *vi, const float *xi, const float *xq, float &re, float &im)
{
    re = 0.f;
    im = 0.f;
    for (int a = 0; a < M; ++a) {
        re = fmaf(vr[a], xi[a], re);
        re = fmaf(-vi[a], xq[a], re);
        im = fmaf(vr[a], xq[a], im);
        im = fmaf(vi[a], xi[a], im);
    }
}

// ---- what is refused before anything is allocated or launched.  true: refused, `msg` holds the reason.
// constraints: [B][M][2] doubles, or null for the unit vector of cfg->reference (then B = 1)
inline bool arr_config_problem(const dpe_arr_config *cfg, const double *constraints, char *msg, size_t len)
{
    DPE_STREAM_REFUSE(!cfg, "[ArrayCombiner] create: null argument");
    const int M = cfg->nElements, L = cfg->blockLength, B = cfg->nConstraints;
    DPE_STREAM_REFUSE(M < kArrMinM || M > kArrMaxM, "[ArrayCombiner] create: %d elements outside %d..%d", M, kArrMinM, kArrMaxM);
    DPE_STREAM_REFUSE(L < kArrMinL || L > kArrMaxL || (L & (L - 1)) != 0, "[ArrayCombiner] create: block length L = %d is no power of two in %d..%d", L,
                      kArrMinL, kArrMaxL);
    DPE_STREAM_REFUSE(B < 1 || B > kArrMaxB, "[ArrayCombiner] create: %d constraints outside 1..%d", B, kArrMaxB);
    DPE_STREAM_REFUSE(!(std::isfinite(cfg->loading) && cfg->loading >= 0.0), "[ArrayCombiner] create: loading not finite or negative");
    if (stream_gain_problem("[ArrayCombiner]", "create", cfg->gain, msg, len)) return true;
    if (stream_format_problem("[ArrayCombiner]", "create", cfg->outputFormat, msg, len)) return true;
    if (!constraints) {
        DPE_STREAM_REFUSE(B != 1, "[ArrayCombiner] create: %d constraints without constraint vectors (the default is one, the reference element's)", B);
        DPE_STREAM_REFUSE(cfg->reference < 0 || cfg->reference >= M, "[ArrayCombiner] create: reference element %d outside 0..%d", cfg->reference, M - 1);
        return false;
    }
    for (int b = 0; b < B; ++b) {
        bool zero = true;
        for (int i = 0; i < 2 * M; ++i) {
            const double v = constraints[(size_t)b * 2 * M + i];
            DPE_STREAM_REFUSE(!std::isfinite(v), "[ArrayCombiner] create: constraint %d is not finite", b);
            zero = zero && v == 0.0;
        }
        DPE_STREAM_REFUSE(zero, "[ArrayCombiner] create: constraint %d is zero", b);
    }
    return false;
}

// the checks process and analyse share: the element buffers and the record.  xAddr: the M device addresses, or null
inline bool arr_input_problem(const char *call, const dpe_arr_config &cfg, const uint64_t *xAddr, int64_t xFirst, int64_t xCount, int64_t recordLength,
                              char *msg, size_t len)
{
    DPE_STREAM_REFUSE(!xAddr, "[ArrayCombiner] %s: null array of input buffers", call);
    for (int a = 0; a < cfg.nElements; ++a) {
        DPE_STREAM_REFUSE(xAddr[a] == 0, "[ArrayCombiner] %s: null input buffer of element %d", call, a);
        DPE_STREAM_REFUSE(xAddr[a] % 4u != 0, "[ArrayCombiner] %s: the input of element %d is not aligned to an I/Q pair (4 bytes)", call, a);
    }
    return stream_held_problem("[ArrayCombiner]", call, xFirst, xCount, recordLength, msg, len);
}

// xAddr [M] / outAddr [B]: the device addresses
inline bool arr_process_problem(const dpe_arr_config &cfg, const uint64_t *xAddr, const uint64_t *outAddr, int64_t xFirst, int64_t xCount,
                                int64_t recordLength, int64_t outFirst, int64_t outCount, char *msg, size_t len)
{
    DPE_STREAM_REFUSE(!outAddr, "[ArrayCombiner] process: null array of output buffers");
    if (arr_input_problem("process", cfg, xAddr, xFirst, xCount, recordLength, msg, len)) return true;
    const unsigned outBytes = cfg.outputFormat == DPE_FE_OUT_F32 ? 8u : 4u;
    for (int b = 0; b < cfg.nConstraints; ++b) {
        DPE_STREAM_REFUSE(outAddr[b] == 0, "[ArrayCombiner] process: null output buffer of constraint %d", b);
        DPE_STREAM_REFUSE(outAddr[b] % outBytes != 0, "[ArrayCombiner] process: the output of constraint %d is not aligned to an I/Q pair (%u bytes)", b, outBytes);
    }
    if (stream_outputs_problem("[ArrayCombiner]", "process", outFirst, outCount, msg, len)) return true;
    int64_t lo, hi;
    arr_needed(outFirst, outCount, cfg.blockLength, recordLength, lo, hi);
    if (stream_coverage_problem("[ArrayCombiner]", "process", "outputs", "the buffers hold", outFirst, outCount, lo, hi, xFirst, xCount, msg, len)) return true;
    for (int b = 0; b < cfg.nConstraints; ++b)
        for (int a = 0; a < cfg.nElements; ++a)
            DPE_STREAM_REFUSE(outAddr[b] < xAddr[a] + 4u * (uint64_t)xCount && xAddr[a] < outAddr[b] + (uint64_t)outBytes * (uint64_t)outCount,
                              "[ArrayCombiner] process: the output of constraint %d overlaps the input of element %d", b, a);
    return false;
}

// covAlign / weightsAlign / appliedAlign: the three result addresses modulo 16 (0 for a null one)
inline bool arr_analyse_problem(const dpe_arr_config &cfg, const uint64_t *xAddr, int64_t xFirst, int64_t xCount, int64_t recordLength, int64_t blockFirst,
                                int64_t blockCount, unsigned covAlign, unsigned weightsAlign, unsigned appliedAlign, char *msg, size_t len)
{
    if (arr_input_problem("analyse", cfg, xAddr, xFirst, xCount, recordLength, msg, len)) return true;
    DPE_STREAM_REFUSE(covAlign % 8u != 0 || weightsAlign % 8u != 0 || appliedAlign % 4u != 0, "[ArrayCombiner] analyse: a result buffer is not aligned to its elements");
    DPE_STREAM_REFUSE(blockCount < 1 || blockCount > kArrMaxBlocks, "[ArrayCombiner] analyse: %lld blocks outside 1..2^24 per call", (long long)blockCount);
    DPE_STREAM_REFUSE(blockFirst < 0 || blockFirst > kStreamMaxIndex / cfg.blockLength - blockCount,
                      "[ArrayCombiner] analyse: first block %lld with %lld blocks outside the blocks 0..2^55 / L - 1 the outputs read", (long long)blockFirst,
                      (long long)blockCount);
    int64_t lo, hi;
    arr_needed_blocks(blockFirst, blockCount, cfg.blockLength, recordLength, lo, hi);
    return stream_coverage_problem("[ArrayCombiner]", "analyse", "blocks", "the buffers hold", blockFirst, blockCount, lo, hi, xFirst, xCount, msg, len);
}

}  // namespace dpe
