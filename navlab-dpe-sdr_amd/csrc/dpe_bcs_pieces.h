// dpe_bcs_pieces.h -- the device pieces the forms of stage 1 share ("Stage 1's shared pieces"), included by
// dpe_bcs.hip ahead of the kernels.  Plain forced-inline functions: every kernel is still one straight text that calls them.
// That every form gives the oracle's banks through one bcs_finalize_kernel rests, where a kernel calls a piece, on one copy of
// that arithmetic.  A body calls a piece only where the generated code allows it (profiles/stage1_pieces_isa.txt); the places
// that keep a piece's text carry a comment "restates <piece>", and a change to that piece is made there as well:
//   bcs_bank_kernel        every piece: its closed-loop instantiations <*,*,false,true,true> have to keep their loops line for
//                          line, and any piece call in that body shifts their scalar registers
//   bcs_bank16_kernel      calls fill_chips, side_active and lag_partial_block; block_map, the replica build (replica_fast in
//                          its batched form, replica_circular through the padded index map), wipe_seed_at and the row-wise
//                          moment store keep their text there, as do the segment and the moments' shift ("---- b16: <name>")
//   bcs_bank_wide_kernel   calls every piece it has a use for; its halo seed is consumed by plain C++ and restates wipe_seed_at
//   bcs_bank_chip_kernel   calls block_map, wipe_seed_at (twiddles) and moment_set_reduce_store (flush); the seeds inside its
//                          pass loop keep their text
//   bcs_bank_chip2_kernel  every piece: block_map, wipe_seed_at, the flush's store, and iq_add4 / iq_add in ride_sum_block and
//                          ride_window_mean -- each of these calls moved a line of its pass loops
#pragma once

namespace dpe {

constexpr int kNMomMax = 6;  // power moments 0..5 at most; 4 when the bin window is narrow (chosen at create)
typedef float f2 __attribute__((ext_vector_type(2)));

// ---- complex arithmetic, phases ------------------------------------------------------------------------------------------------
// Complex product {a.x b.x - a.y b.y, a.x b.y + a.y b.x} in TWO packed instructions.  The compiler's own lowering of
// the same expression is pk_mul + two pk_fma (one per sign) + a v_mov to stitch the halves; the operand-select and
// lane-negate modifiers of v_pk_fma_f32 do it directly:  t = a.x * b;  r = {-a.y, a.y} * {b.y, b.x} + t.
// Inline asm is opaque to the compiler's hazard recogniser: operands that come straight from a transcendental
// (v_sin / v_cos need one wait state before a VALU consumer on gfx94x/95x) must go through wipe_seed() first.
__device__ __forceinline__ f2 cmul(f2 a, f2 b)
{
    f2 t, r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(t) : "v"(a), "v"(b));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]" : "=v"(r) : "v"(a), "v"(b), "v"(t));
    return r;
}

// conj(exp(j 2 pi f)) from the hardware sin/cos (argument in revolutions), safe to feed into cmul()
__device__ __forceinline__ f2 wipe_seed(float f)
{
    f2 w = f2{__builtin_amdgcn_cosf(f), -__builtin_amdgcn_sinf(f)};
    asm volatile("s_nop 1" : "+v"(w));   // covers the trans -> VALU forwarding hazard for the asm consumers
    return w;
}

// Wipe-off seed: the same from an fp64 phase in revolutions, reduced to [0, 1) before it is rounded to fp32
__device__ __forceinline__ f2 wipe_seed_at(double ph)
{
    ph -= floor(ph);
    return wipe_seed((float)ph);
}

// Time of sample n: n/fs, or (TABLE) the reference's ns-rounded table (BCS_GenTimeIdcs,
// batchcorrscores.cu:185-196) when the sampling period is not an integer number of nanoseconds.
template <bool TABLE>
__device__ __forceinline__ double code_phase(const BcsChanDev &ch, const double *tT, int m)
{
    if (TABLE) return fma(tT[m], ch.fc, ch.rc);
    return fma((double)m, ch.codeStep, ch.rc);
}
template <bool TABLE>
__device__ __forceinline__ double carr_phase(const BcsChanDev &ch, const double *tT, int n)
{
    if (TABLE) return fma(tT[n], ch.fi, ch.ri);
    return fma((double)n, ch.carrStep, ch.ri);
}

// TABLE mode: the wipe-off of sample nSeed + i is reached from the seed at nSeed by i uniform rotations exp(-j 2 pi fi / fs), but the
// reference's sample times are rounded to 1 ns (BCS_GenTimeIdcs :191-193), i.e. NOT uniformly spaced: the phase that is still owed,
// eps = 2 pi fi ((t[n] - t[nSeed]) - i / fs) <= 2 pi fi 1 ns, is applied as the first-order rotation w (1 - j eps).  For rates
// whose period is a half-integer number of ns (16 Msps: 62.5 ns) the rounding is systematic (every odd sample +0.5 ns) and the
// omitted term was a first-order error of pi fi 0.5 ns of the peak (8.6e-5 at fi = 60 kHz, 3.6e-6 at 2.5 kHz; found by the round-2
// fuzz sweep -- at 2.046 Msps the rounding is quasi-random and averaged out).
template <bool TABLE>
__device__ __forceinline__ f2 table_fix(f2 wv, const BcsChanDev &ch, const double *tT, int nSeed, int i, int S)
{
    if (!TABLE) return wv;
    int n = nSeed + i;
    n = n < S ? n : S - 1;
    const double d = fma(tT[n] - tT[nSeed < S ? nSeed : S - 1], ch.fi, -(double)(n - (nSeed < S ? nSeed : S - 1)) * ch.carrStep);
    const float eps = (float)(6.283185307179586476925286766559 * d);
    return f2{fmaf(eps, wv.y, wv.x), fmaf(-eps, wv.x, wv.y)};
}

// ---- launch bookkeeping ----------------------------------------------------------------------------------------------------------
// Closed-loop calls (one window, <= 37 channels) pass the channel parameters in the kernel-argument
// segment of the bank and finalize kernels (params_ptr, dpe_common.h): no H2D copy command, no staging
// buffer that must outlive the call.  pb must stay the FIRST argument of those kernels.
struct BcsParamBlock {
    BcsChanDev c[DPE_MAX_CHAN];
    // Re-run of a window whose dpe_bcs_set_dev_hint promise broke (the chip kernel's banks are then out of tolerance): the general
    // kernels are ALWAYS enqueued behind a hinted chip-kernel launch with guard = the handle's device status word, and their blocks
    // leave at once unless its bit 3 is set (written by bcs_prep_kernel / chm_k1 for this window).  nullptr: an ordinary launch.
    const int *guard;
};
__device__ __forceinline__ bool rerun_not_wanted(const BcsParamBlock &pb)
{
    return pb.guard != nullptr && (__hip_atomic_load(pb.guard, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 8) == 0;
}

// Block map.  Linear block bx -> (SV k, window w, tile group blk), XCD-aware: workgroups are dealt round-robin to the 8 XCDs
// (block b -> XCD b % 8, observed; used for speed only), so the K blocks that read the SAME samples (one per SV of a tile group)
// get linear ids that are congruent mod 8 and consecutive on that XCD: one HBM fetch, K - 1 hits in the XCD's L2.
// false: a block past the last tile group (the grid is rounded up to whole groups of 8).
__device__ __forceinline__ bool block_map(int bx, int K, int nBlk, int nW, int &k, int &w, int &blk)
{
    const int slot = bx >> 3, tg = (slot / K) * 8 + (bx & 7);
    k = slot % K;
    if (tg >= nBlk * nW) return false;
    w = tg / nBlk;
    blk = tg - w * nBlk;
    return true;
}

// ---- DC mean -----------------------------------------------------------------------------------------------------------------------
// Exact I/Q sums: packed samples (I in the low, Q in the high 16 bits) added to integer sums
__device__ __forceinline__ void iq_add(int &sI, int &sQ, int v)
{
    sI += (short)(v & 0xFFFF);
    sQ += v >> 16;
}
__device__ __forceinline__ void iq_add4(int &sI, int &sQ, const int4 v)
{
    sI += (short)(v.x & 0xFFFF) + (short)(v.y & 0xFFFF) + (short)(v.z & 0xFFFF) + (short)(v.w & 0xFFFF);
    sQ += (v.x >> 16) + (v.y >> 16) + (v.z >> 16) + (v.w >> 16);
}

// DC mean = sum / (float)S in fp64 (batchcorrscores.cu:1065-1066,1210-1216), then fp32.  The <= 64 slots
// are fetched by one vector load (lane <-> slot) and added across the wave: a single memory latency,
// and integer sums are order-independent.  (Its last four lines, the mean from the lanes' sums, stand in ride_window_mean
// too: as a piece of their own they moved the chip2 kernels' pass loops.)
__device__ __forceinline__ void window_mean(const long long *__restrict__ sums, int w, int nSumBlk, int S, float &mRe, float &mIm)
{
    const int lane = threadIdx.x & 63;
    long long tI = 0, tQ = 0;
    if (lane < nSumBlk) {
        const longlong2 v = *reinterpret_cast<const longlong2 *>(sums + ((size_t)w * kSumSlots + lane) * 2);
        tI = v.x; tQ = v.y;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        tI += __shfl_xor(tI, off, 64);
        tQ += __shfl_xor(tQ, off, 64);
    }
    mRe = (float)((double)tI / (double)(float)S);
    mIm = (float)((double)tQ / (double)(float)S);
}

// ---- replica ---------------------------------------------------------------------------------------------------------------------
// Chip table: chips as +/-1.0f, periodically extended: sChips[i] = chip[i mod 1023]
__device__ __forceinline__ void fill_chips(float (&sChips)[2048], const int8_t *__restrict__ chipTable, int prn, int tid)
{
    for (int i = tid; i < 2048; i += 256) sChips[i] = (float)chipTable[(prn - 1) * 1024 + (i >= kLCA ? i - kLCA : i) % kLCA];
}

// Side rule: is a sub-tile or pass whose replica indices are [lo, hi] active on this nav-bit side?  Without a flip everything
// is side 0; one that wraps around the window's ends is built for both sides (its mask decides per entry).
__device__ __forceinline__ bool side_active(const BcsChanDev &ch, int side, int lo, int hi, int S, bool inWindow)
{
    bool active = inWindow;
    if (active) {
        if (!ch.hasFlip) active = (side == 0);
        else if (lo >= 0 && hi < S) active = (side == 0) ? (lo < ch.idxNext) : (hi >= ch.idxNext);
    }
    return active;
}

// Circular replica (the general build): r[m] = chip[floor(t_m fc + rc) mod 1023] (BCS_ComputeCodeReplica :347-349), masked to
// this side of the nav-bit boundary (:352-367), m wrapped circularly.  Entry e <-> m = lo + e.
template <bool TABLE, int NREP>
__device__ __forceinline__ void replica_circular(float *rep, const float *sChips, const BcsChanDev &ch, const double *tT,
                                                 int lo, int side, int S, int lane)
{
    for (int e = lane; e < NREP; e += 64) {
        int m = lo + e;
        if (m < 0) m += S; else if (m >= S) m -= S;
        const int ci = ((int)floor(code_phase<TABLE>(ch, tT, m))) % kLCA;
        const int sd = ch.hasFlip ? (m >= ch.idxNext) : 0;
        rep[e] = (sd == side) ? sChips[ci] : 0.f;
    }
}

// Fast replica (no circular wrap inside [lo, hi], the chip span fits the extended table): the chip index relative to the
// first entry indexes the periodically extended table -- no modulo, no branch; only a straddling tile pays the side mask
template <bool TABLE, int NREP>
__device__ __forceinline__ void replica_fast(float *rep, const float *sChips, const BcsChanDev &ch, const double *tT, int lo, int hi, int side, int lane)
{
    const int ci0 = (int)floor(code_phase<TABLE>(ch, tT, lo));
    const int shift = (ci0 % kLCA) - ci0;
    const bool straddle = ch.hasFlip && lo < ch.idxNext && hi >= ch.idxNext;
    for (int e = lane; e < NREP; e += 64) {
        const int m = lo + e;
        float r = sChips[(int)floor(code_phase<TABLE>(ch, tT, m)) + shift];
        if (straddle) r = ((m >= ch.idxNext) == (side == 1)) ? r : 0.f;
        rep[e] = r;
    }
}

// ---- results ---------------------------------------------------------------------------------------------------------------------
// Moment-set store: the lanes' moment sums of one (tile, side) added across the wave, stored by lane 63
template <int kNMom>
__device__ __forceinline__ void moment_set_reduce_store(float2 *__restrict__ o, const f2 (&M)[kNMom], int lane)
{
    float mm[2 * kNMom];
#pragma unroll
    for (int p = 0; p < kNMom; ++p) { mm[2 * p] = M[p].x; mm[2 * p + 1] = M[p].y; }
    dpp_sum_lane63(mm);
    if (lane == 63) {
#pragma unroll
        for (int p = 0; p < kNMom; ++p) o[p] = make_float2(mm[2 * p], mm[2 * p + 1]);
    }
}
// ... of a tile that may be inactive on this side: it stores zeros
template <int kNMom>
__device__ __forceinline__ void moment_set_store(float2 *__restrict__ o, const f2 (&M)[kNMom], bool active, int lane)
{
    if (active) moment_set_reduce_store<kNMom>(o, M, lane);
    else if (lane < kNMom) o[lane] = make_float2(0.f, 0.f);
}

// Lag partial, the block's step: the four waves' partials added in fixed order into the (block, side) entry of `part`
template <int NL>
__device__ __forceinline__ void lag_partial_block(float2 *__restrict__ o, const float2 (&sAcc)[4][NL], int tid)
{
    for (int j = tid; j < NL; j += 256) {
        float2 s = sAcc[0][j];
        s.x += sAcc[1][j].x; s.y += sAcc[1][j].y;
        s.x += sAcc[2][j].x; s.y += sAcc[2][j].y;
        s.x += sAcc[3][j].x; s.y += sAcc[3][j].y;
        o[j] = s;
    }
}

}  // namespace dpe
