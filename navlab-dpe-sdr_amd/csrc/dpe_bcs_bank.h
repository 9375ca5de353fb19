// dpe_bcs_bank.h -- the per-sample forms of stage 1: bcs_bank_kernel (dense, 4 samples per lane), bcs_bank16_kernel (batches,
// 16 samples per lane) and bcs_bank_wide_kernel (|lag| <= 32 from the replica's boundaries).  Included by dpe_bcs.hip.
// Straight texts over the pieces of dpe_bcs_pieces.h; same partial / moment layouts, so bcs_finalize_kernel is shared.
#pragma once

namespace dpe {

// ------------------------------------------------------------------------------------------
// FUSE (single windows, closed loop): the DC sum rides along instead of running as a kernel of its own.  The mean only
// enters the Doppler moments, and linearly: M_p[(raw - mean) w r] = M_p[raw w r] - mean * M_p[w r].  So this kernel
// accumulates both moment sets and the k = 0 blocks also write the int64 sample sums of their tiles (one slot per
// block); bcs_finalize_kernel forms the mean from the slots and combines.  One launch and ~4 us less per window.
template <int LH, int kNMom, bool TABLE, bool FUSE, bool CO = false>
__global__ __launch_bounds__(256) void bcs_bank_kernel(BcsParamBlock pb, int inl, const int16_t *__restrict__ iq, long long winStride, int S,
                                                       int K, int nSub, int tilesPerBlock, int nBlk, int vecOK, int nSumBlk, int lagShift,
                                                       const BcsChanDev *__restrict__ chan,
                                                       const long long *__restrict__ sums,
                                                       const int8_t *__restrict__ chipTable,
                                                       const double *__restrict__ tT,
                                                       float2 *__restrict__ part, float2 *__restrict__ mom,
                                                       float2 *__restrict__ momRep, long long *__restrict__ sumSlots, ChmKArgs co)
{
    constexpr int NL = 2 * LH + 1;      // lags
    constexpr int NREP = kSub + 2 * LH;  // replica entries per sub-tile (with halo)
    constexpr int NRR = 4 + 2 * LH;      // entries one lane touches
    __shared__ float sChips[2048];   // chips as +/-1.0f, periodically extended: sChips[i] = chip[i mod 1023]
    __shared__ __align__(16) float sRep[4][NREP + 4];
    __shared__ float2 sAcc[4][NL];
    if (rerun_not_wanted(pb)) return;

    // Closed loop on the device (dpe_chm_dev_*): the channel manager's time update for THIS window's scan rides along as block
    // (0, 0, 0) of the launch -- it needs nothing stage 1 produces and stage 1 nothing of it -- beside the correlator blocks
    // instead of 10 us in front of them; the blocks of row x = 0 are then not correlator blocks.
    // (CO: an instantiation of its own -- the time update's registers and code stay out of the kernel every other caller runs)
    int blkX = blockIdx.x;
    if constexpr (CO) {
        static_assert(FUSE && !TABLE, "the co-block rides in the single-window form");
        if (blkX == 0) {
            if (blockIdx.y == 0 && blockIdx.z == 0) chm_k2(co);
            else if (blockIdx.y == 1 && blockIdx.z == 0) chm_k3(co);   // the NEXT time update's Kepler solutions, one window ahead
            return;
        }
        blkX -= 1;
    }
    const int blk = blkX, k = blockIdx.y, w = blockIdx.z;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    (void)pb;
    const BcsChanDev ch = params_ptr(chan, inl)[w * K + k];
    for (int i = tid; i < 2048; i += 256) sChips[i] = (float)chipTable[(ch.prn - 1) * 1024 + (i >= kLCA ? i - kLCA : i) % kLCA];   // restates fill_chips
    const bool fastIdx = (double)NREP * ch.codeStep < 1000.0;   // chip span of one sub-tile fits the extended table
    float mRe = 0.f, mIm = 0.f;
    if (!FUSE) window_mean(sums, w, nSumBlk, S, mRe, mIm);
    int sumI = 0, sumQ = 0;   // FUSE, k == 0: exact sums of this lane's samples (< 64k samples per lane: no overflow)
    __shared__ int sSum[4][2];
    const int16_t *x = iq + (size_t)w * winStride * 2;
    float xp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) xp[i] = (float)(4 * lane + i) - 127.5f;
    __syncthreads();

    for (int side = 0; side < 2; ++side) {
        f2 acc[NL];   // (re, im) pairs: packed fp32 FMAs against the real replica
#pragma unroll
        for (int j = 0; j < NL; ++j) acc[j] = f2{0.f, 0.f};

        for (int t = 0; t < tilesPerBlock; ++t) {
            const int sub = (blk * tilesPerBlock + t) * 4 + wave;
            const int sub0 = sub * kSub;
            // lagShift: this launch produces the lags [lagShift - LH, lagShift + LH] -- the same sums against the
            // replica delayed by lagShift samples, i.e. every replica index below is taken lagShift earlier
            const int lo = sub0 - LH - lagShift, hi = sub0 + kSub - 1 + LH - lagShift;
            bool active = sub < nSub;   // restates side_active
            if (active) {
                if (!ch.hasFlip) active = (side == 0);
                else if (lo >= 0 && hi < S) active = (side == 0) ? (lo < ch.idxNext) : (hi >= ch.idxNext);
            }
            // samples first: the global-load latency is covered by the replica build below
            const int n0 = sub0 + 4 * lane;
            float re[4], im[4];
            const bool countRaw = FUSE && k == 0 && side == 0 && sub < nSub;   // every sample of the window exactly once
            if (active || countRaw) {
                int rawv[4];
                if (vecOK && n0 + 3 < S) {
                    const int4 v = *reinterpret_cast<const int4 *>(x + 2 * (size_t)n0);
                    rawv[0] = v.x; rawv[1] = v.y; rawv[2] = v.z; rawv[3] = v.w;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) rawv[i] = (n0 + i < S) ? *reinterpret_cast<const int *>(x + 2 * (size_t)(n0 + i)) : 0;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    re[i] = (float)(short)(rawv[i] & 0xFFFF);
                    im[i] = (float)(rawv[i] >> 16);
                    if (countRaw) { sumI += (short)(rawv[i] & 0xFFFF); sumQ += rawv[i] >> 16; }   // restates iq_add
                }
            }
            if (active) {
                // replica r[m] = chip[floor(t_m fc + rc) mod 1023] (BCS_ComputeCodeReplica :347-349),
                // masked to this side of the nav-bit boundary (:352-367), m wrapped circularly.
                if (fastIdx && lo >= 0 && hi < S) {   // restates replica_fast
                    // common case (no circular wrap inside the sub-tile): the chip index relative to the
                    // sub-tile's first entry indexes the periodically extended table -- no modulo, no branch
                    const int ci0 = (int)floor(code_phase<TABLE>(ch, tT, lo));
                    const int shift = (ci0 % kLCA) - ci0;
                    const bool straddle = ch.hasFlip && lo < ch.idxNext && hi >= ch.idxNext;
                    for (int e = lane; e < NREP; e += 64) {
                        const int m = lo + e;
                        const int ci = (int)floor(code_phase<TABLE>(ch, tT, m)) + shift;
                        float r = sChips[ci];
                        if (straddle) r = ((m >= ch.idxNext) == (side == 1)) ? r : 0.f;
                        sRep[wave][e] = r;
                    }
                } else {   // restates replica_circular
                    for (int e = lane; e < NREP; e += 64) {
                        int m = lo + e;
                        if (m < 0) m += S; else if (m >= S) m -= S;
                        const double cph = code_phase<TABLE>(ch, tT, m);
                        const int ci = ((int)floor(cph)) % kLCA;
                        const int sd = ch.hasFlip ? (m >= ch.idxNext) : 0;
                        sRep[wave][e] = (sd == side) ? sChips[ci] : 0.f;
                    }
                }
            }
            // no barrier: sRep[wave] is private to this wave and a wave's DS operations complete in order
            f2 M[kNMom], Mq[FUSE ? kNMom : 1];
#pragma unroll
            for (int p = 0; p < kNMom; ++p) M[p] = f2{0.f, 0.f};
#pragma unroll
            for (int p = 0; p < (FUSE ? kNMom : 1); ++p) Mq[p] = f2{0.f, 0.f};
            if (active) {
                // Doppler wipe-off conj(exp(j 2 pi (fi t + ri))) (BCS_ComputeDopplerWipeoff :294-300):
                // fp64 phase seed per lane, hardware sin/cos in revolutions, 3 fp32 rotations.
                double ph = carr_phase<TABLE>(ch, tT, n0 < S ? n0 : S - 1);   // lanes past the window carry zero samples
                ph -= floor(ph);   // restates wipe_seed_at
                const float f = (float)ph;
                f2 wv = wipe_seed(f);
                const f2 meanv = f2{mRe, mIm}, rotv = f2{ch.rotRe, ch.rotIm};
                float rr[NRR];
#pragma unroll
                for (int q = 0; q < NRR / 4; ++q) {
                    const float4 v = *reinterpret_cast<const float4 *>(&sRep[wave][4 * lane + 4 * q]);
                    rr[4 * q] = v.x; rr[4 * q + 1] = v.y; rr[4 * q + 2] = v.z; rr[4 * q + 3] = v.w;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    // rawWiped = raw * wipe (BCS_BatchMultiply :402); complex products through cmul()
                    const f2 wrot = wv;                                       // the rotation chain stays uniform
                    wv = table_fix<TABLE>(wrot, ch, tT, n0, i, S);           // this sample's wipe-off (ns-rounded time table)
                    const f2 bb = cmul(f2{re[i], im[i]}, wv);
                    // sample n, lag l = j-LH uses replica index n-l -> rr[i - j + 2 LH]
#pragma unroll
                    for (int j = 0; j < NL; ++j) {
                        const float r = rr[i + 2 * LH - j];
                        acc[j] = __builtin_elementwise_fma(bb, f2{r, r}, acc[j]);
                    }
                    // carrier path: (raw - mean) * wipe * replica (:480, :440-448)
                    const float r0 = (n0 + i < S) ? rr[i + LH] : 0.f;  // no sample beyond the window
                    if (FUSE) {
                        f2 cp = bb * r0, cq = wv * r0;         // raw w r and w r: the mean is applied in the finalize kernel
#pragma unroll
                        for (int p = 0; p < kNMom; ++p) {
                            M[p] += cp; Mq[p] += cq;
                            cp *= xp[i]; cq *= xp[i];
                        }
                    } else {
                        f2 cp = (bb - cmul(meanv, wv)) * r0;   // x^p * c, built up by one packed multiply per order
#pragma unroll
                        for (int p = 0; p < kNMom; ++p) {
                            M[p] += cp;
                            cp *= xp[i];
                        }
                    }
                    wv = cmul(wrot, rotv);
                }
            }
            if (sub < nSub && lagShift == 0) {   // the Doppler path belongs to the unshifted replica only
                const size_t mo = ((((size_t)w * K + k) * 2 + side) * nSub + sub) * kNMom;
                float2 *o = mom + mo;
                if (active) {   // restates moment_set_store (FUSE: one `if (active)` around both sets)
                    float mm[2 * kNMom];
#pragma unroll
                    for (int p = 0; p < kNMom; ++p) { mm[2 * p] = M[p].x; mm[2 * p + 1] = M[p].y; }
                    dpp_sum_lane63(mm);
                    if (lane == 63) {
#pragma unroll
                        for (int p = 0; p < kNMom; ++p) o[p] = make_float2(mm[2 * p], mm[2 * p + 1]);
                    }
                    if (FUSE) {
#pragma unroll
                        for (int p = 0; p < kNMom; ++p) { mm[2 * p] = Mq[p].x; mm[2 * p + 1] = Mq[p].y; }
                        dpp_sum_lane63(mm);
                        if (lane == 63) {
#pragma unroll
                            for (int p = 0; p < kNMom; ++p) momRep[mo + p] = make_float2(mm[2 * p], mm[2 * p + 1]);
                        }
                    }
                } else if (lane < kNMom) {
                    o[lane] = make_float2(0.f, 0.f);
                    if (FUSE) momRep[mo + lane] = make_float2(0.f, 0.f);
                }
            }
        }
        // block partial of the lag sums, fixed reduction order (restates lag_partial_block; the wave step stands here and in bank16)
        {
            float aa[2 * NL];
#pragma unroll
            for (int j = 0; j < NL; ++j) { aa[2 * j] = acc[j].x; aa[2 * j + 1] = acc[j].y; }
            dpp_sum_lane63(aa);
            if (lane == 63) {
#pragma unroll
                for (int j = 0; j < NL; ++j) sAcc[wave][j] = make_float2(aa[2 * j], aa[2 * j + 1]);
            }
        }
        if (FUSE && k == 0 && side == 0) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                sumI += __shfl_xor(sumI, off, 64);   // per-wave totals stay far below 2^31 (<= 16 tiles x 256 x 32767)
                sumQ += __shfl_xor(sumQ, off, 64);
            }
            if (lane == 0) { sSum[wave][0] = sumI; sSum[wave][1] = sumQ; }
        }
        __syncthreads();
        if (FUSE && k == 0 && side == 0 && tid < 2)
            sumSlots[((size_t)w * kSumSlots + blk) * 2 + tid] =
                (long long)sSum[0][tid] + (long long)sSum[1][tid] + (long long)sSum[2][tid] + (long long)sSum[3][tid];
        for (int j = tid; j < NL; j += 256) {
            float2 s = sAcc[0][j];
            s.x += sAcc[1][j].x; s.y += sAcc[1][j].y;
            s.x += sAcc[2][j].x; s.y += sAcc[2][j].y;
            s.x += sAcc[3][j].x; s.y += sAcc[3][j].y;
            part[((((size_t)w * K + k) * nBlk + blk) * 2 + side) * NL + j] = s;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------
// Batch variant of bcs_bank_kernel for narrow lag windows (LH <= 8): one wave pass covers 1024 consecutive
// samples, each lane 16 of them, so that a DPP row (16 lanes) is exactly one 256-sample moment sub-tile.
// The arithmetic per sample is the dense kernel's; what changes is the amortisation -- index arithmetic,
// carrier-phase seeds (two per lane, so a rotation chain is never longer than 7 steps), side bookkeeping and the
// cross-lane moment sums (4 row-local DPP steps per 4 sub-tiles instead of 6 wave steps per sub-tile) are paid
// once per 16 samples instead of once per 4.  Used when the batch offers enough passes to fill the chip
// (dpe_bcs_update); single windows keep the 4-samples-per-lane kernel, whose blocks are 4x shorter.
// The parts of a pass are marked "---- b16: <name>" below; DESIGN.md 9 prices the config-R pass by these names.  They stay in
// the kernel's text: as functions (forced-inline, or static and left to the inliner) the segment and the shift took scratch in
// the time-table instantiations and moved the registers and loops of the others, the replica build and the block map moved the loops.
// Where replica entry e of a pass lies in the wave's LDS row
#ifdef DPE_B16_PAD   // experiment (round 3, measured and dropped -- DESIGN.md 9): every 16 replica entries take 20 floats -- a lane's float4 window reads then fall on 16 distinct 4-bank slots
__device__ __forceinline__ constexpr int b16_pad(int e) { return e + 4 * (e >> 4); }
#else
__device__ __forceinline__ constexpr int b16_pad(int e) { return e; }
#endif

template <int LH, int kNMom, bool TABLE>
__global__ __launch_bounds__(256, (LH <= 4 && !TABLE) ? kB16Blocks : 3) void bcs_bank16_kernel(BcsParamBlock pb, int inl, const int16_t *__restrict__ iq, long long winStride,
                                                         int S, int K, int nW, int nSub, int tilesPerBlock, int nBlk, int vecOK, int nSumBlk,
                                                         const BcsChanDev *__restrict__ chan,
                                                         const long long *__restrict__ sums,
                                                         const int8_t *__restrict__ chipTable,
                                                         const double *__restrict__ tT,
                                                         float2 *__restrict__ part, float2 *__restrict__ mom)
{
    constexpr int NL = 2 * LH + 1;       // lags
    constexpr int kPass = 1024;          // samples per wave pass
    constexpr int NREP = kPass + 2 * LH;  // replica entries per pass (with halo)
    static_assert((8 + 2 * LH) % 4 == 0 && LH <= 8, "a segment's replica window is read as float4s");
    __shared__ float sChips[2048];   // fill_chips
#ifdef DPE_B16_PAD
    constexpr int kRepLen = ((NREP + 8 + 15) / 16) * 20;
#else
    constexpr int kRepLen = NREP + 8;
#endif
    __shared__ __align__(16) float sRep[4][kRepLen];
    __shared__ float2 sAcc[4][NL];

    // restates block_map
    const int slot = blockIdx.x >> 3, k = slot % K, tg = (slot / K) * 8 + (blockIdx.x & 7);
    if (tg >= nBlk * nW) return;
    const int w = tg / nBlk, blk = tg - w * nBlk;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    (void)pb;
    const BcsChanDev ch = params_ptr(chan, inl)[w * K + k];
    fill_chips(sChips, chipTable, ch.prn, tid);
    const bool fastIdx = (double)NREP * ch.codeStep < 1000.0;   // chip span of one pass fits the extended table
    float mRe, mIm;
    window_mean(sums, w, nSumBlk, S, mRe, mIm);
    const f2 meanv = f2{mRe, mIm}, rotv = f2{ch.rotRe, ch.rotIm};
    const int16_t *x = iq + (size_t)w * winStride * 2;
    const int padLane = b16_pad(lane);
    (void)padLane;
    const float xbase = (float)(16 * (lane & 15)) - 127.5f;      // moment abscissa of the lane's first sample
    __syncthreads();

    for (int side = 0; side < 2; ++side) {
        f2 acc[NL];   // (re, im) pairs: packed fp32 FMAs against the real replica
#pragma unroll
        for (int j = 0; j < NL; ++j) acc[j] = f2{0.f, 0.f};
        bool anyActive = false;   // wave-uniform: most blocks lie entirely on one side of the nav-bit boundary

        for (int t = 0; t < tilesPerBlock; ++t) {
            // ---- b16: bookkeeping and side selection
            const int pass = (blk * tilesPerBlock + t) * 4 + wave;
            const int c0 = pass * kPass;
            const int lo = c0 - LH, hi = c0 + kPass - 1 + LH;
            const bool active = side_active(ch, side, lo, hi, S, c0 < S);
            anyActive |= active;
            const int n0 = c0 + 16 * lane;
            // ---- b16: replica build (restates replica_fast, batched, and replica_circular through the padded index map)
            if (active) {
                // replica r[m] = chip[floor(t_m fc + rc) mod 1023] (BCS_ComputeCodeReplica :347-349), masked to this
                // side of the nav-bit boundary (:352-367), m wrapped circularly -- as in bcs_bank_kernel
                if (fastIdx && lo >= 0 && hi < S) {
                    // (phases are >= 0 here -- rc >= 0, lo >= 0 -- so the truncating conversion IS the floor)
                    const int ci0 = (int)code_phase<TABLE>(ch, tT, lo);
                    const int shift = (ci0 % kLCA) - ci0;
                    const bool straddle = ch.hasFlip && lo < ch.idxNext && hi >= ch.idxNext;
                    if (!straddle) {   // (two loops: the side mask of the one straddling pass costs 3 of 17 slots per entry)
                        // batches of eight independent entries: the fp64 phase -> table read -> store chains overlap
                        // instead of running one after the other (the loop is latency, not issue)
                        static_assert(NREP >= 1024 && NREP < 1024 + 64, "sixteen full rounds of 64 entries and a partial one");
                        if constexpr (TABLE) {   // (the time-table form reads its sample times from memory: keep the short live range)
                            for (int e = lane; e < NREP; e += 64) sRep[wave][b16_pad(e)] = sChips[(int)code_phase<TABLE>(ch, tT, lo + e) + shift];
                        } else {
#pragma unroll
                        for (int e0 = 0; e0 < 1024; e0 += 512) {
                            float v[8];
#pragma unroll
                            for (int j = 0; j < 8; ++j) v[j] = sChips[(int)code_phase<TABLE>(ch, tT, lo + e0 + 64 * j + lane) + shift];
#pragma unroll
                            for (int j = 0; j < 8; ++j) sRep[wave][b16_pad(e0 + 64 * j) + padLane] = v[j];
                        }
                        if (1024 + lane < NREP) sRep[wave][b16_pad(1024) + padLane] = sChips[(int)code_phase<TABLE>(ch, tT, lo + 1024 + lane) + shift];
                        }
                    } else {
                        for (int e = lane; e < NREP; e += 64) {
                            const int m = lo + e;
                            const float r = sChips[(int)code_phase<TABLE>(ch, tT, m) + shift];
                            sRep[wave][b16_pad(e)] = ((m >= ch.idxNext) == (side == 1)) ? r : 0.f;
                        }
                    }
                } else {
                    for (int e = lane; e < NREP; e += 64) {
                        int m = lo + e;
                        if (m < 0) m += S; else if (m >= S) m -= S;
                        const double cph = code_phase<TABLE>(ch, tT, m);
                        const int ci = ((int)floor(cph)) % kLCA;
                        const int sd = ch.hasFlip ? (m >= ch.idxNext) : 0;
                        sRep[wave][b16_pad(e)] = (sd == side) ? sChips[ci] : 0.f;
                    }
                }
            }
            // no barrier: sRep[wave] is private to this wave and a wave's DS operations complete in order
            f2 M[kNMom];
#pragma unroll
            for (int p = 0; p < kNMom; ++p) M[p] = f2{0.f, 0.f};
            // two segments of 8 samples, deliberately NOT unrolled: the live set stays at one segment's samples and replica
            // window (occupancy), and each segment re-seeds the carrier phase.  allIn: the whole pass lies inside the window
            // (every pass but the window's last) -- no per-sample bound on the carrier path
            auto segments = [&](auto allInTag) {
                constexpr bool kAllIn = decltype(allInTag)::value;
#pragma unroll 1
                for (int seg = 0; seg < 2; ++seg) {
                    // ---- b16: segment (restates wipe_seed_at)
                    const int ns = n0 + 8 * seg;
                    int raw[8];   // packed I/Q
                    // (fetching a segment ahead -- under the replica build / the previous segment -- measured 5 % slower: the
                    // eight extra live registers cost more than the exposed load latency, which the other waves cover)
                    if (vecOK && (kAllIn || ns + 7 < S)) {
#pragma unroll
                        for (int q = 0; q < 2; ++q) {
                            const int4 v = *reinterpret_cast<const int4 *>(x + 2 * (size_t)(ns + 4 * q));
                            raw[4 * q] = v.x; raw[4 * q + 1] = v.y; raw[4 * q + 2] = v.z; raw[4 * q + 3] = v.w;
                        }
                    } else {
#pragma unroll
                        for (int i = 0; i < 8; ++i) raw[i] = (ns + i < S) ? *reinterpret_cast<const int *>(x + 2 * (size_t)(ns + i)) : 0;
                    }
                    float rr[8 + 2 * LH];
#pragma unroll
                    for (int q = 0; q < (8 + 2 * LH) / 4; ++q) {
                        const float4 v = *reinterpret_cast<const float4 *>(&sRep[wave][b16_pad(16 * lane + 8 * seg + 4 * q)]);
                        rr[4 * q] = v.x; rr[4 * q + 1] = v.y; rr[4 * q + 2] = v.z; rr[4 * q + 3] = v.w;
                    }
                    // Doppler wipe-off conj(exp(j 2 pi (fi t + ri))) (BCS_ComputeDopplerWipeoff :294-300): fp64 phase
                    // seed, hardware sin/cos in revolutions, then 7 fp32 rotations -- complex products through cmul()
                    double ph = carr_phase<TABLE>(ch, tT, (kAllIn || ns < S) ? ns : S - 1);   // lanes past the window carry zero samples
                    ph -= floor(ph);
                    f2 wv = wipe_seed((float)ph);
                    const bool inside = kAllIn || ns + 7 < S;   // false only for lanes of the window's last pass
                    // moments of the segment about ITS centre (the powers of i - 3.5 are literals: one packed FMA per order
                    // and sample), moved to the sub-tile's abscissa once per segment
                    f2 m[kNMom];
#pragma unroll
                    for (int p = 0; p < kNMom; ++p) m[p] = f2{0.f, 0.f};
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const f2 rawv = f2{(float)(short)(raw[i] & 0xFFFF), (float)(raw[i] >> 16)};
                        const f2 wrot = wv;                                // the rotation chain stays uniform
                        wv = table_fix<TABLE>(wrot, ch, tT, ns, i, S);    // this sample's wipe-off (ns-rounded time table)
                        const f2 bb = cmul(rawv, wv);                      // rawWiped = raw * wipe (BCS_BatchMultiply :402)
                        // sample n, lag l = j-LH uses replica index n-l -> rr[i - j + 2 LH]
#pragma unroll
                        for (int j = 0; j < NL; ++j) {
                            const float r = rr[i + 2 * LH - j];
                            acc[j] = __builtin_elementwise_fma(bb, f2{r, r}, acc[j]);
                        }
                        // carrier path: (raw - mean) * wipe * replica (:480, :440-448)
                        const float r0 = (inside || ns + i < S) ? rr[i + LH] : 0.f;  // no sample beyond the window
                        const f2 cp = (bb - cmul(meanv, wv)) * r0;
                        const float d = (float)i - 3.5f;
                        float dp = 1.f;
                        m[0] += cp;
#pragma unroll
                        for (int p = 1; p < kNMom; ++p) {
                            dp *= d;   // folded at compile time
                            m[p] = __builtin_elementwise_fma(cp, f2{dp, dp}, m[p]);
                        }
                        wv = cmul(wrot, rotv);
                    }
                    // ---- b16: the moments' shift to the sub-tile abscissa
                    // (x + d)^p = sum_q C(p,q) x^(p-q) d^q, x = the segment centre in sub-tile coordinates
                    const float xc = xbase + (float)(8 * seg) + 3.5f;
                    float xpow[kNMom];
                    xpow[0] = 1.f;
#pragma unroll
                    for (int e = 1; e < kNMom; ++e) xpow[e] = xpow[e - 1] * xc;
                    constexpr float bin[6][6] = {{1, 0, 0, 0, 0, 0}, {1, 1, 0, 0, 0, 0}, {1, 2, 1, 0, 0, 0}, {1, 3, 3, 1, 0, 0}, {1, 4, 6, 4, 1, 0}, {1, 5, 10, 10, 5, 1}};
#pragma unroll
                    for (int p = 0; p < kNMom; ++p) {
                        M[p] += m[p];
#pragma unroll
                        for (int q = 0; q < p; ++q) {
                            const float cf = bin[p][q] * xpow[p - q];
                            M[p] = __builtin_elementwise_fma(m[q], f2{cf, cf}, M[p]);
                        }
                    }
                }
            };
            if (active) {
                if (c0 + kPass <= S) segments(std::true_type{});
                else segments(std::false_type{});
            }
            {
                // ---- b16: moment reduction and store
                // one moment set per DPP row = per 256-sample sub-tile (restates moment_set_store, row-wise)
                const int sub = pass * 4 + (lane >> 4);
                float2 *o = mom + ((((size_t)w * K + k) * 2 + side) * nSub + sub) * kNMom;
                if (active) {
                    float mm[2 * kNMom];
#pragma unroll
                    for (int p = 0; p < kNMom; ++p) { mm[2 * p] = M[p].x; mm[2 * p + 1] = M[p].y; }
                    dpp_sum_rows(mm);
                    if (sub < nSub && (lane & 15) == 15) {
#pragma unroll
                        for (int p = 0; p < kNMom; ++p) o[p] = make_float2(mm[2 * p], mm[2 * p + 1]);
                    }
                } else if (sub < nSub && (lane & 15) < kNMom) {
                    o[lane & 15] = make_float2(0.f, 0.f);
                }
            }
        }
        // block partial of the lag sums, fixed reduction order (a wave without a pass on this side contributes zeros)
        if (anyActive) {
            float aa[2 * NL];
#pragma unroll
            for (int j = 0; j < NL; ++j) { aa[2 * j] = acc[j].x; aa[2 * j + 1] = acc[j].y; }
            dpp_sum_lane63(aa);
            if (lane == 63) {
#pragma unroll
                for (int j = 0; j < NL; ++j) sAcc[wave][j] = make_float2(aa[2 * j], aa[2 * j + 1]);
            }
        } else if (lane < NL) {
            sAcc[wave][lane] = make_float2(0.f, 0.f);
        }
        __syncthreads();
        lag_partial_block<NL>(part + ((((size_t)w * K + k) * nBlk + blk) * 2 + side) * NL, sAcc, tid);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------
// Wide lag windows (|lag| <= 32, i.e. high sampling rates where a chip spans many samples): instead of
// 65 dense multiply-accumulates per sample, use that the replica is piecewise constant:
//     corr[l+1] - corr[l] = sum_m J[m] b[(m + l) mod S],   J[m] = r[m-1] - r[m]
// is a sum over the chip (and nav-bit / mask) boundaries only.  Per sub-tile: one direct lag (l = -32,
// one FMA pair per sample) plus, for each of the ~codeStep*128 boundaries of the tile, one LDS read and
// one FMA per LANE with lanes <-> the 64 lag steps.  The finalize kernel prefix-sums the steps.
// part layout per (block, side): [0] = corr[-32], [1 + i] = D[-32 + i], i = 0..63  (65 entries, as NL).
template <int kNMom, bool TABLE>
__global__ __launch_bounds__(256) void bcs_bank_wide_kernel(BcsParamBlock pb, int inl, const int16_t *__restrict__ iq, long long winStride, int S,
                                                            int K, int nSub, int tilesPerBlock, int nBlk, int vecOK, int nSumBlk, int lagShift,
                                                            const BcsChanDev *__restrict__ chan,
                                                            const long long *__restrict__ sums,
                                                            const int8_t *__restrict__ chipTable,
                                                            const double *__restrict__ tT,
                                                            float2 *__restrict__ part, float2 *__restrict__ mom)
{
    constexpr int LH = 32, NL = 2 * LH + 1;
    constexpr int NREP = kSub + LH + 1;   // replica entries: m = sub0-1 .. sub0+255+LH
    constexpr int NB = kSub + 2 * LH;     // wiped samples:   n = sub0-LH .. sub0+255+LH
    __shared__ float sChips[2048];   // fill_chips
    __shared__ float sRep[4][NREP + 3];
    __shared__ float2 sB[4][NB];
    __shared__ float2 sAcc[4][NL];
    if (rerun_not_wanted(pb)) return;

    const int blk = blockIdx.x, k = blockIdx.y, w = blockIdx.z;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    (void)pb;
    const BcsChanDev ch = params_ptr(chan, inl)[w * K + k];
    fill_chips(sChips, chipTable, ch.prn, tid);
    const bool fastIdx = (double)NREP * ch.codeStep < 1000.0;
    float mRe, mIm;
    window_mean(sums, w, nSumBlk, S, mRe, mIm);
    const int16_t *x = iq + (size_t)w * winStride * 2;
    float xp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) xp[i] = (float)(4 * lane + i) - 127.5f;
    __syncthreads();

    for (int side = 0; side < 2; ++side) {
        f2 acc0 = f2{0.f, 0.f};   // direct sum at lag -LH (per-lane partial)
        f2 D = f2{0.f, 0.f};      // this lane's lag step  l = lane - LH
        for (int t = 0; t < tilesPerBlock; ++t) {
            const int sub = (blk * tilesPerBlock + t) * 4 + wave;
            const int sub0 = sub * kSub;
            const int lo = sub0 - 1 - lagShift, hi = sub0 + kSub - 1 + LH - lagShift;   // replica index range (see lagShift in bcs_bank_kernel)
            const bool active = side_active(ch, side, lo, hi, S, sub < nSub);
            f2 M[kNMom];
#pragma unroll
            for (int p = 0; p < kNMom; ++p) M[p] = f2{0.f, 0.f};
            if (active) {
                // ---- masked replica, entries e <-> m = lo + e (circular)
                if (fastIdx && lo >= 0 && hi < S) replica_fast<TABLE, NREP>(sRep[wave], sChips, ch, tT, lo, hi, side, lane);
                else replica_circular<TABLE, NREP>(sRep[wave], sChips, ch, tT, lo, side, S, lane);
                // ---- wiped samples b[n] (circular), own 4 + one halo sample per lane -> LDS
                const int n0 = sub0 + 4 * lane;
                float re[4], im[4];
                if (vecOK && n0 + 3 < S) {
                    const int4 v = *reinterpret_cast<const int4 *>(x + 2 * (size_t)n0);
                    re[0] = (float)(short)(v.x & 0xFFFF); im[0] = (float)(v.x >> 16);
                    re[1] = (float)(short)(v.y & 0xFFFF); im[1] = (float)(v.y >> 16);
                    re[2] = (float)(short)(v.z & 0xFFFF); im[2] = (float)(v.z >> 16);
                    re[3] = (float)(short)(v.w & 0xFFFF); im[3] = (float)(v.w >> 16);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        int nn = n0 + i;
                        if (nn >= S) nn -= S;   // beyond the window: the circular continuation (masked below where it is not a sample)
                        const int v = *reinterpret_cast<const int *>(x + 2 * (size_t)nn);
                        re[i] = (float)(short)(v & 0xFFFF);
                        im[i] = (float)(v >> 16);
                    }
                }
                f2 bown[4], wown[4];
                {
                    int nn = n0 >= S ? n0 - S : n0;
                    f2 wv = wipe_seed_at(carr_phase<TABLE>(ch, tT, nn));
                    const f2 rotv = f2{ch.rotRe, ch.rotIm};
                    int seedIdx = nn, steps = 0;                               // the chain's seed sample and the rotations since
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (n0 + i == S) {   // phase restarts where the circular continuation begins
                            wv = wipe_seed_at(ch.ri);
                            seedIdx = 0; steps = 0;
                        }
                        const f2 wrot = wv;                                   // the rotation chain stays uniform
                        wv = table_fix<TABLE>(wrot, ch, tT, seedIdx, steps, S);   // this sample's wipe-off (ns-rounded time table)
                        ++steps;
                        wown[i] = wv;
                        bown[i] = cmul(f2{re[i], im[i]}, wv);
                        sB[wave][LH + 4 * lane + i] = make_float2(bown[i].x, bown[i].y);
                        wv = cmul(wrot, rotv);
                    }
                }
                {   // halo: lanes 0..31 -> n = sub0-LH+lane ; lanes 32..63 -> n = sub0+256+(lane-32)
                    int nh = (lane < LH) ? (sub0 - LH + lane) : (sub0 + kSub + lane - LH);
                    const int e = (lane < LH) ? lane : (kSub + lane);
                    if (nh < 0) nh += S; else if (nh >= S) nh -= S;
                    const int v = *reinterpret_cast<const int *>(x + 2 * (size_t)nh);
                    const float hr = (float)(short)(v & 0xFFFF), hi2 = (float)(v >> 16);
                    double ph = carr_phase<TABLE>(ch, tT, nh);
                    ph -= floor(ph);   // restates wipe_seed_at (consumed by plain C++: no s_nop)
                    const float f = (float)ph;
                    const float wr = __builtin_amdgcn_cosf(f), wi = -__builtin_amdgcn_sinf(f);
                    sB[wave][e] = make_float2(hr * wr - hi2 * wi, hr * wi + hi2 * wr);
                }
                // ---- own samples: direct lag -LH, carrier moments (only real samples n < S)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const bool real = n0 + i < S;
                    const float rl = real ? sRep[wave][4 * lane + i + 1 + LH] : 0.f;   // r[n + LH]
                    acc0 = __builtin_elementwise_fma(bown[i], f2{rl, rl}, acc0);
                    const float r0 = real ? sRep[wave][4 * lane + i + 1] : 0.f;        // r[n]
                    f2 cp = (bown[i] - cmul(f2{mRe, mIm}, wown[i])) * r0;
#pragma unroll
                    for (int p = 0; p < kNMom; ++p) {
                        M[p] += cp;
                        cp *= xp[i];
                    }
                }
                // ---- boundaries m = sub0 + 4*lane + i (only m < S exist): J = r[m-1] - r[m]
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int e = 4 * lane + i;   // rep[e] = r[m-1], rep[e+1] = r[m]
                    const float J = (sub0 + e < S) ? (sRep[wave][e] - sRep[wave][e + 1]) : 0.f;
                    unsigned long long mask = __ballot(J != 0.f);
                    while (mask) {
                        const int src = __builtin_ctzll(mask);
                        mask &= mask - 1;
                        const float Jv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, J), src));
                        // b index for lag l = lane - LH:  n = m + l  ->  entry (m - sub0 + LH) + (lane - LH)
                        const float2 bv = sB[wave][4 * src + i + lane];
                        D = __builtin_elementwise_fma(f2{bv.x, bv.y}, f2{Jv, Jv}, D);
                    }
                }
            }
            if (sub < nSub && lagShift == 0)
                moment_set_store<kNMom>(mom + ((((size_t)w * K + k) * 2 + side) * nSub + sub) * kNMom, M, active, lane);
        }
        {
            float aa[3] = {acc0.x, acc0.y, 0.f};
            dpp_sum_lane63(aa);
            if (lane == 63) sAcc[wave][0] = make_float2(aa[0], aa[1]);
            sAcc[wave][1 + lane] = make_float2(D.x, D.y);
        }
        __syncthreads();
        lag_partial_block<NL>(part + ((((size_t)w * K + k) * nBlk + blk) * 2 + side) * NL, sAcc, tid);
        __syncthreads();
    }
}

}  // namespace dpe
