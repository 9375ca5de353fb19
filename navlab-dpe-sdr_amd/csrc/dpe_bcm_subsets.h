// dpe_bcm_subsets.h -- the manifold scan that also yields the arg-max of every SV subset of a window (dpe_bcm_create_subsets),
// included by dpe_bcm.hip after scan_body.
//
// One receiver, K SVs, M subsets per window; subset m is a 64-bit mask over the window's channels.  The per-(point, SV) term
// does not depend on which other SVs are summed with it, so one evaluation serves the full set and every subset: the full
// score is summed exactly as scan_body sums it (SV order, starting from 0), and subset m's score is the sum, in the same order
// and from 0, of the terms whose bit is set in its mask -- the bits dpe_bcm_update gives when it is handed only those channels
// (solution separation: fix with every SV, fix again with each SV left out, compare; leave-one-out is M = K masks).  An excluded
// SV's term is never touched (the add is skipped under a wave-uniform branch), so a NaN of an excluded SV stays out of the sum.
//
// The kernel is scan_body's (both manifolds in one launch, the tile walk, the LDS entries, the index math, the clamp variants, the
// ragged tile, the fused key, scan_publish), written from the same pieces (dpe_bcm_pieces.h) except the
// index and the term of a pair, which stand in the SV loop as text (see there).  What is new:
//  * the masks come from a device array [W][maxSubsets] through wave-uniform (scalar) loads while the banks are staged, and are
//    kept in LDS transposed: one word per SV whose bit m says "subset m holds this SV".  The SV loop broadcasts that word once
//    per SV (16 masks held in SGPRs for the whole tile walk would spill), and tests its bits at constant positions;
//  * per subset a packed-pair accumulator per tile and a running (score, position); only the full row is written, a subset
//    leaves one packed key per manifold;
//  * out-of-window pairs are counted PER SV (LDS atomics in the slow branch); a subset's count is the sum of its SVs' counts,
//    formed on the host, the full set's count the sum of all of them.
// The subset loop is unrolled to kSubsetMax with wave-uniform tests (the membership bit, the subset count), so the accumulators and running maxima are indexed by
// constants and stay in registers (a runtime index would send them to scratch).  SUBS = false drops all of it: the plain scan.
#pragma once

namespace dpe {

constexpr int kSubsetMax = 16;     // subsets per scan

template <int LP, bool SECOND, bool CLAMP, bool SUBS>
__device__ __forceinline__ void subsets_body(const ScanSide &sd, int K, int maxK, int lpower, const unsigned long long *__restrict__ masks, int nSubsets,
                                             int maxSubsets, unsigned long long *__restrict__ keys, unsigned long long *__restrict__ oob,
                                             unsigned long long *__restrict__ subKeys, unsigned long long *__restrict__ svOob, int keySlot)
{
    const f4 *__restrict__ grid = reinterpret_cast<const f4 *>(sd.grid);
    float *__restrict__ scores = sd.scores;
    const long long G = sd.G, indexOffset = sd.indexOffset;
    const int nEnt = sd.nEnt;
    const unsigned nBlkX = (unsigned)sd.split;
    extern __shared__ __align__(16) unsigned char smem[];
    float4 *sE = reinterpret_cast<float4 *>(smem);                           // [K][nEnt] entries {A, B, 0, C} (scan_fill_bank)
    __shared__ unsigned long long sKey[4];
    __shared__ unsigned long long sSubKey[4][kSubsetMax];
    __shared__ unsigned int sSvOob[DPE_MAX_CHAN];
    __shared__ unsigned int sMember[DPE_MAX_CHAN];                           // per SV: bit m = subset m holds it

    const int w = blockIdx.y, tid = threadIdx.x;
    const unsigned nFull = (unsigned)(G / kPtsPerBlock);
    const unsigned nTiles = (unsigned)((G + kPtsPerBlock - 1) / kPtsPerBlock);
    f4 bufA[2 * kPairs], bufB[2 * kPairs];
    const auto load = [&](f4 (&g)[2 * kPairs], unsigned tile) { scan_load_tile(g, grid, tile, tid); };
    if (blockIdx.x < nTiles) load(bufA, blockIdx.x);
    scan_fill_bank(sE, sd.bank + (size_t)w * maxK * nEnt, K * nEnt, nEnt, tid);
    if (CLAMP && tid < K) sSvOob[tid] = 0u;
    if (SUBS && tid < K) {
        const unsigned long long *__restrict__ mw = masks + (size_t)w * maxSubsets;   // wave-uniform -> scalar loads
        unsigned int member = 0u;
        for (int m = 0; m < nSubsets; ++m) member |= (unsigned int)((mw[m] >> tid) & 1ull) << m;
        sMember[tid] = member;
    }
    __syncthreads();

    const unsigned last = (unsigned)(nEnt - 1);
    const BcmSvDev *__restrict__ svw = sd.sv + (size_t)w * maxK;             // wave-uniform -> scalar loads
    // The unrolled subset loops test each subset against the count on its own, where it stands, and close the test before the
    // next subset: a chain of exits makes the compiler carry every subset's compare masks to one common exit, and left to itself
    // it hoists all 16 comparisons out of the tile walk as 64-bit lane masks -- either way the SGPRs spill
    const auto subset_count = [&]() -> int {
        int n = nSubsets;
        asm volatile("" : "+s"(n));
        return n;
    };
    float bestSc = -1.f;          // scores are >= 0
    unsigned int bestTile = 0u, bestIt = 0u;
    // per subset: the running maximum of its score as (score, tile * kPtsPerThread + it)
    float subSc[kSubsetMax];
    unsigned int subAt[kSubsetMax];
#pragma unroll
    for (int m = 0; m < kSubsetMax; ++m) { subSc[m] = -1.f; subAt[m] = 0u; }

    const auto tile_body = [&](const f4 (&g)[2 * kPairs], unsigned tile, auto raggedTag) {
        constexpr bool RAGGED = decltype(raggedTag)::value;
        const long long base = (long long)tile * kPtsPerBlock + tid;   // (ragged tile only)
        ScanPts pt;
        scan_unpack(pt, g);
        f2 score[kPairs];
        f2 sub[kSubsetMax][kPairs];
#pragma unroll
        for (int p = 0; p < kPairs; ++p) score[p] = f2{0.f, 0.f};
#pragma unroll
        for (int m = 0; m < kSubsetMax; ++m) {
#pragma unroll
            for (int p = 0; p < kPairs; ++p) sub[m][p] = f2{0.f, 0.f};
        }
        unsigned emax = 0;
#pragma unroll DPE_SV_UNROLL
        for (int k = 0; k < K; ++k) {
            const BcmSvDev s = svw[k];
            const float4 *bk = sE + k * nEnt;
            f2 term[kPairs];
#pragma unroll
            for (int p = 0; p < kPairs; ++p) {
                // scan_pair_term's text, kept here: through the call this body's kernels take 1 to 3 more VGPRs
                f2 idx;
                if (SECOND) {
                    f2 a = pt.dx[p] * s.ue;
                    a = __builtin_elementwise_fma(pt.dy[p], f2{s.un, s.un}, a);
                    a = __builtin_elementwise_fma(pt.dz[p], f2{s.uu, s.uu}, a);
                    f2 x = pt.dw[p] - a;
                    const f2 t = __builtin_elementwise_fma(-a, a, pt.q[p]);          // q - a^2
                    x = __builtin_elementwise_fma(t, f2{s.h, s.h}, x);               // + (q - a^2) / (2 range)
                    idx = __builtin_elementwise_fma(x, f2{s.g, s.g}, f2{s.idx0, s.idx0});
                } else {
                    idx = __builtin_elementwise_fma(pt.dw[p], f2{s.g, s.g}, f2{s.idx0, s.idx0});
                    idx = __builtin_elementwise_fma(pt.dx[p], f2{-s.h, -s.h}, idx);
                    idx = __builtin_elementwise_fma(pt.dy[p], f2{-s.pad0, -s.pad0}, idx);
                    idx = __builtin_elementwise_fma(pt.dz[p], f2{-s.pad1, -s.pad1}, idx);
                }
                float c[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const float id = idx[j];
                    const float wgt = __builtin_amdgcn_fractf(id);                 // id - floor(id)
                    int ei;
                    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(ei) : "v"(id));          // (int)floor(id), saturating
                    unsigned e = (unsigned)ei;
                    if (CLAMP) {                                                   // negative -> huge -> zero slot
                        e = min(e, last);
                        emax = max(emax, e);
                    }
                    const float2 ab = *reinterpret_cast<const float2 *>(&bk[e]);
                    const float m2 = fmaf(wgt, fmaf(wgt, bk[e].w, ab.y), ab.x);
                    if (LP == 1) c[j] = __builtin_amdgcn_sqrtf(__builtin_fabsf(m2));    // raw v_sqrt_f32 (1 ulp)
                    else if (LP == 2) c[j] = m2;
                    else c[j] = powf(__builtin_amdgcn_sqrtf(__builtin_fabsf(m2)), (float)lpower);
                }
                term[p] = f2{c[0], c[1]};
                score[p] += term[p];
            }
            if (SUBS) {   // the same term into every subset that holds SV k: the mask bit is wave-uniform, the add is skipped, never zeroed
                const unsigned int member = __builtin_amdgcn_readfirstlane(sMember[k]);
#pragma unroll
                for (int m = 0; m < kSubsetMax; ++m) {      // (bits at and above nSubsets are 0)
                    if (member & (1u << m)) {
#pragma unroll
                        for (int p = 0; p < kPairs; ++p) sub[m][p] += term[p];
                    }
                }
            }
        }
        // out-of-window bookkeeping off the fast path, per SV: recount only if this thread ever hit the zero slot
        if (CLAMP && emax == last) scan_recount<SECOND, RAGGED>(pt, svw, K, last, base, G, [&](int k, unsigned n) DPE_INLINE_LAMBDA { if (n) atomicAdd(&sSvOob[k], 1u); });
        if (scores) scan_store_row<RAGGED>(scores + (size_t)w * sd.pitch + (size_t)tile * kPtsPerBlock, score, base, G, tid);
        scan_track_max<RAGGED>(score, base, G, tile, bestSc, bestTile, bestIt);
        if (SUBS) {
#pragma unroll
            for (int m = 0; m < kSubsetMax; ++m) {
                if (m < subset_count())
                    scan_track_max<RAGGED>(sub[m], base, G, tile, subSc[m], subAt[m]);
            }
        }
    };
    unsigned tile = blockIdx.x;
    scan_walk_tiles(tile, nBlkX, nFull, nTiles, bufA, bufB, load, tile_body);

    const unsigned int io = (unsigned int)indexOffset;
    const unsigned long long best = wave_max_key(pack_key(bestSc, io + scan_local_index(bestTile, bestIt, tid)));
    if ((tid & 63) == 0) sKey[tid >> 6] = best;
    if (SUBS) {
#pragma unroll
        for (int m = 0; m < kSubsetMax; ++m) {
            if (m < subset_count()) {
                const unsigned long long b =
                    wave_max_key(pack_key(subSc[m], io + scan_local_index(subAt[m] / (unsigned)kPtsPerThread, subAt[m] % (unsigned)kPtsPerThread, tid)));
                if ((tid & 63) == 0) sSubKey[tid >> 6][m] = b;
            }
        }
    }
    __syncthreads();
    // per-subset keys and per-SV counts: read by the host after the launch has finished, so no ordering against the ticket
    if (SUBS && tid < nSubsets) atomicMax(&subKeys[((size_t)w * 2 + keySlot) * maxSubsets + tid], block_max_key(&sSubKey[0][tid], kSubsetMax));
    if (CLAMP && tid < K) {
        const unsigned int n = sSvOob[tid];
        if (n) atomicAdd(&svOob[((size_t)w * 2 + keySlot) * maxK + tid], (unsigned long long)n);
    }
    if (tid == 0) {
        unsigned int n = 0;     // the full set's count: the sum over SVs
        if (CLAMP)
            for (int k = 0; k < K; ++k) n += sSvOob[k];
        scan_post_key(&keys[(size_t)w * 2 + keySlot], &oob[(size_t)w * 2 + keySlot], block_max_key(sKey), n);
    }
}

// Both manifolds in one launch, as bcm_scan_kernel: blockIdx.z = 0 position, 1 velocity; clears the next Update's key set and
// lets the last block publish the full set's keys and counts into the pinned host mirror.
template <int LP, bool CLAMP_P, bool CLAMP_V, bool SUBS>
__global__ __launch_bounds__(256) void bcm_scan_subsets_kernel(ScanSide sp, ScanSide sv, int K, int maxK, int lpower,
                                                               const unsigned long long *__restrict__ masks, int nSubsets, int maxSubsets,
                                                               unsigned long long *__restrict__ keys, unsigned long long *__restrict__ oob,
                                                               unsigned long long *__restrict__ subKeys, unsigned long long *__restrict__ svOob,
                                                               unsigned long long *__restrict__ clearPtr, int clearN,
                                                               unsigned int *__restrict__ done, unsigned long long *__restrict__ hostKeys,
                                                               unsigned long long *__restrict__ hostOob, unsigned long long seqValue)
{
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0)
        for (int i = threadIdx.x; i < clearN; i += 256) clearPtr[i] = 0ull;
    if (blockIdx.z == 0) {
        if (blockIdx.x < (unsigned)sp.split)
            subsets_body<LP, true, CLAMP_P, SUBS>(sp, K, maxK, lpower, masks, nSubsets, maxSubsets, keys, oob, subKeys, svOob, 0);
    } else {
        if (blockIdx.x < (unsigned)sv.split)
            subsets_body<LP, false, CLAMP_V, SUBS>(sv, K, maxK, lpower, masks, nSubsets, maxSubsets, keys, oob, subKeys, svOob, 1);
    }
    scan_publish(keys, oob, done, hostKeys, hostOob, seqValue);
}

}  // namespace dpe
