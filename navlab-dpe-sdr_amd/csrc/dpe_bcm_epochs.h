// dpe_bcm_epochs.h -- the manifold scan of N consecutive windows (epochs) summed into one score row and one arg-max
// (dpe_bcm_create_epochs), included by dpe_bcm.hip after scan_body.
//
// A group is nEpochs consecutive windows of one receiver along its predicted trajectory; grid point j means "the whole
// trajectory moved by offset j".  The group's score of a point is the sum over its windows of the score scan_body gives that
// window there (non-coherent accumulation over epochs); its first maximum is the group's ML offset.  Every window brings its
// own centre, ENU->ECEF matrix, receive time, channel ends and bank rows, laid out as dpe_bcm_update takes them, so the
// (window, SV) coefficients and banks of group g are rows (g nEpochs + e) maxK + k of the arrays of a plain batch.
//
// The kernel is scan_body's (both manifolds in one launch, the tile walk, the LDS entries, the index math, the clamp variants, the
// ragged tile, the fused key).  The tile load, the tile walk, the bank fill, the key and the reductions are the shared pieces
// (dpe_bcm_pieces.h); the tile body stands here as text, scan_body's operation for operation: written from
// the pieces its tile loop waits for each of the four running-score loads on its own.  What is new:
//  * the per-(window, SV) coefficients come from the device array through wave-uniform (scalar) loads, so the number of pairs
//    is bounded by the LDS alone;
//  * PASSES: the group's windows are cut into runs of winPerPass whole windows whose banks fit the LDS together.  A block fills
//    the LDS with a pass's banks, walks ITS tiles, refills, walks the same tiles again, ...  Tile t of block x is x + t split in
//    every pass and point (tile, it, lane) belongs to the same lane every time, so the running score of a point is read back
//    from the group's fp32 score row by the lane that stored it, in program order: the row is the accumulator and nothing is
//    ordered across blocks.  The first pass stores, later passes load, add and store, the last one also forms the key;
//  * a window's own score is summed exactly as scan_body sums it (same SV order, starting from 0) and then added to the running
//    score in window order.  An fp32 value survives the round trip through the row unchanged, so a group's bits do not depend on
//    where its windows are cut into passes, and a group of one window carries the bits of the single-window scan.
#pragma once

namespace dpe {

template <int LP, bool SECOND, bool CLAMP>
__device__ __forceinline__ void epochs_body(const ScanSide &sd, int nEpochs, int winPerPass, int K, int maxK, int lpower,
                                            unsigned long long *__restrict__ keys, unsigned long long *__restrict__ oob, int keySlot)
{
    const f4 *__restrict__ grid = reinterpret_cast<const f4 *>(sd.grid);
    float *scores = sd.scores;                                               // (read back: no __restrict__, no non-temporal hint until the last pass)
    const long long G = sd.G;
    const int nEnt = sd.nEnt;
    const unsigned nBlkX = (unsigned)sd.split;
    extern __shared__ __align__(16) unsigned char smem[];
    float4 *sE = reinterpret_cast<float4 *>(smem);                           // [windows of the pass][K][nEnt] entries {A, B, 0, C} (see scan_body)
    __shared__ unsigned long long sKey[4];
    __shared__ unsigned int sOob[4];

    const int grp = blockIdx.y, tid = threadIdx.x;
    const int w0 = grp * nEpochs;                                            // the group's first window
    const unsigned nFull = (unsigned)(G / kPtsPerBlock);
    const unsigned nTiles = (unsigned)((G + kPtsPerBlock - 1) / kPtsPerBlock);
    f4 bufA[2 * kPairs], bufB[2 * kPairs];
    const auto load = [&](f4 (&g)[2 * kPairs], unsigned tile) { scan_load_tile(g, grid, tile, tid); };
    const unsigned last = (unsigned)(nEnt - 1);
    const float2 *__restrict__ bankG = sd.bank + (size_t)w0 * maxK * nEnt;   // the group's bank rows
    const BcmSvDev *__restrict__ svG = sd.sv + (size_t)w0 * maxK;            // wave-uniform -> scalar loads
    float *srowG = scores + (size_t)grp * sd.pitch;                          // the group's score row: the accumulator
    float bestSc = -1.f;          // scores are >= 0
    unsigned int bestTile = 0u, bestIt = 0u;
    unsigned int nOob = 0;

    for (int e0 = 0; e0 < nEpochs; e0 += winPerPass) {
        const int nw = min(winPerPass, nEpochs - e0);                        // windows of this pass
        const bool first = e0 == 0, final = e0 + nw >= nEpochs;
        // the pass's first tile: issued before the bank fill so both latencies overlap
        if (blockIdx.x < nTiles) load(bufA, blockIdx.x);
        if (!first) __syncthreads();                                         // the previous pass's banks have been read by every wave
        const int rowLen = K * nEnt;
        for (int e = 0; e < nw; ++e) scan_fill_bank(sE + (size_t)e * rowLen, bankG + (size_t)(e0 + e) * maxK * nEnt, rowLen, nEnt, tid);
        __syncthreads();

        const auto tile_body = [&](const f4 (&g)[2 * kPairs], unsigned tile, auto raggedTag) {
            constexpr bool RAGGED = decltype(raggedTag)::value;
            const long long base = (long long)tile * kPtsPerBlock + tid;   // (ragged tile only)
            float *srow = srowG + (size_t)tile * kPtsPerBlock;               // wave-uniform
            f2 dx[kPairs], dy[kPairs], dz[kPairs], dw[kPairs], q[kPairs], score[kPairs];
            // the running score of the earlier passes: this lane's own stores, loaded ahead of the arithmetic that hides them
            float prev[kPtsPerThread];
#pragma unroll
            for (int it = 0; it < kPtsPerThread; ++it) prev[it] = 0.f;
            if (!first) {
#pragma unroll
                for (int it = 0; it < kPtsPerThread; ++it)
                    if (!RAGGED || base + it * 256 < G) prev[it] = srow[it * 256 + tid];
            }
#pragma unroll
            for (int p = 0; p < kPairs; ++p) {
                dx[p] = g[2 * p].xy; dy[p] = g[2 * p].zw; dz[p] = g[2 * p + 1].xy; dw[p] = g[2 * p + 1].zw;
                q[p] = dx[p] * dx[p] + dy[p] * dy[p] + dz[p] * dz[p];
            }
            for (int e = 0; e < nw; ++e) {
                const BcmSvDev *__restrict__ svw = svG + (size_t)(e0 + e) * maxK;
                const float4 *be = sE + (size_t)e * rowLen;
                f2 own[kPairs];
#pragma unroll
                for (int p = 0; p < kPairs; ++p) own[p] = f2{0.f, 0.f};
                unsigned emax = 0;
#pragma unroll DPE_SV_UNROLL
                for (int k = 0; k < K; ++k) {
                    const BcmSvDev s = svw[k];
                    const float4 *bk = be + k * nEnt;
#pragma unroll
                    for (int p = 0; p < kPairs; ++p) {
                        f2 idx;
                        if (SECOND) {
                            f2 a = dx[p] * s.ue;
                            a = __builtin_elementwise_fma(dy[p], f2{s.un, s.un}, a);
                            a = __builtin_elementwise_fma(dz[p], f2{s.uu, s.uu}, a);
                            f2 x = dw[p] - a;
                            const f2 t = __builtin_elementwise_fma(-a, a, q[p]);          // q - a^2
                            x = __builtin_elementwise_fma(t, f2{s.h, s.h}, x);             // + (q - a^2) / (2 range)
                            idx = __builtin_elementwise_fma(x, f2{s.g, s.g}, f2{s.idx0, s.idx0});
                        } else {
                            idx = __builtin_elementwise_fma(dw[p], f2{s.g, s.g}, f2{s.idx0, s.idx0});
                            idx = __builtin_elementwise_fma(dx[p], f2{-s.h, -s.h}, idx);
                            idx = __builtin_elementwise_fma(dy[p], f2{-s.pad0, -s.pad0}, idx);
                            idx = __builtin_elementwise_fma(dz[p], f2{-s.pad1, -s.pad1}, idx);
                        }
                        float c[2];
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const float id = idx[j];
                            const float wgt = __builtin_amdgcn_fractf(id);                 // id - floor(id)
                            int ei;
                            asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(ei) : "v"(id));          // (int)floor(id), saturating
                            unsigned en = (unsigned)ei;
                            if (CLAMP) {                                                   // negative -> huge -> zero slot
                                en = min(en, last);
                                emax = max(emax, en);
                            }
                            const float2 ab = *reinterpret_cast<const float2 *>(&bk[en]);
                            const float m2 = fmaf(wgt, fmaf(wgt, bk[en].w, ab.y), ab.x);
                            if (LP == 1) c[j] = __builtin_amdgcn_sqrtf(__builtin_fabsf(m2));    // raw v_sqrt_f32 (1 ulp)
                            else if (LP == 2) c[j] = m2;
                            else c[j] = powf(__builtin_amdgcn_sqrtf(__builtin_fabsf(m2)), (float)lpower);
                        }
                        own[p] += f2{c[0], c[1]};
                    }
                }
                // out-of-window bookkeeping off the fast path, per window (see scan_body)
                if (CLAMP && emax == last) {
                    for (int it = 0; it < kPtsPerThread; ++it) {
                        if (RAGGED && base + it * 256 >= G) continue;
                        const float px = dx[it >> 1][it & 1], py = dy[it >> 1][it & 1], pz = dz[it >> 1][it & 1];
                        const float pw = dw[it >> 1][it & 1], pq = q[it >> 1][it & 1];
                        for (int k = 0; k < K; ++k) {
                            const BcmSvDev s = svw[k];
                            float id;
                            if (SECOND) {
                                const float a = fmaf(pz, s.uu, fmaf(py, s.un, px * s.ue));
                                float x = pw - a;
                                x = fmaf(fmaf(-a, a, pq), s.h, x);
                                id = fmaf(x, s.g, s.idx0);
                            } else {   // the fast path's own expression, operation for operation
                                id = fmaf(pz, -s.pad1, fmaf(py, -s.pad0, fmaf(px, -s.h, fmaf(pw, s.g, s.idx0))));
                            }
                            int ei;
                            asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(ei) : "v"(id));
                            nOob += (min((unsigned)ei, last) == last) ? 1u : 0u;
                        }
                    }
                }
                // the running score, in window order: the group's first window starts it (0 + own), every other one adds to it
                if (e == 0) {
#pragma unroll
                    for (int p = 0; p < kPairs; ++p) score[p] = f2{prev[2 * p], prev[2 * p + 1]};
                }
#pragma unroll
                for (int p = 0; p < kPairs; ++p) score[p] += own[p];
            }
            if (final) {   // never read back: non-temporal (see scan_body)
#pragma unroll
                for (int it = 0; it < kPtsPerThread; ++it)
                    if (!RAGGED || base + it * 256 < G) __builtin_nontemporal_store(score[it >> 1][it & 1], &srow[it * 256 + tid]);
#pragma unroll
                for (int it = 0; it < kPtsPerThread; ++it) {
                    const float sc = score[it >> 1][it & 1];
                    if ((!RAGGED || base + it * 256 < G) && sc > bestSc) { bestSc = sc; bestTile = tile; bestIt = (unsigned)it; }
                }
            } else {
#pragma unroll
                for (int it = 0; it < kPtsPerThread; ++it)
                    if (!RAGGED || base + it * 256 < G) srow[it * 256 + tid] = score[it >> 1][it & 1];
            }
        };
        // the tile walk of scan_body; tile n of this block is blockIdx.x + n nBlkX in every pass
        unsigned tile = blockIdx.x;
        scan_walk_tiles(tile, nBlkX, nFull, nTiles, bufA, bufB, load, tile_body);
    }

    const unsigned long long best = wave_max_key(pack_key(bestSc, scan_local_index(bestTile, bestIt, tid)));
    nOob = wave_sum(nOob);
    if ((tid & 63) == 0) { sKey[tid >> 6] = best; sOob[tid >> 6] = nOob; }
    __syncthreads();
    if (tid == 0) scan_post_key(&keys[(size_t)grp * 2 + keySlot], &oob[(size_t)grp * 2 + keySlot], block_max_key(sKey), sOob[0] + sOob[1] + sOob[2] + sOob[3]);
}

// Both manifolds in one launch, as bcm_scan_kernel: blockIdx.z = 0 position, 1 velocity, blockIdx.y = group; clears the next
// Update's key set and lets the last block publish the groups' keys and counts into the pinned host mirror.
template <int LP, bool CLAMP_P, bool CLAMP_V>
__global__ __launch_bounds__(256) void bcm_scan_epochs_kernel(ScanSide sp, ScanSide sv, int nEpochs, int winPerPass, int K, int maxK, int lpower,
                                                              unsigned long long *__restrict__ keys, unsigned long long *__restrict__ oob,
                                                              unsigned long long *__restrict__ clearPtr, int clearN,
                                                              unsigned int *__restrict__ done, unsigned long long *__restrict__ hostKeys,
                                                              unsigned long long *__restrict__ hostOob, unsigned long long seqValue)
{
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0)
        for (int i = threadIdx.x; i < clearN; i += 256) clearPtr[i] = 0ull;
    if (blockIdx.z == 0) {
        if (blockIdx.x < (unsigned)sp.split) epochs_body<LP, true, CLAMP_P>(sp, nEpochs, winPerPass, K, maxK, lpower, keys, oob, 0);
    } else {
        if (blockIdx.x < (unsigned)sv.split) epochs_body<LP, false, CLAMP_V>(sv, nEpochs, winPerPass, K, maxK, lpower, keys, oob, 1);
    }
    scan_publish(keys, oob, done, hostKeys, hostOob, seqValue);
}

}  // namespace dpe
