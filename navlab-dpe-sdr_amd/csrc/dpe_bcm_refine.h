// dpe_bcm_refine.h -- coarse-to-fine manifold scan (dpe_bcm_create_refine): each level's tensor-product grid is scored around
// the point the previous level peaked at, per window and per manifold.  Included by dpe_bcm.hip after dpe_bcm_axes.h.
//
// A level is ONE launch (both manifolds, blockIdx.z), behind the previous level's launch in stream order: the kernel boundary
// is the only ordering between levels, nothing is read back by the host in between.  A block of window w, level l >= 1
//   1. reads level l-1's packed key of (w, manifold) from device memory (wave-uniform: scalar loads),
//   2. decodes the flattened index ((ix ny + iy) nz + iz) nt + it against level l-1's dims,
//   3. forms the CENTRE, the fp32 point level l-1 scored there: level l-1's own centre (0 at level 0; kept in device memory by
//      that level's launch) plus its axis values, each sum rounded once to fp32,
//   4. scores its own axes grid at x = fl32(cx + axX[ix]), y, z, t likewise.
// Everything behind the point is axes_body, from the same pieces (dpe_bcm_pieces.h): level l of window w carries,
// bit for bit, the rows, key and count of a dpe_bcm_create_axes handle whose axes are the fp32 values fl32(c + a_i).
//
// A key of 0 means that no point of the previous level had a score (every sum NaN); it would decode to index 2^32 - 1.  The
// preamble tests for it (and for any index beyond the previous grid) before an axis is indexed: such a (window, manifold) is
// not scanned at this or any later level, its keys stay 0.
#pragma once

namespace dpe {

// One manifold's share of one level's launch
struct RefineSide {
    const float *ax;           // every level's fp32 axes of both manifolds in one block; t axes padded by kAxT zeros
    int offX, offY, offZ, offT;         // this level's axes
    int dimY, dimZ, dimT;
    int chunk, nChunks;        // t entries per chunk (<= kAxT) and chunks per row
    unsigned nRows, G;         // rows and points of this level's grid
    int pOffX, pOffY, pOffZ, pOffT;     // the previous level's axes and dims (level >= 1)
    int pDimY, pDimZ, pDimT;
    unsigned pG;
    const float2 *bank;        // [W][maxK][nEnt] score bank
    const BcmSvDev *sv;        // [W][maxK] coefficients, shared by all levels
    float *scores;             // this level's rows [W][pitch] or nullptr
    long long pitch;
    int nEnt, split;
};

template <int LP, bool SECOND, bool CLAMP>
__device__ __forceinline__ void refine_body(const RefineSide &sd, int level, int K, int maxK, int lpower,
                                            unsigned long long *__restrict__ keys, unsigned long long *__restrict__ oob,
                                            const unsigned long long *__restrict__ prevKeys, float *__restrict__ centres,
                                            const float *__restrict__ prevCentres, int keySlot)
{
    const int w = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    // ---- the centre: wave-uniform, before anything else
    // (a sum of two wave-uniform values is formed by the vector ALU; readfirstlane hands it back to the scalar registers, where
    //  axes_body keeps its t values, so the SV loop below takes the same operands)
    const auto uniform = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
    float cx = 0.f, cy = 0.f, cz = 0.f, ct = 0.f;
    if (level > 0) {
        const unsigned long long pk = prevKeys[(size_t)w * 2 + keySlot];
        if (pk == 0ull) return;                                   // nothing scored one level up: not scanned, the key stays 0
        const unsigned pi = 0xFFFFFFFFu - (unsigned)(pk & 0xFFFFFFFFull);
        if (pi >= sd.pG) return;                                  // (never a key of that level: no axis is indexed with it)
        const unsigned r2 = pi / (unsigned)sd.pDimT, pit = pi - r2 * (unsigned)sd.pDimT;
        const unsigned r1 = r2 / (unsigned)sd.pDimZ, piz = r2 - r1 * (unsigned)sd.pDimZ;
        const unsigned pix = r1 / (unsigned)sd.pDimY, piy = r1 - pix * (unsigned)sd.pDimY;
        const float *pc = prevCentres + ((size_t)w * 2 + keySlot) * 4;
        cx = uniform(pc[0] + sd.ax[sd.pOffX + pix]);
        cy = uniform(pc[1] + sd.ax[sd.pOffY + piy]);
        cz = uniform(pc[2] + sd.ax[sd.pOffZ + piz]);
        ct = uniform(pc[3] + sd.ax[sd.pOffT + pit]);
    }
    if (blockIdx.x == 0 && tid == 0) {                            // for the next level's launch
        float *c = centres + ((size_t)w * 2 + keySlot) * 4;
        c[0] = cx; c[1] = cy; c[2] = cz; c[3] = ct;
    }

    const float *__restrict__ axX = sd.ax + sd.offX;
    const float *__restrict__ axY = sd.ax + sd.offY;
    const float *__restrict__ axZ = sd.ax + sd.offZ;
    const float *__restrict__ axT = sd.ax + sd.offT;
    const int nEnt = sd.nEnt, dimT = sd.dimT;
    const unsigned nBlkX = (unsigned)sd.split;
    extern __shared__ __align__(16) unsigned char smem[];
    float4 *sE = reinterpret_cast<float4 *>(smem);   // [K][nEnt] {A, B, 0, C} (scan_fill_bank)
    __shared__ unsigned long long sKey[4];
    __shared__ unsigned int sOob[4];

    float *stg = reinterpret_cast<float *>(smem + (size_t)K * nEnt * sizeof(float4)) + (tid >> 6) * 64 * kAxStage;   // this wave's stage
    scan_fill_bank(sE, sd.bank + (size_t)w * maxK * nEnt, K * nEnt, nEnt, tid);
    __syncthreads();

    const unsigned last = (unsigned)(nEnt - 1);
    const BcmSvDev *svw = sd.sv + (size_t)w * maxK;   // wave-uniform -> scalar loads
    const unsigned nChunks = (unsigned)sd.nChunks, chunk = (unsigned)sd.chunk;
    const unsigned nTiles = (sd.nRows + 255u) / 256u * nChunks;
    const unsigned rowLast = sd.nRows - 1u;
    float bestSc = -1.f;   // scores are >= 0
    unsigned int bestIdx = 0u, nOob = 0u;
    constexpr int kPairs = kAxT / 2;
    for (unsigned tile = blockIdx.x; tile < nTiles; tile += nBlkX) {
        const unsigned grp = tile / nChunks, c = tile - grp * nChunks;   // (wave-uniform)
        const unsigned row0 = grp * 256u, t0 = c * chunk;
        const unsigned nv = min(chunk, (unsigned)dimT - t0);              // t entries of this chunk
        const bool inner = row0 + 256u <= sd.nRows;                       // no row of the tile beyond the grid
        const unsigned row = row0 + (unsigned)tid;
        // lanes past the last row score that row again (their points are never stored, compared or counted)
        const unsigned rr = min(row, rowLast);
        const unsigned rq = rr / (unsigned)sd.dimZ, iz = rr - rq * (unsigned)sd.dimZ;
        const unsigned ix = rq / (unsigned)sd.dimY, iy = rq - ix * (unsigned)sd.dimY;
        const float x = cx + axX[ix], y = cy + axY[iy], z = cz + axZ[iz];   // the point: each sum rounded once
        const float q = x * x + y * y + z * z;
        f2 tp[kPairs], score[kPairs];
#pragma unroll
        for (int p = 0; p < kPairs; ++p) {
            tp[p] = f2{uniform(ct + axT[t0 + 2 * p]), uniform(ct + axT[t0 + 2 * p + 1])};   // wave-uniform (the axis is padded by kAxT)
            score[p] = f2{0.f, 0.f};
        }
        unsigned emax = 0;
#pragma unroll DPE_SV_UNROLL
        for (int k = 0; k < K; ++k) {
            const BcmSvDev s = svw[k];
            const float4 *bk = sE + k * nEnt;
            const float b = axes_row_index<SECOND>(x, y, z, q, s);
#pragma unroll
            for (int p = 0; p < kPairs; ++p) {
                const f2 idx = __builtin_elementwise_fma(tp[p], f2{s.g, s.g}, f2{b, b});
                const float c0 = scan_term<LP, CLAMP>(idx[0], bk, last, emax, lpower);
                const float c1 = scan_term<LP, CLAMP>(idx[1], bk, last, emax, lpower);
                score[p] += f2{c0, c1};
            }
        }
        const unsigned gi0 = row * (unsigned)dimT + t0;   // index of the lane's slot 0 (fits 32 bits, checked at create)
        const auto valid = [&](int it) { return (unsigned)it < nv && (inner || gi0 + (unsigned)it < sd.G); };
        // out-of-window pairs: recounted, with the fast path's own expressions, only where a clamp happened
        if (CLAMP && emax == last) {
            for (int it = 0; it < kAxT; ++it) {
                if (!valid(it)) continue;
                const float t = ct + axT[t0 + it];
                for (int k = 0; k < K; ++k) {
                    const BcmSvDev s = svw[k];
                    nOob += scan_oob(fmaf(t, s.g, axes_row_index<SECOND>(x, y, z, q, s)), last) ? 1u : 0u;
                }
            }
        }
#pragma unroll
        for (int it = 0; it < kAxT; ++it) {
            const float sc = score[it >> 1][it & 1];
            if (!valid(it)) continue;
            if (sc > bestSc) { bestSc = sc; bestIdx = gi0 + (unsigned)it; }
        }
        if (sd.scores) {
            // the wave's 64 rows x nv scores, in index order, as runs of nv consecutive floats (one run when the chunk is the row)
#pragma unroll
            for (int it = 0; it < kAxT; ++it)
                if ((unsigned)it < nv) stg[lane * kAxStage + it] = score[it >> 1][it & 1];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // a wave's LDS accesses complete in order: no barrier needed
            float *srow = sd.scores + (size_t)w * sd.pitch;
            const unsigned waveRow0 = row0 + (unsigned)(tid & ~63), nOut = 64u * nv;
            const float inv = 1.f / (float)nv;
            for (unsigned qi = (unsigned)lane; qi < nOut; qi += 64u) {
                const unsigned r = (unsigned)(((float)qi + 0.5f) * inv), ti = qi - r * nv;   // exact: qi < 1024, nv <= 16
                const unsigned li = (waveRow0 + r) * (unsigned)dimT + t0 + ti;
                const float v = stg[r * kAxStage + ti];
                if (li < sd.G) __builtin_nontemporal_store(v, &srow[li]);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
    }
    const unsigned long long best = wave_max_key(pack_key(bestSc, bestIdx));
    nOob = wave_sum(nOob);
    if (lane == 0) { sKey[tid >> 6] = best; sOob[tid >> 6] = nOob; }
    __syncthreads();
    // (the next level reads the key behind the kernel boundary)
    if (tid == 0)
        scan_post_key(&keys[(size_t)w * 2 + keySlot], &oob[(size_t)w * 2 + keySlot], block_max_key(sKey), sOob[0] + sOob[1] + sOob[2] + sOob[3]);
}

// One level, both manifolds (blockIdx.z = 0 position, 1 velocity).  Level 0 also clears the key set of the NEXT Update (the two
// sets alternate, as in the other scans).  No block waits for another: the results call copies keys and counts of all levels.
template <int LP, bool CLAMP_P, bool CLAMP_V>
__global__ __launch_bounds__(256) void bcm_scan_refine_kernel(RefineSide sp, RefineSide sv, int level, int K, int maxK, int lpower,
                                                              unsigned long long *__restrict__ keys, unsigned long long *__restrict__ oob,
                                                              const unsigned long long *__restrict__ prevKeys, float *__restrict__ centres,
                                                              const float *__restrict__ prevCentres,
                                                              unsigned long long *__restrict__ clearPtr, int clearN)
{
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0)
        for (int i = threadIdx.x; i < clearN; i += 256) clearPtr[i] = 0ull;
    if (blockIdx.z == 0) {
        if (blockIdx.x < (unsigned)sp.split) refine_body<LP, true, CLAMP_P>(sp, level, K, maxK, lpower, keys, oob, prevKeys, centres, prevCentres, 0);
    } else {
        if (blockIdx.x < (unsigned)sv.split) refine_body<LP, false, CLAMP_V>(sv, level, K, maxK, lpower, keys, oob, prevKeys, centres, prevCentres, 1);
    }
}

}  // namespace dpe
