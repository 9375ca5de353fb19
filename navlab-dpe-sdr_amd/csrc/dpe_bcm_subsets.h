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
// What the kernel keeps from scan_body / joint_body: both manifolds in one launch, the persistent tile loop with double-buffered
// buffer loads of scan_grid_slot tiles, the {A, B, 0, C} LDS entries, the packed-fp32 index math, the clamp variants, the ragged
// last tile, the fused first-maximum key and scan_publish.  What is new:
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
    float4 *sE = reinterpret_cast<float4 *>(smem);                           // [K][nEnt] entries {A, B, 0, C} (see scan_body)
    __shared__ unsigned long long sKey[4];
    __shared__ unsigned long long sSubKey[4][kSubsetMax];
    __shared__ unsigned int sSvOob[DPE_MAX_CHAN];
    __shared__ unsigned int sMember[DPE_MAX_CHAN];                           // per SV: bit m = subset m holds it

    const int w = blockIdx.y, tid = threadIdx.x;
    constexpr int kPairs = kPtsPerThread / 2;
    const unsigned nFull = (unsigned)(G / kPtsPerBlock);
    const unsigned nTiles = (unsigned)((G + kPtsPerBlock - 1) / kPtsPerBlock);
    f4 bufA[2 * kPairs], bufB[2 * kPairs];
    const auto load = [&](f4 (&g)[2 * kPairs], unsigned tile) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<f4 *>(grid + (size_t)tile * kPtsPerBlock), 0, kPtsPerBlock * (int)sizeof(f4), 0x00020000);
#pragma unroll
        for (int j = 0; j < 2 * kPairs; ++j)
            g[j] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rs, tid * (int)sizeof(f4), j * 256 * (int)sizeof(f4), 0));
    };
    if (blockIdx.x < nTiles) load(bufA, blockIdx.x);
    const float2 *bw = sd.bank + (size_t)w * maxK * nEnt;
    for (int i = tid; i < K * nEnt; i += 256) {
        const int k = i / nEnt, j = i - k * nEnt;
        if (j + 1 < nEnt) {      // (entry nEnt - 1 is the all-zero slot out-of-window indices are clamped to)
            const float2 c0 = bw[(size_t)k * nEnt + j], c1 = bw[(size_t)k * nEnt + j + 1];
            const float dr = c1.x - c0.x, di = c1.y - c0.y;
            const float eA = c0.x * c0.x + c0.y * c0.y, eB = 2.f * (c0.x * dr + c0.y * di), eC = dr * dr + di * di;
            sE[i] = make_float4(eA, eB, 0.f, eC);
        } else {
            sE[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
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
        f2 dx[kPairs], dy[kPairs], dz[kPairs], dw[kPairs], q[kPairs], score[kPairs];
        f2 sub[kSubsetMax][kPairs];
#pragma unroll
        for (int p = 0; p < kPairs; ++p) {
            dx[p] = g[2 * p].xy; dy[p] = g[2 * p].zw; dz[p] = g[2 * p + 1].xy; dw[p] = g[2 * p + 1].zw;
            q[p] = dx[p] * dx[p] + dy[p] * dy[p] + dz[p] * dz[p];
            score[p] = f2{0.f, 0.f};
        }
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
        // out-of-window bookkeeping off the fast path, per SV (see scan_body): recount only if this thread ever hit the zero slot
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
                    if (min((unsigned)ei, last) == last) atomicAdd(&sSvOob[k], 1u);
                }
            }
        }
        if (scores) {   // written once, never read back on this path: non-temporal (see scan_body)
            float *srow = scores + (size_t)w * sd.pitch + (size_t)tile * kPtsPerBlock;   // wave-uniform
#pragma unroll
            for (int it = 0; it < kPtsPerThread; ++it)
                if (!RAGGED || base + it * 256 < G) __builtin_nontemporal_store(score[it >> 1][it & 1], &srow[it * 256 + tid]);
        }
#pragma unroll
        for (int it = 0; it < kPtsPerThread; ++it) {
            const float sc = score[it >> 1][it & 1];
            if ((!RAGGED || base + it * 256 < G) && sc > bestSc) { bestSc = sc; bestTile = tile; bestIt = (unsigned)it; }
        }
        if (SUBS) {
#pragma unroll
            for (int m = 0; m < kSubsetMax; ++m) {
                if (m < subset_count()) {
#pragma unroll
                    for (int it = 0; it < kPtsPerThread; ++it) {
                        const float sc = sub[m][it >> 1][it & 1];
                        if ((!RAGGED || base + it * 256 < G) && sc > subSc[m]) { subSc[m] = sc; subAt[m] = tile * (unsigned)kPtsPerThread + (unsigned)it; }
                    }
                }
            }
        }
    };
    unsigned tile = blockIdx.x;
    for (;;) {
        if (tile >= nFull) break;
        const unsigned t1 = tile + nBlkX;
        if (t1 < nTiles) load(bufB, t1);
        tile_body(bufA, tile, std::false_type{});
        tile = t1;
        if (tile >= nFull) {
#pragma unroll
            for (int j = 0; j < 2 * kPairs; ++j) bufA[j] = bufB[j];   // (once per block, for the ragged tile below)
            break;
        }
        const unsigned t2 = tile + nBlkX;
        if (t2 < nTiles) load(bufA, t2);
        tile_body(bufB, tile, std::false_type{});
        tile = t2;
    }
    if (tile < nTiles) tile_body(bufA, tile, std::true_type{});

    const auto make_key = [&](float sc, unsigned int localIdx) -> unsigned long long {
        const unsigned int gi = (unsigned int)indexOffset + localIdx;
        return sc < 0.f ? 0ull : (((unsigned long long)__float_as_uint(sc) << 32) | (unsigned long long)(0xFFFFFFFFu - gi));
    };
    unsigned long long best = make_key(bestSc, bestTile * (unsigned int)kPtsPerBlock + bestIt * 256u + (unsigned int)tid);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off, 64);
        best = o > best ? o : best;
    }
    if ((tid & 63) == 0) sKey[tid >> 6] = best;
    if (SUBS) {
#pragma unroll
        for (int m = 0; m < kSubsetMax; ++m) {
            if (m < subset_count()) {
                unsigned long long b = make_key(subSc[m], (subAt[m] / (unsigned)kPtsPerThread) * (unsigned int)kPtsPerBlock +
                                                              (subAt[m] % (unsigned)kPtsPerThread) * 256u + (unsigned int)tid);
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const unsigned long long o = __shfl_xor(b, off, 64);
                    b = o > b ? o : b;
                }
                if ((tid & 63) == 0) sSubKey[tid >> 6][m] = b;
            }
        }
    }
    __syncthreads();
    // per-subset keys and per-SV counts: read by the host after the launch has finished, so no ordering against the ticket
    if (SUBS && tid < nSubsets) {
        unsigned long long b = sSubKey[0][tid];
        b = sSubKey[1][tid] > b ? sSubKey[1][tid] : b;
        b = sSubKey[2][tid] > b ? sSubKey[2][tid] : b;
        b = sSubKey[3][tid] > b ? sSubKey[3][tid] : b;
        atomicMax(&subKeys[((size_t)w * 2 + keySlot) * maxSubsets + tid], b);
    }
    if (CLAMP && tid < K) {
        const unsigned int n = sSvOob[tid];
        if (n) atomicAdd(&svOob[((size_t)w * 2 + keySlot) * maxK + tid], (unsigned long long)n);
    }
    if (tid == 0) {
        unsigned long long b = sKey[0];
        b = sKey[1] > b ? sKey[1] : b;
        b = sKey[2] > b ? sKey[2] : b;
        b = sKey[3] > b ? sKey[3] : b;
        // RETURNING atomics, waited for before this block takes its ticket (see scan_body / scan_publish)
        unsigned long long seen = atomicMax(&keys[(size_t)w * 2 + keySlot], b);
        if (CLAMP) {            // the full set's count: the sum over SVs
            unsigned int n = 0;
            for (int k = 0; k < K; ++k) n += sSvOob[k];
            if (n) seen += atomicAdd(&oob[(size_t)w * 2 + keySlot], (unsigned long long)n);
        }
        asm volatile("" ::"v"(seen) : "memory");
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
