// dpe_bcm_joint.h -- the manifold scan for several receivers over one pair of grids (dpe_bcm_create_joint), included by
// dpe_bcm.hip after scan_body.
//
// N receivers (rigid set, one oscillator or calibrated clock offsets) each bring their own centre state, receive time, tracked
// SVs and score banks; the grids of ENU-dt offsets are shared and grid point j means "every receiver at its own centre moved by
// offset j" (PyGNSS' multi receiver mode, receiver.py:266-274,337-345,385-388, with gX_r = X_r + offsets).  The joint score of a
// point is the sum over receivers of the score scan_body would give that receiver there; its first maximum is the joint ML offset.
//
// What the kernel keeps from scan_body: both manifolds in one launch, the persistent tile loop with double-buffered buffer loads
// of scan_grid_slot tiles, the {A, B, 0, C} LDS entries, the packed-fp32 index math, the clamp variants, the ragged last tile and
// the fused first-maximum key.  What is new:
//  * the LDS fill reads each receiver's banks through that receiver's own pointers (JointRxDev), rows kOff .. kOff + nChan - 1;
//  * the per-(receiver, SV) coefficients come from a device array through wave-uniform (scalar) loads -- 64 channels x 2
//    manifolds x 32 B would be the whole kernel-argument segment;
//  * the SV loop runs receiver by receiver: a receiver's own score is summed exactly as scan_body sums it (same order, starting
//    from 0) and then added to the joint score, so that a receiver's own row, and the joint row of a single receiver, carry the
//    bits of the single-receiver scan;
//  * OWN: a running (score, position) per receiver beside the joint one -- one launch yields the joint key and nRx own keys per
//    manifold.  Out-of-window pairs are counted per receiver in every clamped variant.
// The receiver loop is unrolled to kJointMaxRx with a wave-uniform exit, so the per-receiver accumulators are indexed by
// constants and stay in registers (a runtime index would send them to scratch).
#pragma once

namespace dpe {

constexpr int kJointMaxRx = 8;     // receivers per scan
constexpr int kJointMaxK = 64;     // (receiver, SV) pairs per scan

// One receiver of one window, as the kernel reads it (scalar loads): 32 bytes
struct JointRxDev {
    const float2 *code, *carr;   // its banks of this window: [nChan][nEnt] rows
    int nChan, kOff;             // its SVs are rows kOff .. kOff + nChan - 1 of the window's coefficient block and of the LDS
    int pad0, pad1;
};

template <int LP, bool SECOND, bool CLAMP, bool OWN>
__device__ __forceinline__ void joint_body(const ScanSide &sd, const JointRxDev *__restrict__ rx, int nRx, int maxRx, int maxKT, int lpower,
                                           unsigned long long *__restrict__ keys, unsigned long long *__restrict__ oob,
                                           unsigned long long *__restrict__ ownKeys, unsigned long long *__restrict__ ownOob, int keySlot)
{
    const f4 *__restrict__ grid = reinterpret_cast<const f4 *>(sd.grid);
    float *__restrict__ scores = sd.scores;
    const long long G = sd.G, indexOffset = sd.indexOffset;
    const int nEnt = sd.nEnt;
    const unsigned nBlkX = (unsigned)sd.split;
    extern __shared__ __align__(16) unsigned char smem[];
    float4 *sE = reinterpret_cast<float4 *>(smem);                           // [sum K][nEnt] entries {A, B, 0, C} (see scan_body)
    __shared__ unsigned long long sKey[4];
    __shared__ unsigned long long sOwnKey[4][kJointMaxRx];
    __shared__ unsigned int sOwnOob[4][kJointMaxRx];

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
    const JointRxDev *__restrict__ rxw = rx + (size_t)w * maxRx;             // wave-uniform -> scalar loads
    for (int r = 0; r < nRx; ++r) {
        const float2 *__restrict__ bw = SECOND ? rxw[r].code : rxw[r].carr;
        float4 *dst = sE + (size_t)rxw[r].kOff * nEnt;
        const int n = rxw[r].nChan * nEnt;
        for (int i = tid; i < n; i += 256) {
            const int k = i / nEnt, j = i - k * nEnt;
            if (j + 1 < nEnt) {      // (entry nEnt - 1 is the all-zero slot out-of-window indices are clamped to)
                const float2 c0 = bw[(size_t)k * nEnt + j], c1 = bw[(size_t)k * nEnt + j + 1];
                const float dr = c1.x - c0.x, di = c1.y - c0.y;
                const float eA = c0.x * c0.x + c0.y * c0.y, eB = 2.f * (c0.x * dr + c0.y * di), eC = dr * dr + di * di;
                dst[i] = make_float4(eA, eB, 0.f, eC);
            } else {
                dst[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    }
    __syncthreads();

    const unsigned last = (unsigned)(nEnt - 1);
    const BcmSvDev *__restrict__ svw = sd.sv + (size_t)w * maxKT;            // wave-uniform -> scalar loads
    float bestSc = -1.f;          // scores are >= 0
    unsigned int bestTile = 0u, bestIt = 0u;
    // per receiver: the running maximum of its own score as (score, tile * kPtsPerThread + it), and its out-of-window pairs
    float ownSc[kJointMaxRx];
    unsigned int ownAt[kJointMaxRx], nOob[kJointMaxRx];
#pragma unroll
    for (int r = 0; r < kJointMaxRx; ++r) { ownSc[r] = -1.f; ownAt[r] = 0u; nOob[r] = 0u; }

    const auto tile_body = [&](const f4 (&g)[2 * kPairs], unsigned tile, auto raggedTag) {
        constexpr bool RAGGED = decltype(raggedTag)::value;
        const long long base = (long long)tile * kPtsPerBlock + tid;   // (ragged tile only)
        f2 dx[kPairs], dy[kPairs], dz[kPairs], dw[kPairs], q[kPairs], score[kPairs];
#pragma unroll
        for (int p = 0; p < kPairs; ++p) {
            dx[p] = g[2 * p].xy; dy[p] = g[2 * p].zw; dz[p] = g[2 * p + 1].xy; dw[p] = g[2 * p + 1].zw;
            q[p] = dx[p] * dx[p] + dy[p] * dy[p] + dz[p] * dz[p];
            score[p] = f2{0.f, 0.f};
        }
#pragma unroll
        for (int r = 0; r < kJointMaxRx; ++r) {
            if (r >= nRx) break;
            const int K = rxw[r].nChan, k0 = rxw[r].kOff;
            f2 own[kPairs];
#pragma unroll
            for (int p = 0; p < kPairs; ++p) own[p] = f2{0.f, 0.f};
            unsigned emax = 0;
#pragma unroll DPE_SV_UNROLL
            for (int k = 0; k < K; ++k) {
                const BcmSvDev s = svw[k0 + k];
                const float4 *bk = sE + (k0 + k) * nEnt;
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
                    own[p] += f2{c[0], c[1]};
                }
            }
            // out-of-window bookkeeping off the fast path, per receiver (see scan_body)
            if (CLAMP && emax == last) {
                for (int it = 0; it < kPtsPerThread; ++it) {
                    if (RAGGED && base + it * 256 >= G) continue;
                    const float px = dx[it >> 1][it & 1], py = dy[it >> 1][it & 1], pz = dz[it >> 1][it & 1];
                    const float pw = dw[it >> 1][it & 1], pq = q[it >> 1][it & 1];
                    for (int k = 0; k < K; ++k) {
                        const BcmSvDev s = svw[k0 + k];
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
                        nOob[r] += (min((unsigned)ei, last) == last) ? 1u : 0u;
                    }
                }
            }
#pragma unroll
            for (int p = 0; p < kPairs; ++p) score[p] += own[p];
            if (OWN) {
#pragma unroll
                for (int it = 0; it < kPtsPerThread; ++it) {
                    const float sc = own[it >> 1][it & 1];
                    if ((!RAGGED || base + it * 256 < G) && sc > ownSc[r]) { ownSc[r] = sc; ownAt[r] = tile * (unsigned)kPtsPerThread + (unsigned)it; }
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
#pragma unroll
    for (int r = 0; r < kJointMaxRx; ++r) {
        if (r >= nRx) break;
        if (OWN) {
            unsigned long long b = make_key(ownSc[r], (ownAt[r] / (unsigned)kPtsPerThread) * (unsigned int)kPtsPerBlock +
                                                          (ownAt[r] % (unsigned)kPtsPerThread) * 256u + (unsigned int)tid);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long o = __shfl_xor(b, off, 64);
                b = o > b ? o : b;
            }
            if ((tid & 63) == 0) sOwnKey[tid >> 6][r] = b;
        }
        if (CLAMP) {
            unsigned int n = nOob[r];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
            if ((tid & 63) == 0) sOwnOob[tid >> 6][r] = n;
        }
    }
    __syncthreads();
    // per-receiver results: thread r < nRx reduces receiver r over the four waves (read by the host after the launch has
    // finished: no ordering against the ticket is needed)
    unsigned int nMine = 0;
    if (tid < nRx) {
        const size_t slot = ((size_t)w * 2 + keySlot) * maxRx + tid;
        if (OWN) {
            unsigned long long b = sOwnKey[0][tid];
            b = sOwnKey[1][tid] > b ? sOwnKey[1][tid] : b;
            b = sOwnKey[2][tid] > b ? sOwnKey[2][tid] : b;
            b = sOwnKey[3][tid] > b ? sOwnKey[3][tid] : b;
            atomicMax(&ownKeys[slot], b);
        }
        if (CLAMP) {
            nMine = sOwnOob[0][tid] + sOwnOob[1][tid] + sOwnOob[2][tid] + sOwnOob[3][tid];
            if (nMine) atomicAdd(&ownOob[slot], (unsigned long long)nMine);
        }
    }
    if (CLAMP && tid < 64) {      // the joint count: the sum over receivers (nRx <= 8 lanes of the first wave hold them)
#pragma unroll
        for (int off = 4; off > 0; off >>= 1) nMine += __shfl_xor(nMine, off, 64);
    }
    if (tid == 0) {
        unsigned long long b = sKey[0];
        b = sKey[1] > b ? sKey[1] : b;
        b = sKey[2] > b ? sKey[2] : b;
        b = sKey[3] > b ? sKey[3] : b;
        // RETURNING atomics, waited for before this block takes its ticket (see scan_body / scan_publish)
        unsigned long long seen = atomicMax(&keys[(size_t)w * 2 + keySlot], b);
        if (CLAMP && nMine) seen += atomicAdd(&oob[(size_t)w * 2 + keySlot], (unsigned long long)nMine);
        asm volatile("" ::"v"(seen) : "memory");
    }
}

// Both manifolds in one launch, as bcm_scan_kernel: blockIdx.z = 0 position, 1 velocity; clears the next Update's key set and
// lets the last block publish the joint keys and counts into the pinned host mirror.
template <int LP, bool CLAMP_P, bool CLAMP_V, bool OWN>
__global__ __launch_bounds__(256) void bcm_scan_joint_kernel(ScanSide sp, ScanSide sv, const JointRxDev *__restrict__ rx, int nRx, int maxRx,
                                                             int maxKT, int lpower, unsigned long long *__restrict__ keys,
                                                             unsigned long long *__restrict__ oob, unsigned long long *__restrict__ ownKeys,
                                                             unsigned long long *__restrict__ ownOob,
                                                             unsigned long long *__restrict__ clearPtr, int clearN,
                                                             unsigned int *__restrict__ done, unsigned long long *__restrict__ hostKeys,
                                                             unsigned long long *__restrict__ hostOob, unsigned long long seqValue)
{
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0)
        for (int i = threadIdx.x; i < clearN; i += 256) clearPtr[i] = 0ull;
    if (blockIdx.z == 0) {
        if (blockIdx.x < (unsigned)sp.split) joint_body<LP, true, CLAMP_P, OWN>(sp, rx, nRx, maxRx, maxKT, lpower, keys, oob, ownKeys, ownOob, 0);
    } else {
        if (blockIdx.x < (unsigned)sv.split) joint_body<LP, false, CLAMP_V, OWN>(sv, rx, nRx, maxRx, maxKT, lpower, keys, oob, ownKeys, ownOob, 1);
    }
    scan_publish(keys, oob, done, hostKeys, hostOob, seqValue);
}

}  // namespace dpe
