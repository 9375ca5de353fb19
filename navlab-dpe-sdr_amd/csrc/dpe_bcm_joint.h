// dpe_bcm_joint.h -- the manifold scan for several receivers over one pair of grids (dpe_bcm_create_joint), included by
// dpe_bcm.hip after scan_body.
//
// N receivers (rigid set, one oscillator or calibrated clock offsets) each bring their own centre state, receive time, tracked
// SVs and score banks; the grids of ENU-dt offsets are shared and grid point j means "every receiver at its own centre moved by
// offset j" (PyGNSS' multi receiver mode, receiver.py:266-274,337-345,385-388, with gX_r = X_r + offsets).  The joint score of a
// point is the sum over receivers of the score scan_body would give that receiver there; its first maximum is the joint ML offset.
//
// The kernel is scan_body's (both manifolds in one launch, the tile walk, the LDS entries, the index math, the clamp variants, the
// ragged tile, the fused key), written from the same pieces (dpe_bcm_pieces.h) except the out-of-window
// recount, which stands here as text (through scan_recount two general-power variants take 1 to 3 more VGPRs).  What is new:
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
    float4 *sE = reinterpret_cast<float4 *>(smem);                           // [sum K][nEnt] entries {A, B, 0, C} (scan_fill_bank)
    __shared__ unsigned long long sKey[4];
    __shared__ unsigned long long sOwnKey[4][kJointMaxRx];
    __shared__ unsigned int sOwnOob[4][kJointMaxRx];

    const int w = blockIdx.y, tid = threadIdx.x;
    const unsigned nFull = (unsigned)(G / kPtsPerBlock);
    const unsigned nTiles = (unsigned)((G + kPtsPerBlock - 1) / kPtsPerBlock);
    f4 bufA[2 * kPairs], bufB[2 * kPairs];
    const auto load = [&](f4 (&g)[2 * kPairs], unsigned tile) { scan_load_tile(g, grid, tile, tid); };
    if (blockIdx.x < nTiles) load(bufA, blockIdx.x);
    const JointRxDev *__restrict__ rxw = rx + (size_t)w * maxRx;             // wave-uniform -> scalar loads
    for (int r = 0; r < nRx; ++r)
        scan_fill_bank(sE + (size_t)rxw[r].kOff * nEnt, SECOND ? rxw[r].code : rxw[r].carr, rxw[r].nChan * nEnt, nEnt, tid);
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
        ScanPts pt;
        scan_unpack(pt, g);
        f2 score[kPairs];
#pragma unroll
        for (int p = 0; p < kPairs; ++p) score[p] = f2{0.f, 0.f};
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
                for (int p = 0; p < kPairs; ++p) own[p] += scan_pair_term<LP, SECOND, CLAMP>(pt, p, s, bk, last, emax, lpower);
            }
            // out-of-window bookkeeping off the fast path, per receiver
            if (CLAMP && emax == last) {
                for (int it = 0; it < kPtsPerThread; ++it) {
                    if (RAGGED && base + it * 256 >= G) continue;
                    const float px = pt.dx[it >> 1][it & 1], py = pt.dy[it >> 1][it & 1], pz = pt.dz[it >> 1][it & 1];
                    const float pw = pt.dw[it >> 1][it & 1], pq = pt.q[it >> 1][it & 1];
                    for (int k = 0; k < K; ++k) {
                        const BcmSvDev s = svw[k0 + k];
                        float id;
                        if (SECOND) {
                            const float a = fmaf(pz, s.uu, fmaf(py, s.un, px * s.ue));
                            float x = pw - a;
                            x = fmaf(fmaf(-a, a, pq), s.h, x);
                            id = fmaf(x, s.g, s.idx0);
                        } else {
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
            if (OWN) scan_track_max<RAGGED>(own, base, G, tile, ownSc[r], ownAt[r]);
        }
        if (scores) scan_store_row<RAGGED>(scores + (size_t)w * sd.pitch + (size_t)tile * kPtsPerBlock, score, base, G, tid);
        scan_track_max<RAGGED>(score, base, G, tile, bestSc, bestTile, bestIt);
    };
    unsigned tile = blockIdx.x;
    scan_walk_tiles(tile, nBlkX, nFull, nTiles, bufA, bufB, load, tile_body);

    const unsigned int io = (unsigned int)indexOffset;
    const unsigned long long best = wave_max_key(pack_key(bestSc, io + scan_local_index(bestTile, bestIt, tid)));
    if ((tid & 63) == 0) sKey[tid >> 6] = best;
#pragma unroll
    for (int r = 0; r < kJointMaxRx; ++r) {
        if (r >= nRx) break;
        if (OWN) {
            const unsigned long long b =
                wave_max_key(pack_key(ownSc[r], io + scan_local_index(ownAt[r] / (unsigned)kPtsPerThread, ownAt[r] % (unsigned)kPtsPerThread, tid)));
            if ((tid & 63) == 0) sOwnKey[tid >> 6][r] = b;
        }
        if (CLAMP) {
            const unsigned int n = wave_sum(nOob[r]);
            if ((tid & 63) == 0) sOwnOob[tid >> 6][r] = n;
        }
    }
    __syncthreads();
    // per-receiver results: thread r < nRx reduces receiver r over the four waves (read by the host after the launch has
    // finished: no ordering against the ticket is needed)
    unsigned int nMine = 0;
    if (tid < nRx) {
        const size_t slot = ((size_t)w * 2 + keySlot) * maxRx + tid;
        if (OWN) atomicMax(&ownKeys[slot], block_max_key(&sOwnKey[0][tid], kJointMaxRx));
        if (CLAMP) {
            nMine = sOwnOob[0][tid] + sOwnOob[1][tid] + sOwnOob[2][tid] + sOwnOob[3][tid];
            if (nMine) atomicAdd(&ownOob[slot], (unsigned long long)nMine);
        }
    }
    if (CLAMP && tid < 64) {      // the joint count: the sum over receivers (nRx <= 8 lanes of the first wave hold them)
#pragma unroll
        for (int off = 4; off > 0; off >>= 1) nMine += __shfl_xor(nMine, off, 64);
    }
    if (tid == 0) scan_post_key(&keys[(size_t)w * 2 + keySlot], &oob[(size_t)w * 2 + keySlot], block_max_key(sKey), CLAMP ? nMine : 0u);
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
