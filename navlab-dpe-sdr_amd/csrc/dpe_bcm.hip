// dpe_bcm.hip -- BatchCorrManifold for MI355X (gfx950): score every point of the ENU-dt
// (and velocity-drift) manifold grid against the per-SV score banks, fused arg-max.
//
// Replaces BCM_PosMeasML / BCM_VelMeasML + thrust::max_element + BCM_MakePosMeas/MakeVelMeas
// (cudarecv/modules/src/batchcorrmanifold.cu:1710-1828,1861-1963,2589-2596).
//
// The reference evaluates, per (grid point, SV), an fp64 range with ~2e7 m magnitude and maps it
// to a fractional index into the SV's score row.  Here the geometry is expanded about the grid
// centre on the HOST in fp64 (per window, per SV: unit line of sight in ENU, index at the centre,
// index-per-metre scale, 1/(2 range)); the kernel then needs only fp32 DIFFERENCES:
//   pos:  d_rho = |d - R delta| - |d| = -a + (q - a^2) h + O(|delta|^3 / range^2),
//         a = u_enu . delta, q = |delta|^2, h = 1/(2 range)       (error < 1.3e-5 m for |delta| < 3 km)
//         idx  = idx0 + g (delta_t + d_rho)                         (g = fs F_CA / (fc C), :1783-1791)
//   vel:  idx  = idx0 + g_v (u_enu . delta_v - delta_tdot)          (exactly linear, :1917-1936)
// followed by the reference's floor / floor(+1) linear interpolation (:1798-1812) and |.|^L.
//
// HBM traffic per window per manifold: 16 B/point grid read (scan layout, coalesced) + 4 B/point score
// write; banks (K x (2L+1) float4 pairs) and SV coefficients live in LDS.
#include <algorithm>
#include <atomic>
#include <type_traits>

#include "dpe_common.h"
#include "dpe_prep.h"

namespace dpe {

// Single-window calls pass both manifolds' coefficients in the kernel-argument segment of the scan
// kernels (params_ptr, dpe_common.h); pb must stay their FIRST argument.
struct BcmParamBlock {
    BcmSvDev s[2][DPE_MAX_CHAN];
};

typedef float f2 __attribute__((ext_vector_type(2)));

#ifndef DPE_PTS_PER_THREAD
#define DPE_PTS_PER_THREAD 4
#endif
#ifndef DPE_SV_UNROLL
#define DPE_SV_UNROLL 2
#endif
constexpr int kPtsPerThread = DPE_PTS_PER_THREAD;
constexpr int kPtsPerBlock = 256 * kPtsPerThread;

// One manifold's share of the fused launch
struct ScanSide {
    const float4 *grid;       // [nTiles * kPtsPerBlock] ENU-dt offsets of this rank's shard in the scan layout (scan_grid_slot)
    const float2 *bank;       // [W][maxK][nEnt] score bank
    const BcmSvDev *sv;       // [W][maxK] coefficients (ignored when they ride in the kernel arguments)
    float *scores;            // [W][pitch] or nullptr (rows start on 128-byte lines, see dpe_bcm_scores_pitch)
    double *wsum;             // weighted-sum partials (WMEAN) or nullptr
    long long G, indexOffset, pitch;
    int nEnt, split;          // bank entries per SV; blocks along x that work on this manifold
};

// The scan layout of a grid.  Point i = tile * kPtsPerBlock + lane + 256 it (lane < 256, it < kPtsPerThread) is one of the pair
// (it & ~1, it | 1) of its lane; the tile holds, per pair p, the 256 lanes' {x_a, x_b, y_a, y_b} followed by their
// {z_a, z_b, t_a, t_b} (a = point 2p, b = point 2p + 1).  Every load instruction of the scan reads 64 lanes x 16 B contiguous
// and leaves the x / y / z / t pairs in the register pairs the packed fp32 math takes as they are; the grid is padded with
// zeros to whole tiles, so no load needs a bounds check.  Returns the float index of coordinate c (0 x, 1 y, 2 z, 3 t).
__host__ __device__ inline size_t scan_grid_slot(long long i, int c)
{
    const long long tile = i / kPtsPerBlock, r = i - tile * kPtsPerBlock;
    const int it = (int)(r >> 8), lane = (int)(r & 255);
    const long long v = tile * kPtsPerBlock + (long long)((it & ~1) + (c >> 1)) * 256 + lane;   // float4 slot
    return (size_t)v * 4 + (size_t)((c & 1) * 2 + (it & 1));
}

typedef float f4 __attribute__((ext_vector_type(4)));

}  // namespace dpe

#include "dpe_bcm_pieces.h"

namespace dpe {

// COMPACT: 12-byte LDS entries {A, B, C} instead of 16 (three dword reads per pair instead of b64 + b32): the layout for
// bank sets that do not fit the LDS otherwise (37 channels with +-130 .. +-172 entries) -- slower, always with the clamps.
template <int LP, bool SECOND, bool CLAMP, bool WMEAN, bool COMPACT = false>
__device__ __forceinline__ void scan_body(const ScanSide &sd, int inl, int K, int maxK, int lpower,
                                          unsigned long long *__restrict__ keys, unsigned long long *__restrict__ oob,
                                          int keyStride, int keySlot)
{
    const f4 *__restrict__ grid = reinterpret_cast<const f4 *>(sd.grid);
    float *__restrict__ scores = sd.scores;
    double *__restrict__ wsum = sd.wsum;
    const long long G = sd.G, indexOffset = sd.indexOffset;
    const int nEnt = sd.nEnt;
    const unsigned nBlkX = (unsigned)sd.split;   // persistent stride of this manifold's blocks
    extern __shared__ __align__(16) unsigned char smem[];
    float4 *sE = reinterpret_cast<float4 *>(smem);                           // [K][nEnt] {A, B, 0, C} (scan_fill_bank)
    float *sF = reinterpret_cast<float *>(smem);                             // COMPACT: [K][nEnt][3]
    __shared__ unsigned long long sKey[4];
    __shared__ unsigned int sOob[4];
    __shared__ double sW[4][5];

    const int w = blockIdx.y, tid = threadIdx.x;
    // Persistent over point tiles: block (x, w) scores tiles x, x+gridDim.x, ... of window w, so the bank
    // fill below is paid once per block and the next tile's grid points are prefetched under the
    // current tile's arithmetic.  gridDim.x is a multiple of 8: blocks are dealt to the 8 XCDs round
    // robin, so each XCD's L2 keeps re-serving the same 1/8 of the grid for every window.
    // A thread's points: tile*1024 + tid + 256*it, held as PAIRS (scan_grid_slot) so that the geometry runs on packed fp32
    // (v_pk_fma_f32: two points per instruction).  The tile count and offsets fit 32 bits (G < 2^32, checked at create).
    const unsigned nFull = (unsigned)(G / kPtsPerBlock);                         // tiles without padding
    const unsigned nTiles = (unsigned)((G + kPtsPerBlock - 1) / kPtsPerBlock);
    // two register sets for the grid points: tile n computes from one while tile n + nBlkX lands in the other
    f4 bufA[2 * kPairs], bufB[2 * kPairs];
    const auto load = [&](f4 (&g)[2 * kPairs], unsigned tile) { scan_load_tile(g, grid, tile, tid); };
    // first tile's grid points: issued before the bank fill so both latencies overlap
    if (blockIdx.x < nTiles) load(bufA, blockIdx.x);
    const float2 *bw = sd.bank + (size_t)w * maxK * nEnt;
    scan_fill_bank<COMPACT>(sE, bw, K * nEnt, nEnt, tid);
    __syncthreads();

    const unsigned last = (unsigned)(nEnt - 1);
    // wave-uniform address -> scalar loads; inl: this manifold's coefficients come from pb.s[SECOND ? 0 : 1]
    const BcmSvDev *svw = params_ptr(sd.sv + (size_t)w * maxK, inl) + ((inl && !SECOND) ? DPE_MAX_CHAN : 0);
    // per-lane running maximum as (score, tile, it); the packed 64-bit key is built once, after the tile loop
    float bestSc = -1.f;          // scores are >= 0
    unsigned int bestTile = 0u, bestIt = 0u;
    unsigned int nOob = 0;
    // "Method 1" weighted-mean estimator (optional: wsum != nullptr): sum s, sum s*{x,y,z,t}, pair-packed fp32
    f2 w0 = f2{0.f, 0.f}, w1 = w0, w2 = w0, w3 = w0, w4 = w0;
    // One tile from the registers g.  RAGGED: the last tile of a grid whose size is not a multiple of kPtsPerBlock -- its
    // padded points are scored like the others but never stored, compared, summed or counted.  Every other tile runs without
    // a per-point predicate.
    const auto tile_body = [&](const f4 (&g)[2 * kPairs], unsigned tile, auto raggedTag) {
        constexpr bool RAGGED = decltype(raggedTag)::value;
        const long long base = (long long)tile * kPtsPerBlock + tid;   // (ragged tile only)
        ScanPts pt;
        scan_unpack(pt, g);
        f2 score[kPairs];
#pragma unroll
        for (int p = 0; p < kPairs; ++p) score[p] = f2{0.f, 0.f};
        unsigned emax = 0;
#pragma unroll DPE_SV_UNROLL
        for (int k = 0; k < K; ++k) {
            const BcmSvDev s = svw[k];
            const void *bk = COMPACT ? (const void *)sF : (const void *)(sE + k * nEnt);   // COMPACT: the bank; the row goes with the entry
#pragma unroll
            for (int p = 0; p < kPairs; ++p)
                score[p] += scan_pair_term<LP, SECOND, CLAMP, COMPACT>(pt, p, s, bk, last, emax, lpower, COMPACT ? (size_t)k * nEnt : 0);
        }
        // recount only if this thread ever hit the zero slot (the ragged tile's padded points may have: they are skipped)
        if (CLAMP && emax == last) scan_recount<SECOND, RAGGED>(pt, svw, K, last, base, G, [&](int, unsigned n) DPE_INLINE_LAMBDA { nOob += n; });
        if (WMEAN) {
#pragma unroll
            for (int p = 0; p < kPairs; ++p) {
                f2 sc = score[p];
                if (RAGGED) {   // padded points must not count
                    if (base + (2 * p) * 256 >= G) sc.x = 0.f;
                    if (base + (2 * p + 1) * 256 >= G) sc.y = 0.f;
                }
                w0 += sc;
                w1 = __builtin_elementwise_fma(sc, pt.dx[p], w1);
                w2 = __builtin_elementwise_fma(sc, pt.dy[p], w2);
                w3 = __builtin_elementwise_fma(sc, pt.dz[p], w3);
                w4 = __builtin_elementwise_fma(sc, pt.dw[p], w4);
            }
        }
        if (scores) scan_store_row<RAGGED>(scores + (size_t)w * sd.pitch + (size_t)tile * kPtsPerBlock, score, base, G, tid);
        // the running maximum remembers (tile, it) of its point; the index is formed once, after the tile loop
        scan_track_max<RAGGED>(score, base, G, tile, bestSc, bestTile, bestIt);
    };
    unsigned tile = blockIdx.x;
    scan_walk_tiles(tile, nBlkX, nFull, nTiles, bufA, bufB, load, tile_body);
    // global index of the lane's best point (< 2^32, checked at create)
    const unsigned int bestIdx = (unsigned int)indexOffset + scan_local_index(bestTile, bestIt, tid);
    const unsigned long long best = wave_max_key(pack_key(bestSc, bestIdx));
    nOob = wave_sum(nOob);
    double ws[5] = {(double)w0.x + (double)w0.y, (double)w1.x + (double)w1.y, (double)w2.x + (double)w2.y,
                    (double)w3.x + (double)w3.y, (double)w4.x + (double)w4.y};
    if (WMEAN) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int j = 0; j < 5; ++j) ws[j] += __shfl_xor(ws[j], off, 64);
        }
    }
    if ((tid & 63) == 0) {
        sKey[tid >> 6] = best; sOob[tid >> 6] = nOob;
        if (WMEAN) {
#pragma unroll
            for (int j = 0; j < 5; ++j) sW[tid >> 6][j] = ws[j];
        }
    }
    __syncthreads();
    if (tid == 0) {
        // per-block partial of the weighted sums, reduced on the host in block order (deterministic)
        if (WMEAN) {
            double *o = wsum + ((size_t)w * nBlkX + blockIdx.x) * 5;   // wsum already points at this manifold's half
#pragma unroll
            for (int j = 0; j < 5; ++j) o[j] = ((sW[0][j] + sW[1][j]) + sW[2][j]) + sW[3][j];
        }
        scan_post_key(&keys[(size_t)w * keyStride + keySlot], &oob[(size_t)w * keyStride + keySlot], block_max_key(sKey),
                      sOob[0] + sOob[1] + sOob[2] + sOob[3]);
    }
}

// ---- the scans' common epilogue: the last block out publishes the results
__device__ __forceinline__ void scan_publish(unsigned long long *__restrict__ keys, unsigned long long *__restrict__ oob,
                                             unsigned int *__restrict__ done, unsigned long long *__restrict__ hostKeys,
                                             unsigned long long *__restrict__ hostOob, unsigned long long seqValue)
{
    // Thread 0 issued this block's key / counter atomics and has their return values, i.e. they are
    // performed at the device's coherence point; its ticket follows in program order.  The block that
    // draws the last ticket therefore reads final values with agent-scope loads.
    // (done == nullptr: nobody reads the host mirror -- the device-resident loop's next kernel takes the keys from device memory
    //  behind the kernel boundary -- so the ticket, the agent-scope reads and the stores over the host link are skipped)
    if (!done) return;
    __shared__ unsigned int sLast;
    if (threadIdx.x == 0) {
        const unsigned int total = gridDim.x * gridDim.y * gridDim.z;
        sLast = (atomicInc(done, total - 1) == total - 1) ? 1u : 0u;
    }
    __syncthreads();
    if (sLast) {
        const int n = 2 * (int)gridDim.y;
        if (gridDim.y == 1) {
            // One window: keys, counts and a sequence word share one 64-byte line of the host mirror and are written by
            // ONE lane in program order (same line -> same memory channel -> they arrive in that order), the sequence
            // word last.  The host may poll it instead of waiting on the stream (dpe_bcm_results).
            if (threadIdx.x == 0) {
                unsigned long long v[4];
                v[0] = __hip_atomic_load(&keys[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                v[1] = __hip_atomic_load(&keys[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                v[2] = __hip_atomic_load(&oob[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                v[3] = __hip_atomic_load(&oob[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&hostKeys[0], v[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                __hip_atomic_store(&hostKeys[1], v[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                __hip_atomic_store(&hostOob[0], v[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                __hip_atomic_store(&hostOob[1], v[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(&hostOob[2], seqValue, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // sequence word
            }
        } else {
            for (int i = threadIdx.x; i < n; i += 256) {
                const unsigned long long kv = __hip_atomic_load(&keys[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned long long ov = __hip_atomic_load(&oob[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&hostKeys[i], kv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                __hip_atomic_store(&hostOob[i], ov, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// Both manifolds in ONE launch: blockIdx.z = 0 scores the position grid, 1 the velocity grid (a lone
// window then pays one launch instead of two and the two scans overlap).  Around the scans the kernel
//  * clears the key / counter set of the NEXT Update (the two sets alternate), so that no clearing
//    launch or memset node sits on the critical path, and
//  * lets the last block to finish publish keys and out-of-window counts of all windows straight
//    into the pinned host mirror (system-scope stores): dpe_bcm_results needs no D2H copy command.
// `done` cycles 0 .. total-1 through atomicInc and is back at 0 when the kernel ends.
template <int LP, bool CLAMP_P, bool CLAMP_V, bool WMEAN, bool COMPACT = false>
__global__ __launch_bounds__(256) void bcm_scan_kernel(BcmParamBlock pb, int inl, ScanSide sp, ScanSide sv, int K, int maxK,
                                                       int lpower, unsigned long long *__restrict__ keys,
                                                       unsigned long long *__restrict__ oob,
                                                       unsigned long long *__restrict__ clearPtr, int clearN,
                                                       unsigned int *__restrict__ done,
                                                       unsigned long long *__restrict__ hostKeys,
                                                       unsigned long long *__restrict__ hostOob,
                                                       unsigned long long seqValue)
{
    (void)pb;
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0)
        for (int i = threadIdx.x; i < clearN; i += 256) clearPtr[i] = 0ull;
    if (blockIdx.z == 0) {
        if (blockIdx.x < (unsigned)sp.split) scan_body<LP, true, CLAMP_P, WMEAN, COMPACT>(sp, inl, K, maxK, lpower, keys, oob, 2, 0);
    } else {
        if (blockIdx.x < (unsigned)sv.split) scan_body<LP, false, CLAMP_V, WMEAN, COMPACT>(sv, inl, K, maxK, lpower, keys, oob, 2, 1);
    }
    scan_publish(keys, oob, done, hostKeys, hostOob, seqValue);
}

}  // namespace dpe

#include "dpe_bcm_axes.h"
#include "dpe_bcm_refine.h"
#include "dpe_bcm_joint.h"
#include "dpe_bcm_epochs.h"
#include "dpe_bcm_subsets.h"
#include "dpe_bcm_moments.h"

namespace dpe {

// Device-resident inputs (dpe_bcm_update_dev): the per-SV coefficients of both manifolds from the reference's own port arrays
// on the device (cuChanMgr / cuEKF outputs, dpeflow.cpp:178-191,212; captured once by the reference at
// batchcorrmanifold.cu:2512-2540) -- what the host loop of dpe_bcm_update computes, in fp64.  The host form carries the centre
// index in long double because rxTime - pr / C (rxTime ~ 4e5 s) rounds at 5.8e-11 s in fp64; here the same difference is kept
// as an unevaluated sum (TwoSum, bcm_prep_one in dpe_prep.h).  One block, thread <-> channel; thread 0 also leaves the window's
// frame (xCurrkk1, ENU2ECEFMat, DopplerSign) in pinned host memory for dpe_bcm_results.  rxTimeDev != nullptr: the receive
// time is read from the device (a channel manager that lives there), else it is the host scalar of the reference (:2536-2537).
struct BcmPortsDev {
    const double *x, *R, *sat, *rcEnd, *fc, *fi;
    const int *cpRefTOW, *cpElaEnd, *cpRef, *dopplerSign;
    int dimT;
};
__global__ void bcm_prep_kernel(BcmPortsDev p, int K, double rxTime, const double *__restrict__ rxTimeDev, double fs, double Cf, int S, int L, int B,
                                long long C, BcmSvDev *__restrict__ svPos, BcmSvDev *__restrict__ svVel, BcmDevWin *__restrict__ hostWin)
{
    const int k = threadIdx.x;
    const double *c = p.x, *R = p.R;
    const int dsRaw = p.dopplerSign[0];
    const int ds = (dsRaw == 1 || dsRaw == -1) ? dsRaw : 1;   // (a bad value is flagged; the scan must stay finite)
    if (rxTimeDev) rxTime = *rxTimeDev;
    if (k == 0) {
        for (int i = 0; i < 8; ++i) hostWin->xCurrkk1[i] = c[i];
        for (int i = 0; i < 9; ++i) hostWin->enu2ecef[i] = R[i];
        hostWin->dopplerSign = ds;
        hostWin->bad = (dsRaw == 1 || dsRaw == -1) ? 0 : 1;
    }
    if (k >= K) return;
    const double *s = p.sat + ((size_t)k * p.dimT + p.dimT / 2) * 8;                      // mid-time entry, :1775
    BcmSvDev a, v;
    bcm_prep_one(c, R, s, p.rcEnd[k], p.fc[k], p.fi[k], p.cpRefTOW[k], p.cpElaEnd[k], p.cpRef[k], ds, rxTime, fs, Cf, S, L, B, C, a, v);
    svPos[k] = a;
    svVel[k] = v;
}

// PosScores in the reference's port type: one dense fp64 row (ConfigOutput(3, "PosScores", DOUBLE_t, GRID, ...), :2300)
__global__ void bcm_export_f64_kernel(const float *__restrict__ row, long long G, double *__restrict__ out)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < G; i += (long long)gridDim.x * blockDim.x) out[i] = (double)row[i];
}

// referencePair mode, step 1: grid points whose FIRST-channel index lies within `tol` entries of the centre lag (bank entry L)
// -- the only ones the reference's floor(idx) / floor(idx + 1) pair can treat differently (see ref_pair_fixup).  Candidates
// are appended as (window << 40 | point); cand[0] counts them (it may run past the capacity: the host then grows the list).
__global__ __launch_bounds__(256) void bcm_refpair_candidates_kernel(const float4 *__restrict__ grid, long long G, const BcmSvDev *__restrict__ sv,
                                                                     int maxK, int L, double tol, unsigned long long *__restrict__ cand,
                                                                     unsigned long long capacity)
{
    const int w = blockIdx.y;
    const BcmSvDev p0 = sv[(size_t)w * maxK];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < G; i += (long long)gridDim.x * 256) {
        const float *gf = reinterpret_cast<const float *>(grid);   // (the scan layout)
        const float4 g = make_float4(gf[scan_grid_slot(i, 0)], gf[scan_grid_slot(i, 1)], gf[scan_grid_slot(i, 2)], gf[scan_grid_slot(i, 3)]);
        const double a = (double)p0.ue * g.x + (double)p0.un * g.y + (double)p0.uu * g.z;
        const double q = (double)g.x * g.x + (double)g.y * g.y + (double)g.z * g.z;
        const double idx0 = (double)p0.idx0 + (double)p0.g * ((double)g.w - a + (q - a * a) * (double)p0.h);
        if (fabs(idx0 - (double)L) <= tol) {
            const unsigned long long slot = atomicAdd(&cand[0], 1ull);
            if (slot < capacity) cand[1 + slot] = ((unsigned long long)w << 40) | (unsigned long long)i;
        }
    }
}

// step 3: the re-evaluated scores go in with one launch; the scores they replace come back (weighted-mean correction)
__global__ void bcm_patch_kernel(float *__restrict__ scores, long long pitch, const unsigned long long *__restrict__ where,
                                 const float *__restrict__ value, float *__restrict__ old, int n)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const unsigned long long wi = where[j];
    float *dst = scores + (size_t)(wi >> 40) * pitch + (size_t)(wi & ((1ull << 40) - 1));
    old[j] = *dst;
    *dst = value[j];
}

// step 4: arg-max of the position manifold re-derived from the patched score array.
__global__ void bcm_zero_pos_keys_kernel(unsigned long long *__restrict__ keys, int nWindows)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w < nWindows) keys[2 * (size_t)w] = 0ull;
}

__global__ __launch_bounds__(256) void bcm_rekey_kernel(const float *__restrict__ scores, long long G, long long pitch, long long indexOffset,
                                                        unsigned long long *__restrict__ keys)
{
    const int w = blockIdx.y;
    const float *row = scores + (size_t)w * pitch;
    float bestSc = -1.f;
    unsigned int bestIdx = 0u;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < G; i += (long long)gridDim.x * 256) {
        const float sc = row[i];
        if (sc > bestSc) { bestSc = sc; bestIdx = (unsigned int)(i + indexOffset); }   // increasing i per lane: first maximum kept
    }
    unsigned long long best = bestSc < 0.f ? 0ull
                                           : (((unsigned long long)__float_as_uint(bestSc) << 32) | (unsigned long long)(0xFFFFFFFFu - bestIdx));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off, 64);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0 && best) atomicMax(&keys[2 * (size_t)w], best);
}

// referencePair for the device-parameter form (dpe_bcm_update_dev), step 2 on the device: one thread per candidate re-evaluates its
// point with the reference's own expression in fp64 (batchcorrmanifold.cu:1760-1816, the host form's ref_pair_index / ref_pair_fixup
// operation for operation) from the port arrays, and where the neighbour pair is two apart writes the score in place.  A candidate
// list that overflowed its capacity cannot be grown without the host: bit 1 of the window frame's `bad` (the results call reports it).
#pragma clang fp contract(off)
__device__ static inline bool ref_pair_index_dev(const double *R, const double *c, const double *s, double rxTime, double rcEnd, double fc,
                                                 int cpRefTOW, int cpElaEnd, int cpRef, const double *g, double fs, int S, int k,
                                                 double *idxOut, double *fiOut, double *ciOut)
{
    const double px = R[0] * g[0] + R[1] * g[1] + R[2] * g[2] + c[0];        // :1760-1763
    const double py = R[3] * g[0] + R[4] * g[1] + R[5] * g[2] + c[1];
    const double pz = R[6] * g[0] + R[7] * g[1] + R[8] * g[2] + c[2];
    const double pdt = g[3] + c[3];
    const double lx = s[0] - px, ly = s[1] - py, lz = s[2] - pz;            // :1779-1781
    const double range = sqrt(lx * lx + ly * ly + lz * lz);                 // :1782
    const double pr = range - kC * s[3] + pdt;                              // :1783
    const double txT = rxTime - pr / kC;                                    // :1784
    const double cfd = txT - cpRefTOW - ((cpElaEnd - cpRef) * kTCA);
    const double rcbc = cfd * kFCA;                                         // :1786
    const double rc0 = rcbc - rcEnd;                                        // :1790
    const double base = (fs / fc) * (-rc0) + S / 2.0;                       // :1791
    if (!(base < S && base > 0)) return false;                              // :1795
    const double idx = base + ((double)S * k);                              // :1797
    *idxOut = idx;
    *fiOut = floor(idx);                                                    // :1798
    *ciOut = floor(idx + 1);                                                // :1799
    return true;
}
__global__ __launch_bounds__(64) void bcm_refpair_eval_kernel(BcmPortsDev p, int K, double rxTime, const double *__restrict__ rxTimeDev, double fs, int S, int L, int lPower,
                                                               const double *__restrict__ grid64, const float2 *__restrict__ bank, int maxK,
                                                               const unsigned long long *__restrict__ cand, unsigned long long capacity,
                                                               float *__restrict__ scores, long long pitch, BcmDevWin *__restrict__ hostWin,
                                                               unsigned long long *__restrict__ patched)
{
    const unsigned long long nAll = cand[0], n = nAll < capacity ? nAll : capacity;
    if (nAll > capacity && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&hostWin->bad, 2);
    if (rxTimeDev) rxTime = *rxTimeDev;   // (the prepared form: the receiver time is the channel manager's device port)
    const int nLag = 2 * L + 1;
    for (unsigned long long j = (unsigned long long)blockIdx.x * 64 + threadIdx.x; j < n; j += (unsigned long long)gridDim.x * 64) {
        const unsigned long long wi = cand[1 + j];
        const long long i = (long long)(wi & ((1ull << 40) - 1));   // (one window in this form)
        const double *g = grid64 + 4 * i;
        double idx, fi_, ci_;
        const double *s0 = p.sat + ((size_t)0 * p.dimT + p.dimT / 2) * 8;
        if (!ref_pair_index_dev(p.R, p.x, s0, rxTime, p.rcEnd[0], p.fc[0], p.cpRefTOW[0], p.cpElaEnd[0], p.cpRef[0], g, fs, S, 0, &idx, &fi_, &ci_)) continue;
        if (ci_ - fi_ != 2.0) continue;                                   // the ordinary pair: the scan's value stands
        double score = 0.0;
        for (int k = 0; k < K; ++k) {
            const double *s = p.sat + ((size_t)k * p.dimT + p.dimT / 2) * 8;
            if (!ref_pair_index_dev(p.R, p.x, s, rxTime, p.rcEnd[k], p.fc[k], p.cpRefTOW[k], p.cpElaEnd[k], p.cpRef[k], g, fs, S, k, &idx, &fi_, &ci_)) continue;
            const long long fin = (long long)fi_ - (long long)S * k - (S / 2 - L);
            const long long cin = (long long)ci_ - (long long)S * k - (S / 2 - L);
            if (fin < 0 || cin < 0 || fin >= nLag || cin >= nLag) continue;
            const float2 *row = bank + (size_t)k * nLag;
            const double wc = idx - fi_, wf = ci_ - idx;                 // :1810-1811
            const double vr = (double)row[cin].x * wc + (double)row[fin].x * wf;
            const double vi = (double)row[cin].y * wc + (double)row[fin].y * wf;
            score += pow(hypot(vr, vi), (double)lPower);                  // :1816
        }
        scores[(size_t)i] = (float)score;
        atomicAdd(patched, 1ull);
        (void)maxK; (void)pitch;
    }
}

}  // namespace dpe

// ============================================================================================
struct dpe_bcm {
    dpe_bcm_config cfg;
    std::vector<double> posGrid_h, velGrid_h;  // local shard, fp64 (for zVal)
    float4 *posGrid_d = nullptr, *velGrid_d = nullptr;   // fp32, in the scan layout (dpe::scan_grid_slot)
    dpe_owner_detach_fn ownerDetach = nullptr;   // an attached device-resident channel manager: told first when this handle is destroyed
    void *owner = nullptr;
    bool gridsBorrowed = false;   // the fp32 device grids belong to another handle of the same dpe_pipe (dpe_bcm_create_sharing)
    double *posGrid64_d = nullptr, *velGrid64_d = nullptr;   // fp64 copies for a measurement formed on the device (dpe_bcm_hook_get)
    float *posScores_d = nullptr, *velScores_d = nullptr;
    long long posPitch = 0, velPitch = 0;   // floats between the score rows of consecutive windows (grid size rounded up to 32)
    dpe::BcmSvDev *sv_d = nullptr;  // [2][W][maxK]  (manifold-major)
    // pinned staging ring (see dpe_bcs): Updates may be issued kStaging - 1 deep without waiting
    static constexpr int kStaging = 4;
    dpe::BcmSvDev *svBase_h = nullptr, *sv_h = nullptr, *svBase_hd = nullptr;   // _hd: the pinned block's device address
    hipEvent_t stagingFree[kStaging] = {};
    int slot = 0;
    unsigned long long *keys_d = nullptr;  // [2 sets][{keys [W][2], counts [W][2]}], alternating between Updates
    int cur = 1;                           // set of the latest Update
    unsigned int *done_d = nullptr;        // finished-block ticket of the scan kernel (returns to 0 by itself)
    unsigned long long *keys_hd = nullptr; // device view of the pinned mirror keys_h
    unsigned long long seq = 0;            // single-window Updates: sequence number the kernel writes behind the results
    bool pollable = false, pollAllowed = true;   // last Update was a single eager window; DPE_BCM_NO_POLL=1 disables
    double *wsum_d = nullptr;   // [W][2][split][5] per-block weighted sums
    unsigned long long *keys_h = nullptr, *oob_h = nullptr;   // pinned mirrors, filled by async copies at the end of Update
    unsigned lastSplit[2] = {0, 0};
    int splitForce = 0;                     // -DDPE_EXPERIMENTS builds only: DPE_BCM_SPLIT at create
    static constexpr unsigned kMaxSplit = 4096;
    size_t wsumHalf = 0;
    // referencePair mode (dpe_bcm_config): active only when S / 2 is a power of two
    bool compact = false;                   // 12-byte LDS bank entries (the banks of all channels would not fit otherwise)
    bool refPair = false;
    float2 *refBank_h = nullptr;            // pinned copy of the code banks of the last Update
    unsigned long long *refCand_d = nullptr;   // [1 + refCap] candidate list of the device prefilter (entry 0: count)
    unsigned long long refCap = 0;
    unsigned long long *refWhere_d = nullptr;  // [refPatchCap] patches: (window << 40 | point), value, replaced value
    float *refValue_d = nullptr, *refOld_d = nullptr;
    size_t refPatchCap = 0;
    std::vector<double> refWsum;            // [W][5] corrections of the weighted sums (patched - scanned score at offset x,y,z,t)
    long long refPatched = 0;               // points patched by the last Update (diagnostic)
    dpe::BcmPortsDev refPorts{};            // the device ports of the dpe_bcm_update_dev in progress (referencePair on the device)
    double refRxTime = 0.0;
    const double *refRxTime_d = nullptr;    // the prepared form: rxTime as a device port of the attached channel manager (dpe_bcm_hook_set_ref_ports)
    bool refPortsAttached = false;
    unsigned long long *refPatched_d = nullptr;
    std::vector<dpe_bcm_window> win_h;
    dpe::BcmDevWin *devWin_h = nullptr, *devWin_hd = nullptr;   // pinned [2]: window frame of a device-parameter Update (written by bcm_prep_kernel),
                                                                // one per alternating key set, so that the results of Update n can still be
                                                                // decoded after Update n + 1 has been enqueued
    bool lastDev = false;
    int lastW = 0;
    bool publish = true;        // false: the scan leaves keys / counts in device memory only (set by the device-resident channel manager's attach)
    bool lastPublished = true;  // what the last Update did
    double posExtent = 0, velExtent = 0;
    // grids given by their axes (dpe_bcm_create_axes): the handle keeps the global axes, never a per-point copy
    bool axes = false;
    struct Axes {
        int dim[4];
        std::vector<double> v[4];   // fp64, for decoding an index into a point
    } posAx, velAx;
    float *axes_d = nullptr;        // both manifolds' fp32 axes in one block (layout: AxesSide), t padded by kAxT
    int axOff[2][4] = {};           // float offsets of the x, y, z, t axes of each manifold in axes_d
    bool axesBorrowed = false;      // axes_d belongs to another lane of the same dpe_pipe
    double *posAx64_d = nullptr, *velAx64_d = nullptr;   // fp64 global axes for a measurement formed on the device (dpe_bcm_hook_get)
    // several receivers over one pair of grids (dpe_bcm_create_joint): cfg.maxChannels is then the per-receiver bound
    bool joint = false;
    int jointMaxRx = 0, jointMaxK = 0;      // receivers and (receiver, SV) pairs per window
    dpe::JointRxDev *jrx_d = nullptr, *jrxBase_h = nullptr;   // [W][maxRx] per-receiver bank pointers and row ranges; pinned staging ring
    unsigned long long *own_d = nullptr;    // {own keys [W][2][maxRx], own out-of-window counts [W][2][maxRx]}
    std::vector<unsigned long long> own_h;
    std::vector<dpe_bcm_window> jwin_h;     // [W][maxRx] window frames of the last joint Update
    int lastRx = 0;
    bool ownKeys = true, lastOwn = false;   // dpe_bcm_joint_set_own_keys; what the last joint Update ran with
    // N consecutive windows summed into one row and one arg-max (dpe_bcm_create_epochs): lastW then counts GROUPS
    bool epochs = false;
    int epMaxEpochs = 0, epPairsPerPass = 0;   // windows per group; (window, SV) pairs whose banks share the LDS in one pass
    int lastEpochs = 0, lastPasses = 0;     // what the last epochs Update ran with
    // the arg-max of every SV subset of a window from one scan (dpe_bcm_create_subsets)
    bool subsets = false;
    int subMax = 0, lastSubsets = 0, lastChan = 0;   // subsets per window the handle holds; what the last subsets Update ran with
    bool lastCounted = false;               // the last subsets Update ran a clamped variant (only then are the per-SV counters written)
    unsigned long long *sub_d = nullptr;    // {masks [W][subMax], subset keys [W][2][subMax], per-SV out-of-window counts [W][2][maxK]}
    unsigned long long *subMaskBase_h = nullptr;   // pinned staging ring of the masks
    std::vector<unsigned long long> sub_h, subMask_h;   // host copies: keys and counts of the last Update; its masks
    // coarse-to-fine levels, each scanned around the previous arg-max (dpe_bcm_create_refine): the level axes share axes_d
    bool refine = false;
    int rfLevels = 0;
    struct RefineLevel {
        int dim[2][4];                   // [manifold][axis]
        std::vector<float> v[2][4];      // the fp32 axis values the device adds to the centre
        int off[2][4];                   // their float offsets in axes_d
        long long G[2], pitch[2];
        float *scores[2];                // [W][pitch] or nullptr
    } rf[DPE_REFINE_MAX_LEVELS] = {};
    unsigned long long *rfKeys_d = nullptr;   // [2 sets][{keys [levels][W][2], counts [levels][W][2]}], alternating between Updates
    float *rfCentre_d = nullptr;              // [levels][W][2][4]: the fp32 centre each level scanned around
    std::vector<unsigned long long> rfKeys_h; // one set: the last Update's keys and counts (dpe_bcm_results_refine)
    // thresholded moments of the score rows (dpe_bcm_moments): everything here is allocated by the first call, not at create
    double *momPartial_d = nullptr;           // [W][2][blocks per row][kMomSlots] per-block partials of the last call
    double *momSums_d = nullptr;              // [maxWindows][2][15]
    long long *momAbove_d = nullptr;          // [maxWindows][2]
    dpe::MomMirror *momMirror_h = nullptr, *momMirror_hd = nullptr;   // pinned [maxWindows][2], filled on the stream
    int momW = 0;                             // windows of the last call
    dpe::KernelProfiler prof;  // slot 0: the fused position + velocity scan
    dpe::GraphCache graphs;
};

// The device copy is the scan layout (dpe::scan_grid_slot), zero-padded to whole tiles: the only fp32 copy on the device
static int upload_grid(const double *src, int64_t G, std::vector<double> &keep, float4 **dst)
{
    using namespace dpe;
    keep.assign(src, src + 4 * G);
    const size_t nPad = (size_t)((G + kPtsPerBlock - 1) / kPtsPerBlock) * kPtsPerBlock;
    std::vector<float> f(4 * nPad, 0.f);
    for (int64_t i = 0; i < G; ++i)
        for (int c = 0; c < 4; ++c) f[scan_grid_slot(i, c)] = (float)src[4 * i + c];
    *dst = dev_alloc<float4>(nPad);
    DPE_REQUIRE(*dst, "[BatchCorrManifold] create: grid allocation failed (%lld points)", (long long)G);
    DPE_CHECK_HIP(hipMemcpy(*dst, f.data(), sizeof(float4) * nPad, hipMemcpyHostToDevice));
    return 0;
}

// Blocks along x per window: ~4096 blocks in flight overall for batches, a multiple of 8 (XCD round robin, see the
// kernel) and never more than the number of 1024-point tiles.
static unsigned scan_split(long long G, int nWindows, int forced)
{
    const long long nTiles = (G + dpe::kPtsPerBlock - 1) / dpe::kPtsPerBlock;
    long long s = 4096 / nWindows;
    // one or two windows (closed loop): latency, not throughput -- 128 blocks per manifold (one block per CU over both
    // manifolds), each walking several tiles, beat one block per tile: the per-block costs (bank staging, key atomics,
    // ticket) are paid fewer times.  Measured on the 25^4 grids: 53.5 -> 49.3 us per window.
    if (nWindows <= 2 && s > 128) s = 128;
    // batches: ~768 blocks per manifold are enough to fill the chip, and each extra block stages the banks again (K x nEnt
    // entries).  Measured: config H (12 SVs x 63 entries, 32 windows) scan 0.090 ms at 96 blocks per window, 0.040 at 24;
    // config R (256 windows) 0.538 at 16, 0.533 at 24.
    if (nWindows > 2) {
        const long long cap = 768 / nWindows > 24 ? 768 / nWindows : 24;
        if (s > cap) s = cap;
    }
    if (forced > 0) s = forced;   // (-DDPE_EXPERIMENTS builds: DPE_BCM_SPLIT, read at create)
    if (s < 8) s = 8;
    s = (s + 7) / 8 * 8;
    if (s > nTiles) s = nTiles;
    return (unsigned)s;
}

// What every scan launch carries behind its own arguments: the key / counter set it reduces into, the set it clears, the
// publishing epilogue's pointers (scan_publish) and the launch geometry
struct ScanTail {
    unsigned long long *keys, *oob, *clr;
    int clrN;
    unsigned int *done;
    unsigned long long *hostKeys, *hostOob, seq;
    dim3 grid;
    size_t lds;
    hipStream_t st;
};

// The runtime (lPower, clampP, clampV, fourth flag) of a launch as template arguments: f(LP, CP, CV, X) is called once, with
// std::integral_constant values (LP: 1, 2, or 0 for the general power).  clampP / clampV = false only when the host has proved
// that every index of every (point, SV) pair of that manifold stays inside the bank (then the kernel drops the range clamp and
// the out-of-window bookkeeping); the fourth flag is the family's own (weighted mean, own keys, subsets; unused by some).
template <class F>
static void scan_dispatch(int lp, bool clampP, bool clampV, bool x, const F &f)
{
    const auto pick = [](bool b, const auto &g) { if (b) g(std::true_type{}); else g(std::false_type{}); };
    const auto with_lp = [&](auto LP) {
        pick(clampP, [&](auto CP) { pick(clampV, [&](auto CV) { pick(x, [&](auto X) { f(LP, CP, CV, X); }); }); });
    };
    if (lp == 1) with_lp(std::integral_constant<int, 1>{});
    else if (lp == 2) with_lp(std::integral_constant<int, 2>{});
    else with_lp(std::integral_constant<int, 0>{});
}

// f(LP, CP, CV, X) once for every variant of a family (fourth: the family has a fourth flag; without one X is always false);
// big_lds lets one of them use the whole LDS (create calls it for all)
template <class F>
static void scan_every_variant(bool fourth, const F &f)
{
    for (int lp = 0; lp < 3; ++lp)
        for (int m = 0; m < (fourth ? 8 : 4); ++m) scan_dispatch(lp, (m & 1) != 0, (m & 2) != 0, (m & 4) != 0, f);
}

template <class Kernel>
static void big_lds(Kernel *kernel)
{
    (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 155 * 1024);
}

#define DPE_V(T) decltype(T)::value   // the value of a dispatch argument, as a template argument

struct ScanLaunch : ScanTail {
    dpe::BcmParamBlock pb;
    int inl, K, maxK, lp;
    dpe::ScanSide sp, sv;
};

// wmean selects the variant that also accumulates the weighted-mean sums; compact the 12-byte LDS entries (always clamped)
static void launch_scan(bool clampP, bool clampV, bool wmean, bool compact, const ScanLaunch &a)
{
    scan_dispatch(a.lp, clampP, clampV, wmean, [&](auto LP, auto CP, auto CV, auto WM) {
        if (compact)
            hipLaunchKernelGGL((dpe::bcm_scan_kernel<DPE_V(LP), true, true, DPE_V(WM), true>), a.grid, dim3(256), a.lds, a.st, a.pb, a.inl, a.sp, a.sv,
                               a.K, a.maxK, a.lp, a.keys, a.oob, a.clr, a.clrN, a.done, a.hostKeys, a.hostOob, a.seq);
        else
            hipLaunchKernelGGL((dpe::bcm_scan_kernel<DPE_V(LP), DPE_V(CP), DPE_V(CV), DPE_V(WM)>), a.grid, dim3(256), a.lds, a.st, a.pb, a.inl, a.sp,
                               a.sv, a.K, a.maxK, a.lp, a.keys, a.oob, a.clr, a.clrN, a.done, a.hostKeys, a.hostOob, a.seq);
    });
}

static void allow_big_lds_scan()
{
    scan_every_variant(true, [](auto LP, auto CP, auto CV, auto WM) {
        big_lds(dpe::bcm_scan_kernel<DPE_V(LP), DPE_V(CP), DPE_V(CV), DPE_V(WM)>);
        if (DPE_V(CP) && DPE_V(CV)) big_lds(dpe::bcm_scan_kernel<DPE_V(LP), true, true, DPE_V(WM), true>);   // compact: always clamped
    });
}

// Grids given by their axes (dpe_bcm_create_axes): the same launch with AxesSide in place of ScanSide
struct AxesLaunch {
    ScanLaunch a;
    dpe::AxesSide sp, sv;
};

static void launch_axes(bool clampP, bool clampV, bool wmean, const AxesLaunch &x)
{
    const ScanLaunch &a = x.a;
    scan_dispatch(a.lp, clampP, clampV, wmean, [&](auto LP, auto CP, auto CV, auto WM) {
        hipLaunchKernelGGL((dpe::bcm_scan_axes_kernel<DPE_V(LP), DPE_V(CP), DPE_V(CV), DPE_V(WM)>), a.grid, dim3(256), a.lds, a.st, a.pb, a.inl, x.sp, x.sv,
                           a.K, a.maxK, a.lp, a.keys, a.oob, a.clr, a.clrN, a.done, a.hostKeys, a.hostOob, a.seq);
    });
}

static void allow_big_lds_axes()
{
    scan_every_variant(true, [](auto LP, auto CP, auto CV, auto WM) { big_lds(dpe::bcm_scan_axes_kernel<DPE_V(LP), DPE_V(CP), DPE_V(CV), DPE_V(WM)>); });
}

// One manifold's AxesSide (m = 0 position, 1 velocity) for this handle's slice; the tile count comes back in *nTiles
static dpe::AxesSide axes_side(const dpe_bcm *h, int m, long long *nTiles)
{
    const dpe_bcm::Axes &ax = m ? h->velAx : h->posAx;
    const long long off = m ? h->cfg.velGridIndexOffset : h->cfg.posGridIndexOffset, G = m ? h->cfg.velGridSize : h->cfg.posGridSize;
    const long long dimT = ax.dim[3];
    dpe::AxesSide s{};
    s.ax = h->axes_d;
    s.offX = h->axOff[m][0]; s.offY = h->axOff[m][1]; s.offZ = h->axOff[m][2]; s.offT = h->axOff[m][3];
    s.dimY = ax.dim[1]; s.dimZ = ax.dim[2]; s.dimT = (int)dimT;
    s.nChunks = (int)((dimT + dpe::kAxT - 1) / dpe::kAxT);
    s.chunk = (int)((dimT + s.nChunks - 1) / s.nChunks);   // chunks of (nearly) equal length: no chunk of a few entries
    const long long rowBegin = off / dimT, rowEnd = (off + G + dimT - 1) / dimT;
    s.rowBegin = (unsigned)rowBegin; s.nRows = (unsigned)(rowEnd - rowBegin);
    s.fullBegin = (unsigned)((off + dimT - 1) / dimT); s.fullEnd = (unsigned)((off + G) / dimT);
    s.gBegin = (unsigned)off; s.G = (unsigned)G;
    *nTiles = (rowEnd - rowBegin + 255) / 256 * s.nChunks;
    return s;
}

// Several receivers over one pair of grids (dpe_bcm_update_joint)
struct JointLaunch : ScanTail {
    dpe::ScanSide sp, sv;
    const dpe::JointRxDev *rx;
    int nRx, maxRx, maxKT, lp;
    unsigned long long *ownKeys, *ownOob;
};

static void launch_joint(bool clampP, bool clampV, bool own, const JointLaunch &a)
{
    scan_dispatch(a.lp, clampP, clampV, own, [&](auto LP, auto CP, auto CV, auto OWN) {
        hipLaunchKernelGGL((dpe::bcm_scan_joint_kernel<DPE_V(LP), DPE_V(CP), DPE_V(CV), DPE_V(OWN)>), a.grid, dim3(256), a.lds, a.st, a.sp, a.sv, a.rx, a.nRx,
                           a.maxRx, a.maxKT, a.lp, a.keys, a.oob, a.ownKeys, a.ownOob, a.clr, a.clrN, a.done, a.hostKeys, a.hostOob, a.seq);
    });
}

static void allow_big_lds_joint()
{
    scan_every_variant(true, [](auto LP, auto CP, auto CV, auto OWN) { big_lds(dpe::bcm_scan_joint_kernel<DPE_V(LP), DPE_V(CP), DPE_V(CV), DPE_V(OWN)>); });
}

// N consecutive windows per score row (dpe_bcm_update_epochs)
struct EpochsLaunch : ScanTail {
    dpe::ScanSide sp, sv;
    int nEpochs, winPerPass, K, maxK, lp;
};

static void launch_epochs(bool clampP, bool clampV, const EpochsLaunch &a)
{
    scan_dispatch(a.lp, clampP, clampV, false, [&](auto LP, auto CP, auto CV, auto) {
        hipLaunchKernelGGL((dpe::bcm_scan_epochs_kernel<DPE_V(LP), DPE_V(CP), DPE_V(CV)>), a.grid, dim3(256), a.lds, a.st, a.sp, a.sv, a.nEpochs, a.winPerPass,
                           a.K, a.maxK, a.lp, a.keys, a.oob, a.clr, a.clrN, a.done, a.hostKeys, a.hostOob, a.seq);
    });
}

static void allow_big_lds_epochs()
{
    scan_every_variant(false, [](auto LP, auto CP, auto CV, auto) { big_lds(dpe::bcm_scan_epochs_kernel<DPE_V(LP), DPE_V(CP), DPE_V(CV)>); });
}

// Every SV subset's arg-max from one scan (dpe_bcm_update_subsets)
struct SubsetsLaunch : ScanTail {
    dpe::ScanSide sp, sv;
    int K, maxK, lp, nSubsets, maxSubsets;
    const unsigned long long *masks;
    unsigned long long *subKeys, *svOob;
};

static void launch_subsets(bool clampP, bool clampV, const SubsetsLaunch &a)
{
    scan_dispatch(a.lp, clampP, clampV, a.nSubsets > 0, [&](auto LP, auto CP, auto CV, auto SUBS) {
        hipLaunchKernelGGL((dpe::bcm_scan_subsets_kernel<DPE_V(LP), DPE_V(CP), DPE_V(CV), DPE_V(SUBS)>), a.grid, dim3(256), a.lds, a.st, a.sp, a.sv, a.K, a.maxK,
                           a.lp, a.masks, a.nSubsets, a.maxSubsets, a.keys, a.oob, a.subKeys, a.svOob, a.clr, a.clrN, a.done, a.hostKeys, a.hostOob, a.seq);
    });
}

static void allow_big_lds_subsets()
{
    scan_every_variant(true, [](auto LP, auto CP, auto CV, auto SUBS) { big_lds(dpe::bcm_scan_subsets_kernel<DPE_V(LP), DPE_V(CP), DPE_V(CV), DPE_V(SUBS)>); });
}

// One level of a coarse-to-fine Update (dpe_bcm_update_refine): nothing is published, so of the tail only keys, oob, clr, clrN
// and the geometry are used
struct RefineLaunch : ScanTail {
    dpe::RefineSide sp, sv;
    int level, K, maxK, lp;
    const unsigned long long *prevKeys;
    float *centres;
    const float *prevCentres;
};

static void launch_refine(bool clampP, bool clampV, const RefineLaunch &a)
{
    scan_dispatch(a.lp, clampP, clampV, false, [&](auto LP, auto CP, auto CV, auto) {
        hipLaunchKernelGGL((dpe::bcm_scan_refine_kernel<DPE_V(LP), DPE_V(CP), DPE_V(CV)>), a.grid, dim3(256), a.lds, a.st, a.sp, a.sv, a.level, a.K, a.maxK, a.lp,
                           a.keys, a.oob, a.prevKeys, a.centres, a.prevCentres, a.clr, a.clrN);
    });
}

static void allow_big_lds_refine()
{
    scan_every_variant(false, [](auto LP, auto CP, auto CV, auto) { big_lds(dpe::bcm_scan_refine_kernel<DPE_V(LP), DPE_V(CP), DPE_V(CV)>); });
}

#undef DPE_V

// ---- referencePair mode ---------------------------------------------------------------------
// The reference forms the neighbour pair as floor(idx) and floor(idx + 1) on idx = base + S k (batchcorrmanifold.cu:1797-1799).
// For k = 0 and S / 2 = 2^m an index one fp64 step below 2^m has idx + 1 rounding UP to 2^m + 1: the neighbours are two apart and
// both weights ~1, so the pair contributes c[n+1] + c[n-1] instead of ~c[n].  Because the reference's rxTime - pr / C rounds at
// 1.4e-4 samples, every grid point within that distance of the centre lag collapses onto the same fp64 value.  This pass finds
// those points (cheap fp64 prefilter on the first channel, then the reference's own expression), evaluates their scores exactly
// as :1760-1816 do, patches the score array and re-derives the arg-max from it.
#pragma clang fp contract(off)
static bool ref_pair_index(const dpe_bcm_window &win, const dpe_chan_end &ch, const double *g, double fs, int S, int k,
                           double *idxOut, double *fiOut, double *ciOut)
{
    using namespace dpe;
    const double *R = win.enu2ecef, *c = win.xCurrkk1, *s = ch.satState;
    const double px = R[0] * g[0] + R[1] * g[1] + R[2] * g[2] + c[0];        // :1760-1763
    const double py = R[3] * g[0] + R[4] * g[1] + R[5] * g[2] + c[1];
    const double pz = R[6] * g[0] + R[7] * g[1] + R[8] * g[2] + c[2];
    const double pdt = g[3] + c[3];
    const double lx = s[0] - px, ly = s[1] - py, lz = s[2] - pz;            // :1779-1781
    const double range = std::sqrt(lx * lx + ly * ly + lz * lz);            // :1782
    const double pr = range - kC * s[3] + pdt;                              // :1783
    const double txT = win.rxTime - pr / kC;                                // :1784
    const double cfd = txT - ch.cpRefTOW - ((ch.cpElapsedEnd - ch.cpRef) * kTCA);
    const double rcbc = cfd * kFCA;                                         // :1786
    const double rc0 = rcbc - ch.codePhaseEnd;                              // :1790
    const double base = (fs / ch.codeFrequency) * (-rc0) + S / 2.0;         // :1791
    if (!(base < S && base > 0)) return false;                              // :1795
    const double idx = base + ((double)S * k);                              // :1797
    *idxOut = idx;
    *fiOut = std::floor(idx);                                               // :1798
    *ciOut = std::floor(idx + 1);                                           // :1799
    return true;
}

static int ref_pair_fixup(dpe_bcm *h, const float *codeBank_dev, int nWindows, int nChan, const dpe_chan_end *chan_host,
                          unsigned long long *keys_d, hipStream_t stream)
{
    using namespace dpe;
    const int S = h->cfg.samplesPerWindow, L = h->cfg.lagHalfWidth, nLag = 2 * L + 1;
    const int maxK = h->cfg.maxChannels, W = h->cfg.maxWindows;
    const long long G = h->cfg.posGridSize;
    const double fs = h->cfg.samplingFrequency;
    h->refPatched = 0;
    h->refWsum.assign((size_t)nWindows * 5, 0.0);
    // ---- 1. candidates, on the device: one pass over the grid per window instead of W x G fp64 iterations on the host.
    // The coefficients of this Update are in sv_d for batches; a single window passed them as kernel arguments: upload.
    if (nWindows == 1) DPE_CHECK_HIP(hipMemcpyAsync(h->sv_d, h->sv_h, sizeof(BcmSvDev) * maxK, hipMemcpyHostToDevice, stream));
    std::vector<unsigned long long> cand;
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (!h->refCand_d) {
            if (h->refCap == 0) h->refCap = 1 << 16;
            h->refCand_d = dev_alloc<unsigned long long>(1 + h->refCap);
            DPE_REQUIRE(h->refCand_d, "[BatchCorrManifold] Update: referencePair: candidate list allocation failed (%llu entries)", h->refCap);
        }
        DPE_CHECK_HIP(hipMemsetAsync(h->refCand_d, 0, sizeof(unsigned long long), stream));
        const unsigned gx = (unsigned)((G + 256 * 8 - 1) / (256 * 8));
        hipLaunchKernelGGL(bcm_refpair_candidates_kernel, dim3(gx > 1024 ? 1024 : gx, nWindows), dim3(256), 0, stream, h->posGrid_d, G,
                           h->sv_d, maxK, L, 5e-4, h->refCand_d, h->refCap);
        unsigned long long n = 0;
        DPE_CHECK_HIP(hipMemcpyAsync(&n, h->refCand_d, sizeof(n), hipMemcpyDeviceToHost, stream));
        DPE_CHECK_HIP(hipStreamSynchronize(stream));
        if (n > h->refCap) {   // more candidates than the list holds: grow it and run the pass again (nothing was modified yet)
            DPE_REQUIRE(attempt == 0, "[BatchCorrManifold] Update: referencePair: candidate list overflow after growing");
            (void)hipFree(h->refCand_d);
            h->refCand_d = nullptr;
            h->refCap = n + n / 4;
            continue;
        }
        cand.resize((size_t)n);
        if (n) DPE_CHECK_HIP(hipMemcpy(cand.data(), h->refCand_d + 1, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost));
        break;
    }
    if (cand.empty()) return 0;
    std::sort(cand.begin(), cand.end());   // (the append order is not deterministic; the patches are)
    // ---- 2. the reference's own expression (:1760-1816) for the candidates, fp64 on the host
    DPE_CHECK_HIP(hipMemcpyAsync(h->refBank_h, codeBank_dev, sizeof(float2) * (size_t)nWindows * maxK * nLag, hipMemcpyDeviceToHost, stream));
    DPE_CHECK_HIP(hipStreamSynchronize(stream));
    std::vector<unsigned long long> where;
    std::vector<float> value;
    for (unsigned long long wi : cand) {
        const int w = (int)(wi >> 40);
        const long long i = (long long)(wi & ((1ull << 40) - 1));
        const dpe_bcm_window &win = h->win_h[w];
        const double *g = h->posGrid_h.data() + 4 * i;
        double idx, fi_, ci_;
        if (!ref_pair_index(win, chan_host[(size_t)w * nChan], g, fs, S, 0, &idx, &fi_, &ci_)) continue;
        if (ci_ - fi_ != 2.0) continue;                                   // the ordinary pair: the scan's value stands
        double score = 0.0;
        for (int k = 0; k < nChan; ++k) {
            if (!ref_pair_index(win, chan_host[(size_t)w * nChan + k], g, fs, S, k, &idx, &fi_, &ci_)) continue;
            const long long fin = (long long)fi_ - (long long)S * k - (S / 2 - L);
            const long long cin = (long long)ci_ - (long long)S * k - (S / 2 - L);
            if (fin < 0 || cin < 0 || fin >= nLag || cin >= nLag) continue;
            const float2 *row = h->refBank_h + ((size_t)w * maxK + k) * nLag;
            const double wc = idx - fi_, wf = ci_ - idx;                 // :1810-1811
            const double vr = (double)row[cin].x * wc + (double)row[fin].x * wf;
            const double vi = (double)row[cin].y * wc + (double)row[fin].y * wf;
            score += std::pow(std::hypot(vr, vi), (double)h->cfg.lPower); // :1816
        }
        where.push_back(wi);
        value.push_back((float)score);
    }
    h->refPatched = (long long)where.size();
    if (where.empty()) return 0;
    // ---- 3. one upload, one scatter launch (the buffers grow with the patch count: no fixed limit)
    const size_t n = where.size();
    if (n > h->refPatchCap) {
        (void)hipFree(h->refWhere_d); (void)hipFree(h->refValue_d); (void)hipFree(h->refOld_d);
        h->refPatchCap = n + n / 4 + 256;
        h->refWhere_d = dev_alloc<unsigned long long>(h->refPatchCap);
        h->refValue_d = dev_alloc<float>(h->refPatchCap);
        h->refOld_d = dev_alloc<float>(h->refPatchCap);
        if (!h->refWhere_d || !h->refValue_d || !h->refOld_d) {
            h->refPatchCap = 0;
            set_error("[BatchCorrManifold] Update: referencePair: patch buffers (%zu entries) allocation failed; the published scores are the scan's, unpatched", n);
            return -1;
        }
    }
    DPE_CHECK_HIP(hipMemcpyAsync(h->refWhere_d, where.data(), sizeof(unsigned long long) * n, hipMemcpyHostToDevice, stream));
    DPE_CHECK_HIP(hipMemcpyAsync(h->refValue_d, value.data(), sizeof(float) * n, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(bcm_patch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, h->posScores_d, h->posPitch, h->refWhere_d,
                       h->refValue_d, h->refOld_d, (int)n);
    if (h->cfg.weightedMean) {
        std::vector<float> old(n);
        DPE_CHECK_HIP(hipMemcpyAsync(old.data(), h->refOld_d, sizeof(float) * n, hipMemcpyDeviceToHost, stream));
        DPE_CHECK_HIP(hipStreamSynchronize(stream));
        for (size_t j = 0; j < n; ++j) {
            const int w = (int)(where[j] >> 40);
            const double *g = h->posGrid_h.data() + 4 * (long long)(where[j] & ((1ull << 40) - 1));
            const double d = (double)value[j] - (double)old[j];
            double *c = h->refWsum.data() + (size_t)w * 5;
            c[0] += d; c[1] += d * g[0]; c[2] += d * g[1]; c[3] += d * g[2]; c[4] += d * g[3];
        }
    }
    // ---- 4. arg-max from the patched scores
    hipLaunchKernelGGL(bcm_zero_pos_keys_kernel, dim3((nWindows + 63) / 64), dim3(64), 0, stream, keys_d, nWindows);
    const unsigned gx = (unsigned)((G + 256 * 16 - 1) / (256 * 16));
    hipLaunchKernelGGL(bcm_rekey_kernel, dim3(gx > 512 ? 512 : gx, nWindows), dim3(256), 0, stream, h->posScores_d, G, h->posPitch,
                       (long long)h->cfg.posGridIndexOffset, keys_d);
    DPE_CHECK_HIP(hipMemcpyAsync(h->keys_h, keys_d, sizeof(unsigned long long) * 2 * (size_t)nWindows, hipMemcpyDeviceToHost, stream));
    DPE_CHECK_HIP(hipStreamSynchronize(stream));
    return 0;
}

// ---- host pieces the entry points of the six handle kinds share: plain functions, each written once; `who`
// is the entry point's name as its messages spell it ------------------------------------------------
static size_t sv_stride(const dpe_bcm *h)   // channels per window of sv_d / sv_h
{
    return h->joint ? (size_t)h->jointMaxK : (size_t)h->cfg.maxChannels;
}

static size_t sv_bytes(const dpe_bcm *h)   // both manifolds' coefficient blocks, [2][W][stride]
{
    return sizeof(dpe::BcmSvDev) * 2 * (size_t)h->cfg.maxWindows * sv_stride(h);
}

static size_t n_ent_max(const dpe_bcm_config &cfg)   // entries of the longer of a channel's two score banks: a bank row in LDS
{
    return (size_t)(2 * (cfg.lagHalfWidth > cfg.binHalfWidth ? cfg.lagHalfWidth : cfg.binHalfWidth) + 1);
}

static size_t lds_per_channel(const dpe_bcm_config &cfg)   // the LDS budget rule of dpe_bcm_config: 16-byte entries + 32 B
{
    return n_ent_max(cfg) * 16 + 32;
}

static int check_max_counts(const dpe_bcm_config *cfg, const char *who)
{
    DPE_REQUIRE(cfg->maxWindows >= 1 && cfg->maxChannels >= 1 && cfg->maxChannels <= DPE_MAX_CHAN,
                "[BatchCorrManifold] %s: maxWindows/maxChannels out of range", who);
    return 0;
}

static int check_cfg(const dpe_bcm_config *cfg, const char *who)
{
    DPE_REQUIRE(cfg->samplesPerWindow > 0 && (cfg->samplesPerWindow % 2) == 0, "[BatchCorrManifold] %s: samplesPerWindow must be even and positive", who);
    DPE_REQUIRE(cfg->samplingFrequency > 0 && cfg->numFFTPoints > 0, "[BatchCorrManifold] %s: bad fs / numFFTPoints", who);
    if (check_max_counts(cfg, who)) return -1;
    DPE_REQUIRE(cfg->lagHalfWidth >= 1 && cfg->binHalfWidth >= 1 && cfg->lPower >= 1, "[BatchCorrManifold] %s: bad L/B/LPower", who);
    return 0;
}

static int check_no_shards(const dpe_bcm_config *cfg, const char *who)
{
    DPE_REQUIRE(cfg->posGridIndexOffset == 0 && cfg->velGridIndexOffset == 0,
                "[BatchCorrManifold] %s: grid shards are not supported (the index offsets must be 0)", who);
    return 0;
}

static int check_axes_lds(const dpe_bcm_config *cfg, const char *who)   // grid axes: the banks share the LDS with the score stage
{
    DPE_REQUIRE((size_t)cfg->maxChannels * lds_per_channel(*cfg) + (size_t)dpe::kAxStageBytes <= 150 * 1024,
                "[BatchCorrManifold] %s: score banks (%zu B) and the score stage (%d B) exceed the LDS (no 12-byte bank entries with grid axes)", who,
                (size_t)cfg->maxChannels * n_ent_max(*cfg) * 16, dpe::kAxStageBytes);
    return 0;
}

// One manifold's four axes: dimension >= 1 with an array, finite entries, a product that fits 32 bits.  mx[c] comes back as the
// largest |entry| of axis c, *prod as the number of points; `level` is "" or the "level %d " of the messages.
static int check_axes(const char *who, const char *level, const char *name, const dpe_grid_axes *ga, double mx[4], int64_t *prod)
{
    *prod = 1;
    for (int c = 0; c < 4; ++c) {
        mx[c] = 0;
        DPE_REQUIRE(ga->dim[c] >= 1 && ga->axis[c], "[BatchCorrManifold] %s: %s%s axis %d: dim %d < 1 or no array", who, level, name, c, ga->dim[c]);
        for (int i = 0; i < ga->dim[c]; ++i) {
            const double v = ga->axis[c][i];
            DPE_REQUIRE(std::isfinite(v), "[BatchCorrManifold] %s: %s%s axis %d entry %d is not finite", who, level, name, c, i);
            mx[c] = std::max(mx[c], std::fabs(v));
        }
        DPE_REQUIRE(*prod <= 0xFFFFFFFFll / ga->dim[c], "[BatchCorrManifold] %s: %s%s grid index does not fit 32 bits", who, level, name);
        *prod *= ga->dim[c];
    }
    return 0;
}

// The buffers every handle has, whatever holds its grids (create and create_axes)
static int bcm_finish_create(dpe_bcm *h, const dpe_bcm_config *cfg, dpe_bcm **out)
{
    using namespace dpe;
    const size_t W = cfg->maxWindows, K = sv_stride(h);
    // score rows start on 128-byte lines: a wave's 64 consecutive scores are then two whole lines instead of one whole and two
    // partial ones (config R, 390 625-point rows: 0.779 -> 0.755 ms per step, the write-back of a step's 0.8 GB drains faster)
    h->posPitch = (cfg->posGridSize + 31) / 32 * 32;
    h->velPitch = (cfg->velGridSize + 31) / 32 * 32;
    if (cfg->writeScores) {
        h->posScores_d = dev_alloc<float>(W * (size_t)h->posPitch);
        h->velScores_d = dev_alloc<float>(W * (size_t)h->velPitch);
    }
    h->sv_d = dev_alloc<BcmSvDev>(2 * W * K);
    h->keys_d = dev_alloc<unsigned long long>(8 * W);   // two alternating sets of {keys [W][2], out-of-window counts [W][2]}
    h->wsumHalf = (size_t)(dpe_bcm::kMaxSplit + 8 * W) * 5;   // >= nWindows * blocks-per-window of any launch
    h->wsum_d = dev_alloc<double>(2 * h->wsumHalf);
    if ((cfg->writeScores && (!h->posScores_d || !h->velScores_d)) || !h->sv_d || !h->keys_d || !h->wsum_d ||
        hipHostMalloc((void **)&h->svBase_h, dpe_bcm::kStaging * 2 * W * K * sizeof(BcmSvDev), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void **)&h->devWin_h, 2 * sizeof(BcmDevWin), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void **)&h->keys_h, (4 * W + 8) * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess) {
        set_error("[BatchCorrManifold] create: device allocation failed");
        dpe_bcm_destroy(h);
        return -1;
    }
    // dynamic LDS above 64 KB needs the opt-in attribute
    allow_big_lds_scan();
    if (h->refPair &&
        hipHostMalloc((void **)&h->refBank_h, W * K * (size_t)(2 * cfg->lagHalfWidth + 1) * sizeof(float2), hipHostMallocDefault) != hipSuccess) {
        set_error("[BatchCorrManifold] create: host allocation failed");
        dpe_bcm_destroy(h);
        return -1;
    }
    h->oob_h = h->keys_h + 2 * W;
    for (size_t i = 0; i < 4 * W + 8; ++i) h->keys_h[i] = 0ull;
    h->pollAllowed = getenv("DPE_BCM_NO_POLL") == nullptr;
#ifdef DPE_EXPERIMENTS
    if (const char *e = getenv("DPE_BCM_SPLIT")) h->splitForce = atoi(e) > 0 && atoi(e) <= (int)dpe_bcm::kMaxSplit ? atoi(e) : 0;
#endif
    h->sv_h = h->svBase_h;
    const auto finish = [&]() -> int {   // a failure from here on must not leak the handle
        for (hipEvent_t &e : h->stagingFree) DPE_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        DPE_CHECK_HIP(hipMemset(h->keys_d, 0, 8 * W * sizeof(unsigned long long)));
        h->done_d = dev_alloc<unsigned int>(1);
        DPE_REQUIRE(h->done_d, "[BatchCorrManifold] create: device allocation failed");
        DPE_CHECK_HIP(hipMemset(h->done_d, 0, sizeof(unsigned int)));
        DPE_CHECK_HIP(hipHostGetDevicePointer((void **)&h->keys_hd, h->keys_h, 0));
        DPE_CHECK_HIP(hipHostGetDevicePointer((void **)&h->svBase_hd, h->svBase_h, 0));
        DPE_CHECK_HIP(hipHostGetDevicePointer((void **)&h->devWin_hd, h->devWin_h, 0));
        return 0;
    };
    if (finish()) {
        dpe_bcm_destroy(h);
        return -1;
    }
    h->win_h.resize(W);
    *out = h;
    return 0;
}

// Point-list grids.  maxRx > 0: a handle that scans several receivers per window (dpe_bcm_create_joint) -- cfg->maxChannels is
// then the bound per receiver, maxKTotal the bound on the (receiver, SV) pairs of a window, which is what the LDS holds.
static int bcm_create_points(const dpe_bcm_config *cfg, dpe_bcm *donor, int maxRx, int maxKTotal, dpe_bcm **out)
{
    using namespace dpe;
    DPE_REQUIRE(cfg && out, "[BatchCorrManifold] create: null argument");
    const bool joint = maxRx > 0;
    const int ldsChannels = joint ? maxKTotal : cfg->maxChannels;
    DPE_REQUIRE(!donor || ((int64_t)donor->posGrid_h.size() == 4 * cfg->posGridSize && (int64_t)donor->velGrid_h.size() == 4 * cfg->velGridSize &&
                           !donor->gridsBorrowed), "[BatchCorrManifold] create: the grids to share are not these grids");
    if (check_cfg(cfg, "create")) return -1;
    DPE_REQUIRE(cfg->posGrid && cfg->velGrid && cfg->posGridSize > 0 && cfg->velGridSize > 0,
                "[BatchCorrManifold] create: grids missing");
    DPE_REQUIRE(cfg->posGridSize + cfg->posGridIndexOffset < 0xFFFFFFFFll &&
                cfg->velGridSize + cfg->velGridIndexOffset < 0xFFFFFFFFll,
                "[BatchCorrManifold] create: global grid index exceeds 32 bits");
    const size_t nEntMax = n_ent_max(*cfg), ldsNeed = (size_t)ldsChannels * lds_per_channel(*cfg);
    const bool compact = ldsNeed > 150 * 1024;   // 12-byte entries (slower scan variant) when the 16-byte ones do not fit
    DPE_REQUIRE(!joint || !compact, "[BatchCorrManifold] create_joint: the score banks of %d (receiver, SV) pairs x %zu entries (%zu B) exceed the "
                                    "150 KB the joint scan keeps in LDS", ldsChannels, nEntMax, ldsNeed);
    DPE_REQUIRE(!compact || (size_t)cfg->maxChannels * nEntMax * 12 <= 152 * 1024,
                "[BatchCorrManifold] create: score banks (%zu B even as 12-byte entries) exceed the 160 KB LDS",
                (size_t)cfg->maxChannels * nEntMax * 12);
    // validity of the range expansion (file header): |delta| must stay far below the SV range
    double maxR2 = 0, posExt = 0, velExt = 0;   // extents: max(|delta_xyz| + |delta_t|), bounds |delta_t - u.delta|
    for (int64_t i = 0; i < cfg->posGridSize; ++i) {
        const double *p = cfg->posGrid + 4 * i;
        const double r2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
        if (r2 > maxR2) maxR2 = r2;
        const double e = std::sqrt(r2) + std::fabs(p[3]);
        if (e > posExt) posExt = e;
    }
    for (int64_t i = 0; i < cfg->velGridSize; ++i) {
        const double *p = cfg->velGrid + 4 * i;
        const double e = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]) + std::fabs(p[3]);
        if (e > velExt) velExt = e;
    }
    DPE_REQUIRE(maxR2 < 3.0e3 * 3.0e3, "[BatchCorrManifold] create: position grid extends beyond 3 km from its centre");
    dpe_bcm *h = new dpe_bcm();
    h->cfg = *cfg;
    h->cfg.posGrid = h->cfg.velGrid = nullptr;
    h->compact = compact;
    h->joint = joint; h->jointMaxRx = maxRx; h->jointMaxK = maxKTotal;
    {
        const int half = cfg->samplesPerWindow / 2;
        h->refPair = cfg->referencePair != 0 && (half & (half - 1)) == 0;   // only then can floor(idx + 1) - floor(idx) be 2
        if (cfg->referencePair && !cfg->writeScores) {
            set_error("[BatchCorrManifold] create: referencePair needs writeScores (the arg-max is re-derived from the patched scores)");
            delete h;
            return -1;
        }
    }
    h->posExtent = posExt * 1.000001 + maxR2 / 2.0e7 + 1e-3;   // + second-order term bound (range > 2e7 m) + fp32 slack
    h->velExtent = velExt * 1.000001 + 1e-6;
    if (donor) {      // a further lane of a dpe_pipe: the same grids, one device copy
        h->posGrid_h = donor->posGrid_h; h->velGrid_h = donor->velGrid_h;
        h->posGrid_d = donor->posGrid_d; h->velGrid_d = donor->velGrid_d;
        h->gridsBorrowed = true;
    } else if (upload_grid(cfg->posGrid, cfg->posGridSize, h->posGrid_h, &h->posGrid_d) ||
               upload_grid(cfg->velGrid, cfg->velGridSize, h->velGrid_h, &h->velGrid_d)) {
        dpe_bcm_destroy(h);
        return -1;
    }
    return bcm_finish_create(h, cfg, out);
}

extern "C" {

int dpe_bcm_create(const dpe_bcm_config *cfg, dpe_bcm **out)
{
    return bcm_create_points(cfg, nullptr, 0, 0, out);
}

// donor != nullptr: a handle for the same configuration and grids as `donor` (a further lane of a dpe_pipe) that uses donor's device
// copy of the fp32 grids; donor must outlive it.
int dpe_bcm_create_sharing(const dpe_bcm_config *cfg, dpe_bcm *donor, dpe_bcm **out)
{
    return bcm_create_points(cfg, donor, 0, 0, out);
}

int dpe_bcm_create_joint(const dpe_bcm_config *cfg, int32_t maxRx, int32_t maxChannelsTotal, dpe_bcm **out)
{
    using namespace dpe;
    DPE_REQUIRE(cfg && out, "[BatchCorrManifold] create_joint: null argument");
    DPE_REQUIRE(maxRx >= 1 && maxRx <= kJointMaxRx, "[BatchCorrManifold] create_joint: maxRx %d out of range (1 .. %d receivers)", maxRx, kJointMaxRx);
    DPE_REQUIRE(maxChannelsTotal >= 1 && maxChannelsTotal <= kJointMaxK,
                "[BatchCorrManifold] create_joint: maxChannelsTotal %d out of range (1 .. %d (receiver, SV) pairs)", maxChannelsTotal, kJointMaxK);
    DPE_REQUIRE(cfg->maxChannels <= maxChannelsTotal, "[BatchCorrManifold] create_joint: maxChannels %d (the bound per receiver) exceeds maxChannelsTotal %d",
                cfg->maxChannels, maxChannelsTotal);
    DPE_REQUIRE(!cfg->weightedMean, "[BatchCorrManifold] create_joint: the weighted-mean estimator is not formed for several receivers (weightedMean must be 0)");
    DPE_REQUIRE(!cfg->referencePair, "[BatchCorrManifold] create_joint: referencePair is a single-receiver mode (it re-evaluates one receiver's first channel)");
    if (check_no_shards(cfg, "create_joint")) return -1;
    dpe_bcm *h = nullptr;
    if (bcm_create_points(cfg, nullptr, maxRx, maxChannelsTotal, &h)) return -1;
    const size_t W = cfg->maxWindows, n = W * (size_t)maxRx;
    const auto finish = [&]() -> int {
        h->jrx_d = dev_alloc<JointRxDev>(n);
        h->own_d = dev_alloc<unsigned long long>(4 * n);
        DPE_REQUIRE(h->jrx_d && h->own_d, "[BatchCorrManifold] create_joint: device allocation failed");
        DPE_CHECK_HIP(hipHostMalloc((void **)&h->jrxBase_h, dpe_bcm::kStaging * n * sizeof(JointRxDev), hipHostMallocDefault));
        return 0;
    };
    if (finish()) {
        dpe_bcm_destroy(h);
        return -1;
    }
    h->own_h.assign(4 * n, 0ull);
    h->jwin_h.resize(n);
    allow_big_lds_joint();
    *out = h;
    return 0;
}

// N consecutive windows per score row and arg-max (dpe_bcm_epochs.h).  The LDS budget rule of dpe_bcm_config bounds the (window, SV)
// pairs of ONE PASS; a group of any length up to maxEpochs is scanned in as many passes as that takes.
int dpe_bcm_create_epochs(const dpe_bcm_config *cfg, int32_t maxEpochs, int32_t pairsPerPass, dpe_bcm **out)
{
    using namespace dpe;
    DPE_REQUIRE(cfg && out, "[BatchCorrManifold] create_epochs: null argument");
    if (check_max_counts(cfg, "create_epochs")) return -1;
    DPE_REQUIRE(maxEpochs >= 1 && maxEpochs <= cfg->maxWindows, "[BatchCorrManifold] create_epochs: maxEpochs %d out of range (1 .. maxWindows = %d)",
                maxEpochs, cfg->maxWindows);
    DPE_REQUIRE(cfg->lagHalfWidth >= 1 && cfg->binHalfWidth >= 1, "[BatchCorrManifold] create_epochs: bad L/B");
    DPE_REQUIRE(!cfg->weightedMean, "[BatchCorrManifold] create_epochs: the weighted-mean estimator is not formed for summed windows (weightedMean must be 0)");
    DPE_REQUIRE(!cfg->referencePair, "[BatchCorrManifold] create_epochs: referencePair is a single-window mode (it re-evaluates one window's first channel)");
    if (check_no_shards(cfg, "create_epochs")) return -1;
    const size_t budget = (size_t)150 * 1024 / lds_per_channel(*cfg);   // pairs * ((2 max(L, B) + 1) * 16 + 32) <= 150 KB
    DPE_REQUIRE(budget >= (size_t)cfg->maxChannels, "[BatchCorrManifold] create_epochs: the score banks of one window (%d channels x %zu entries, %zu B) exceed "
                                                    "the 150 KB the epochs scan keeps in LDS (no 12-byte bank entries here)",
                cfg->maxChannels, n_ent_max(*cfg), (size_t)cfg->maxChannels * lds_per_channel(*cfg));
    DPE_REQUIRE(pairsPerPass == 0 || pairsPerPass >= cfg->maxChannels,
                "[BatchCorrManifold] create_epochs: pairsPerPass %d is below maxChannels %d (a pass holds whole windows; 0 = as many as the LDS holds)",
                pairsPerPass, cfg->maxChannels);
    dpe_bcm_config c = *cfg;
    c.writeScores = 1;   // the score row is the accumulator
    dpe_bcm *h = nullptr;
    if (bcm_create_points(&c, nullptr, 0, 0, &h)) return -1;
    h->epochs = true;
    h->epMaxEpochs = maxEpochs;
    h->epPairsPerPass = (pairsPerPass > 0 && (size_t)pairsPerPass < budget) ? pairsPerPass : (int)budget;
    allow_big_lds_epochs();
    *out = h;
    return 0;
}

// One scan, the arg-max of every SV subset (dpe_bcm_subsets.h).  The masks, the subset keys and the per-SV out-of-window counts
// live in one device block beside the handle's ordinary key sets.
int dpe_bcm_create_subsets(const dpe_bcm_config *cfg, int32_t maxSubsets, dpe_bcm **out)
{
    using namespace dpe;
    DPE_REQUIRE(cfg && out, "[BatchCorrManifold] create_subsets: null argument");
    DPE_REQUIRE(maxSubsets >= 1 && maxSubsets <= kSubsetMax, "[BatchCorrManifold] create_subsets: maxSubsets %d out of range (1 .. %d subsets per window)",
                maxSubsets, kSubsetMax);
    if (check_max_counts(cfg, "create_subsets")) return -1;
    DPE_REQUIRE(cfg->lagHalfWidth >= 1 && cfg->binHalfWidth >= 1, "[BatchCorrManifold] create_subsets: bad L/B");
    DPE_REQUIRE(!cfg->weightedMean, "[BatchCorrManifold] create_subsets: the weighted-mean estimator is not formed per subset (weightedMean must be 0)");
    DPE_REQUIRE(!cfg->referencePair, "[BatchCorrManifold] create_subsets: referencePair re-evaluates the full set only (referencePair must be 0)");
    if (check_no_shards(cfg, "create_subsets")) return -1;
    const size_t ldsNeed = (size_t)cfg->maxChannels * lds_per_channel(*cfg);
    DPE_REQUIRE(ldsNeed <= 150 * 1024, "[BatchCorrManifold] create_subsets: the score banks of %d channels x %zu entries (%zu B) exceed the 150 KB the "
                                       "subsets scan keeps in LDS (no 12-byte bank entries here)", cfg->maxChannels, n_ent_max(*cfg), ldsNeed);
    dpe_bcm *h = nullptr;
    if (bcm_create_points(cfg, nullptr, 0, 0, &h)) return -1;
    const size_t W = cfg->maxWindows, n = W * (size_t)maxSubsets + 2 * W * (size_t)maxSubsets + 2 * W * (size_t)cfg->maxChannels;
    const auto finish = [&]() -> int {
        h->sub_d = dev_alloc<unsigned long long>(n);
        DPE_REQUIRE(h->sub_d, "[BatchCorrManifold] create_subsets: device allocation failed");
        DPE_CHECK_HIP(hipHostMalloc((void **)&h->subMaskBase_h, dpe_bcm::kStaging * W * (size_t)maxSubsets * sizeof(unsigned long long), hipHostMallocDefault));
        return 0;
    };
    if (finish()) {
        dpe_bcm_destroy(h);
        return -1;
    }
    h->subsets = true;
    h->subMax = maxSubsets;
    h->sub_h.assign(n, 0ull);
    h->subMask_h.assign(W * (size_t)maxSubsets, 0ull);
    allow_big_lds_subsets();
    *out = h;
    return 0;
}

// Grids given by their axes.  donor != nullptr: a further lane of a dpe_pipe, which uses donor's device copy of the axes.
int dpe_bcm_create_axes_sharing(const dpe_bcm_config *cfg, const dpe_grid_axes *pos, const dpe_grid_axes *vel, dpe_bcm *donor,
                                dpe_bcm **out)
{
    using namespace dpe;
    DPE_REQUIRE(cfg && pos && vel && out, "[BatchCorrManifold] create_axes: null argument");
    DPE_REQUIRE(!cfg->posGrid && !cfg->velGrid, "[BatchCorrManifold] create_axes: posGrid / velGrid must be NULL (the grids are the axes)");
    DPE_REQUIRE(!cfg->referencePair, "[BatchCorrManifold] create_axes: referencePair is not supported with grid axes");
    if (check_cfg(cfg, "create_axes") || check_axes_lds(cfg, "create_axes")) return -1;
    const dpe_grid_axes *ga[2] = {pos, vel};
    const int64_t size[2] = {cfg->posGridSize, cfg->velGridSize}, offset[2] = {cfg->posGridIndexOffset, cfg->velGridIndexOffset};
    double ext[2], r2[2];
    for (int m = 0; m < 2; ++m) {
        const char *name = m ? "velocity" : "position";
        double mx[4];
        int64_t prod;
        if (check_axes("create_axes", "", name, ga[m], mx, &prod)) return -1;
        DPE_REQUIRE(size[m] > 0 && offset[m] >= 0 && offset[m] + size[m] <= prod,
                    "[BatchCorrManifold] create_axes: %s slice [%lld, %lld) beyond the axis product %lld", name, (long long)offset[m],
                    (long long)(offset[m] + size[m]), (long long)prod);
        // every index the scan forms, including those of the lanes that run past the slice's last row, fits 32 bits
        const int64_t dimT = ga[m]->dim[3], rowEnd = (offset[m] + size[m] + dimT - 1) / dimT;
        DPE_REQUIRE((rowEnd + 256) * dimT + kAxT < 0xFFFFFFFFll, "[BatchCorrManifold] create_axes: %s grid index does not fit 32 bits", name);
        r2[m] = mx[0] * mx[0] + mx[1] * mx[1] + mx[2] * mx[2];
        ext[m] = std::sqrt(r2[m]) + mx[3];   // bounds |delta_t| + |delta_xyz| over the grid, as the point-list extents
    }
    DPE_REQUIRE(r2[0] < 3.0e3 * 3.0e3, "[BatchCorrManifold] create_axes: position grid extends beyond 3 km from its centre");
    dpe_bcm *h = new dpe_bcm();
    h->cfg = *cfg;
    h->axes = true;
    h->posExtent = ext[0] * 1.000001 + r2[0] / 2.0e7 + 1e-3;
    h->velExtent = ext[1] * 1.000001 + 1e-6;
    dpe_bcm::Axes *ax[2] = {&h->posAx, &h->velAx};
    size_t nf = 0;
    for (int m = 0; m < 2; ++m)
        for (int c = 0; c < 4; ++c) {
            ax[m]->dim[c] = ga[m]->dim[c];
            ax[m]->v[c].assign(ga[m]->axis[c], ga[m]->axis[c] + ga[m]->dim[c]);
            h->axOff[m][c] = (int)nf;
            nf += (size_t)ga[m]->dim[c] + (c == 3 ? kAxT : 0);
        }
    if (donor) {
        DPE_REQUIRE(donor->axes && !donor->axesBorrowed, "[BatchCorrManifold] create: the grids to share are not these grids");
        h->axes_d = donor->axes_d;
        h->axesBorrowed = true;
    } else {
        std::vector<float> f(nf, 0.f);
        for (int m = 0; m < 2; ++m)
            for (int c = 0; c < 4; ++c)
                for (int i = 0; i < ax[m]->dim[c]; ++i) f[(size_t)h->axOff[m][c] + i] = (float)ax[m]->v[c][i];
        h->axes_d = dev_alloc<float>(nf);
        if (!h->axes_d) {
            set_error("[BatchCorrManifold] create_axes: device allocation failed");
            dpe_bcm_destroy(h);
            return -1;
        }
        if (hipMemcpy(h->axes_d, f.data(), sizeof(float) * nf, hipMemcpyHostToDevice) != hipSuccess) {
            set_error("[BatchCorrManifold] create_axes: axes upload failed");
            dpe_bcm_destroy(h);
            return -1;
        }
    }
    allow_big_lds_axes();
    return bcm_finish_create(h, cfg, out);
}

int dpe_bcm_create_axes(const dpe_bcm_config *cfg, const dpe_grid_axes *pos, const dpe_grid_axes *vel, dpe_bcm **out)
{
    return dpe_bcm_create_axes_sharing(cfg, pos, vel, nullptr, out);
}

// Coarse-to-fine levels (dpe_bcm_refine.h): every level's axes in one device block, per-level score rows, two alternating sets of
// per-level keys and counts, and the fp32 centres the levels hand on.
int dpe_bcm_create_refine(const dpe_bcm_config *cfg, int32_t nLevels, const dpe_grid_axes *pos, const dpe_grid_axes *vel, dpe_bcm **out)
{
    using namespace dpe;
    DPE_REQUIRE(cfg && pos && vel && out, "[BatchCorrManifold] create_refine: null argument");
    DPE_REQUIRE(nLevels >= 1 && nLevels <= DPE_REFINE_MAX_LEVELS, "[BatchCorrManifold] create_refine: nLevels %d out of range (1 .. %d levels)", nLevels,
                DPE_REFINE_MAX_LEVELS);
    DPE_REQUIRE(!cfg->posGrid && !cfg->velGrid, "[BatchCorrManifold] create_refine: posGrid / velGrid must be NULL (the grids are the levels' axes)");
    DPE_REQUIRE(!cfg->weightedMean, "[BatchCorrManifold] create_refine: the weighted-mean estimator is not formed per level (weightedMean must be 0)");
    DPE_REQUIRE(!cfg->referencePair, "[BatchCorrManifold] create_refine: referencePair is not supported with grid axes (referencePair must be 0)");
    if (check_no_shards(cfg, "create_refine") || check_cfg(cfg, "create_refine") || check_axes_lds(cfg, "create_refine")) return -1;
    // the reach of a chain of levels: a point is a sum of one entry per level, so per-level corner distances and |t| maxima add up
    double corner[2] = {0, 0}, tmax[2] = {0, 0};
    for (int l = 0; l < nLevels; ++l) {
        const dpe_grid_axes *ga[2] = {pos + l, vel + l};
        char level[24];
        snprintf(level, sizeof(level), "level %d ", l);
        for (int m = 0; m < 2; ++m) {
            const char *name = m ? "velocity" : "position";
            double mx[4];
            int64_t prod;
            if (check_axes("create_refine", level, name, ga[m], mx, &prod)) return -1;
            // every index the scan forms, including those of the lanes that run past the last row, fits 32 bits
            const int64_t dimT = ga[m]->dim[3];
            DPE_REQUIRE((prod / dimT + 256) * dimT + kAxT < 0xFFFFFFFFll, "[BatchCorrManifold] create_refine: level %d %s grid index does not fit 32 bits", l,
                        name);
            corner[m] += std::sqrt(mx[0] * mx[0] + mx[1] * mx[1] + mx[2] * mx[2]);
            tmax[m] += mx[3];
        }
    }
    DPE_REQUIRE(corner[0] < 3.0e3, "[BatchCorrManifold] create_refine: the levels' position grids together extend beyond 3 km from the window centre "
                                   "(sum of the corner distances %.1f m)", corner[0]);
    dpe_bcm *h = new dpe_bcm();
    h->cfg = *cfg;
    h->refine = true;
    h->rfLevels = nLevels;
    // (the fp32 roundings of the centres, a few ulp of a kilometre, are inside the slack terms)
    h->posExtent = (corner[0] + tmax[0]) * 1.000001 + corner[0] * corner[0] / 2.0e7 + 1e-3;
    h->velExtent = (corner[1] + tmax[1]) * 1.000001 + 1e-6;
    size_t nf = 0;
    for (int l = 0; l < nLevels; ++l) {
        dpe_bcm::RefineLevel &lv = h->rf[l];
        const dpe_grid_axes *ga[2] = {pos + l, vel + l};
        for (int m = 0; m < 2; ++m) {
            lv.G[m] = 1;
            for (int c = 0; c < 4; ++c) {
                lv.dim[m][c] = ga[m]->dim[c];
                lv.v[m][c].resize((size_t)ga[m]->dim[c]);
                for (int i = 0; i < ga[m]->dim[c]; ++i) lv.v[m][c][(size_t)i] = (float)ga[m]->axis[c][i];
                lv.off[m][c] = (int)nf;
                nf += (size_t)ga[m]->dim[c] + (c == 3 ? kAxT : 0);
                lv.G[m] *= ga[m]->dim[c];
            }
            lv.pitch[m] = (lv.G[m] + 31) / 32 * 32;
        }
    }
    dpe_bcm_config c = *cfg;
    c.writeScores = 0;   // (the rows are per level: allocated below)
    c.posGridSize = h->rf[nLevels - 1].G[0];
    c.velGridSize = h->rf[nLevels - 1].G[1];
    h->cfg.posGridSize = c.posGridSize; h->cfg.velGridSize = c.velGridSize;
    dpe_bcm *made = nullptr;
    if (bcm_finish_create(h, &c, &made)) return -1;   // (h is destroyed on failure)
    const size_t W = cfg->maxWindows;
    const auto finish = [&]() -> int {
        std::vector<float> f(nf, 0.f);
        for (int l = 0; l < nLevels; ++l)
            for (int m = 0; m < 2; ++m)
                for (int cc = 0; cc < 4; ++cc) std::copy(h->rf[l].v[m][cc].begin(), h->rf[l].v[m][cc].end(), f.begin() + h->rf[l].off[m][cc]);
        h->axes_d = dev_alloc<float>(nf);
        h->rfKeys_d = dev_alloc<unsigned long long>(2 * 4 * W * (size_t)nLevels);
        h->rfCentre_d = dev_alloc<float>((size_t)nLevels * W * 8);
        DPE_REQUIRE(h->axes_d && h->rfKeys_d && h->rfCentre_d, "[BatchCorrManifold] create_refine: device allocation failed");
        for (int l = 0; cfg->writeScores && l < nLevels; ++l)
            for (int m = 0; m < 2; ++m) {
                h->rf[l].scores[m] = dev_alloc<float>(W * (size_t)h->rf[l].pitch[m]);
                DPE_REQUIRE(h->rf[l].scores[m], "[BatchCorrManifold] create_refine: score rows of level %d: device allocation failed", l);
            }
        DPE_CHECK_HIP(hipMemcpy(h->axes_d, f.data(), sizeof(float) * nf, hipMemcpyHostToDevice));
        DPE_CHECK_HIP(hipMemset(h->rfKeys_d, 0, sizeof(unsigned long long) * 2 * 4 * W * (size_t)nLevels));
        DPE_CHECK_HIP(hipMemset(h->rfCentre_d, 0, sizeof(float) * (size_t)nLevels * W * 8));
        return 0;
    };
    if (finish()) {
        dpe_bcm_destroy(h);
        return -1;
    }
    h->rfKeys_h.assign(4 * W * (size_t)nLevels, 0ull);
    allow_big_lds_refine();
    *out = h;
    return 0;
}

int dpe_bcm_destroy(dpe_bcm *h)
{
    if (!h) return 0;
    if (h->ownerDetach) h->ownerDetach(h->owner, 1);
    if (h->gridsBorrowed) h->posGrid_d = h->velGrid_d = nullptr;
    if (h->axesBorrowed) h->axes_d = nullptr;
    (void)hipFree(h->axes_d);
    (void)hipFree(h->posAx64_d); (void)hipFree(h->velAx64_d);
    void *bufs[] = {h->posGrid64_d, h->velGrid64_d, h->posGrid_d, h->velGrid_d, h->posScores_d, h->velScores_d, h->sv_d, h->keys_d, h->wsum_d, h->done_d, h->refPatched_d};
    for (void *b : bufs) (void)hipFree(b);
    if (h->svBase_h) (void)hipHostFree(h->svBase_h);
    if (h->keys_h) (void)hipHostFree(h->keys_h);
    if (h->devWin_h) (void)hipHostFree(h->devWin_h);
    if (h->refBank_h) (void)hipHostFree(h->refBank_h);
    if (h->jrxBase_h) (void)hipHostFree(h->jrxBase_h);
    (void)hipFree(h->jrx_d); (void)hipFree(h->own_d);
    if (h->subMaskBase_h) (void)hipHostFree(h->subMaskBase_h);
    (void)hipFree(h->sub_d);
    (void)hipFree(h->rfKeys_d); (void)hipFree(h->rfCentre_d);
    for (auto &lv : h->rf) { (void)hipFree(lv.scores[0]); (void)hipFree(lv.scores[1]); }
    (void)hipFree(h->refCand_d); (void)hipFree(h->refWhere_d); (void)hipFree(h->refValue_d); (void)hipFree(h->refOld_d);
    (void)hipFree(h->momPartial_d); (void)hipFree(h->momSums_d); (void)hipFree(h->momAbove_d);
    if (h->momMirror_h) (void)hipHostFree(h->momMirror_h);
    for (hipEvent_t e : h->stagingFree)
        if (e) (void)hipEventDestroy(e);
    h->graphs.clear();
    delete h;
    return 0;
}

// The expansion of one (window, SV) pair about the window's centre, in fp64 (file header): the coefficient blocks of the two
// manifolds, and whether every index of the pair provably stays inside the banks (cleared, never set).
static void bcm_expand(const dpe_bcm *h, const dpe_bcm_window &win, const dpe_chan_end &ch, dpe::BcmSvDev &p, dpe::BcmSvDev &v,
                       bool &posInside, bool &velInside)
{
    using namespace dpe;
    const int S = h->cfg.samplesPerWindow, L = h->cfg.lagHalfWidth, B = h->cfg.binHalfWidth;
    const double fs = h->cfg.samplingFrequency, Cf = (double)h->cfg.numFFTPoints;
    const double *c = win.xCurrkk1, *R = win.enu2ecef;
    const double *s = ch.satState;
    const double dx = s[0] - c[0], dy = s[1] - c[1], dz = s[2] - c[2];       // :1779-1781
    const double range = std::sqrt(dx * dx + dy * dy + dz * dz);               // :1782
    const double ux = dx / range, uy = dy / range, uz = dz / range;
    const double ue = R[0] * ux + R[3] * uy + R[6] * uz;                        // R^T u
    const double un = R[1] * ux + R[4] * uy + R[7] * uz;
    const double uu = R[2] * ux + R[5] * uy + R[8] * uz;
    // position manifold, centre index (:1783-1791).  Carried in long double: the reference's
    // fp64 "rxTime - pr/C" (rxTime ~4e5 s) rounds at 5.8e-11 s = 1.4e-4 samples PER POINT; the
    // expansion below is exact about the centre, so the centre itself is kept exact too.
    const long double pr = (long double)range - (long double)kC * s[3] + c[3];
    const long double txT = (long double)win.rxTime - pr / (long double)kC;
    const long double cfd = txT - ch.cpRefTOW - ((long double)(ch.cpElapsedEnd - ch.cpRef) * (long double)kTCA);
    const long double rc0 = cfd * (long double)kFCA - ch.codePhaseEnd;
    const double basePos = (double)(((long double)fs / ch.codeFrequency) * (-rc0) + S / 2.0L);
    p.ue = (float)ue; p.un = (float)un; p.uu = (float)uu;
    p.g = (float)(fs * kFCA / (ch.codeFrequency * kC));
    p.h = (float)(0.5 / range);
    p.idx0 = (float)(basePos - (double)(S / 2 - L));
    p.pad0 = p.pad1 = 0.f;
    {
        const double reach = std::fabs((double)p.g) * h->posExtent + 1e-3;
        if (!((double)p.idx0 - reach >= 0.0 && (double)p.idx0 + reach < (double)(2 * L))) posInside = false;
    }
    // velocity manifold, centre index (:1917-1936)
    const double ex = c[4] - kOEDot * c[1], ey = c[5] + kOEDot * c[0], ez = c[6];
    const double lrr = ux * (ex - s[4]) + uy * (ey - s[5]) + uz * (ez - s[6]);
    const double fbc = kFL1 * ((lrr - c[7]) / kC + s[7]) / win.dopplerSign;
    const double baseVel = (Cf / fs) * (fbc - ch.carrierFrequency) + Cf / 2.0;
    const double gv = (Cf / fs) * kFL1 / (kC * win.dopplerSign);
    v.ue = (float)ue; v.un = (float)un; v.uu = (float)uu;
    v.g = (float)(-gv);   // index = idx0 + g (delta_tdot - u . delta_v)
    v.idx0 = (float)(baseVel - (double)(h->cfg.numFFTPoints / 2 - B));
    v.h = (float)(-gv * ue); v.pad0 = (float)(-gv * un); v.pad1 = (float)(-gv * uu);   // g u, products formed in fp64
    {
        const double reach = std::fabs(gv) * h->velExtent + 1e-3;
        if (!((double)v.idx0 - reach >= 0.0 && (double)v.idx0 + reach < (double)(2 * B))) velInside = false;
    }
}

// ---- the host pieces of an Update ------------------------------------------------------------
static int check_kind(bool is, const char *who, const char *maker)
{
    DPE_REQUIRE(is, "[BatchCorrManifold] %s: the handle was not made by %s", who, maker);
    return 0;
}

static int check_windows(const dpe_bcm *h, const char *who, int nWindows)
{
    DPE_REQUIRE(nWindows >= 1 && nWindows <= h->cfg.maxWindows, "[BatchCorrManifold] %s: nWindows %d out of range", who, nWindows);
    return 0;
}

static int check_chan(const dpe_bcm *h, const char *who, int nChan)
{
    DPE_REQUIRE(nChan >= 1 && nChan <= h->cfg.maxChannels, "[BatchCorrManifold] %s: nChan %d out of range", who, nChan);
    return 0;
}

static int check_sign(const char *who, const dpe_bcm_window *win, int n)
{
    for (int w = 0; w < n; ++w)
        DPE_REQUIRE(win[w].dopplerSign == 1 || win[w].dopplerSign == -1, "[BatchCorrManifold] %s: dopplerSign must be +/-1", who);
    return 0;
}

// Stage begin: the next block of the pinned ring (an Update kStaging calls ago may still be copying it) becomes sv_h.  Called
// once every check has passed: a refused call takes no slot.
static int stage_begin(dpe_bcm *h, bool dev)
{
    h->lastDev = dev;
    h->slot = (h->slot + 1) % dpe_bcm::kStaging;
    DPE_CHECK_HIP(hipEventSynchronize(h->stagingFree[h->slot]));
    h->sv_h = h->svBase_h + (size_t)h->slot * 2 * h->cfg.maxWindows * sv_stride(h);
    return 0;
}

// One window's channels into both manifolds' rows of sv_h, from channel kOff on, each about that window's own centre
static void expand_window(dpe_bcm *h, int w, const dpe_bcm_window &win, const dpe_chan_end *ch, int nChan, int kOff, bool &posInside, bool &velInside)
{
    dpe::BcmSvDev *p = h->sv_h + (size_t)w * sv_stride(h) + kOff, *v = p + (size_t)h->cfg.maxWindows * sv_stride(h);
    for (int k = 0; k < nChan; ++k) bcm_expand(h, win, ch[k], p[k], v[k], posInside, velInside);
}

// Stage begin, then nWin windows of nChan channels kept in win_h and expanded (win == nullptr: a device-parameter Update,
// whose coefficients bcm_prep_kernel writes)
static int stage_windows(dpe_bcm *h, const dpe_bcm_window *win, const dpe_chan_end *chan, int nWin, int nChan, bool &posInside, bool &velInside)
{
    if (stage_begin(h, win == nullptr)) return -1;
    for (int w = 0; win && w < nWin; ++w) {
        h->win_h[w] = win[w];
        expand_window(h, w, win[w], chan + (size_t)w * nChan, nChan, 0, posInside, velInside);
    }
    return 0;
}

// Two key / counter sets of setLen words ({keys, counts}) alternate between Updates: a call reduces into set `use` (zero since
// the previous call's position scan, or create, cleared it) and clears `other`
struct KeySet {
    int use;
    unsigned long long *keys, *oob, *other;
};

static KeySet next_key_set(const dpe_bcm *h, unsigned long long *base, size_t setLen)
{
    const int use = h->cur ^ 1;
    return KeySet{use, base + (size_t)use * setLen, base + (size_t)use * setLen + setLen / 2, base + (size_t)(use ^ 1) * setLen};
}

// The two manifolds' ScanSides over the handle's point lists; the splits are h->lastSplit.  (The handle kinds that scan whole
// grids and form no weighted mean were refused index offsets and weightedMean at create, so cfg says 0 for them.)
static void scan_sides(const dpe_bcm *h, const float *codeBank_dev, const float *carrBank_dev, dpe::ScanSide &sp, dpe::ScanSide &sv)
{
    const int nLag = 2 * h->cfg.lagHalfWidth + 1, nBin = 2 * h->cfg.binHalfWidth + 1;
    sp = dpe::ScanSide{h->posGrid_d, reinterpret_cast<const float2 *>(codeBank_dev), h->sv_d, h->posScores_d,
                       h->cfg.weightedMean ? h->wsum_d : nullptr, h->cfg.posGridSize, h->cfg.posGridIndexOffset, h->posPitch, nLag,
                       (int)h->lastSplit[0]};
    sv = dpe::ScanSide{h->velGrid_d, reinterpret_cast<const float2 *>(carrBank_dev), h->sv_d + (size_t)h->cfg.maxWindows * sv_stride(h), h->velScores_d,
                       h->cfg.weightedMean ? h->wsum_d + h->wsumHalf : nullptr, h->cfg.velGridSize, h->cfg.velGridIndexOffset, h->velPitch, nBin,
                       (int)h->lastSplit[1]};
}

// The tail of a publishing family's launch over `rows` windows (groups): key sets, publishing pointers (publish = false: the
// scan leaves keys and counts in device memory only) and the geometry from h->lastSplit.  It also moves the handle's state that
// goes with them: seq advances (the launch carries the new value), lastPublished = publish, pollable = false.
static void fill_tail(dpe_bcm *h, ScanTail &t, const KeySet &ks, int clrN, bool publish, int rows, size_t lds, hipStream_t st)
{
    t.keys = ks.keys; t.oob = ks.oob; t.clr = ks.other; t.clrN = clrN;
    t.done = publish ? h->done_d : nullptr; t.hostKeys = h->keys_hd; t.hostOob = h->keys_hd + 2 * h->cfg.maxWindows;
    h->lastPublished = publish;
    h->pollable = false;   // (the plain single-window Update sets it afterwards; the rest fetch behind a stream wait)
    t.seq = ++h->seq;
    t.grid = dim3(h->lastSplit[0] > h->lastSplit[1] ? h->lastSplit[0] : h->lastSplit[1], rows, 2);
    t.lds = lds; t.st = st;
}

// Launch finish: cur advances only after a launch that succeeded (a call that fails earlier must not skip a clearing)
static int launch_finish(dpe_bcm *h, int use)
{
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) {
        h->pollable = false;   // nothing will ever write the sequence word of this Update
        dpe::set_error("%s:%d: launch failed -> %s", __FILE__, __LINE__, hipGetErrorString(le));
        return -1;
    }
    h->cur = use;
    return 0;
}

// win_host == nullptr: one window whose coefficients bcm_prep_kernel has already written to h->sv_d on `stream`
// (dpe_bcm_update_dev) -- nothing the host decides below may then depend on their values.
static int bcm_update_impl(dpe_bcm *h, const float *codeBank_dev, const float *carrBank_dev, int32_t nWindows, int32_t nChan,
                           const dpe_bcm_window *win_host, const dpe_chan_end *chan_host, dpe_stream_t stream_)
{
    using namespace dpe;
    const bool dev = win_host == nullptr;
    DPE_REQUIRE(h && codeBank_dev && carrBank_dev, "[BatchCorrManifold] Update: null argument");
    DPE_REQUIRE(!h->joint, "[BatchCorrManifold] Update: this handle scans several receivers (dpe_bcm_create_joint): use dpe_bcm_update_joint");
    DPE_REQUIRE(!h->epochs, "[BatchCorrManifold] Update: this handle sums consecutive windows (dpe_bcm_create_epochs): use dpe_bcm_update_epochs");
    DPE_REQUIRE(!h->subsets, "[BatchCorrManifold] Update: this handle scans SV subsets (dpe_bcm_create_subsets): use dpe_bcm_update_subsets");
    DPE_REQUIRE(!h->refine, "[BatchCorrManifold] Update: this handle scans coarse-to-fine levels (dpe_bcm_create_refine): use dpe_bcm_update_refine");
    if (check_windows(h, "Update", nWindows) || check_chan(h, "Update", nChan) || (!dev && check_sign("Update", win_host, nWindows))) return -1;
    hipStream_t stream = (hipStream_t)stream_;
    const int maxK = h->cfg.maxChannels, W = h->cfg.maxWindows;
    bool posInside = !dev, velInside = !dev;   // every index provably inside the banks?  (device parameters: not known here)
    if (stage_windows(h, win_host, chan_host, nWindows, nChan, posInside, velInside)) return -1;
    h->lastW = nWindows;
    long long axTiles[2] = {0, 0};
    AxesLaunch ax{};
    if (h->axes) {   // (scan_split sizes the launch in 1024-point tiles; an axes tile is 256 rows x one chunk of up to kAxT slots,
                     //  up to 4096 point evaluations, so this gives a quarter of the blocks per evaluation of the point-list scan)
        ax.sp = axes_side(h, 0, &axTiles[0]);
        ax.sv = axes_side(h, 1, &axTiles[1]);
    }
    h->lastSplit[0] = scan_split(h->axes ? axTiles[0] * kPtsPerBlock : h->cfg.posGridSize, nWindows, h->splitForce);
    h->lastSplit[1] = scan_split(h->axes ? axTiles[1] * kPtsPerBlock : h->cfg.velGridSize, nWindows, h->splitForce);
    const KeySet ks = next_key_set(h, h->keys_d, 4 * (size_t)W);
    GraphCache::Guard graphGuard{h->graphs, stream};
    if (h->graphs.enabled && !h->prof.enabled && !h->refPair && !dev) {
        const int rc = h->graphs.begin({codeBank_dev, carrBank_dev, 0, nWindows, nChan,
                                        (posInside ? 1 : 0) | (velInside ? 2 : 0) | (ks.use << 2) | (h->slot << 8), stream}, stream);
        DPE_REQUIRE(rc >= 0, "[BatchCorrManifold] Update: hipGraph capture/replay failed");
        if (rc == 1) {
            DPE_CHECK_HIP(hipEventRecord(h->stagingFree[h->slot], stream));   // the replayed graph reads this slot
            h->cur = ks.use;
            h->pollable = false;
            return 0;
        }
    }
    // one window: coefficients as kernel arguments of the scans (a captured graph would freeze them, so
    // that path copies); batches: one copy covers both manifolds' coefficient blocks
    const bool inlineParams = nWindows == 1 && !h->graphs.capturing && !dev;
    BcmParamBlock pb{};
    if (dev) {}
    else if (inlineParams) {
        memcpy(pb.s[0], h->sv_h, sizeof(BcmSvDev) * nChan);
        memcpy(pb.s[1], h->sv_h + (size_t)W * maxK, sizeof(BcmSvDev) * nChan);
    } else {
        if (h->graphs.capturing) DPE_CHECK_HIP(hipMemcpyAsync(h->sv_d, h->sv_h, sv_bytes(h), hipMemcpyHostToDevice, stream));
        else upload_params(h->sv_d, h->svBase_hd + (h->sv_h - h->svBase_h), sv_bytes(h), stream);
        if (!h->graphs.capturing) DPE_CHECK_HIP(hipEventRecord(h->stagingFree[h->slot], stream));
    }
    ScanLaunch a;
    a.pb = pb; a.inl = inlineParams ? 1 : 0; a.K = nChan; a.maxK = maxK; a.lp = h->cfg.lPower;
    scan_sides(h, codeBank_dev, carrBank_dev, a.sp, a.sv);
    const bool publishNow = h->publish || !dev || h->cfg.weightedMean;   // (only the device-parameter forms may skip it)
    fill_tail(h, a, ks, 4 * W, publishNow, nWindows, (size_t)nChan * n_ent_max(h->cfg) * (h->compact ? 12 : 16), stream);
    // (a replayed graph carries a stale sequence argument: polling only for eager single-window launches whose mirror
    //  has the sequence word right behind the results, i.e. maxWindows == 1)
    // (with the weighted-mean estimator the per-block sums are fetched with a copy after the results arrive: that copy must
    //  see the finished kernel, so the stream is waited for instead)
    h->pollable = nWindows == 1 && W == 1 && !h->graphs.capturing && h->pollAllowed && !h->cfg.weightedMean && publishNow;
    // the kernel's last block writes keys and counts into the pinned host mirror: dpe_bcm_results only
    // has to synchronise
    h->prof.begin(0, stream);
    if (h->axes) {
        ax.a = a;
        ax.a.lds = (size_t)nChan * n_ent_max(h->cfg) * 16 + kAxStageBytes;
        ax.sp.bank = a.sp.bank; ax.sp.sv = a.sp.sv; ax.sp.scores = a.sp.scores; ax.sp.wsum = a.sp.wsum;
        ax.sp.pitch = a.sp.pitch; ax.sp.nEnt = a.sp.nEnt; ax.sp.split = a.sp.split;
        ax.sv.bank = a.sv.bank; ax.sv.sv = a.sv.sv; ax.sv.scores = a.sv.scores; ax.sv.wsum = a.sv.wsum;
        ax.sv.pitch = a.sv.pitch; ax.sv.nEnt = a.sv.nEnt; ax.sv.split = a.sv.split;
        launch_axes(!posInside, !velInside, h->cfg.weightedMean != 0, ax);
    } else {
        launch_scan(!posInside, !velInside, h->cfg.weightedMean != 0, h->compact, a);
    }
    h->prof.end(0, stream);
    const bool captured = h->graphs.capturing;
    DPE_REQUIRE(h->graphs.end(stream) == 0, "[BatchCorrManifold] Update: hipGraph instantiate/launch failed");
    if (captured) DPE_CHECK_HIP(hipEventRecord(h->stagingFree[h->slot], stream));
    if (launch_finish(h, ks.use)) return -1;
    if (h->refPair && !dev) {
        h->pollable = false;
        if (ref_pair_fixup(h, codeBank_dev, nWindows, nChan, chan_host, ks.keys, stream)) return -1;
    } else if (h->refPair) {
        // device-parameter form (dpe_bcm_update_dev): candidates, re-evaluation, patch and arg-max all on the device, nothing read back
        h->pollable = false;
        const long long G = h->cfg.posGridSize;
        if (!h->refCand_d) {
            if (h->refCap == 0) h->refCap = 1 << 16;
            h->refCand_d = dev_alloc<unsigned long long>(1 + h->refCap);
        }
        if (!h->refPatched_d) h->refPatched_d = dev_alloc<unsigned long long>(1);
        DPE_REQUIRE(h->refCand_d && h->refPatched_d, "[BatchCorrManifold] Update: referencePair: candidate list allocation failed");
        if (!h->posGrid64_d) { dpe_bcm_hook hk; if (dpe_bcm_hook_get(h, &hk)) return -1; }   // (makes the fp64 copies of the grids)
        DPE_CHECK_HIP(hipMemsetAsync(h->refCand_d, 0, sizeof(unsigned long long), stream));
        DPE_CHECK_HIP(hipMemsetAsync(h->refPatched_d, 0, sizeof(unsigned long long), stream));
        const unsigned gx = (unsigned)((G + 256 * 8 - 1) / (256 * 8));
        hipLaunchKernelGGL(bcm_refpair_candidates_kernel, dim3(gx > 1024 ? 1024 : gx, 1), dim3(256), 0, stream, h->posGrid_d, G, h->sv_d,
                           h->cfg.maxChannels, h->cfg.lagHalfWidth, 5e-4, h->refCand_d, h->refCap);
        hipLaunchKernelGGL(bcm_refpair_eval_kernel, dim3(64), dim3(64), 0, stream, h->refPorts, (int)nChan, h->refRxTime, h->refRxTime_d, h->cfg.samplingFrequency,
                           h->cfg.samplesPerWindow, h->cfg.lagHalfWidth, h->cfg.lPower, h->posGrid64_d, reinterpret_cast<const float2 *>(codeBank_dev),
                           h->cfg.maxChannels, h->refCand_d, h->refCap, h->posScores_d, h->posPitch, h->devWin_hd + ks.use, h->refPatched_d);
        hipLaunchKernelGGL(bcm_zero_pos_keys_kernel, dim3(1), dim3(64), 0, stream, ks.keys, 1);
        const unsigned gr = (unsigned)((G + 256 * 16 - 1) / (256 * 16));
        hipLaunchKernelGGL(bcm_rekey_kernel, dim3(gr > 512 ? 512 : gr, 1), dim3(256), 0, stream, h->posScores_d, G, h->posPitch,
                           (long long)h->cfg.posGridIndexOffset, ks.keys);
        DPE_CHECK_HIP(hipGetLastError());
        h->lastPublished = false;   // (the pinned mirror holds the scan's keys from before the patch: the results call fetches the re-derived ones)
    }
    return 0;
}

int dpe_bcm_update(dpe_bcm *h, const float *codeBank_dev, const float *carrBank_dev, int32_t nWindows, int32_t nChan,
                   const dpe_bcm_window *win_host, const dpe_chan_end *chan_host, dpe_stream_t stream)
{
    DPE_REQUIRE(win_host && chan_host, "[BatchCorrManifold] Update: null argument");
    return bcm_update_impl(h, codeBank_dev, carrBank_dev, nWindows, nChan, win_host, chan_host, stream);
}

// Several receivers over one pair of grids: one launch scores, per grid point, every (receiver, SV) pair of the window.
int dpe_bcm_update_joint(dpe_bcm *h, int32_t nWindows, int32_t nRx, const dpe_bcm_joint_rx *rx, dpe_stream_t stream_)
{
    using namespace dpe;
    DPE_REQUIRE(h && rx, "[BatchCorrManifold] update_joint: null argument");
    if (check_kind(h->joint, "update_joint", "dpe_bcm_create_joint") || check_windows(h, "update_joint", nWindows)) return -1;
    DPE_REQUIRE(nRx >= 1 && nRx <= h->jointMaxRx, "[BatchCorrManifold] update_joint: nRx %d out of range (the handle holds %d receivers)", nRx, h->jointMaxRx);
    hipStream_t stream = (hipStream_t)stream_;
    const int W = h->cfg.maxWindows, maxRx = h->jointMaxRx, maxKT = h->jointMaxK;
    // everything is checked before anything is staged or launched
    for (int w = 0; w < nWindows; ++w) {
        int total = 0;
        for (int r = 0; r < nRx; ++r) {
            const dpe_bcm_joint_rx &x = rx[(size_t)w * nRx + r];
            DPE_REQUIRE(x.codeBank_dev && x.carrBank_dev && x.chan_host, "[BatchCorrManifold] update_joint: window %d receiver %d: null pointer", w, r);
            DPE_REQUIRE(x.nChan >= 1 && x.nChan <= h->cfg.maxChannels, "[BatchCorrManifold] update_joint: window %d receiver %d: nChan %d out of range (1 .. %d)",
                        w, r, x.nChan, h->cfg.maxChannels);
            if (check_sign("update_joint", &x.win, 1)) return -1;
            DPE_REQUIRE(memcmp(x.win.enu2ecef, rx[(size_t)w * nRx].win.enu2ecef, sizeof(x.win.enu2ecef)) == 0,
                        "[BatchCorrManifold] update_joint: window %d: receiver %d's enu2ecef differs from receiver 0's (one grid offset must mean one "
                        "ECEF displacement for every receiver: pass bit-equal matrices)", w, r);
            total += x.nChan;
        }
        DPE_REQUIRE(total <= maxKT, "[BatchCorrManifold] update_joint: window %d has %d (receiver, SV) pairs, the handle holds %d", w, total, maxKT);
    }
    bool posInside = true, velInside = true;
    if (stage_begin(h, false)) return -1;
    JointRxDev *jrx_h = h->jrxBase_h + (size_t)h->slot * W * maxRx;
    int ldsRows = 0;
    for (int w = 0; w < nWindows; ++w) {
        int kOff = 0;
        for (int r = 0; r < nRx; ++r) {
            const dpe_bcm_joint_rx &x = rx[(size_t)w * nRx + r];
            h->jwin_h[(size_t)w * maxRx + r] = x.win;
            // each expansion about its own receiver's centre, with that receiver's receive time
            expand_window(h, w, x.win, x.chan_host, x.nChan, kOff, posInside, velInside);
            jrx_h[(size_t)w * maxRx + r] = JointRxDev{reinterpret_cast<const float2 *>(x.codeBank_dev), reinterpret_cast<const float2 *>(x.carrBank_dev),
                                                     x.nChan, kOff, 0, 0};
            kOff += x.nChan;
        }
        if (kOff > ldsRows) ldsRows = kOff;
    }
    h->lastW = nWindows;
    h->lastRx = nRx;
    h->lastOwn = h->ownKeys;
    h->lastSplit[0] = scan_split(h->cfg.posGridSize, nWindows, h->splitForce);
    h->lastSplit[1] = scan_split(h->cfg.velGridSize, nWindows, h->splitForce);
    const KeySet ks = next_key_set(h, h->keys_d, 4 * (size_t)W);
    DPE_CHECK_HIP(hipMemcpyAsync(h->sv_d, h->sv_h, sv_bytes(h), hipMemcpyHostToDevice, stream));
    DPE_CHECK_HIP(hipMemcpyAsync(h->jrx_d, jrx_h, sizeof(JointRxDev) * (size_t)W * maxRx, hipMemcpyHostToDevice, stream));
    DPE_CHECK_HIP(hipEventRecord(h->stagingFree[h->slot], stream));
    DPE_CHECK_HIP(hipMemsetAsync(h->own_d, 0, sizeof(unsigned long long) * 4 * (size_t)W * maxRx, stream));
    JointLaunch a;
    scan_sides(h, nullptr, nullptr, a.sp, a.sv);   // (the banks are per receiver: a.rx)
    a.rx = h->jrx_d; a.nRx = nRx; a.maxRx = maxRx; a.maxKT = maxKT; a.lp = h->cfg.lPower;
    a.ownKeys = h->own_d; a.ownOob = h->own_d + 2 * (size_t)W * maxRx;
    // (<= maxKT rows of LDS: inside the budget create checked)
    fill_tail(h, a, ks, 4 * W, true, nWindows, (size_t)ldsRows * n_ent_max(h->cfg) * 16, stream);
    h->prof.begin(0, stream);
    launch_joint(!posInside, !velInside, h->lastOwn, a);
    h->prof.end(0, stream);
    return launch_finish(h, ks.use);
}

// N consecutive windows per group: one launch scores, per grid point, every (window, SV) pair of the group, in passes of whole
// windows whose banks fit the LDS together (dpe_bcm_epochs.h).
int dpe_bcm_update_epochs(dpe_bcm *h, const float *codeBank_dev, const float *carrBank_dev, int32_t nGroups, int32_t nEpochs, int32_t nChan,
                          const dpe_bcm_window *win_host, const dpe_chan_end *chan_host, dpe_stream_t stream_)
{
    using namespace dpe;
    DPE_REQUIRE(h && codeBank_dev && carrBank_dev && win_host && chan_host, "[BatchCorrManifold] update_epochs: null argument");
    if (check_kind(h->epochs, "update_epochs", "dpe_bcm_create_epochs")) return -1;
    // everything is checked before anything is staged or launched
    DPE_REQUIRE(nEpochs >= 1 && nEpochs <= h->epMaxEpochs, "[BatchCorrManifold] update_epochs: nEpochs %d out of range (the handle holds %d windows per group)",
                nEpochs, h->epMaxEpochs);
    DPE_REQUIRE(nGroups >= 1 && (long long)nGroups * nEpochs <= h->cfg.maxWindows,
                "[BatchCorrManifold] update_epochs: %d groups of %d windows out of range (maxWindows %d)", nGroups, nEpochs, h->cfg.maxWindows);
    const int nWin = nGroups * nEpochs;
    if (check_chan(h, "update_epochs", nChan) || check_sign("update_epochs", win_host, nWin)) return -1;
    hipStream_t stream = (hipStream_t)stream_;
    const int maxK = h->cfg.maxChannels, W = h->cfg.maxWindows;
    bool posInside = true, velInside = true;
    if (stage_windows(h, win_host, chan_host, nWin, nChan, posInside, velInside)) return -1;
    const int winPerPass = std::min(h->epPairsPerPass / nChan, (int)nEpochs);   // >= 1: epPairsPerPass >= maxChannels >= nChan
    h->lastW = nGroups;
    h->lastEpochs = nEpochs;
    h->lastPasses = (nEpochs + winPerPass - 1) / winPerPass;
    h->lastSplit[0] = scan_split(h->cfg.posGridSize, nGroups, h->splitForce);
    h->lastSplit[1] = scan_split(h->cfg.velGridSize, nGroups, h->splitForce);
    const KeySet ks = next_key_set(h, h->keys_d, 4 * (size_t)W);
    DPE_CHECK_HIP(hipMemcpyAsync(h->sv_d, h->sv_h, sv_bytes(h), hipMemcpyHostToDevice, stream));
    DPE_CHECK_HIP(hipEventRecord(h->stagingFree[h->slot], stream));
    EpochsLaunch a;
    scan_sides(h, codeBank_dev, carrBank_dev, a.sp, a.sv);
    a.nEpochs = nEpochs; a.winPerPass = winPerPass; a.K = nChan; a.maxK = maxK; a.lp = h->cfg.lPower;
    // (<= epPairsPerPass pairs in LDS: inside the budget create checked)
    fill_tail(h, a, ks, 4 * W, true, nGroups, (size_t)winPerPass * nChan * n_ent_max(h->cfg) * 16, stream);
    h->prof.begin(0, stream);
    launch_epochs(!posInside, !velInside, a);
    h->prof.end(0, stream);
    return launch_finish(h, ks.use);
}

// One launch scores every (point, SV) pair once and reduces the full set and every subset to its own first maximum
// (dpe_bcm_subsets.h).
int dpe_bcm_update_subsets(dpe_bcm *h, const float *codeBank_dev, const float *carrBank_dev, int32_t nWindows, int32_t nChan,
                           const dpe_bcm_window *win_host, const dpe_chan_end *chan_host, int32_t nSubsets, const uint64_t *masks_host,
                           dpe_stream_t stream_)
{
    using namespace dpe;
    DPE_REQUIRE(h && codeBank_dev && carrBank_dev && win_host && chan_host, "[BatchCorrManifold] update_subsets: null argument");
    // everything is checked before anything is staged or launched
    if (check_kind(h->subsets, "update_subsets", "dpe_bcm_create_subsets") || check_windows(h, "update_subsets", nWindows) ||
        check_chan(h, "update_subsets", nChan))
        return -1;
    DPE_REQUIRE(nSubsets >= 0 && nSubsets <= h->subMax, "[BatchCorrManifold] update_subsets: nSubsets %d out of range (the handle holds %d subsets per window)",
                nSubsets, h->subMax);
    DPE_REQUIRE(nSubsets == 0 || masks_host, "[BatchCorrManifold] update_subsets: null masks");
    for (int w = 0; w < nWindows; ++w) {
        if (check_sign("update_subsets", win_host + w, 1)) return -1;
        for (int m = 0; m < nSubsets; ++m) {
            const uint64_t mask = masks_host[(size_t)w * nSubsets + m];
            DPE_REQUIRE(mask != 0, "[BatchCorrManifold] update_subsets: window %d subset %d: empty mask", w, m);
            DPE_REQUIRE(nChan >= 64 || (mask >> nChan) == 0, "[BatchCorrManifold] update_subsets: window %d subset %d: mask 0x%llx has a bit at or above nChan %d",
                        w, m, (unsigned long long)mask, nChan);
        }
    }
    hipStream_t stream = (hipStream_t)stream_;
    const int maxK = h->cfg.maxChannels, W = h->cfg.maxWindows, maxS = h->subMax;
    bool posInside = true, velInside = true;
    if (stage_windows(h, win_host, chan_host, nWindows, nChan, posInside, velInside)) return -1;
    unsigned long long *mask_h = h->subMaskBase_h + (size_t)h->slot * W * maxS;
    for (int w = 0; w < nWindows; ++w) {
        for (int m = 0; m < maxS; ++m)
            h->subMask_h[(size_t)w * maxS + m] = mask_h[(size_t)w * maxS + m] = m < nSubsets ? masks_host[(size_t)w * nSubsets + m] : 0ull;
    }
    h->lastW = nWindows;
    h->lastSubsets = nSubsets;
    h->lastChan = nChan;
    h->lastSplit[0] = scan_split(h->cfg.posGridSize, nWindows, h->splitForce);
    h->lastSplit[1] = scan_split(h->cfg.velGridSize, nWindows, h->splitForce);
    const KeySet ks = next_key_set(h, h->keys_d, 4 * (size_t)W);
    unsigned long long *masks_d = h->sub_d, *subKeys_d = masks_d + (size_t)W * maxS, *svOob_d = subKeys_d + 2 * (size_t)W * maxS;
    DPE_CHECK_HIP(hipMemcpyAsync(h->sv_d, h->sv_h, sv_bytes(h), hipMemcpyHostToDevice, stream));
    // nSubsets = 0 with every index inside the banks is the plain scan on the launch side as well: no mask copy, nothing to clear
    // (the kernel then touches neither the subset keys nor the per-SV counters, which the results call reports as 0)
    if (nSubsets > 0) DPE_CHECK_HIP(hipMemcpyAsync(masks_d, mask_h, sizeof(unsigned long long) * (size_t)W * maxS, hipMemcpyHostToDevice, stream));
    DPE_CHECK_HIP(hipEventRecord(h->stagingFree[h->slot], stream));
    h->lastCounted = !posInside || !velInside;
    if (nSubsets > 0) DPE_CHECK_HIP(hipMemsetAsync(subKeys_d, 0, sizeof(unsigned long long) * (2 * (size_t)W * maxS + 2 * (size_t)W * maxK), stream));
    else if (h->lastCounted) DPE_CHECK_HIP(hipMemsetAsync(svOob_d, 0, sizeof(unsigned long long) * 2 * (size_t)W * maxK, stream));
    SubsetsLaunch a;
    scan_sides(h, codeBank_dev, carrBank_dev, a.sp, a.sv);
    a.K = nChan; a.maxK = maxK; a.lp = h->cfg.lPower; a.nSubsets = nSubsets; a.maxSubsets = maxS;
    a.masks = masks_d; a.subKeys = subKeys_d; a.svOob = svOob_d;
    // (<= maxChannels rows of LDS: inside the budget create checked)
    fill_tail(h, a, ks, 4 * W, true, nWindows, (size_t)nChan * n_ent_max(h->cfg) * 16, stream);
    h->prof.begin(0, stream);
    launch_subsets(!posInside, !velInside, a);
    h->prof.end(0, stream);
    return launch_finish(h, ks.use);
}

// One launch per level, in stream order; level l >= 1 takes its centre from level l-1's key in device memory (dpe_bcm_refine.h).
// The coefficients are expanded once and shared by the levels; the clamp variants follow from the summed reach (create_refine).
int dpe_bcm_update_refine(dpe_bcm *h, const float *codeBank_dev, const float *carrBank_dev, int32_t nWindows, int32_t nChan,
                          const dpe_bcm_window *win_host, const dpe_chan_end *chan_host, dpe_stream_t stream_)
{
    using namespace dpe;
    DPE_REQUIRE(h && codeBank_dev && carrBank_dev && win_host && chan_host, "[BatchCorrManifold] update_refine: null argument");
    // everything is checked before anything is staged or launched
    if (check_kind(h->refine, "update_refine", "dpe_bcm_create_refine") || check_windows(h, "update_refine", nWindows) ||
        check_chan(h, "update_refine", nChan) || check_sign("update_refine", win_host, nWindows))
        return -1;
    hipStream_t stream = (hipStream_t)stream_;
    const int maxK = h->cfg.maxChannels, W = h->cfg.maxWindows, nL = h->rfLevels;
    bool posInside = true, velInside = true;
    if (stage_windows(h, win_host, chan_host, nWindows, nChan, posInside, velInside)) return -1;
    h->lastW = nWindows;
    const size_t setLen = 4 * (size_t)W * nL;   // {keys [levels][W][2], counts [levels][W][2]}
    const KeySet ks = next_key_set(h, h->rfKeys_d, setLen);
    upload_params(h->sv_d, h->svBase_hd + (h->sv_h - h->svBase_h), sv_bytes(h), stream);
    DPE_CHECK_HIP(hipEventRecord(h->stagingFree[h->slot], stream));
    const int nLag = 2 * h->cfg.lagHalfWidth + 1, nBin = 2 * h->cfg.binHalfWidth + 1;
    h->pollable = false;
    h->lastPublished = false;
    h->prof.begin(0, stream);
    for (int l = 0; l < nL; ++l) {
        const dpe_bcm::RefineLevel &lv = h->rf[l];
        RefineLaunch a{};
        RefineSide *side[2] = {&a.sp, &a.sv};
        for (int m = 0; m < 2; ++m) {
            RefineSide &s = *side[m];
            const long long dimT = lv.dim[m][3], nRows = lv.G[m] / dimT;
            s.ax = h->axes_d;
            s.offX = lv.off[m][0]; s.offY = lv.off[m][1]; s.offZ = lv.off[m][2]; s.offT = lv.off[m][3];
            s.dimY = lv.dim[m][1]; s.dimZ = lv.dim[m][2]; s.dimT = (int)dimT;
            s.nChunks = (int)((dimT + kAxT - 1) / kAxT);
            s.chunk = (int)((dimT + s.nChunks - 1) / s.nChunks);   // chunks of (nearly) equal length, as axes_side
            s.nRows = (unsigned)nRows; s.G = (unsigned)lv.G[m];
            if (l > 0) {
                const dpe_bcm::RefineLevel &pv = h->rf[l - 1];
                s.pOffX = pv.off[m][0]; s.pOffY = pv.off[m][1]; s.pOffZ = pv.off[m][2]; s.pOffT = pv.off[m][3];
                s.pDimY = pv.dim[m][1]; s.pDimZ = pv.dim[m][2]; s.pDimT = pv.dim[m][3];
                s.pG = (unsigned)pv.G[m];
            } else {
                s.pDimY = s.pDimZ = s.pDimT = 1;
            }
            s.bank = reinterpret_cast<const float2 *>(m ? carrBank_dev : codeBank_dev);
            s.sv = h->sv_d + (size_t)m * W * maxK;
            s.scores = lv.scores[m];
            s.pitch = lv.pitch[m];
            s.nEnt = m ? nBin : nLag;
            // scan_split per level from that level's tile count (a tile: 256 rows x one chunk)
            const long long nTiles = (nRows + 255) / 256 * s.nChunks;
            h->lastSplit[m] = scan_split(nTiles * kPtsPerBlock, nWindows, h->splitForce);
            s.split = (int)h->lastSplit[m];
        }
        a.level = l; a.K = nChan; a.maxK = maxK; a.lp = h->cfg.lPower;
        a.prevKeys = l ? ks.keys + (size_t)(l - 1) * 2 * W : nullptr;
        a.centres = h->rfCentre_d + (size_t)l * W * 8;
        a.prevCentres = l ? h->rfCentre_d + (size_t)(l - 1) * W * 8 : nullptr;
        // this level's rows of the set; nothing is published (no fill_tail: of the tail only these are used, and seq stays);
        // the whole other set is cleared once, by level 0
        a.keys = ks.keys + (size_t)l * 2 * W; a.oob = ks.oob + (size_t)l * 2 * W;
        a.clr = ks.other; a.clrN = l == 0 ? (int)setLen : 0;
        a.grid = dim3(h->lastSplit[0] > h->lastSplit[1] ? h->lastSplit[0] : h->lastSplit[1], nWindows, 2);
        a.lds = (size_t)nChan * n_ent_max(h->cfg) * 16 + kAxStageBytes;
        a.st = stream;
        launch_refine(!posInside, !velInside, a);
    }
    h->prof.end(0, stream);
    return launch_finish(h, ks.use);
}

int dpe_bcm_joint_set_own_keys(dpe_bcm *h, int32_t enable)
{
    DPE_REQUIRE(h && h->joint, "[BatchCorrManifold] joint_set_own_keys: not a handle of dpe_bcm_create_joint");
    h->ownKeys = enable != 0;
    return 0;
}

int dpe_bcm_update_dev(dpe_bcm *h, const float *codeBank_dev, const float *carrBank_dev, int32_t nChan, const dpe_bcm_ports_dev *ports,
                       double rxTime, dpe_stream_t stream)
{
    using namespace dpe;
    DPE_REQUIRE(h && ports, "[BatchCorrManifold] Update: null argument");
    DPE_REQUIRE(!h->joint, "[BatchCorrManifold] Update: this handle scans several receivers (dpe_bcm_create_joint): use dpe_bcm_update_joint");   // (before the prep kernel: a refusal launches nothing)
    DPE_REQUIRE(!h->epochs, "[BatchCorrManifold] Update: this handle sums consecutive windows (dpe_bcm_create_epochs): use dpe_bcm_update_epochs");
    DPE_REQUIRE(!h->subsets, "[BatchCorrManifold] Update: this handle scans SV subsets (dpe_bcm_create_subsets): use dpe_bcm_update_subsets");
    DPE_REQUIRE(!h->refine, "[BatchCorrManifold] Update: this handle scans coarse-to-fine levels (dpe_bcm_create_refine): use dpe_bcm_update_refine");   // (before the prep kernel)
    if (check_chan(h, "Update", nChan)) return -1;
    DPE_REQUIRE(!h->refPair || (h->cfg.writeScores && !h->cfg.weightedMean),
                "[BatchCorrManifold] Update: referencePair with the device ports patches the scores on the device: it needs writeScores and no weightedMean "
                "(the weighted sums are corrected on the host in the host form only)");
    DPE_REQUIRE(ports->xCurrkk1 && ports->enu2ecef && ports->satStates && ports->codePhaseEnd && ports->codeFrequency &&
                ports->carrierFrequency && ports->cpRefTOW && ports->cpElapsedEnd && ports->cpRef && ports->dopplerSign && ports->dimT >= 1,
                "[BatchCorrManifold] Update: a device port pointer is null / dimT < 1");
    const BcmPortsDev p = {ports->xCurrkk1, ports->enu2ecef, ports->satStates, ports->codePhaseEnd, ports->codeFrequency, ports->carrierFrequency,
                           ports->cpRefTOW, ports->cpElapsedEnd, ports->cpRef, ports->dopplerSign, ports->dimT};
    const size_t W = h->cfg.maxWindows, maxK = h->cfg.maxChannels;
    h->refPorts = p;
    h->refRxTime = rxTime;
    h->refRxTime_d = nullptr;
    hipLaunchKernelGGL(bcm_prep_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, p, (int)nChan, rxTime, (const double *)nullptr, h->cfg.samplingFrequency,
                       (double)h->cfg.numFFTPoints, h->cfg.samplesPerWindow, h->cfg.lagHalfWidth, h->cfg.binHalfWidth, (long long)h->cfg.numFFTPoints,
                       h->sv_d, h->sv_d + W * maxK, h->devWin_hd + (h->cur ^ 1));   // (the frame of the key set this Update reduces into)
    return bcm_update_impl(h, codeBank_dev, carrBank_dev, 1, nChan, nullptr, nullptr, stream);
}

int dpe_bcm_update_prepared(dpe_bcm *h, const float *codeBank_dev, const float *carrBank_dev, int32_t nChan, dpe_stream_t stream)
{
    DPE_REQUIRE(h, "[BatchCorrManifold] Update: null argument");
    DPE_REQUIRE(!h->joint, "[BatchCorrManifold] Update: this handle scans several receivers (dpe_bcm_create_joint): use dpe_bcm_update_joint");
    DPE_REQUIRE(!h->refine, "[BatchCorrManifold] Update: this handle scans coarse-to-fine levels (dpe_bcm_create_refine): use dpe_bcm_update_refine");
    if (check_chan(h, "Update", nChan)) return -1;
    // referencePair (batchcorrmanifold.cu:1798-1812): the prepared blocks hold expansion coefficients only, so the fp64 re-evaluation
    // reads the port arrays of the channel manager that wrote them (handed over at dpe_chm_dev_attach) -- the same device-side
    // candidates / re-evaluation / patch / arg-max kernels as dpe_bcm_update_dev, nothing read back
    DPE_REQUIRE(!h->refPair || h->refPortsAttached, "[BatchCorrManifold] Update: referencePair needs the port arrays: attach the device-resident channel "
                                                    "manager (dpe_chm_dev_attach), or use dpe_bcm_update_dev / the host form of the inputs");
    DPE_REQUIRE(!h->refPair || (h->cfg.writeScores && !h->cfg.weightedMean),
                "[BatchCorrManifold] Update: referencePair on the device patches the scores in place: it needs writeScores and no weightedMean");
    return bcm_update_impl(h, codeBank_dev, carrBank_dev, 1, nChan, nullptr, nullptr, stream);
}

int dpe_bcm_hook_set_ref_ports(dpe_bcm *h, const dpe_bcm_ports_dev *ports, const double *rxTime_dev)
{
    using namespace dpe;
    DPE_REQUIRE(h, "[BatchCorrManifold] hook: null handle");
    if (!ports) { h->refPortsAttached = false; h->refRxTime_d = nullptr; return 0; }
    h->refPorts = BcmPortsDev{ports->xCurrkk1, ports->enu2ecef, ports->satStates, ports->codePhaseEnd, ports->codeFrequency, ports->carrierFrequency,
                              ports->cpRefTOW, ports->cpElapsedEnd, ports->cpRef, ports->dopplerSign, ports->dimT};
    h->refRxTime_d = rxTime_dev;
    h->refPortsAttached = true;
    return 0;
}

int dpe_bcm_hook_get(dpe_bcm *h, dpe_bcm_hook *out)
{
    using namespace dpe;
    DPE_REQUIRE(h && out, "[BatchCorrManifold] hook: null argument");
    DPE_REQUIRE(!h->joint, "[BatchCorrManifold] hook: a joint handle (dpe_bcm_create_joint) cannot serve the device-resident loop or a dpe_pipe lane");
    DPE_REQUIRE(!h->epochs, "[BatchCorrManifold] hook: an epochs handle (dpe_bcm_create_epochs) cannot serve the device-resident loop or a dpe_pipe lane");
    DPE_REQUIRE(!h->subsets, "[BatchCorrManifold] hook: a subsets handle (dpe_bcm_create_subsets) cannot serve the device-resident loop or a dpe_pipe lane");
    DPE_REQUIRE(!h->refine, "[BatchCorrManifold] hook: a refine handle (dpe_bcm_create_refine) cannot serve the device-resident loop or a dpe_pipe lane");
    const size_t W = h->cfg.maxWindows, maxK = h->cfg.maxChannels;
    if (h->axes && !h->posAx64_d) {   // the global axes in fp64 (a few KB): the measurement kernel decodes its index from them
        dpe_bcm::Axes *ax[2] = {&h->posAx, &h->velAx};
        double **dst[2] = {&h->posAx64_d, &h->velAx64_d};
        for (int m = 0; m < 2; ++m) {
            std::vector<double> v;
            for (int c = 0; c < 4; ++c) v.insert(v.end(), ax[m]->v[c].begin(), ax[m]->v[c].end());
            *dst[m] = dev_alloc<double>(v.size());
            DPE_REQUIRE(*dst[m], "[BatchCorrManifold] hook: axes allocation failed");
            DPE_CHECK_HIP(hipMemcpy(*dst[m], v.data(), sizeof(double) * v.size(), hipMemcpyHostToDevice));
        }
    }
    if (!h->axes && !h->posGrid64_d) {
        h->posGrid64_d = dev_alloc<double>(h->posGrid_h.size());
        h->velGrid64_d = dev_alloc<double>(h->velGrid_h.size());
        DPE_REQUIRE(h->posGrid64_d && h->velGrid64_d, "[BatchCorrManifold] hook: fp64 grid allocation failed");
        DPE_CHECK_HIP(hipMemcpy(h->posGrid64_d, h->posGrid_h.data(), sizeof(double) * h->posGrid_h.size(), hipMemcpyHostToDevice));
        DPE_CHECK_HIP(hipMemcpy(h->velGrid64_d, h->velGrid_h.data(), sizeof(double) * h->velGrid_h.size(), hipMemcpyHostToDevice));
    }
    out->svPos_d = h->sv_d;
    out->svVel_d = h->sv_d + W * maxK;
    out->devWin_hd = h->devWin_hd + (h->cur ^ 1);   // the frame of the NEXT Update's key set (re-queried per window by the channel manager)
    out->keys_d[0] = h->keys_d;
    out->keys_d[1] = h->keys_d + 4 * W;
    out->posGrid64_d = h->posGrid64_d;
    out->velGrid64_d = h->velGrid64_d;
    out->posAx64_d = h->posAx64_d;
    out->velAx64_d = h->velAx64_d;
    for (int c = 0; c < 4; ++c) {
        out->posDim[c] = h->axes ? h->posAx.dim[c] : 0;
        out->velDim[c] = h->axes ? h->velAx.dim[c] : 0;
    }
    out->posG = h->cfg.posGridSize; out->velG = h->cfg.velGridSize;
    out->posOffset = h->cfg.posGridIndexOffset; out->velOffset = h->cfg.velGridIndexOffset;
    out->fs = h->cfg.samplingFrequency; out->Cf = (double)h->cfg.numFFTPoints;
    out->S = h->cfg.samplesPerWindow; out->L = h->cfg.lagHalfWidth; out->B = h->cfg.binHalfWidth;
    out->maxWindows = h->cfg.maxWindows; out->maxChannels = h->cfg.maxChannels;
    out->C = h->cfg.numFFTPoints;
    return 0;
}

int dpe_bcm_hook_set_owner(dpe_bcm *h, dpe_owner_detach_fn detach, void *owner)
{
    DPE_REQUIRE(h, "[BatchCorrManifold] hook: null handle");
    DPE_REQUIRE(!owner || !h->owner || h->owner == owner, "[BatchCorrManifold] hook: the handle is attached to another channel manager");
    h->ownerDetach = owner ? detach : nullptr;
    h->owner = owner;
    return 0;
}

int dpe_bcm_hook_set_publish(dpe_bcm *h, int enable)
{
    DPE_REQUIRE(h, "[BatchCorrManifold] hook: null argument");
    h->publish = enable != 0;
    return 0;
}

int dpe_bcm_set_graph(dpe_bcm *h, int32_t enable)
{
    DPE_REQUIRE(h, "[BatchCorrManifold] set_graph: null handle");
    DPE_REQUIRE(!h->joint || !enable, "[BatchCorrManifold] set_graph: joint Updates (dpe_bcm_update_joint) always launch eagerly");
    DPE_REQUIRE(!h->epochs || !enable, "[BatchCorrManifold] set_graph: epochs Updates (dpe_bcm_update_epochs) always launch eagerly");
    DPE_REQUIRE(!h->subsets || !enable, "[BatchCorrManifold] set_graph: subsets Updates (dpe_bcm_update_subsets) always launch eagerly");
    DPE_REQUIRE(!h->refine || !enable, "[BatchCorrManifold] set_graph: refine Updates (dpe_bcm_update_refine) always launch eagerly");
    h->graphs.enabled = enable != 0;
    if (!enable) h->graphs.clear();
    return 0;
}

static void make_meas(const dpe_bcm_window &win, const double *p, const double *v, double z[8])
{
    const double *R = win.enu2ecef, *c = win.xCurrkk1;
    z[0] = R[0] * p[0] + R[1] * p[1] + R[2] * p[2] + c[0];   // BCM_MakePosMeas :1990-1999
    z[1] = R[3] * p[0] + R[4] * p[1] + R[5] * p[2] + c[1];
    z[2] = R[6] * p[0] + R[7] * p[1] + R[8] * p[2] + c[2];
    z[3] = p[3] + c[3];
    z[4] = R[0] * v[0] + R[1] * v[1] + R[2] * v[2] + c[4];   // BCM_MakeVelMeas :2042-2051
    z[5] = R[3] * v[0] + R[4] * v[1] + R[5] * v[2] + c[5];
    z[6] = R[6] * v[0] + R[7] * v[1] + R[8] * v[2] + c[6];
    z[7] = v[3] + c[7];
}

// Point `index` (global) of manifold m: a row of the point list, or decoded from the axes ((ix dimY + iy) dimZ + iz) dimT + it
static const double *grid_point(const dpe_bcm *h, int m, int64_t index, double tmp[4])
{
    if (!h->axes) return (m ? h->velGrid_h.data() : h->posGrid_h.data()) + 4 * (index - (m ? h->cfg.velGridIndexOffset : h->cfg.posGridIndexOffset));
    const dpe_bcm::Axes &ax = m ? h->velAx : h->posAx;
    for (int c = 3; c >= 0; --c) {
        tmp[c] = ax.v[c][(size_t)(index % ax.dim[c])];
        index /= ax.dim[c];
    }
    return tmp;
}

static int64_t axes_size(const dpe_bcm::Axes &ax)
{
    return (int64_t)ax.dim[0] * ax.dim[1] * ax.dim[2] * ax.dim[3];
}

static void decode_key(unsigned long long key, float *score, int64_t *index)
{
    const unsigned int bits = (unsigned int)(key >> 32);
    memcpy(score, &bits, sizeof(float));
    *index = (int64_t)(0xFFFFFFFFu - (unsigned int)(key & 0xFFFFFFFFull));
}

// The arg-max fields the five result structs spell alike, from a key pair and its pair of out-of-window counts
extern "C++" {   // (a template inside the C-ABI block)
template <class R>
static void fill_argmax(R &r, unsigned long long posKey, unsigned long long velKey, unsigned long long posOob, unsigned long long velOob)
{
    decode_key(posKey, &r.posScore, &r.posIndex);
    decode_key(velKey, &r.velScore, &r.velIndex);
    r.posOutOfWindow = (int64_t)posOob;
    r.velOutOfWindow = (int64_t)velOob;
}
}

// The point-list rows of an arg-max pair, range-checked (index -1, which only the subsets results form: no point of the row
// had a score, a row of NaN), and the offset[8] they make
static int fill_offset(const dpe_bcm *h, const char *who, int64_t posIndex, int64_t velIndex, double offset[8], const double **pp, const double **vp)
{
    static const double nan4[4] = {NAN, NAN, NAN, NAN};
    DPE_REQUIRE(posIndex >= -1 && posIndex < h->cfg.posGridSize && velIndex >= -1 && velIndex < h->cfg.velGridSize,
                "[BatchCorrManifold] %s: arg-max index outside the grids", who);
    *pp = posIndex < 0 ? nan4 : h->posGrid_h.data() + 4 * posIndex;
    *vp = velIndex < 0 ? nan4 : h->velGrid_h.data() + 4 * velIndex;
    for (int c = 0; c < 4; ++c) { offset[c] = (*pp)[c]; offset[4 + c] = (*vp)[c]; }
    return 0;
}

// Device-parameter Updates: the window's frame (xCurrkk1, ENU2ECEFMat, DopplerSign) came from device arrays; bcm_prep_kernel
// left a copy in pinned memory ahead of the scan, valid once the stream has been waited for (or the result polled).
static int fetch_device_frame(dpe_bcm *h)
{
    if (!h->lastDev) return 0;
    const dpe::BcmDevWin &fw = h->devWin_h[h->cur];
    DPE_REQUIRE(!(fw.bad & 1), "[BatchCorrManifold] results: DopplerSign on the device is not +/-1");
    DPE_REQUIRE(!(fw.bad & 2), "[BatchCorrManifold] results: referencePair: more candidate points than the device list holds (%llu): scores partly unpatched",
                (unsigned long long)h->refCap);
    memcpy(h->win_h[0].xCurrkk1, fw.xCurrkk1, sizeof(double) * 8);
    memcpy(h->win_h[0].enu2ecef, fw.enu2ecef, sizeof(double) * 9);
    h->win_h[0].dopplerSign = fw.dopplerSign;
    return 0;
}

int dpe_bcm_results(dpe_bcm *h, dpe_bcm_result *results, dpe_stream_t stream)
{
    DPE_REQUIRE(h && results && h->lastW > 0, "[BatchCorrManifold] results: no update yet");
    DPE_REQUIRE(!h->joint, "[BatchCorrManifold] results: this handle scans several receivers (dpe_bcm_create_joint): use dpe_bcm_results_joint");
    DPE_REQUIRE(!h->epochs, "[BatchCorrManifold] results: this handle sums consecutive windows (dpe_bcm_create_epochs): use dpe_bcm_results_epochs");
    DPE_REQUIRE(!h->subsets, "[BatchCorrManifold] results: this handle scans SV subsets (dpe_bcm_create_subsets): use dpe_bcm_results_subsets");
    DPE_REQUIRE(!h->refine, "[BatchCorrManifold] results: this handle scans coarse-to-fine levels (dpe_bcm_create_refine): use dpe_bcm_results_refine");
    // Single-window Updates: the scan's last block writes a sequence word right behind the results in the pinned
    // mirror.  Polling it returns the fix as soon as it lands, without the stream-wait wake-up (a few us of a ~58 us
    // closed-loop window); anything unexpected falls back to the stream wait.
    bool arrived = false;
    if (h->pollable) {
        const unsigned long long *seqWord = h->oob_h + 2;
        for (int spin = 0; spin < 200000 && !arrived; ++spin)
            arrived = (__atomic_load_n(seqWord, __ATOMIC_ACQUIRE) == h->seq);   // acquire: the results are read after it
    }
    if (!arrived) DPE_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    const int W = h->lastW;
    if (!h->lastPublished) {   // the scan did not write the host mirror (device-resident loop): fetch keys and counts of the set it used
        const size_t Wm = h->cfg.maxWindows;
        DPE_CHECK_HIP(hipMemcpy(h->keys_h, h->keys_d + (size_t)h->cur * 4 * Wm, sizeof(unsigned long long) * 2 * Wm, hipMemcpyDeviceToHost));
        DPE_CHECK_HIP(hipMemcpy(h->oob_h, h->keys_d + (size_t)h->cur * 4 * Wm + 2 * Wm, sizeof(unsigned long long) * 2 * Wm, hipMemcpyDeviceToHost));
    }
    if (fetch_device_frame(h)) return -1;
    const unsigned long long *keys = h->keys_h, *oob = h->oob_h;
    std::vector<double> ws;   // per-block weighted sums: fetched only when the estimator is on (this call sits on the
                              // closed loop's critical path: no 300 KB of scratch per window otherwise)
    if (h->cfg.weightedMean) {
        ws.resize(2 * h->wsumHalf);
        DPE_CHECK_HIP(hipMemcpy(ws.data(), h->wsum_d, sizeof(double) * 2 * h->wsumHalf, hipMemcpyDeviceToHost));
    }
    for (int w = 0; w < W; ++w) {
        dpe_bcm_result &r = results[w];
        // "Method 1" score-weighted mean of the manifold (BCM_PosMeasReduction / BCM_ReduceAndPosMeas,
        // batchcorrmanifold.cu:816-1056,1365-1510; PyGNSS receiver.py:317-318): LOCAL shard only
        double m[2][5] = {};
        for (int slot = 0; slot < 2; ++slot) {
            if (h->cfg.weightedMean) {
                const double *base = ws.data() + slot * h->wsumHalf + (size_t)w * h->lastSplit[slot] * 5;
                for (unsigned b = 0; b < h->lastSplit[slot]; ++b)
                    for (int j = 0; j < 5; ++j) m[slot][j] += base[(size_t)b * 5 + j];
                if (slot == 0 && h->refPair && !h->refWsum.empty())
                    for (int j = 0; j < 5; ++j) m[0][j] += h->refWsum[(size_t)w * 5 + j];
            }
            for (int j = 0; j < 5; ++j) r.weightedSums[slot][j] = m[slot][j];
        }
        if (!h->cfg.weightedMean) {
            for (int j = 0; j < 8; ++j) r.zValMean[j] = 0.0;
        } else {
            const double pm[4] = {m[0][1] / m[0][0], m[0][2] / m[0][0], m[0][3] / m[0][0], m[0][4] / m[0][0]};
            const double vm[4] = {m[1][1] / m[1][0], m[1][2] / m[1][0], m[1][3] / m[1][0], m[1][4] / m[1][0]};
            make_meas(h->win_h[w], pm, vm, r.zValMean);
        }
        fill_argmax(r, keys[2 * w], keys[2 * w + 1], oob[2 * w], oob[2 * w + 1]);
        const int64_t pl = r.posIndex - h->cfg.posGridIndexOffset, vl = r.velIndex - h->cfg.velGridIndexOffset;
        DPE_REQUIRE(pl >= 0 && pl < h->cfg.posGridSize && vl >= 0 && vl < h->cfg.velGridSize,
                    "[BatchCorrManifold] results: arg-max index outside the local shard");
        double pt[4], vt[4];
        make_meas(h->win_h[w], grid_point(h, 0, r.posIndex, pt), grid_point(h, 1, r.velIndex, vt), r.zVal);
    }
    return 0;
}

int dpe_bcm_results_joint(dpe_bcm *h, dpe_bcm_joint_result *joint, dpe_bcm_joint_rx_result *perRx, dpe_stream_t stream)
{
    DPE_REQUIRE(h && joint && perRx, "[BatchCorrManifold] results_joint: null argument");
    DPE_REQUIRE(h->joint && h->lastW > 0 && h->lastRx > 0, "[BatchCorrManifold] results_joint: no joint update yet");
    DPE_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    const int W = h->lastW, nRx = h->lastRx, maxRx = h->jointMaxRx;
    const size_t Wm = h->cfg.maxWindows, half = 2 * Wm * maxRx;
    DPE_CHECK_HIP(hipMemcpy(h->own_h.data(), h->own_d, sizeof(unsigned long long) * 2 * half, hipMemcpyDeviceToHost));
    const unsigned long long *keys = h->keys_h, *oob = h->oob_h;
    for (int w = 0; w < W; ++w) {
        dpe_bcm_joint_result &j = joint[w];
        fill_argmax(j, keys[2 * w], keys[2 * w + 1], oob[2 * w], oob[2 * w + 1]);
        const double *pp, *vp;
        if (fill_offset(h, "results_joint", j.posIndex, j.velIndex, j.offset, &pp, &vp)) return -1;
        for (int r = 0; r < nRx; ++r) {
            dpe_bcm_joint_rx_result &o = perRx[(size_t)w * nRx + r];
            make_meas(h->jwin_h[(size_t)w * maxRx + r], pp, vp, o.zVal);   // this receiver's centre moved by the joint offset
            const size_t ps = ((size_t)w * 2 + 0) * maxRx + r, vs = ((size_t)w * 2 + 1) * maxRx + r;
            fill_argmax(o, h->own_h[ps], h->own_h[vs], h->own_h[half + ps], h->own_h[half + vs]);
            if (!h->lastOwn) {
                o.posIndex = o.velIndex = -1;
                o.posScore = o.velScore = 0.f;
            }
        }
    }
    return 0;
}

int dpe_bcm_results_epochs(dpe_bcm *h, dpe_bcm_epochs_result *results, dpe_stream_t stream)
{
    DPE_REQUIRE(h && results, "[BatchCorrManifold] results_epochs: null argument");
    if (check_kind(h->epochs, "results_epochs", "dpe_bcm_create_epochs")) return -1;
    DPE_REQUIRE(h->lastW > 0 && h->lastEpochs > 0, "[BatchCorrManifold] results_epochs: no epochs update yet");
    DPE_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    const unsigned long long *keys = h->keys_h, *oob = h->oob_h;
    for (int g = 0; g < h->lastW; ++g) {
        dpe_bcm_epochs_result &r = results[g];
        fill_argmax(r, keys[2 * g], keys[2 * g + 1], oob[2 * g], oob[2 * g + 1]);
        r.nPasses = h->lastPasses;
        r.reserved = 0;
        const double *pp, *vp;
        if (fill_offset(h, "results_epochs", r.posIndex, r.velIndex, r.offset, &pp, &vp)) return -1;
        make_meas(h->win_h[(size_t)g * h->lastEpochs + h->lastEpochs - 1], pp, vp, r.zVal);   // the LAST window's centre moved by the ML offset
    }
    return 0;
}

int dpe_bcm_results_subsets(dpe_bcm *h, dpe_bcm_subset_result *full, dpe_bcm_subset_result *subs, int64_t *oobPerSv, dpe_stream_t stream)
{
    DPE_REQUIRE(h && full, "[BatchCorrManifold] results_subsets: null argument");
    if (check_kind(h->subsets, "results_subsets", "dpe_bcm_create_subsets")) return -1;
    DPE_REQUIRE(h->lastW > 0, "[BatchCorrManifold] results_subsets: no subsets update yet");
    DPE_REQUIRE(subs || h->lastSubsets == 0, "[BatchCorrManifold] results_subsets: null argument (the last Update ran %d subsets)", h->lastSubsets);
    DPE_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    const int W = h->lastW, M = h->lastSubsets, K = h->lastChan, maxS = h->subMax, maxK = h->cfg.maxChannels;
    const size_t Wm = h->cfg.maxWindows;
    // keys and counts only (the masks in front of them are the host's own); nothing was written when no subset was asked for and
    // no variant clamped
    if (M > 0 || h->lastCounted)
        DPE_CHECK_HIP(hipMemcpy(h->sub_h.data() + Wm * maxS, h->sub_d + Wm * maxS, sizeof(unsigned long long) * (h->sub_h.size() - Wm * maxS),
                                hipMemcpyDeviceToHost));
    if (!h->lastCounted) std::fill(h->sub_h.begin() + 3 * Wm * maxS, h->sub_h.end(), 0ull);
    const unsigned long long *subKeys = h->sub_h.data() + Wm * maxS, *svOob = subKeys + 2 * Wm * maxS;
    const unsigned long long *keys = h->keys_h, *oob = h->oob_h;
    // A key of 0 means that no point of the row had a score (every sum NaN: a channel with NaN banks in the set): index -1,
    // score 0 and NaN offsets / zVal for that manifold -- the other subsets of the window, which leave that channel out, stand.
    const auto fill = [&](dpe_bcm_subset_result &r, int w, unsigned long long pk, unsigned long long vk, unsigned long long pc, unsigned long long vc) -> int {
        fill_argmax(r, pk, vk, pc, vc);
        if (!pk) { r.posIndex = -1; r.posScore = 0.f; }
        if (!vk) { r.velIndex = -1; r.velScore = 0.f; }
        const double *pp, *vp;
        if (fill_offset(h, "results_subsets", r.posIndex, r.velIndex, r.offset, &pp, &vp)) return -1;
        make_meas(h->win_h[w], pp, vp, r.zVal);
        return 0;
    };
    for (int w = 0; w < W; ++w) {
        if (fill(full[w], w, keys[2 * w], keys[2 * w + 1], oob[2 * w], oob[2 * w + 1])) return -1;
        const unsigned long long *po = svOob + ((size_t)w * 2 + 0) * maxK, *vo = svOob + ((size_t)w * 2 + 1) * maxK;
        for (int k = 0; oobPerSv && k < K; ++k) {
            oobPerSv[((size_t)w * 2 + 0) * K + k] = (int64_t)po[k];
            oobPerSv[((size_t)w * 2 + 1) * K + k] = (int64_t)vo[k];
        }
        for (int m = 0; m < M; ++m) {
            const unsigned long long mask = h->subMask_h[(size_t)w * maxS + m];
            unsigned long long pc = 0, vc = 0;
            for (int k = 0; k < K; ++k)
                if ((mask >> k) & 1ull) { pc += po[k]; vc += vo[k]; }   // a subset's count: the sum of its SVs'
            if (fill(subs[(size_t)w * M + m], w, subKeys[((size_t)w * 2 + 0) * maxS + m], subKeys[((size_t)w * 2 + 1) * maxS + m], pc, vc)) return -1;
        }
    }
    return 0;
}

int dpe_bcm_results_refine(dpe_bcm *h, dpe_bcm_refine_result *results, dpe_stream_t stream)
{
    DPE_REQUIRE(h && results, "[BatchCorrManifold] results_refine: null argument");
    if (check_kind(h->refine, "results_refine", "dpe_bcm_create_refine")) return -1;
    DPE_REQUIRE(h->lastW > 0, "[BatchCorrManifold] results_refine: no refine update yet");
    DPE_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    const int W = h->lastW, nL = h->rfLevels;
    const size_t Wm = h->cfg.maxWindows, setLen = 4 * Wm * nL;
    DPE_CHECK_HIP(hipMemcpy(h->rfKeys_h.data(), h->rfKeys_d + (size_t)h->cur * setLen, sizeof(unsigned long long) * setLen, hipMemcpyDeviceToHost));
    const unsigned long long *keys = h->rfKeys_h.data(), *oob = keys + 2 * Wm * nL;
    for (int w = 0; w < W; ++w) {
        dpe_bcm_refine_result &r = results[w];
        double pt[2][4];
        for (int m = 0; m < 2; ++m) {
            int64_t *index = m ? r.velIndex : r.posIndex, *count = m ? r.velOutOfWindow : r.posOutOfWindow;
            float *score = m ? r.velScore : r.posScore;
            float c[4] = {0.f, 0.f, 0.f, 0.f};   // the centre chain, with the device's own fp32 additions
            bool alive = true;
            for (int l = 0; l < DPE_REFINE_MAX_LEVELS; ++l) {
                index[l] = -1; score[l] = 0.f; count[l] = 0;
                if (l >= nL) continue;
                const unsigned long long key = keys[((size_t)l * Wm + w) * 2 + m];
                if (!key) alive = false;   // no point scored here: this and every later level were not scanned
                if (!alive) continue;
                decode_key(key, &score[l], &index[l]);
                count[l] = (int64_t)oob[((size_t)l * Wm + w) * 2 + m];
                const dpe_bcm::RefineLevel &lv = h->rf[l];
                DPE_REQUIRE(index[l] >= 0 && index[l] < lv.G[m], "[BatchCorrManifold] results_refine: arg-max index outside level %d's grid", l);
                int64_t rest = index[l];
                for (int a = 3; a >= 0; --a) {
                    c[a] = c[a] + lv.v[m][a][(size_t)(rest % lv.dim[m][a])];   // fp32: rounded once, as on the device
                    rest /= lv.dim[m][a];
                }
            }
            for (int a = 0; a < 4; ++a) pt[m][a] = alive ? (double)c[a] : (double)NAN;
        }
        for (int a = 0; a < 4; ++a) { r.offset[a] = pt[0][a]; r.offset[4 + a] = pt[1][a]; }
        make_meas(h->win_h[w], pt[0], pt[1], r.zVal);
    }
    return 0;
}

static int check_refine_level(const dpe_bcm *h, const char *who, int level)
{
    if (check_kind(h->refine, who, "dpe_bcm_create_refine")) return -1;
    DPE_REQUIRE(level >= 0 && level < h->rfLevels, "[BatchCorrManifold] %s: level %d out of range (the handle holds %d levels)", who, level, h->rfLevels);
    return 0;
}

int dpe_bcm_refine_scores(dpe_bcm *h, int32_t level, const float **pos_dev, const float **vel_dev, int64_t *posPitch, int64_t *velPitch)
{
    DPE_REQUIRE(h, "[BatchCorrManifold] refine_scores: null handle");
    if (check_refine_level(h, "refine_scores", level)) return -1;
    DPE_REQUIRE(h->cfg.writeScores, "[BatchCorrManifold] refine_scores: created with writeScores=0");
    if (pos_dev) *pos_dev = h->rf[level].scores[0];
    if (vel_dev) *vel_dev = h->rf[level].scores[1];
    if (posPitch) *posPitch = h->rf[level].pitch[0];
    if (velPitch) *velPitch = h->rf[level].pitch[1];
    return 0;
}

int dpe_bcm_refine_keys(dpe_bcm *h, int32_t level, const uint64_t **keys_dev)
{
    DPE_REQUIRE(h && keys_dev, "[BatchCorrManifold] refine_keys: null argument");
    if (check_refine_level(h, "refine_keys", level)) return -1;
    const size_t W = h->cfg.maxWindows;
    *keys_dev = reinterpret_cast<const uint64_t *>(h->rfKeys_d + (size_t)h->cur * 4 * W * h->rfLevels + (size_t)level * 2 * W);
    return 0;
}

int dpe_bcm_profile(dpe_bcm *h, int32_t enable, float *ms, int32_t *count)
{
    DPE_REQUIRE(h, "[BatchCorrManifold] profile: null handle");
    float m[dpe::KernelProfiler::kSlots];
    int c[dpe::KernelProfiler::kSlots];
    h->prof.collect(m, c);
    for (int i = 0; i < 2; ++i) {
        if (ms) ms[i] = m[i];
        if (count) count[i] = c[i];
    }
    h->prof.enabled = enable != 0;
    return 0;
}

int dpe_bcm_scores(dpe_bcm *h, const float **posScores_dev, const float **velScores_dev)
{
    DPE_REQUIRE(h, "[BatchCorrManifold] scores: null handle");
    DPE_REQUIRE(!h->refine, "[BatchCorrManifold] scores: a refine handle (dpe_bcm_create_refine) keeps rows per level: use dpe_bcm_refine_scores");
    DPE_REQUIRE(h->cfg.writeScores, "[BatchCorrManifold] scores: created with writeScores=0");
    if (posScores_dev) *posScores_dev = h->posScores_d;
    if (velScores_dev) *velScores_dev = h->velScores_d;
    return 0;
}

int dpe_bcm_export_scores_f64(dpe_bcm *h, int32_t window, double *posScores_dev, double *velScores_dev, dpe_stream_t stream)
{
    DPE_REQUIRE(h && h->cfg.writeScores, "[BatchCorrManifold] export_scores_f64: created with writeScores=0");
    DPE_REQUIRE(!h->refine, "[BatchCorrManifold] export_scores_f64: a refine handle (dpe_bcm_create_refine) keeps rows per level: use dpe_bcm_refine_scores");
    DPE_REQUIRE(window >= 0 && window < h->lastW, "[BatchCorrManifold] export_scores_f64: bad window %d", window);
    const long long Gp = h->cfg.posGridSize, Gv = h->cfg.velGridSize;
    if (posScores_dev)
        hipLaunchKernelGGL(dpe::bcm_export_f64_kernel, dim3((unsigned)((Gp + 1023) / 1024 > 1024 ? 1024 : (Gp + 1023) / 1024)), dim3(256), 0,
                           (hipStream_t)stream, h->posScores_d + (size_t)window * h->posPitch, Gp, posScores_dev);
    if (velScores_dev)
        hipLaunchKernelGGL(dpe::bcm_export_f64_kernel, dim3((unsigned)((Gv + 1023) / 1024 > 1024 ? 1024 : (Gv + 1023) / 1024)), dim3(256), 0,
                           (hipStream_t)stream, h->velScores_d + (size_t)window * h->velPitch, Gv, velScores_dev);
    DPE_CHECK_HIP(hipGetLastError());
    return 0;
}

int dpe_bcm_scores_pitch(dpe_bcm *h, int64_t *posPitch, int64_t *velPitch)
{
    DPE_REQUIRE(h, "[BatchCorrManifold] scores_pitch: null handle");
    DPE_REQUIRE(!h->refine, "[BatchCorrManifold] scores_pitch: a refine handle (dpe_bcm_create_refine) keeps rows per level: use dpe_bcm_refine_scores");
    if (posPitch) *posPitch = h->posPitch;
    if (velPitch) *velPitch = h->velPitch;
    return 0;
}

int dpe_bcm_keys(dpe_bcm *h, const uint64_t **keys_dev)
{
    DPE_REQUIRE(h && keys_dev, "[BatchCorrManifold] keys: null argument");
    DPE_REQUIRE(!h->refine, "[BatchCorrManifold] keys: a refine handle (dpe_bcm_create_refine) keeps keys per level: use dpe_bcm_refine_keys");
    *keys_dev = reinterpret_cast<const uint64_t *>(h->keys_d + (size_t)h->cur * 4 * h->cfg.maxWindows);
    return 0;
}

int dpe_bcm_last_split(dpe_bcm *h, int32_t split[2])
{
    DPE_REQUIRE(h && split, "[BatchCorrManifold] last_split: null argument");
    DPE_REQUIRE(h->lastSplit[0] > 0 && h->lastSplit[1] > 0, "[BatchCorrManifold] last_split: no Update yet");
    split[0] = (int32_t)h->lastSplit[0];
    split[1] = (int32_t)h->lastSplit[1];
    return 0;
}

int dpe_bcm_exchange_keys(dpe_bcm *h, dpe_comm *c, uint64_t *keys_host, dpe_stream_t stream)
{
    DPE_REQUIRE(h && c && h->lastW > 0, "[BatchCorrManifold] exchange_keys: no update yet / null communicator");
    DPE_REQUIRE(!h->joint, "[BatchCorrManifold] exchange_keys: a joint handle (dpe_bcm_create_joint) scans whole grids: sharding is not supported");
    DPE_REQUIRE(!h->epochs, "[BatchCorrManifold] exchange_keys: an epochs handle (dpe_bcm_create_epochs) scans whole grids: sharding is not supported");
    DPE_REQUIRE(!h->subsets, "[BatchCorrManifold] exchange_keys: a subsets handle (dpe_bcm_create_subsets) scans whole grids: sharding is not supported");
    DPE_REQUIRE(!h->refine, "[BatchCorrManifold] exchange_keys: a refine handle (dpe_bcm_create_refine) scans whole grids: sharding is not supported");
    unsigned long long *keys = h->keys_d + (size_t)h->cur * 4 * h->cfg.maxWindows;
    if (dpe_comm_allreduce_max_u64(c, reinterpret_cast<uint64_t *>(keys), 2 * (int64_t)h->lastW, stream)) return -1;
    if (keys_host) {
        DPE_CHECK_HIP(hipMemcpyAsync(keys_host, keys, sizeof(uint64_t) * 2 * (size_t)h->lastW, hipMemcpyDeviceToHost, (hipStream_t)stream));
        DPE_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    }
    h->pollable = false;   // the host mirror still holds this rank's LOCAL keys
    return 0;
}

int dpe_bcm_results_from_keys(dpe_bcm *h, const uint64_t *keys_host, int32_t nWindows, const double *posGridGlobal,
                              int64_t posGridGlobalSize, const double *velGridGlobal, int64_t velGridGlobalSize,
                              dpe_bcm_result *results)
{
    DPE_REQUIRE(h && keys_host && results && (posGridGlobal != nullptr) == (velGridGlobal != nullptr) && (posGridGlobal || h->axes),
                "[BatchCorrManifold] results_from_keys: null argument (both global grids, or neither for a handle with grid axes)");
    DPE_REQUIRE(!h->joint, "[BatchCorrManifold] results_from_keys: a joint handle (dpe_bcm_create_joint) scans whole grids: use dpe_bcm_results_joint");
    DPE_REQUIRE(!h->epochs, "[BatchCorrManifold] results_from_keys: an epochs handle (dpe_bcm_create_epochs) scans whole grids: use dpe_bcm_results_epochs");
    DPE_REQUIRE(!h->subsets, "[BatchCorrManifold] results_from_keys: a subsets handle (dpe_bcm_create_subsets) scans whole grids: use dpe_bcm_results_subsets");
    DPE_REQUIRE(!h->refine, "[BatchCorrManifold] results_from_keys: a refine handle (dpe_bcm_create_refine) scans whole grids: use dpe_bcm_results_refine");
    if (!posGridGlobal) {   // an axes handle decodes from its axes, which are the global ones
        posGridGlobalSize = axes_size(h->posAx);
        velGridGlobalSize = axes_size(h->velAx);
    }
    DPE_REQUIRE(nWindows >= 1 && nWindows <= h->lastW, "[BatchCorrManifold] results_from_keys: bad nWindows");
    if (fetch_device_frame(h)) return -1;   // (the reduced keys came through a synchronising copy: the scan has finished)
    for (int w = 0; w < nWindows; ++w) {
        dpe_bcm_result &r = results[w];
        DPE_REQUIRE(keys_host[2 * w] != 0 && keys_host[2 * w + 1] != 0,
                    "[BatchCorrManifold] results_from_keys: window %d has no valid score (key 0)", w);
        decode_key(keys_host[2 * w], &r.posScore, &r.posIndex);
        decode_key(keys_host[2 * w + 1], &r.velScore, &r.velIndex);
        DPE_REQUIRE(r.posIndex >= 0 && r.posIndex < posGridGlobalSize && r.velIndex >= 0 && r.velIndex < velGridGlobalSize,
                    "[BatchCorrManifold] results_from_keys: window %d: arg-max index (%lld, %lld) outside the global grids (%lld, %lld)",
                    w, (long long)r.posIndex, (long long)r.velIndex, (long long)posGridGlobalSize, (long long)velGridGlobalSize);
        r.posOutOfWindow = r.velOutOfWindow = -1;
        for (int j = 0; j < 8; ++j) r.zValMean[j] = 0.0;   // needs the all-reduced weightedSums; see sharding.py
        for (int j = 0; j < 10; ++j) (&r.weightedSums[0][0])[j] = 0.0;
        double pt[4], vt[4];
        make_meas(h->win_h[w], posGridGlobal ? posGridGlobal + 4 * r.posIndex : grid_point(h, 0, r.posIndex, pt),
                  velGridGlobal ? velGridGlobal + 4 * r.velIndex : grid_point(h, 1, r.velIndex, vt), r.zVal);
    }
    return 0;
}

// ---- thresholded moments of the score rows (dpe_bcm_moments.h) ----------------
// Blocks along x per row, by scan_split's rule of thumb: 128 for one or two windows (latency), 24 for batches, never more than
// the row's 1024-point tiles
static unsigned moments_split(long long G, int nWindows)
{
    const long long nTiles = (G + dpe::kPtsPerBlock - 1) / dpe::kPtsPerBlock;
    const long long s = nWindows <= 2 ? 128 : 24;
    return (unsigned)(s < nTiles ? s : nTiles);
}

static size_t moments_partial_len(int maxWindows)   // doubles: >= nWindows * 2 * blocks per row * kMomSlots of any launch
{
    const size_t rows = (size_t)std::max(2 * 128, 24 * maxWindows);
    return 2 * rows * dpe::kMomSlots;
}

// The launch set-up dpe_bcm_moments and the device-resident loop (dpe_bcm_hook_moments_launch) share: the two manifolds' sides from
// the handle's rows and grids (or cfg's overrides), and the launch over (blocks per row, nW, 2) into partial_d.  Returns gridDim.x.
static unsigned moments_launch(dpe_bcm *h, const dpe_bcm_moments_config *cfg, int nW, const unsigned long long *keys, double *partial_d,
                               dpe::MomSide (&sd)[2], hipStream_t stream)
{
    using namespace dpe;
    const long long G[2] = {h->cfg.posGridSize, h->cfg.velGridSize};
    sd[0] = MomSide{}; sd[1] = MomSide{};
    for (int m = 0; m < 2; ++m) {
        MomSide &s = sd[m];
        const float *over = m ? cfg->velScores_dev : cfg->posScores_dev;
        s.scores = over ? over : (m ? h->velScores_d : h->posScores_d);
        s.pitch = over ? (long long)(m ? cfg->velPitch : cfg->posPitch) : (m ? h->velPitch : h->posPitch);
        s.G = G[m];
        s.vec = ((uintptr_t)s.scores % 16 == 0 && s.pitch % 4 == 0) ? 1 : 0;
        s.rho = (float)cfg->rho[m];
        s.split = (int)moments_split(G[m], nW);
        if (h->axes) {
            const dpe_bcm::Axes &ax = m ? h->velAx : h->posAx;
            s.ax = h->axes_d;
            s.offX = h->axOff[m][0]; s.offY = h->axOff[m][1]; s.offZ = h->axOff[m][2]; s.offT = h->axOff[m][3];
            s.dimY = (unsigned)ax.dim[1]; s.dimZ = (unsigned)ax.dim[2]; s.dimT = (unsigned)ax.dim[3];
            s.gBegin = (unsigned)(m ? h->cfg.velGridIndexOffset : h->cfg.posGridIndexOffset);
        } else {
            s.grid = m ? h->velGrid_d : h->posGrid_d;
        }
    }
    const unsigned nBlk = (unsigned)std::max(sd[0].split, sd[1].split);
    const dim3 grid(nBlk, (unsigned)nW, 2);
    if (h->axes) hipLaunchKernelGGL(bcm_moments_kernel<true>, grid, dim3(256), 0, stream, sd[0], sd[1], keys, partial_d);
    else hipLaunchKernelGGL(bcm_moments_kernel<false>, grid, dim3(256), 0, stream, sd[0], sd[1], keys, partial_d);
    return nBlk;
}

int dpe_bcm_moments(dpe_bcm *h, const dpe_bcm_moments_config *cfg, dpe_stream_t stream_)
{
    using namespace dpe;
    DPE_REQUIRE(cfg, "[BatchCorrManifold] moments: null config");
    for (int m = 0; m < 2; ++m)
        DPE_REQUIRE(std::isfinite(cfg->rho[m]) && cfg->rho[m] >= 0.0 && cfg->rho[m] < 1.0,
                    "[BatchCorrManifold] moments: rho[%d] = %g outside [0, 1) (%s manifold)", m, cfg->rho[m], m ? "velocity" : "position");
    DPE_REQUIRE(h, "[BatchCorrManifold] moments: null handle");
    DPE_REQUIRE(!h->joint, "[BatchCorrManifold] moments: a joint handle (dpe_bcm_create_joint) is not supported (its rows sum several receivers)");
    DPE_REQUIRE(!h->epochs, "[BatchCorrManifold] moments: an epochs handle (dpe_bcm_create_epochs) is not supported (its rows sum several windows)");
    DPE_REQUIRE(!h->subsets, "[BatchCorrManifold] moments: a subsets handle (dpe_bcm_create_subsets) is not supported (its keys are per subset)");
    DPE_REQUIRE(!h->refine, "[BatchCorrManifold] moments: a refine handle (dpe_bcm_create_refine) is not supported (its rows and grids are per level)");
    DPE_REQUIRE(h->lastW > 0, "[BatchCorrManifold] moments: no update yet");
    hipStream_t stream = (hipStream_t)stream_;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (stream) (void)hipStreamIsCapturing(stream, &cap);
    DPE_REQUIRE(!h->graphs.capturing && cap == hipStreamCaptureStatusNone,
                "[BatchCorrManifold] moments: the stream is being captured (the call allocates on first use and is not part of the Update's graph)");
    DPE_REQUIRE(h->cfg.writeScores || (cfg->posScores_dev && cfg->velScores_dev),
                "[BatchCorrManifold] moments: created with writeScores=0 (the handle has no score rows: pass posScores_dev and velScores_dev)");
    const int maxW = h->cfg.maxWindows;
    const bool allOver = cfg->keys_dev && cfg->posScores_dev && cfg->velScores_dev;
    const int nW = cfg->nWindows ? cfg->nWindows : h->lastW, limit = allOver ? maxW : h->lastW;
    DPE_REQUIRE(nW >= 1 && nW <= limit, "[BatchCorrManifold] moments: nWindows %d out of range (1 .. %d: %s)", nW, limit,
                allOver ? "maxWindows, rows and keys overridden" : "the last Update's count");
    const long long G[2] = {h->cfg.posGridSize, h->cfg.velGridSize};
    DPE_REQUIRE(!cfg->posScores_dev || cfg->posPitch >= G[0], "[BatchCorrManifold] moments: posPitch %lld is below the position grid size %lld",
                (long long)cfg->posPitch, G[0]);
    DPE_REQUIRE(!cfg->velScores_dev || cfg->velPitch >= G[1], "[BatchCorrManifold] moments: velPitch %lld is below the velocity grid size %lld",
                (long long)cfg->velPitch, G[1]);
    if (!h->momPartial_d) {   // first use
        double *partial = dev_alloc<double>(moments_partial_len(maxW)), *sums = dev_alloc<double>((size_t)maxW * 2 * kMomSums);
        long long *above = dev_alloc<long long>((size_t)maxW * 2);
        MomMirror *mirror = nullptr, *mirrorDev = nullptr;
        if (!partial || !sums || !above || hipHostMalloc((void **)&mirror, sizeof(MomMirror) * 2 * maxW, hipHostMallocDefault) != hipSuccess ||
            hipHostGetDevicePointer((void **)&mirrorDev, mirror, 0) != hipSuccess) {
            (void)hipFree(partial); (void)hipFree(sums); (void)hipFree(above);
            if (mirror) (void)hipHostFree(mirror);
            set_error("[BatchCorrManifold] moments: allocation failed");
            return -1;
        }
        memset(mirror, 0, sizeof(MomMirror) * 2 * maxW);
        h->momPartial_d = partial; h->momSums_d = sums; h->momAbove_d = above; h->momMirror_h = mirror; h->momMirror_hd = mirrorDev;
    }
    const unsigned long long *keys = cfg->keys_dev ? reinterpret_cast<const unsigned long long *>(cfg->keys_dev)
                                                   : h->keys_d + (size_t)h->cur * 4 * maxW;
    MomSide sd[2];
    const unsigned nBlk = moments_launch(h, cfg, nW, keys, h->momPartial_d, sd, stream);
    hipLaunchKernelGGL(bcm_moments_finish_kernel, dim3((unsigned)((2 * nW * kMomSlots + 255) / 256)), dim3(256), 0, stream, h->momPartial_d, (int)nBlk,
                       sd[0].split, sd[1].split, keys, sd[0].rho, sd[1].rho, nW, h->momSums_d, h->momAbove_d, h->momMirror_hd);
    DPE_CHECK_HIP(hipGetLastError());
    h->momW = nW;
    return 0;
}

int dpe_bcm_moments_from_sums(const double sums[2][15], const double centre[8], const double enu2ecef[9], double zValMom[8], double RValMom[64])
{
#pragma clang fp contract(off)   // (S2 - mu S1 must cancel to an exact 0 for a single point: no fused multiply-add)
    DPE_REQUIRE(sums && centre && enu2ecef && zValMom && RValMom, "[BatchCorrManifold] moments_from_sums: null argument");
    double J[4][4];
    dpe::mom_frame(enu2ecef, J);
    for (int i = 0; i < 64; ++i) RValMom[i] = 0.0;
    for (int m = 0; m < 2; ++m) {
        double mu[4], M[4][4];
        dpe::mom_cov_block(sums[m], J, mu, M);   // (shared with dpe_bcm_moments_rval and the device loop: dpe_bcm_moments_cov.h)
        for (int a = 0; a < 4; ++a) {
            double z = centre[4 * m + a];
            for (int b = 0; b < 4; ++b) z += J[a][b] * mu[b];   // (J is exact 0 / 1 outside the rotation: dt adds as it is)
            zValMom[4 * m + a] = z;
        }
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) RValMom[(4 * m + a) * 8 + 4 * m + b] = M[a][b];
    }
    return 0;
}

int dpe_bcm_moments_rval(const double sums[2][15], const double enu2ecef[9], const double floorVar[2][4], double R[64], int32_t *fallback)
{
    DPE_REQUIRE(sums && enu2ecef && floorVar && R && fallback, "[BatchCorrManifold] moments_rval: null argument");
    for (int m = 0; m < 2; ++m)
        for (int c = 0; c < 4; ++c)
            DPE_REQUIRE(std::isfinite(floorVar[m][c]) && floorVar[m][c] >= 0.0, "[BatchCorrManifold] moments_rval: floorVar[%d][%d] = %g is negative or not finite",
                        m, c, floorVar[m][c]);
    *fallback = dpe::mom_rval(&sums[0][0], enu2ecef, &floorVar[0][0], R);
    return 0;
}

int dpe_bcm_moments_results(dpe_bcm *h, dpe_bcm_moments_result *out, dpe_stream_t stream)
{
    DPE_REQUIRE(h && out, "[BatchCorrManifold] moments_results: null argument");
    DPE_REQUIRE(h->momW > 0 && h->momMirror_h, "[BatchCorrManifold] moments_results: no moments call yet");
    DPE_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    for (int w = 0; w < h->momW; ++w) {
        dpe_bcm_moments_result &r = out[w];
        for (int m = 0; m < 2; ++m) {
            const dpe::MomMirror &mm = h->momMirror_h[2 * w + m];
            for (int j = 0; j < dpe::kMomSums; ++j) r.sums[m][j] = mm.sums[j];
            r.nAbove[m] = (int64_t)mm.nAbove;
            r.threshold[m] = mm.tau;
        }
        // the window's frame: a device-parameter Update left it in the pinned frame of its key set (bcm_prep_kernel)
        if (w >= h->lastW) {   // overridden rows beyond the last Update's windows: sums, but no frame to move them into
            for (double &v : r.zValMom) v = (double)NAN;
            for (double &v : r.RValMom) v = (double)NAN;
            continue;
        }
        const bool devFrame = h->lastDev && w == 0;
        const double *centre = devFrame ? h->devWin_h[h->cur].xCurrkk1 : h->win_h[w].xCurrkk1;
        const double *R = devFrame ? h->devWin_h[h->cur].enu2ecef : h->win_h[w].enu2ecef;
        if (dpe_bcm_moments_from_sums(r.sums, centre, R, r.zValMom, r.RValMom)) return -1;
    }
    return 0;
}

int dpe_bcm_moments_dev(dpe_bcm *h, const double **sums_dev, const int64_t **nAbove_dev)
{
    DPE_REQUIRE(h, "[BatchCorrManifold] moments_dev: null handle");
    DPE_REQUIRE(h->momW > 0 && h->momSums_d, "[BatchCorrManifold] moments_dev: no moments call yet");
    if (sums_dev) *sums_dev = h->momSums_d;
    if (nAbove_dev) *nAbove_dev = reinterpret_cast<const int64_t *>(h->momAbove_d);
    return 0;
}

// ---- the device-resident loop's share (dpe_chm_dev_set_measurement_cov, dpe_prep.h): what dpe_bcm_moments refuses of a handle is
// refused when the loop is set up, and the per-window entry launches the moments kernel alone, into the caller's buffer
int dpe_bcm_hook_moments_check(dpe_bcm *h, size_t *partialLen)
{
    DPE_REQUIRE(h, "[BatchCorrManifold] moments: null handle");
    DPE_REQUIRE(!h->joint && !h->epochs && !h->subsets && !h->refine,
                "[BatchCorrManifold] moments: a %s handle is not supported (dpe_bcm_moments refuses its family)",
                h->joint ? "joint" : h->epochs ? "epochs" : h->subsets ? "subsets" : "refine");
    DPE_REQUIRE(h->cfg.writeScores, "[BatchCorrManifold] moments: created with writeScores=0 (the handle has no score rows)");
    if (partialLen) *partialLen = moments_partial_len(h->cfg.maxWindows);
    return 0;
}

int dpe_bcm_hook_moments_launch(dpe_bcm *h, const double rho[2], double *partial_d, dpe_bcm_mom_geom *geom, void *stream)
{
    using namespace dpe;
    DPE_REQUIRE(h && rho && partial_d && geom, "[BatchCorrManifold] moments: null argument");
    DPE_REQUIRE(h->lastW == 1, "[BatchCorrManifold] moments: the device-resident loop scans one window per Update");
    dpe_bcm_moments_config cfg{};
    cfg.rho[0] = rho[0]; cfg.rho[1] = rho[1];
    MomSide sd[2];
    const unsigned long long *keys = h->keys_d + (size_t)h->cur * 4 * h->cfg.maxWindows;
    geom->nBlk = (int)moments_launch(h, &cfg, 1, keys, partial_d, sd, (hipStream_t)stream);
    geom->split[0] = sd[0].split; geom->split[1] = sd[1].split;
    geom->rho[0] = sd[0].rho; geom->rho[1] = sd[1].rho;
    return 0;
}

// bcm_moments_finish_kernel behind such a launch (the two-launch form of the loop): one window's sums, counts and thresholds into device
// memory (mirror_d: MomMirror [2], any memory the device can write)
int dpe_bcm_hook_moments_finish(dpe_bcm *h, const double *partial_d, const dpe_bcm_mom_geom *geom, double *sums_d, long long *nAbove_d,
                                void *mirror_d, void *stream)
{
    using namespace dpe;
    DPE_REQUIRE(h && partial_d && geom && sums_d && nAbove_d && mirror_d, "[BatchCorrManifold] moments: null argument");
    const unsigned long long *keys = h->keys_d + (size_t)h->cur * 4 * h->cfg.maxWindows;
    hipLaunchKernelGGL(bcm_moments_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial_d, geom->nBlk, geom->split[0], geom->split[1],
                       keys, geom->rho[0], geom->rho[1], 1, sums_d, nAbove_d, static_cast<MomMirror *>(mirror_d));
    return 0;
}

}  // extern "C"
