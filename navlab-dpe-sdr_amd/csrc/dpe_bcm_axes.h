// dpe_bcm_axes.h -- the manifold scan for tensor-product grids given by their four axes (dpe_bcm_create_axes), included by
// dpe_bcm.hip after scan_body.
//
// Every grid the reference builds for itself (Uniform, ArthurBasis: BCM_InitPosGrid, batchcorrmanifold.cu:160-246; PyGNSS'
// spread grids) is a tensor product of x, y, z and delta_t axes, flattened ((ix dimY + iy) dimZ + iz) dimT + it, t fastest.
// The part of a point's index that does not depend on t is fixed by its (x, y, z) ROW and the SV:
//   pos:  B = idx0 + g (-a + (q - a^2) h),  a = u . (x, y, z),  q = |(x, y, z)|^2
//   vel:  B = idx0 - (g ue) x - (g un) y - (g uu) z
// and the point's index is B + g t: one packed FMA per two points instead of the point cloud's 3 (pos) / 2 (vel) per point.
//
// Mapping: a lane owns one row and one CHUNK of at most kAxT consecutive t entries of it; the 64 lanes of a wave own 64
// consecutive rows and the same chunk, so the chunk's t values are wave-uniform (scalar loads, scalar registers) and the chunk's
// scores stay in VGPRs across the SV loop.  A tile is 256 rows x one chunk; tiles are numbered row group major, so a lane meets
// its points in increasing index order (a strict "greater" keeps the first maximum).  Score rows go out through a per-wave LDS
// stage as runs of consecutive floats (non-temporal stores), not at the lane's dimT-float stride.
// The bank fill, the row index, the recount test, the key and the reductions are scan_body's pieces (dpe_bcm_pieces.h;
// DESIGN.md 2.4a); the per-point term stands in the SV loop as text (through scan_term the four general-power weighted-mean
// variants take one more VGPR).
#pragma once

namespace dpe {

constexpr int kAxT = 16;              // t entries a lane scores per tile
constexpr int kAxStage = kAxT + 1;    // LDS stage stride per lane (odd: the writes are conflict-free)
constexpr int kAxStageBytes = 256 * kAxStage * 4;

// One manifold's share of the fused axes launch.  The shard [gBegin, gEnd) may start and end inside a row.
struct AxesSide {
    const float *ax;           // device axes: x [dim0], y [dim1], z [dim2], t [dim3 + kAxT] (zero padded), at offX .. offT
    int offX, offY, offZ, offT;
    int dimY, dimZ, dimT;
    int chunk, nChunks;        // t entries per chunk (<= kAxT) and chunks per row
    unsigned rowBegin, nRows;  // global row of the shard's first point; rows the shard touches
    unsigned fullBegin, fullEnd;   // rows wholly inside the shard: [fullBegin, fullEnd)
    unsigned gBegin, G;        // the shard as global indices [gBegin, gBegin + G)
    const float2 *bank;        // [W][maxK][nEnt] score bank
    const BcmSvDev *sv;        // [W][maxK] coefficients (ignored when they ride in the kernel arguments)
    float *scores;             // [W][pitch] or nullptr
    double *wsum;              // weighted-sum partials (WMEAN) or nullptr
    long long pitch;
    int nEnt, split;
};

template <int LP, bool SECOND, bool CLAMP, bool WMEAN>
__device__ __forceinline__ void axes_body(const AxesSide &sd, int inl, int K, int maxK, int lpower, unsigned long long *__restrict__ keys,
                                          unsigned long long *__restrict__ oob, int keyStride, int keySlot)
{
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
    __shared__ double sW[4][5];

    const int w = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    float *stg = reinterpret_cast<float *>(smem + (size_t)K * nEnt * sizeof(float4)) + (tid >> 6) * 64 * kAxStage;   // this wave's stage
    scan_fill_bank(sE, sd.bank + (size_t)w * maxK * nEnt, K * nEnt, nEnt, tid);
    __syncthreads();

    const unsigned last = (unsigned)(nEnt - 1);
    const BcmSvDev *svw = params_ptr(sd.sv + (size_t)w * maxK, inl) + ((inl && !SECOND) ? DPE_MAX_CHAN : 0);
    const unsigned nChunks = (unsigned)sd.nChunks, chunk = (unsigned)sd.chunk;
    const unsigned nTiles = (sd.nRows + 255u) / 256u * nChunks;
    const unsigned rowLast = sd.rowBegin + sd.nRows - 1u;
    float bestSc = -1.f;   // scores are >= 0
    unsigned int bestIdx = 0u, nOob = 0u;
    float w0 = 0.f, w1 = 0.f, w2 = 0.f, w3 = 0.f, w4 = 0.f;
    constexpr int kPairs = kAxT / 2;
    for (unsigned tile = blockIdx.x; tile < nTiles; tile += nBlkX) {
        const unsigned grp = tile / nChunks, c = tile - grp * nChunks;   // (wave-uniform)
        const unsigned row0 = sd.rowBegin + grp * 256u, t0 = c * chunk;
        const unsigned nv = min(chunk, (unsigned)dimT - t0);              // t entries of this chunk
        const bool inner = row0 >= sd.fullBegin && row0 + 256u <= sd.fullEnd;   // no point of the tile outside the shard
        const unsigned row = row0 + (unsigned)tid;
        // lanes past the shard's last row score that row again (their points are never stored, compared, summed or counted)
        const unsigned rr = min(row, rowLast);
        const unsigned rq = rr / (unsigned)sd.dimZ, iz = rr - rq * (unsigned)sd.dimZ;
        const unsigned ix = rq / (unsigned)sd.dimY, iy = rq - ix * (unsigned)sd.dimY;
        const float x = axX[ix], y = axY[iy], z = axZ[iz];
        const float q = x * x + y * y + z * z;
        f2 tp[kPairs], score[kPairs];
#pragma unroll
        for (int p = 0; p < kPairs; ++p) {
            tp[p] = f2{axT[t0 + 2 * p], axT[t0 + 2 * p + 1]};   // wave-uniform: scalar loads (the axis is padded by kAxT)
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
                float cc[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const float id = idx[j];
                    const float wgt = __builtin_amdgcn_fractf(id);
                    int ei;
                    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(ei) : "v"(id));   // (int)floor(id), saturating
                    unsigned e = (unsigned)ei;
                    if (CLAMP) {
                        e = min(e, last);
                        emax = max(emax, e);
                    }
                    const float2 ab = *reinterpret_cast<const float2 *>(&bk[e]);
                    const float m2 = fmaf(wgt, fmaf(wgt, bk[e].w, ab.y), ab.x);
                    if (LP == 1) cc[j] = __builtin_amdgcn_sqrtf(__builtin_fabsf(m2));
                    else if (LP == 2) cc[j] = m2;
                    else cc[j] = powf(__builtin_amdgcn_sqrtf(__builtin_fabsf(m2)), (float)lpower);
                }
                score[p] += f2{cc[0], cc[1]};
            }
        }
        const unsigned gi0 = row * (unsigned)dimT + t0;   // global index of the lane's slot 0 (fits 32 bits, checked at create)
        const auto valid = [&](int it) { return (unsigned)it < nv && (inner || (gi0 + (unsigned)it) - sd.gBegin < sd.G); };
        // out-of-window pairs: recounted, with the fast path's own expressions, only where a clamp happened
        if (CLAMP && emax == last) {
            for (int it = 0; it < kAxT; ++it) {
                if (!valid(it)) continue;
                const float t = axT[t0 + it];
                for (int k = 0; k < K; ++k) {
                    const BcmSvDev s = svw[k];
                    nOob += scan_oob(fmaf(t, s.g, axes_row_index<SECOND>(x, y, z, q, s)), last) ? 1u : 0u;
                }
            }
        }
        float rs = 0.f, rt = 0.f;   // the row's sum of scores and of score * t (weighted mean)
#pragma unroll
        for (int it = 0; it < kAxT; ++it) {
            const float sc = score[it >> 1][it & 1];
            if (!valid(it)) continue;
            if (WMEAN) { rs += sc; rt = fmaf(sc, tp[it >> 1][it & 1], rt); }
            if (sc > bestSc) { bestSc = sc; bestIdx = gi0 + (unsigned)it; }
        }
        if (WMEAN) { w0 += rs; w1 = fmaf(rs, x, w1); w2 = fmaf(rs, y, w2); w3 = fmaf(rs, z, w3); w4 += rt; }
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
                const unsigned li = ((waveRow0 + r) * (unsigned)dimT + t0 + ti) - sd.gBegin;
                const float v = stg[r * kAxStage + ti];
                if (li < sd.G) __builtin_nontemporal_store(v, &srow[li]);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
    }
    const unsigned long long best = wave_max_key(pack_key(bestSc, bestIdx));
    nOob = wave_sum(nOob);
    double ws[5] = {(double)w0, (double)w1, (double)w2, (double)w3, (double)w4};
    if (WMEAN) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int j = 0; j < 5; ++j) ws[j] += __shfl_xor(ws[j], off, 64);
        }
    }
    if (lane == 0) {
        sKey[tid >> 6] = best; sOob[tid >> 6] = nOob;
        if (WMEAN) {
#pragma unroll
            for (int j = 0; j < 5; ++j) sW[tid >> 6][j] = ws[j];
        }
    }
    __syncthreads();
    if (tid == 0) {
        if (WMEAN) {
            double *o = sd.wsum + ((size_t)w * nBlkX + blockIdx.x) * 5;
#pragma unroll
            for (int j = 0; j < 5; ++j) o[j] = ((sW[0][j] + sW[1][j]) + sW[2][j]) + sW[3][j];
        }
        scan_post_key(&keys[(size_t)w * keyStride + keySlot], &oob[(size_t)w * keyStride + keySlot], block_max_key(sKey),
                      sOob[0] + sOob[1] + sOob[2] + sOob[3]);
    }
}

// Both manifolds of an axes handle in ONE launch (blockIdx.z = 0 position, 1 velocity), with bcm_scan_kernel's epilogue: the next
// key set is cleared, and the last block out publishes keys, counts and the sequence word to the pinned mirror.
template <int LP, bool CLAMP_P, bool CLAMP_V, bool WMEAN>
__global__ __launch_bounds__(256) void bcm_scan_axes_kernel(BcmParamBlock pb, int inl, AxesSide sp, AxesSide sv, int K, int maxK,
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
        if (blockIdx.x < (unsigned)sp.split) axes_body<LP, true, CLAMP_P, WMEAN>(sp, inl, K, maxK, lpower, keys, oob, 2, 0);
    } else {
        if (blockIdx.x < (unsigned)sv.split) axes_body<LP, false, CLAMP_V, WMEAN>(sv, inl, K, maxK, lpower, keys, oob, 2, 1);
    }
    scan_publish(keys, oob, done, hostKeys, hostOob, seqValue);
}

}  // namespace dpe
