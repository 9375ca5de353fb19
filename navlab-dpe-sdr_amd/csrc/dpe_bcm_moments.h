// dpe_bcm_moments.h -- thresholded moments of the manifold score rows (dpe_bcm_moments), included by dpe_bcm.hip after the scans.
//
// Every scan ends in an arg-max; the shape of the score surface around it is what tells a sharp peak from a smeared one.  This is
// a separate launch BEHIND the scan, over the score rows the scan already wrote: the scan kernels are not touched.
// Per window w and manifold m, with smax = the fp32 in the high word of key [w][m], tau = rho * smax (one fp32 multiply):
//     w_i = s_i > tau ? (double)s_i - (double)tau : 0                 (a NaN score fails the compare and contributes nothing)
//     S   = sum_i w_i {1, x, y, z, t, xx, xy, xz, xt, yy, yz, yt, zz, zt, tt}     about the grid origin = the window centre
// with every product and accumulation in fp64 from the fp32 scores and the fp32 grid the scan scored.  Sums about the origin add
// across shards; fp64 per point makes the cancellation in S2 / S0 - mu mu^T harmless.
//
// Mapping: a wave takes UNITS of 512 consecutive points of the row, two runs of 256; a lane reads four consecutive scores of each
// run with one 16-byte load (a wave-instruction reads 1 KB contiguous).  In the scan layout of a point list (scan_grid_slot) the
// two runs of a unit are the two points of a pair, so the lane's eight points are eight whole float4 of the grid.  The grid (or
// the axes) is read only by a wave with at least one lane above tau: at a useful rho most waves read 4 B per point and add
// nothing.  The traffic of the stage is the scores; the grids are shared by the windows of a batch and stay in cache.
// Reduction: lanes by xor butterfly, the four waves in wave order through LDS, the blocks of a row in block order by
// bcm_moments_finish_kernel behind the kernel boundary -- no atomics on doubles, the bits depend on inputs and geometry only.
#pragma once
#include "dpe_bcm_moments_cov.h"   // kMomSums, kMomSlots; what becomes of the sums (the filter's R)

namespace dpe {

constexpr int kMomUnit = 512;    // points per wave step

// One manifold's share of the launch
struct MomSide {
    const float *scores;       // [W][pitch]; the pitch - G pad floats of a row are never read
    long long pitch, G;
    const float4 *grid;        // point list: the scan layout, zero padded to whole tiles
    const float *ax;           // axes: x [dim0], y [dim1], z [dim2], t [dim3] at offX .. offT (AxesSide's block)
    int offX, offY, offZ, offT;
    unsigned dimY, dimZ, dimT;
    unsigned gBegin;           // axes: global index of the row's first point (the handle's slice offset)
    int split;                 // blocks along x that work on this manifold
    int vec;                   // every row starts on a 16-byte boundary: four scores per load
    float rho;
};

// One (window, manifold) of the pinned mirror
struct MomMirror {
    double sums[kMomSums];
    long long nAbove;
    float tau, pad;
};

__device__ __forceinline__ float mom_tau(const unsigned long long *__restrict__ keys, int w, int m, float rho)
{
    const float smax = __uint_as_float((unsigned int)(keys[2 * (size_t)w + m] >> 32));
    return __fmul_rn(rho, smax);   // one IEEE fp32 multiply, never contracted
}

__device__ __forceinline__ void mom_add(double (&S)[kMomSums], float s, float tau, float x, float y, float z, float t)
{
    const double wg = (double)s - (double)tau;
    const double dx = (double)x, dy = (double)y, dz = (double)z, dt = (double)t;
    const double wx = wg * dx, wy = wg * dy, wz = wg * dz, wt = wg * dt;
    S[0] += wg; S[1] += wx; S[2] += wy; S[3] += wz; S[4] += wt;
    S[5] = fma(wx, dx, S[5]); S[6] = fma(wx, dy, S[6]); S[7] = fma(wx, dz, S[7]); S[8] = fma(wx, dt, S[8]);
    S[9] = fma(wy, dy, S[9]); S[10] = fma(wy, dz, S[10]); S[11] = fma(wy, dt, S[11]);
    S[12] = fma(wz, dz, S[12]); S[13] = fma(wz, dt, S[13]);
    S[14] = fma(wt, dt, S[14]);
}

// Four consecutive scores from local index i (a multiple of 4); points at or beyond G read as -inf, which no tau lies below
__device__ __forceinline__ void mom_load4(float (&s)[4], const float *__restrict__ row, long long i, long long G, int vec)
{
    if (vec && i + 3 < G) {
        const float4 v = *reinterpret_cast<const float4 *>(row + i);
        s[0] = v.x; s[1] = v.y; s[2] = v.z; s[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = i + j < G ? row[i + j] : -INFINITY;
    }
}

template <bool AXES>
__global__ __launch_bounds__(256) void bcm_moments_kernel(MomSide sp, MomSide sv, const unsigned long long *__restrict__ keys,
                                                          double *__restrict__ partial)
{
    const int m = blockIdx.z, w = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform, and known to be: the unit walk runs on scalars
    const MomSide sd = m ? sv : sp;
    if (blockIdx.x >= (unsigned)sd.split) return;   // (the wider manifold sets gridDim.x)
    __shared__ double sW[4][kMomSlots];
    const float tau = mom_tau(keys, w, m, sd.rho);
    const float *__restrict__ row = sd.scores + (size_t)w * sd.pitch;
    const long long G = sd.G;
    const unsigned nUnits = (unsigned)((G + kMomUnit - 1) / kMomUnit);
    double S[kMomSums];
#pragma unroll
    for (int j = 0; j < kMomSums; ++j) S[j] = 0.0;
    unsigned int nAbove = 0;   // per lane: at most G / 64 + 8
    for (unsigned u = blockIdx.x * 4u + (unsigned)wv; u < nUnits; u += (unsigned)sd.split * 4u) {
        const long long i0 = (long long)u * kMomUnit + 4 * lane;
        float s[8];
        mom_load4(reinterpret_cast<float(&)[4]>(s[0]), row, i0, G, sd.vec);
        mom_load4(reinterpret_cast<float(&)[4]>(s[4]), row, i0 + 256, G, sd.vec);
        bool any = false;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool above = s[j] > tau;
            nAbove += above ? 1u : 0u;
            any |= above;
        }
        if (!__any(any)) continue;   // wave-uniform: no lane above tau, nothing to add and no grid to read
        if (AXES) {
            const float *__restrict__ axX = sd.ax + sd.offX;
            const float *__restrict__ axY = sd.ax + sd.offY;
            const float *__restrict__ axZ = sd.ax + sd.offZ;
            const float *__restrict__ axT = sd.ax + sd.offT;
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                // global index ((ix dimY + iy) dimZ + iz) dimT + it, t fastest (fits 32 bits, checked at create); the run's other
                // three points follow by carry.  Indices of points beyond G may leave the axes: they are never above tau.
                const unsigned g = sd.gBegin + (unsigned)i0 + 256u * r;
                unsigned rw = g / sd.dimT, it = g - rw * sd.dimT;
                unsigned q = rw / sd.dimZ, iz = rw - q * sd.dimZ;
                unsigned ix = q / sd.dimY, iy = q - ix * sd.dimY;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (s[4 * r + j] > tau) mom_add(S, s[4 * r + j], tau, axX[ix], axY[iy], axZ[iz], axT[it]);
                    if (++it == sd.dimT) {
                        it = 0;
                        if (++iz == sd.dimZ) {
                            iz = 0;
                            if (++iy == sd.dimY) { iy = 0; ++ix; }
                        }
                    }
                }
            }
        } else {
            // the unit's two runs are the points (a, b) of one pair of the scan layout: float4 {x_a, x_b, y_a, y_b} of lane
            // 4 lane + j at slot u * 512 + 4 lane + j, {z_a, z_b, t_a, t_b} 256 slots on (the grid is padded to whole tiles)
            // (buffer loads over the unit's 8 KB, as scan_load_tile: whole 16-byte loads whatever the branches below use of them)
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<float4 *>(sd.grid + (size_t)u * kMomUnit), 0, kMomUnit * (int)sizeof(float4), 0x00020000);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f4 xy = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rs, lane * 64, j * 16, 0));
                const f4 zt = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rs, lane * 64, 256 * 16 + j * 16, 0));
                if (s[j] > tau) mom_add(S, s[j], tau, xy.x, xy.z, zt.x, zt.z);
                if (s[4 + j] > tau) mom_add(S, s[4 + j], tau, xy.y, xy.w, zt.y, zt.w);
            }
        }
    }
    // lanes: xor butterfly (a + b and b + a carry the same bits, so every lane ends with the wave's sum)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int j = 0; j < kMomSums; ++j) S[j] += __shfl_xor(S[j], off, 64);
        nAbove += __shfl_xor(nAbove, off, 64);   // (a wave's count is at most 64 * (G / 64 + 8): fits 32 bits, G < 2^32)
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < kMomSums; ++j) sW[wv][j] = S[j];
        sW[wv][kMomSums] = __longlong_as_double((long long)nAbove);
    }
    __syncthreads();
    // waves in wave order; the block's partial goes to its own slot, summed in block order behind the kernel boundary
    if (tid < kMomSlots) {
        double *o = partial + (((size_t)w * 2 + m) * gridDim.x + blockIdx.x) * kMomSlots;
        if (tid < kMomSums) o[tid] = ((sW[0][tid] + sW[1][tid]) + sW[2][tid]) + sW[3][tid];
        else o[tid] = __longlong_as_double(__double_as_longlong(sW[0][tid]) + __double_as_longlong(sW[1][tid]) +
                                           __double_as_longlong(sW[2][tid]) + __double_as_longlong(sW[3][tid]));
    }
}

// One thread per (window, manifold, slot): the row's block partials in block order, into device memory and the pinned mirror
__global__ __launch_bounds__(256) void bcm_moments_finish_kernel(const double *__restrict__ partial, int nBlk, int splitP, int splitV,
                                                                 const unsigned long long *__restrict__ keys, float rhoP, float rhoV,
                                                                 int nWindows, double *__restrict__ sums, long long *__restrict__ nAbove,
                                                                 MomMirror *__restrict__ mirror)
{
    const int t = blockIdx.x * 256 + threadIdx.x, j = t & (kMomSlots - 1), wm = t / kMomSlots;
    if (wm >= 2 * nWindows) return;
    const int m = wm & 1, split = m ? splitV : splitP;
    const double *p = partial + (size_t)wm * nBlk * kMomSlots + j;
    if (j < kMomSums) {
        double a = p[0];
        for (int b = 1; b < split; ++b) a += p[(size_t)b * kMomSlots];
        sums[(size_t)wm * kMomSums + j] = a;
        mirror[wm].sums[j] = a;
    } else {
        long long n = 0;
        for (int b = 0; b < split; ++b) n += __double_as_longlong(p[(size_t)b * kMomSlots]);
        nAbove[wm] = n;
        mirror[wm].nAbove = n;
        mirror[wm].tau = mom_tau(keys, wm >> 1, m, m ? rhoV : rhoP);
        mirror[wm].pad = 0.f;
    }
}

}  // namespace dpe
