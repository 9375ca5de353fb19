// dpe_arr.hip -- the dpe_arr_ family: M antenna element streams of int16 I/Q in device buffers combined with block-adaptive weights
// into B streams written into device buffers.  Exact integer covariance per block, fp64 loading, Cholesky and constraint solves,
// fp32 apply, in one kernel.  DESIGN.md 7j.
//
// A workgroup owns arr_unit_blocks(L) consecutive blocks (dpe_arr_plan.h).  Pass 1: per block the lanes stride over the samples,
// one dword per element and sample, and accumulate the M^2 packed entries of the Hermitian covariance in 64-bit integers; a wave
// folds its lanes' values by halving the set each lane carries at every exchange, and the waves' sums meet in the LDS.  Integer
// sums do not depend on the order, so S is the same bits however the block is cut.  Solve: lane (block, constraint) of the first
// wave loads R, factors it and solves in fp64 on registers, one fixed sequence of operations.  Pass 2: the same lanes re-read the
// block and write the B outputs through arr_apply.  dpe_arr_analyse runs the same kernel up to the weights and writes S, w and v.
#include "dpe_common.h"
#include "dpe_arr_plan.h"

namespace dpe {

struct ArrArgs {
    const int *x[kArrMaxM];         // element a: input sample xFirst at dword 0
    void *out[kArrMaxB];            // constraint b: output outFirst at element 0
    const double *cons;             // [B][M][2]
    unsigned long long *counters;   // blocks, fallback blocks, clipped
    long long *cov;                 // analyse: [blocks][M][M][2], [blocks][B][M][2], [blocks][B][M][2]; each may be null
    double *weights;
    float *applied;
    long long xFirst;
    int64_t lo, hi;                 // the input samples that exist and lie in the buffers: [0, recordLength) cut to the buffers' range
    long long recordLength;
    long long outFirst, outEnd;
    long long k0, k1;               // the call's first and last block
    double loading, gain;
    int L, B, outF32, analyse;
    ArrLds lds;
};

// One exchange per half: the lanes whose bit MASK is set keep the upper H of their 2 H values, the others the lower, and each adds
// what its partner sends.  With one value left the remaining exchanges are plain sums.  Lane l ends with the wave's total of entry
// l / (64 / VP) in acc[0].
template <int H, int MASK>
__device__ __forceinline__ void arr_fold(long long *acc, int lane)
{
    if constexpr (H >= 1) {
        const bool up = (lane & MASK) != 0;
#pragma unroll
        for (int j = 0; j < H; ++j) {
            const long long send = up ? acc[j] : acc[j + H];
            const long long keep = up ? acc[j + H] : acc[j];
            acc[j] = keep + __shfl_xor(send, MASK, 64);
        }
        arr_fold<H / 2, MASK / 2>(acc, lane);
    } else if constexpr (MASK >= 1) {
        acc[0] += __shfl_xor(acc[0], MASK, 64);
        arr_fold<0, MASK / 2>(acc, lane);
    }
}

// The weights of one block and one constraint from the packed covariance p: w = R^-1 c / (c^H R^-1 c), R = S + loading (tr S / M) I,
// by a Cholesky factorisation row by row, a forward and a backward substitution; or the fallback c / (c^H c).  true: fallback.
template <int M>
__device__ __forceinline__ bool arr_weights(const long long *p, const double *c, double loading, long long samples, double *wr, double *wi)
{
    double cr[M], ci[M];
#pragma unroll
    for (int a = 0; a < M; ++a) {
        cr[a] = c[2 * a];
        ci[a] = c[2 * a + 1];
    }
    long long tr = 0;
#pragma unroll
    for (int a = 0; a < M; ++a) tr += p[a * M + a];
    bool fb = samples < 2 * M || tr == 0;
    const double load = loading * ((double)tr / (double)M);
    double gr[M][M], gi[M][M], d[M];        // the factor's lower triangle, and 1 / its diagonal
#pragma unroll
    for (int i = 0; i < M; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double sr, si;
            if (i == j) {
                sr = (double)p[i * M + i] + load;
                si = 0.0;
            } else {
                sr = (double)p[i * M + j];
                si = (double)p[j * M + i];
            }
#pragma unroll
            for (int k = 0; k < j; ++k) {       // s -= G[i][k] conj(G[j][k])
                sr -= gr[i][k] * gr[j][k] + gi[i][k] * gi[j][k];
                si -= gi[i][k] * gr[j][k] - gr[i][k] * gi[j][k];
            }
            if (i == j) {
                gr[i][i] = sqrt(sr);
                gi[i][i] = 0.0;
                d[i] = 1.0 / gr[i][i];
            } else {
                gr[i][j] = sr * d[j];
                gi[i][j] = si * d[j];
            }
        }
    }
    double yr[M], yi[M], ur[M], ui[M];
#pragma unroll
    for (int i = 0; i < M; ++i) {               // G y = c
        double sr = cr[i], si = ci[i];
#pragma unroll
        for (int k = 0; k < i; ++k) {
            sr -= gr[i][k] * yr[k] - gi[i][k] * yi[k];
            si -= gr[i][k] * yi[k] + gi[i][k] * yr[k];
        }
        yr[i] = sr * d[i];
        yi[i] = si * d[i];
    }
#pragma unroll
    for (int i = M - 1; i >= 0; --i) {          // G^H u = y
        double sr = yr[i], si = yi[i];
#pragma unroll
        for (int k = i + 1; k < M; ++k) {       // s -= conj(G[k][i]) u[k]
            sr -= gr[k][i] * ur[k] + gi[k][i] * ui[k];
            si -= gr[k][i] * ui[k] - gi[k][i] * ur[k];
        }
        ur[i] = sr * d[i];
        ui[i] = si * d[i];
    }
    double dr = 0.0, di = 0.0, cc = 0.0;        // c^H u and c^H c
#pragma unroll
    for (int a = 0; a < M; ++a) {
        dr += cr[a] * ur[a] + ci[a] * ui[a];
        di += cr[a] * ui[a] - ci[a] * ur[a];
        cc += cr[a] * cr[a] + ci[a] * ci[a];
    }
    const double den = dr * dr + di * di;
#pragma unroll
    for (int a = 0; a < M; ++a) {               // u / (c^H u)
        wr[a] = (ur[a] * dr + ui[a] * di) / den;
        wi[a] = (ui[a] * dr - ur[a] * di) / den;
        fb = fb || !isfinite(ur[a]) || !isfinite(ui[a]) || !isfinite(wr[a]) || !isfinite(wi[a]);
    }
    if (fb) {
#pragma unroll
        for (int a = 0; a < M; ++a) {
            wr[a] = cr[a] / cc;
            wi[a] = ci[a] / cc;
        }
    }
    return fb;
}

template <int M>
__global__ __launch_bounds__(kArrThreads) void arr_kernel(ArrArgs a)
{
    constexpr int V = M * M, VP = arr_padded(M);
    extern __shared__ __attribute__((aligned(16))) unsigned char sRaw[];
    long long *__restrict__ sCov = reinterpret_cast<long long *>(sRaw + a.lds.cov);
    long long *__restrict__ sPart = reinterpret_cast<long long *>(sRaw + a.lds.part);
    float *__restrict__ sV = reinterpret_cast<float *>(sRaw + a.lds.applied);
    unsigned *__restrict__ sFb = reinterpret_cast<unsigned *>(sRaw + a.lds.fallback);
    unsigned *__restrict__ sCnt = reinterpret_cast<unsigned *>(sRaw + a.lds.counts);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, L = a.L, B = a.B;
    int64_t ka, kb;
    arr_unit_range(a.k0, a.k1, blockIdx.x, L, ka, kb);
    const int nb = (int)(kb - ka + 1);

    if (tid < 4) sCnt[tid] = 0u;                // (the first use lies behind the barriers below)
    if (tid < nb) sFb[tid] = 0u;

    // ---- pass 1: the packed covariance of each block
    for (int j = 0; j < nb; ++j) {
        const long long n0 = (ka + j) * L;
        long long acc[VP];
#pragma unroll
        for (int e = 0; e < VP; ++e) acc[e] = 0;
#pragma unroll 2
        for (int i = tid; i < L; i += kArrThreads) {
            const long long n = n0 + i;
            if (n >= a.lo && n < a.hi) {
                int xi[M], xq[M];
#pragma unroll
                for (int e = 0; e < M; ++e) {
                    stream_unpack(a.x[e][n - a.xFirst], xi[e], xq[e]);
                }
#pragma unroll
                for (int e = 0; e < M; ++e) {
                    acc[e * M + e] += (long long)xi[e] * xi[e] + (long long)xq[e] * xq[e];
#pragma unroll
                    for (int f = 0; f < e; ++f) {
                        acc[e * M + f] += (long long)xi[e] * xi[f] + (long long)xq[e] * xq[f];
                        acc[f * M + e] += (long long)xq[e] * xi[f] - (long long)xi[e] * xq[f];
                    }
                }
            }
        }
        arr_fold<VP / 2, 32>(acc, lane);
        long long *part = sPart + (j & 1) * kArrWaves * VP;
        if ((lane & (64 / VP - 1)) == 0) part[wave * VP + lane / (64 / VP)] = acc[0];
        __syncthreads();
        if (tid < V) {
            long long s = 0;
#pragma unroll
            for (int w = 0; w < kArrWaves; ++w) s += part[w * VP + tid];
            sCov[j * V + tid] = s;
        }
        // (the next block writes the other buffer; the one after it writes this one behind the next block's barrier)
    }
    __syncthreads();

    if (a.analyse && a.cov)
        for (int idx = tid; idx < nb * V; idx += kArrThreads) {
            const int j = idx / V, r = idx % V;
            int64_t re, im;
            arr_cov_entry(reinterpret_cast<const int64_t *>(sCov) + j * V, M, r / M, r % M, re, im);
            const long long at = ((ka + j - a.k0) * V + r) * 2;
            a.cov[at] = re;
            a.cov[at + 1] = im;
        }

    // ---- solve: lane (block j, constraint b)
    if (tid < nb * B) {
        const int j = tid / B, b = tid % B;
        double wr[M], wi[M];
        const bool fb = arr_weights<M>(sCov + j * V, a.cons + (size_t)b * 2 * M, a.loading, arr_block_samples(ka + j, L, a.recordLength), wr, wi);
        if (fb) atomicOr(&sFb[j], 1u);
        const long long at = ((ka + j - a.k0) * B + b) * M * 2;
#pragma unroll
        for (int e = 0; e < M; ++e) {
            const float vr = (float)(a.gain * wr[e]), vi = (float)(-(a.gain * wi[e]));
            sV[((j * kArrMaxB + b) * M + e) * 2] = vr;
            sV[((j * kArrMaxB + b) * M + e) * 2 + 1] = vi;
            if (a.analyse && a.weights) {
                a.weights[at + 2 * e] = wr[e];
                a.weights[at + 2 * e + 1] = wi[e];
            }
            if (a.analyse && a.applied) {
                a.applied[at + 2 * e] = vr;
                a.applied[at + 2 * e + 1] = vi;
            }
        }
    }
    if (a.analyse) return;
    __syncthreads();

    unsigned nBlocks = 0, nFallback = 0, nClipped = 0;
    if (tid < nb && arr_counted(ka + tid, L, a.outFirst, a.outEnd - a.outFirst, a.recordLength)) {
        nBlocks = 1u;
        nFallback = sFb[tid] != 0u;
    }

    // ---- pass 2: the outputs of each block and constraint
    for (int j = 0; j < nb; ++j) {
        const long long n0 = (ka + j) * L;
        for (int b = 0; b < B; ++b) {
            float vr[M], vi[M];
#pragma unroll
            for (int e = 0; e < M; ++e) {
                vr[e] = sV[((j * kArrMaxB + b) * M + e) * 2];
                vi[e] = sV[((j * kArrMaxB + b) * M + e) * 2 + 1];
            }
#pragma unroll 2
            for (int i = tid; i < L; i += kArrThreads) {
                const long long n = n0 + i;
                if (n < a.outFirst || n >= a.outEnd) continue;
                float xi[M], xq[M];
                const bool in = n >= a.lo && n < a.hi;
#pragma unroll
                for (int e = 0; e < M; ++e) {
                    stream_unpack(in ? a.x[e][n - a.xFirst] : 0, xi[e], xq[e]);
                }
                float re, im;
                arr_apply(M, vr, vi, xi, xq, re, im);
                stream_store(a.out[b], n - a.outFirst, re, im, a.outF32, nClipped);
            }
        }
    }

    // ---- the workgroup's counters: one atomic per counter
    if (nBlocks) atomicAdd(&sCnt[0], nBlocks);
    if (nFallback) atomicAdd(&sCnt[1], nFallback);
    if (nClipped) atomicAdd(&sCnt[2], nClipped);
    __syncthreads();
    if (tid < 3 && sCnt[tid]) atomicAdd(a.counters + tid, (unsigned long long)sCnt[tid]);
}

}  // namespace dpe

using namespace dpe;

struct dpe_arr {
    dpe_arr_config cfg{};
    ArrLds lds{};
    double *cons_d = nullptr;                   // [B][M][2]
    unsigned long long *counters_d = nullptr;   // [4]
    hipStream_t last = nullptr;
};

static ArrArgs arr_args(const dpe_arr *h, const void *const *x_dev, int64_t xFirst, int64_t xCount, int64_t recordLength)
{
    ArrArgs a{};
    for (int e = 0; e < h->cfg.nElements; ++e) a.x[e] = static_cast<const int *>(x_dev[e]);
    a.cons = h->cons_d;
    a.counters = h->counters_d;
    a.xFirst = xFirst;
    a.lo = xFirst;
    a.hi = xFirst + xCount;
    stream_cut(recordLength, a.lo, a.hi);
    a.recordLength = recordLength;
    a.loading = h->cfg.loading;
    a.gain = h->cfg.gain;
    a.L = h->cfg.blockLength;
    a.B = h->cfg.nConstraints;
    a.outF32 = h->cfg.outputFormat == DPE_FE_OUT_F32;
    a.lds = h->lds;
    return a;
}

static void arr_launch_kernel(int M, unsigned units, int ldsBytes, hipStream_t stream, const ArrArgs &a)
{
    const dim3 grid(units), block(kArrThreads);
    switch (M) {
    case 2: arr_kernel<2><<<grid, block, ldsBytes, stream>>>(a); break;
    case 3: arr_kernel<3><<<grid, block, ldsBytes, stream>>>(a); break;
    case 4: arr_kernel<4><<<grid, block, ldsBytes, stream>>>(a); break;
    case 5: arr_kernel<5><<<grid, block, ldsBytes, stream>>>(a); break;
    case 6: arr_kernel<6><<<grid, block, ldsBytes, stream>>>(a); break;
    case 7: arr_kernel<7><<<grid, block, ldsBytes, stream>>>(a); break;
    default: arr_kernel<8><<<grid, block, ldsBytes, stream>>>(a); break;
    }
}

extern "C" {

int dpe_arr_create(const dpe_arr_config *cfg, const double *constraints, dpe_arr **out)
{
    char msg[256];
    if (arr_config_problem(cfg, constraints, msg, sizeof(msg))) {
        set_error("%s", msg);
        return -1;
    }
    DPE_REQUIRE(out != nullptr, "[ArrayCombiner] create: null argument");
    dpe_arr *h = new dpe_arr;
    h->cfg = *cfg;
    h->lds = arr_lds(cfg->nElements, cfg->blockLength);
    const int M = cfg->nElements, B = cfg->nConstraints;
    std::vector<double> cons((size_t)B * M * 2, 0.0);
    if (constraints)
        cons.assign(constraints, constraints + cons.size());
    else
        cons[(size_t)2 * cfg->reference] = 1.0;
    const bool ok = hipMalloc((void **)&h->cons_d, cons.size() * sizeof(double)) == hipSuccess &&
                    hipMalloc((void **)&h->counters_d, 4 * sizeof(unsigned long long)) == hipSuccess &&
                    hipMemcpy(h->cons_d, cons.data(), cons.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
                    hipMemset(h->counters_d, 0, 4 * sizeof(unsigned long long)) == hipSuccess;
    if (!ok) {
        const hipError_t e = hipGetLastError();
        dpe_arr_destroy(h);
        set_error("[ArrayCombiner] create: no device memory (%s)", hipGetErrorString(e));
        return -1;
    }
    *out = h;
    return 0;
}

int dpe_arr_destroy(dpe_arr *h)
{
    if (!h) return 0;
    if (h->cons_d) (void)hipFree(h->cons_d);
    if (h->counters_d) (void)hipFree(h->counters_d);
    delete h;
    return 0;
}

int dpe_arr_info(const dpe_arr *h, dpe_arr_info_t *info)
{
    DPE_REQUIRE(h && info, "[ArrayCombiner] info: null argument");
    *info = dpe_arr_info_t{};
    info->blockLength = h->cfg.blockLength;
    info->blocksPerUnit = arr_unit_blocks(h->cfg.blockLength);
    info->ldsBytes = h->lds.bytes;
    info->minSamples = 2 * h->cfg.nElements;
    return 0;
}

int dpe_arr_process(dpe_arr *h, const void *const *x_dev, int64_t xFirst, int64_t xCount, int64_t recordLength, void *const *out_dev,
                    int64_t outFirst, int64_t outCount, dpe_stream_t stream_)
{
    DPE_REQUIRE(h != nullptr, "[ArrayCombiner] process: null handle");
    char msg[320];
    uint64_t xAddr[kArrMaxM] = {}, outAddr[kArrMaxB] = {};
    for (int e = 0; x_dev && e < h->cfg.nElements; ++e) xAddr[e] = (uint64_t)reinterpret_cast<uintptr_t>(x_dev[e]);
    for (int b = 0; out_dev && b < h->cfg.nConstraints; ++b) outAddr[b] = (uint64_t)reinterpret_cast<uintptr_t>(out_dev[b]);
    if (arr_process_problem(h->cfg, x_dev ? xAddr : nullptr, out_dev ? outAddr : nullptr, xFirst, xCount, recordLength, outFirst, outCount, msg,
                            sizeof(msg))) {
        set_error("%s", msg);
        return -1;
    }
    const hipStream_t stream = (hipStream_t)stream_;
    ArrArgs a = arr_args(h, x_dev, xFirst, xCount, recordLength);
    const ArrLaunch l = arr_launch(outFirst, outCount, h->cfg.blockLength);
    for (int b = 0; b < h->cfg.nConstraints; ++b) a.out[b] = out_dev[b];
    a.outFirst = outFirst;
    a.outEnd = outFirst + outCount;
    a.k0 = l.k0;
    a.k1 = l.k1;
    DPE_CHECK_HIP(hipMemsetAsync(h->counters_d, 0, 4 * sizeof(unsigned long long), stream));
    arr_launch_kernel(h->cfg.nElements, (unsigned)l.units, h->lds.bytes, stream, a);
    DPE_CHECK_HIP(hipGetLastError());
    h->last = stream;
    return 0;
}

int dpe_arr_stats(dpe_arr *h, dpe_arr_stats_t *stats)
{
    DPE_REQUIRE(h && stats, "[ArrayCombiner] stats: null argument");
    unsigned long long v[4] = {};
    if (read_counters(v, h->counters_d, 4, h->last)) return -1;
    stats->blocks = (int64_t)v[0];
    stats->fallbackBlocks = (int64_t)v[1];
    stats->clipped = (int64_t)v[2];
    return 0;
}

int dpe_arr_analyse(dpe_arr *h, const void *const *x_dev, int64_t xFirst, int64_t xCount, int64_t recordLength, int64_t blockFirst,
                    int64_t blockCount, int64_t *cov_dev, double *weights_dev, float *applied_dev, dpe_stream_t stream_)
{
    DPE_REQUIRE(h != nullptr, "[ArrayCombiner] analyse: null handle");
    char msg[320];
    uint64_t xAddr[kArrMaxM] = {};
    for (int e = 0; x_dev && e < h->cfg.nElements; ++e) xAddr[e] = (uint64_t)reinterpret_cast<uintptr_t>(x_dev[e]);
    if (arr_analyse_problem(h->cfg, x_dev ? xAddr : nullptr, xFirst, xCount, recordLength, blockFirst, blockCount,
                            (unsigned)(reinterpret_cast<uintptr_t>(cov_dev) & 15), (unsigned)(reinterpret_cast<uintptr_t>(weights_dev) & 15),
                            (unsigned)(reinterpret_cast<uintptr_t>(applied_dev) & 15), msg, sizeof(msg))) {
        set_error("%s", msg);
        return -1;
    }
    ArrArgs a = arr_args(h, x_dev, xFirst, xCount, recordLength);
    a.analyse = 1;
    a.cov = reinterpret_cast<long long *>(cov_dev);
    a.weights = weights_dev;
    a.applied = applied_dev;
    a.k0 = blockFirst;
    a.k1 = blockFirst + blockCount - 1;
    const int ub = arr_unit_blocks(h->cfg.blockLength);
    arr_launch_kernel(h->cfg.nElements, (unsigned)((blockCount + ub - 1) / ub), h->lds.bytes, (hipStream_t)stream_, a);
    DPE_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
