// dpe_cd.hip -- the dpe_cd_ family: collective detection, i.e. acquisition in the position domain.  Every SV's delay x Doppler
// surface (dpe_acq_surface's layout, or any device array of it) is summed over position offset x clock bias x clock drift and one
// arg-max taken over the sum (include/dpe_hip.h has the definition, DESIGN.md 7g the reasoning and the numbers).
//
// Three launches per update, all on the caller's stream, parameters in the kernel-argument segment (no staging, nothing to wait for):
//   cd_tau_kernel    per (point, SV) the delay tau in fp64 from exact ranges -> floor(tau) mod M, the lerp weight as fp32, tau itself;
//                    clears the per-point keys.
//   cd_scan_kernel   block (x, jj) stages the K rows s[row_k][b_k(j)][0..M) (plus a wrap pad of one run) in LDS -- or reads them from
//                    L2 where K rows exceed the LDS a block may have -- and walks the points x, x + gridDim.x, ...  A lane owns runs of
//                    kCdRun consecutive clock values: the lerp weight is the same for every clock value of a (point, SV) and
//                    consecutive clock values share a sample, so a run costs kCdRun + 1 reads for kCdRun terms.  Per point each
//                    lane keeps its first maximum, the lanes' maxima become one packed key (score bits, ~(jj M + m)) per wave, one
//                    LDS atomic per wave, and every kCdFlush points one device-wide atomicMax per point.
//   cd_final_kernel  one block: the map (score and (j, m) per point) from the keys, the first maximum over points, and each SV's
//                    own term and delay index there.
#include "dpe_common.h"
#include "dpe_cd_plan.h"

namespace dpe {

struct CdDevResult {
    int32_t point, j, m, reserved;
    float score;
    float peak[DPE_CD_MAX_SV];
    int32_t codeIdx[DPE_CD_MAX_SV];
};

__global__ __launch_bounds__(256) void cd_tau_kernel(CdArgs a, const double *__restrict__ grid, double *__restrict__ tau,
                                                     int2 *__restrict__ baseFrac, unsigned long long *__restrict__ keys)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.P * DPE_CD_MAX_SV) return;
    const int p = i / DPE_CD_MAX_SV, k = i - p * DPE_CD_MAX_SV;
    if (k == 0) keys[p] = 0ull;
    if (k >= a.K) return;
    const double e = grid[3 * p], n = grid[3 * p + 1], u = grid[3 * p + 2];
    const CdSv s = a.sv[k];
    const double lx = s.sx - (a.p0[0] + (a.R[0] * e + a.R[1] * n + a.R[2] * u));
    const double ly = s.sy - (a.p0[1] + (a.R[3] * e + a.R[4] * n + a.R[5] * u));
    const double lz = s.sz - (a.p0[2] + (a.R[6] * e + a.R[7] * n + a.R[8] * u));
    const double range = sqrt(lx * lx + ly * ly + lz * lz);
    const double t = s.delay0 + (range - s.range0) * a.fs / kC;
    const double fl = floor(t);
    long long b = (long long)fl % a.M;
    if (b < 0) b += a.M;
    tau[i] = t;
    baseFrac[i] = make_int2((int)b, __float_as_int((float)(t - fl)));   // floor(tau) mod M and the lerp weight: one 8-byte scalar load
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, off, 64), hi = __shfl_xor((unsigned)(v >> 32), off, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

template <bool LDS>
__global__ __launch_bounds__(kCdThreads) void cd_scan_kernel(CdArgs a, const float *__restrict__ surf, const int2 *__restrict__ baseFrac,
                                                             unsigned long long *__restrict__ keys)
{
    extern __shared__ float sRows[];   // [K][pitch]
    __shared__ unsigned long long sKey[kCdFlush];
    const int tid = threadIdx.x, jj = blockIdx.y, j = jj - a.J, M = a.M;
    unsigned valid = 0;
    for (int k = 0; k < a.K; ++k) {
        const int b = a.sv[k].bin + j;
        if (b >= 0 && b < a.nBins) valid |= 1u << k;
    }
    if (LDS) {
        for (int k = 0; k < a.K; ++k) {
            float *__restrict__ dst = sRows + (size_t)k * a.pitch;
            if (!((valid >> k) & 1u)) {   // outside the raster: a row of zeros (its terms also get zero weights below)
                for (int i = tid; i < a.pitch; i += kCdThreads) dst[i] = 0.f;
                continue;
            }
            const float *__restrict__ src = surf + ((size_t)a.sv[k].row * a.nBins + (a.sv[k].bin + j)) * (size_t)M;
            for (int i = tid; i < a.pitch; i += kCdThreads) dst[i] = src[i < M ? i : i - M];
        }
    }
    if (tid < kCdFlush) sKey[tid] = 0ull;
    __syncthreads();

    int n = 0;
    for (int p = blockIdx.x; p < a.P; p += gridDim.x, ++n) {
        const int slot = n % kCdFlush;
        float bestV = -1.f;   // scores are >= 0: the first clock value of a lane always enters
        int bestM = 0;
        for (int q = tid; q < a.nRuns; q += kCdThreads) {
            const int m0 = q * kCdRun;
            float acc[kCdRun];
#pragma unroll
            for (int r = 0; r < kCdRun; ++r) acc[r] = 0.f;
            // No branch on `valid` in here: an SV outside the raster keeps its loads (a zero row in LDS, its row at the nearest bin
            // from L2) and gets zero weights, so that the SV loop unrolls into straight code whose loads issue ahead of the FMAs.
#pragma unroll 4
            for (int k = 0; k < a.K; ++k) {
                const int2 bf = baseFrac[p * DPE_CD_MAX_SV + k];
                const bool ok = (valid >> k) & 1u;
                const float f = ok ? __int_as_float(bf.y) : 0.f, w0 = ok ? 1.f - f : 0.f;
                int i = bf.x + m0;   // < 2 M
                if (i >= M) i -= M;
                float v[kCdRun + 1];
                if (LDS) {
                    const float *__restrict__ row = sRows + (size_t)k * a.pitch + i;   // i + kCdRun < pitch
#pragma unroll
                    for (int r = 0; r <= kCdRun; ++r) v[r] = row[r];
                } else {
                    const int bin = min(max(a.sv[k].bin + j, 0), a.nBins - 1);
                    const float *__restrict__ row = surf + ((size_t)a.sv[k].row * a.nBins + bin) * (size_t)M;
#pragma unroll
                    for (int r = 0; r <= kCdRun; ++r) {
                        int x = i + r;
                        if (x >= M) x -= M;
                        v[r] = row[x];
                    }
                }
#pragma unroll
                for (int r = 0; r < kCdRun; ++r) acc[r] = fmaf(f, v[r + 1], fmaf(w0, v[r], acc[r]));
            }
#pragma unroll
            for (int r = 0; r < kCdRun; ++r) {
                const int m = m0 + r;   // ascending within a lane, so a strict comparison keeps the first maximum
                if (m < M && acc[r] > bestV) {
                    bestV = acc[r];
                    bestM = m;
                }
            }
        }
        // (a lane without a run -- nRuns below the block's lanes -- keeps -1: key 0 below)
        unsigned long long best = bestV < 0.f ? 0ull : ((unsigned long long)__float_as_uint(bestV) << 32) | (unsigned)~(unsigned)(jj * M + bestM);
        best = wave_max_u64(best);
        if ((tid & 63) == 0) atomicMax(&sKey[slot], best);
        const bool last = p + (int)gridDim.x >= a.P;
        if (slot == kCdFlush - 1 || last) {
            __syncthreads();
            if (tid <= slot) {
                atomicMax(&keys[p - (slot - tid) * (int)gridDim.x], sKey[tid]);
                sKey[tid] = 0ull;
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(256) void cd_final_kernel(CdArgs a, const float *__restrict__ surf, const double *__restrict__ tau,
                                                       const int2 *__restrict__ baseFrac, const unsigned long long *__restrict__ keys, float *__restrict__ mapScore,
                                                       int *__restrict__ mapJM, CdDevResult *__restrict__ res)
{
    __shared__ unsigned long long sBest[4];
    const int tid = threadIdx.x, M = a.M;
    unsigned long long best = 0ull;
    for (int p = tid; p < a.P; p += 256) {
        const unsigned long long key = keys[p];
        const unsigned idx = ~(unsigned)key;
        mapScore[p] = __uint_as_float((unsigned)(key >> 32));
        mapJM[2 * p] = (int)(idx / (unsigned)M) - a.J;
        mapJM[2 * p + 1] = (int)(idx % (unsigned)M);
        const unsigned long long kp = (key & 0xFFFFFFFF00000000ull) | (unsigned)~(unsigned)p;   // the first point among equal scores
        if (kp > best) best = kp;
    }
    best = wave_max_u64(best);
    if ((tid & 63) == 0) sBest[tid >> 6] = best;
    __syncthreads();
    unsigned long long b = sBest[0];
    for (int w = 1; w < 4; ++w) b = sBest[w] > b ? sBest[w] : b;
    const int p = (int)~(unsigned)b;
    const unsigned idx = ~(unsigned)keys[p];
    const int jj = (int)(idx / (unsigned)M), m = (int)(idx % (unsigned)M), j = jj - a.J;
    if (tid == 0) {
        res->point = p; res->j = j; res->m = m; res->reserved = 0;
        res->score = __uint_as_float((unsigned)(b >> 32));
    }
    if (tid < DPE_CD_MAX_SV) {
        float term = 0.f;
        int ci = 0;
        if (tid < a.K) {
            const int i = p * DPE_CD_MAX_SV + tid, bin = a.sv[tid].bin + j;
            long long c = (long long)rint(tau[i] + (double)m) % M;
            if (c < 0) c += M;
            ci = (int)c;
            if (bin >= 0 && bin < a.nBins) {
                const float *__restrict__ row = surf + ((size_t)a.sv[tid].row * a.nBins + bin) * (size_t)M;
                int i0 = baseFrac[i].x + m;
                if (i0 >= M) i0 -= M;
                const int i1 = i0 + 1 == M ? 0 : i0 + 1;
                const float f = __int_as_float(baseFrac[i].y);
                term = fmaf(f, row[i1], (1.f - f) * row[i0]);
            }
        }
        res->peak[tid] = term;
        res->codeIdx[tid] = ci;
    }
}

}  // namespace dpe

using namespace dpe;

struct dpe_cd {
    dpe_cd_config cfg{};
    std::vector<double> grid;      // host copy [P][3]: the fix of a result
    double *grid_d = nullptr, *tau_d = nullptr;
    int2 *bf_d = nullptr;          // [P][DPE_CD_MAX_SV]: floor(tau) mod M, the lerp weight's bits
    int *jm_d = nullptr;
    float *score_d = nullptr;
    unsigned long long *keys_d = nullptr;
    CdDevResult *res_d = nullptr;
    // the last update, for results
    bool updated = false;
    hipStream_t stream = nullptr;
    int nSv = 0, binsOut = 0;
    double p0[3] = {}, R[9] = {};
    int32_t prn[DPE_CD_MAX_SV] = {}, bin[DPE_CD_MAX_SV] = {};
};

extern "C" {

int dpe_cd_create(const dpe_cd_config *cfg, dpe_cd **out)
{
    DPE_REQUIRE(cfg && out, "[CollectiveDetector] create: null argument");
    const char *why = cd_config_problem(*cfg);
    DPE_REQUIRE(!why, "[CollectiveDetector] create: %s", why);
    dpe_cd *h = new dpe_cd;
    h->cfg = *cfg;
    const size_t P = (size_t)cfg->nPoints;
    h->grid.assign(cfg->enuGrid, cfg->enuGrid + 3 * P);
    h->cfg.enuGrid = nullptr;   // the caller's array is not kept
    h->grid_d = dev_alloc<double>(3 * P);
    h->tau_d = dev_alloc<double>(P * DPE_CD_MAX_SV);
    h->bf_d = dev_alloc<int2>(P * DPE_CD_MAX_SV);
    h->keys_d = dev_alloc<unsigned long long>(P);
    h->score_d = dev_alloc<float>(P);
    h->jm_d = dev_alloc<int>(2 * P);
    h->res_d = dev_alloc<CdDevResult>(1);
    bool ok = h->grid_d && h->tau_d && h->bf_d && h->keys_d && h->score_d && h->jm_d && h->res_d;
    ok = ok && hipMemcpy(h->grid_d, h->grid.data(), sizeof(double) * 3 * P, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipFuncSetAttribute(reinterpret_cast<const void *>(cd_scan_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)kCdLdsMax) == hipSuccess;
    if (!ok) {
        const hipError_t e = hipGetLastError();
        dpe_cd_destroy(h);
        set_error("[CollectiveDetector] create: no device memory, or the scan kernel's LDS was refused (%s)", hipGetErrorString(e));
        return -1;
    }
    *out = h;
    return 0;
}

int dpe_cd_destroy(dpe_cd *h)
{
    if (!h) return 0;
    if (h->updated) (void)hipStreamSynchronize(h->stream);
    for (void *p : {(void *)h->grid_d, (void *)h->tau_d, (void *)h->bf_d, (void *)h->keys_d, (void *)h->score_d,
                    (void *)h->jm_d, (void *)h->res_d})
        if (p) (void)hipFree(p);
    delete h;
    return 0;
}

int dpe_cd_predict(const dpe_cd_config *cfg, int32_t nSv, const double *eph, const int32_t *prn, const int32_t *row, const double *p0,
                   double rxTime, dpe_cd_sv *sv)
{
    DPE_REQUIRE(cfg && eph && prn && row && p0 && sv, "[CollectiveDetector] predict: null argument");
    DPE_REQUIRE(nSv >= 1 && nSv <= DPE_CD_MAX_SV, "[CollectiveDetector] predict: nSv %d outside 1..%d", nSv, DPE_CD_MAX_SV);
    DPE_REQUIRE(cfg->M >= kCdMinM && cfg->M <= kCdMaxM && std::isfinite(cfg->samplingFrequency) && cfg->samplingFrequency > 0.0 &&
                    std::isfinite(cfg->binStartHz) && std::isfinite(cfg->binStepHz) && cfg->binStepHz != 0.0 &&
                    (cfg->dopplerSign == 1.0 || cfg->dopplerSign == -1.0),
                "[CollectiveDetector] predict: M, the sampling frequency, the bin raster or dopplerSign is not what create accepts");
    DPE_REQUIRE(std::isfinite(p0[0]) && std::isfinite(p0[1]) && std::isfinite(p0[2]) && std::isfinite(rxTime),
                "[CollectiveDetector] predict: p0 or the receive time is not finite");
    for (int k = 0; k < nSv; ++k) {
        const char *why = cd_predict_sv(eph + (size_t)k * DPE_NAV_EPH_DOUBLES, prn[k], row[k], p0, rxTime, cfg->samplingFrequency,
                                        cfg->binStartHz, cfg->binStepHz, cfg->dopplerSign, cfg->M, sv[k]);
        DPE_REQUIRE(!why, "[CollectiveDetector] predict: SV %d (PRN %d): %s", k, prn[k], why);
    }
    return 0;
}

int dpe_cd_update(dpe_cd *h, const float *surface_dev, int32_t nRows, const double *p0, const double *enu2ecef, int32_t nSv,
                  const dpe_cd_sv *sv_host, dpe_stream_t stream_)
{
    DPE_REQUIRE(h && surface_dev && p0 && enu2ecef && sv_host, "[CollectiveDetector] update: null argument");
    DPE_REQUIRE(nSv >= 1 && nSv <= h->cfg.maxSv, "[CollectiveDetector] update: nSv %d outside 1..%d (the handle's maximum)", nSv, h->cfg.maxSv);
    DPE_REQUIRE(nRows >= 1, "[CollectiveDetector] update: a surface of %d rows", nRows);
    for (int i = 0; i < 3; ++i) DPE_REQUIRE(std::isfinite(p0[i]), "[CollectiveDetector] update: p0 is not finite");
    for (int i = 0; i < 9; ++i) DPE_REQUIRE(std::isfinite(enu2ecef[i]), "[CollectiveDetector] update: enu2ecef is not finite");
    for (int k = 0; k < nSv; ++k) {
        const char *why = cd_sv_problem(sv_host[k], h->cfg.M, nRows);
        DPE_REQUIRE(!why, "[CollectiveDetector] update: SV %d (PRN %d, row %d of %d): %s", k, sv_host[k].prn, sv_host[k].row, nRows, why);
    }
    const dpe_cd_config &c = h->cfg;
    const CdPlan pl = cd_plan(c.M, nSv, c.driftHalfWidth, c.nPoints);
    const CdArgs a = cd_args(c, pl, p0, enu2ecef, nSv, sv_host);
    const hipStream_t st = (hipStream_t)stream_;
    const int nTau = c.nPoints * DPE_CD_MAX_SV;
    cd_tau_kernel<<<dim3((nTau + 255) / 256), dim3(256), 0, st>>>(a, h->grid_d, h->tau_d, h->bf_d, h->keys_d);
    const dim3 grid((unsigned)pl.blocksX, (unsigned)pl.nJ);
    if (pl.useLds) cd_scan_kernel<true><<<grid, dim3(kCdThreads), pl.ldsBytes, st>>>(a, surface_dev, h->bf_d, h->keys_d);
    else cd_scan_kernel<false><<<grid, dim3(kCdThreads), 0, st>>>(a, surface_dev, h->bf_d, h->keys_d);
    cd_final_kernel<<<dim3(1), dim3(256), 0, st>>>(a, surface_dev, h->tau_d, h->bf_d, h->keys_d, h->score_d, h->jm_d, h->res_d);
    DPE_CHECK_HIP(hipGetLastError());
    h->updated = true;
    h->stream = st;
    h->nSv = nSv;
    for (int i = 0; i < 3; ++i) h->p0[i] = p0[i];
    for (int i = 0; i < 9; ++i) h->R[i] = enu2ecef[i];
    for (int k = 0; k < nSv; ++k) {
        h->prn[k] = sv_host[k].prn;
        h->bin[k] = a.sv[k].bin;
    }
    h->binsOut = cd_bins_out_of_range(h->bin, nSv, c.driftHalfWidth, c.nBins);
    return 0;
}

int dpe_cd_results(dpe_cd *h, dpe_cd_result *res, dpe_cd_sv_result *sv)
{
    DPE_REQUIRE(h && res, "[CollectiveDetector] results: null argument");
    DPE_REQUIRE(h->updated, "[CollectiveDetector] results: no update yet");
    CdDevResult d;
    DPE_CHECK_HIP(hipMemcpyAsync(&d, h->res_d, sizeof(d), hipMemcpyDeviceToHost, h->stream));
    DPE_CHECK_HIP(hipStreamSynchronize(h->stream));
    const dpe_cd_config &c = h->cfg;
    DPE_REQUIRE(d.point >= 0 && d.point < c.nPoints && d.m >= 0 && d.m < c.M && d.j >= -c.driftHalfWidth && d.j <= c.driftHalfWidth,
                "[CollectiveDetector] results: the device reported an index outside the grid (point %d, m %d, j %d)", d.point, d.m, d.j);
    res->point = d.point; res->m = d.m; res->j = d.j;
    res->binsOutOfRange = h->binsOut;
    res->nSv = h->nSv; res->reserved = 0;
    res->score = d.score;
    const double *g = h->grid.data() + 3 * (size_t)d.point;
    for (int i = 0; i < 3; ++i) res->fixEcef[i] = h->p0[i] + (h->R[3 * i] * g[0] + h->R[3 * i + 1] * g[1] + h->R[3 * i + 2] * g[2]);
    res->clockBiasM = (double)d.m / c.samplingFrequency * kC;
    res->clockDriftMps = -c.dopplerSign * (double)d.j * c.binStepHz * kC / kFL1;
    if (sv)
        for (int k = 0; k < h->nSv; ++k) {
            dpe_cd_sv_result &r = sv[k];
            const int di = h->bin[k] + d.j;
            r.prn = h->prn[k];
            r.found = (di >= 0 && di < c.nBins) ? 1 : 0;
            r.maxCodeIdx = d.codeIdx[k];
            r.maxDoppIdx = di;
            r.rc = (double)kLCA - ((double)d.codeIdx[k] / c.samplingFrequency) * kFCA;   // as dpe_acq_results
            r.fi = c.binStartHz + c.binStepHz * di;
            r.fc = kFCA + (c.dopplerSign * kFCA / kFL1) * r.fi;
            r.peak = d.peak[k];
        }
    return 0;
}

int dpe_cd_map(dpe_cd *h, const float **score_dev, const int32_t **jm_dev)
{
    DPE_REQUIRE(h, "[CollectiveDetector] map: null handle");
    if (score_dev) *score_dev = h->score_d;
    if (jm_dev) *jm_dev = h->jm_d;
    return 0;
}

}  // extern "C"
