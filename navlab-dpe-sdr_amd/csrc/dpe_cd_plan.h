// dpe_cd_plan.h -- collective detection's host-side planning as plain C++: the prediction of an SV's delay and Doppler bin at the
// a-priori position from its ephemeris, the launch plan of the scan (run length, LDS pitch and bytes per K and M, the split of the
// grid over blocks and drift hypotheses), the per-call parameter block, and what create / predict / update refuse.  Nothing here
// launches: dpe_cd.hip passes sizes in, its kernels read the same constants, and host/test_cd_plan.cpp holds predictions and plans
// to tests/test_cd_plan_cpu.py's numpy values and table with a host compiler.  DESIGN.md 7g.
//
// The Kepler / SV-clock arithmetic is dpe_sat.h's sat_state and rotate_state; nothing of it is restated.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/dpe_hip.h"
#include "dpe_sat.h"

namespace dpe {

constexpr int kCdThreads = 512;            // lanes per block: 500 runs of 5 delays cover M = 2 500 in one pass
constexpr int kCdRun = 5;                  // consecutive clock values per lane: 6 reads serve 5 lerps; odd, so a wave's ds_read_b32
                                           // addresses (stride 5 dwords) fall on 32 distinct banks per half-wave
constexpr int kCdFlush = 8;                // points a block scores between two flushes of its LDS keys to the device-wide ones
constexpr int kCdTargetBlocks = 1024;      // at most two rounds of the 2 x 256 blocks that fit the device at 80 KB of LDS each
constexpr size_t kCdLdsMax = 155 * 1024;   // dynamic LDS a block may ask for (of the CU's 160 KB)
constexpr int kCdMinM = 16, kCdMaxM = 32768, kCdMaxPoints = 65536, kCdMaxBins = 65536;

// One SV of an update as the kernels read it (block-uniform: scalar loads from the kernel-argument segment).
struct CdSv {
    double sx, sy, sz;     // ECEF
    double delay0, range0;
    int32_t row, bin;      // surface row; round_half_even(bin0)
};
struct CdArgs {
    CdSv sv[DPE_CD_MAX_SV];
    double p0[3], R[9];
    double fs;
    int32_t K, M, nBins, J, P, pitch, nRuns, reserved;
};

struct CdPlan {
    int run, nRuns;        // delays per lane and runs per row: ceil(M / run)
    int pitch;             // floats per staged row: M + run (the wrap pad a run may read into)
    int useLds;            // 1: the K rows of a block's bin are staged in LDS; 0: read from L2 (K pitch 4 B above kCdLdsMax)
    size_t ldsBytes;       // dynamic LDS of the staged form
    int nJ, blocksX;       // grid: blocksX x nJ blocks; block (x, jj) scores points x, x + blocksX, ... at drift jj - J
    int pointsPerBlock;    // ceil(P / blocksX)
};
inline CdPlan cd_plan(int M, int K, int J, int P)
{
    CdPlan p{};
    p.run = kCdRun;
    p.nRuns = (M + kCdRun - 1) / kCdRun;
    p.pitch = M + kCdRun;
    p.ldsBytes = (size_t)K * p.pitch * sizeof(float);
    p.useLds = p.ldsBytes <= kCdLdsMax ? 1 : 0;
    if (!p.useLds) p.ldsBytes = 0;
    p.nJ = 2 * J + 1;
    const int want = kCdTargetBlocks / p.nJ;   // rounded down (nJ <= 65): one block over the target would open a third, nearly empty round
    p.blocksX = P < want ? P : want;
    p.pointsPerBlock = (P + p.blocksX - 1) / p.blocksX;
    return p;
}

// ---- refusals.  Each returns nullptr or the reason.
inline double cd_corner_m(const double *enu, int P)
{
    double far2 = 0.0;
    for (int i = 0; i < P; ++i) {
        const double *d = enu + 3 * (size_t)i;
        const double r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        if (!(r2 <= far2)) far2 = r2;   // (a NaN ends up here and is refused as not finite)
    }
    return std::sqrt(far2);
}
inline double cd_max_corner_m(double binStepHz) { return 0.5 * std::fabs(binStepHz) / DPE_CD_DOPPLER_HZ_PER_KM * 1000.0; }
inline const char *cd_config_problem(const dpe_cd_config &c)
{
    if (c.M < kCdMinM || c.M > kCdMaxM) return "M outside 16..32768";
    if (c.nBins < 1 || c.nBins > kCdMaxBins) return "nBins outside 1..65536";
    if (c.maxSv < 1 || c.maxSv > DPE_CD_MAX_SV) return "maxSv outside 1..16";
    if (c.driftHalfWidth < 0 || c.driftHalfWidth > DPE_CD_MAX_DRIFT) return "driftHalfWidth outside 0..32";
    if (c.nPoints < 1 || c.nPoints > kCdMaxPoints) return "nPoints outside 1..65536";
    if (!c.enuGrid) return "null enuGrid";
    if (!(std::isfinite(c.samplingFrequency) && c.samplingFrequency > 0.0)) return "sampling frequency not positive";
    if (!(std::isfinite(c.binStartHz) && std::isfinite(c.binStepHz) && c.binStepHz != 0.0)) return "bin raster not finite, or a zero bin step";
    if (!(c.dopplerSign == 1.0 || c.dopplerSign == -1.0)) return "dopplerSign is neither +1 nor -1";
    const double far = cd_corner_m(c.enuGrid, c.nPoints);
    if (!std::isfinite(far)) return "a grid point is not finite";
    if (far > cd_max_corner_m(c.binStepHz))
        return "the grid reaches farther from p0 than half a bin step allows at 1.1 Hz per km (the Doppler's change over the grid is not modelled)";
    return nullptr;
}
inline const char *cd_sv_problem(const dpe_cd_sv &s, int M, int nRows)
{
    if (s.row < 0 || s.row >= nRows) return "surface row outside the surface";
    if (!(std::isfinite(s.sat[0]) && std::isfinite(s.sat[1]) && std::isfinite(s.sat[2]))) return "satellite position not finite";
    if (!(s.delay0 >= 0.0 && s.delay0 < (double)M)) return "delay0 outside [0, M)";
    if (!(std::fabs(s.bin0) < 1.0e6)) return "bin0 not finite or beyond 1e6 bins";
    return nullptr;
}

// (SV, j) pairs whose bin leaves the raster
inline int cd_bins_out_of_range(const int32_t *bin, int K, int J, int nBins)
{
    int n = 0;
    for (int k = 0; k < K; ++k)
        for (int j = -J; j <= J; ++j) n += (bin[k] + j < 0 || bin[k] + j >= nBins) ? 1 : 0;
    return n;
}

// ---- prediction.  Light time by fixed-point iteration (three rounds: the third moves the range by < 1e-6 m); the ephemeris is
// evaluated at the SV's own clock reading of the transmit time, the state rotated into the receive-time frame (rotate_state), the
// range rate taken as propagate() takes it for a receiver at rest in ECEF.  Returns nullptr or the reason.
inline const char *cd_predict_sv(const double *eph21, int prn, int row, const double *p0, double rxTime, double fs, double binStartHz,
                                 double binStepHz, double dopplerSign, int M, dpe_cd_sv &out)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (prn < 1 || prn > 37) return "PRN outside 1..37";
    if (row < 0) return "negative surface row";
    for (int i = 0; i < DPE_NAV_EPH_DOUBLES; ++i)
        if (!std::isfinite(eph21[i])) return "ephemeris not finite";
    Eph e;
    static_assert(sizeof(Eph) == DPE_NAV_EPH_DOUBLES * sizeof(double), "Eph is the 21 doubles of DPE_NAV_EPH_DOUBLES, in order");
    std::memcpy(&e, eph21, sizeof(e));
    if (!(e.sqrtA > 1000.0 && e.e >= 0.0 && e.e < 0.5)) return "ephemeris is not a GPS orbit (sqrt_A, e)";
    double tau = 0.07, dt = 0.0, range = 0.0, s[8], sr[8];
    for (int it = 0; it < 3; ++it) {
        if (sat_state(e, rxTime - tau + dt, s)) return "Kepler's equation did not converge";
        rotate_state(s, tau, sr);
        const double lx = sr[0] - p0[0], ly = sr[1] - p0[1], lz = sr[2] - p0[2];
        range = std::sqrt(lx * lx + ly * ly + lz * lz);
        tau = range / kC;
        dt = s[3];
    }
    if (!(range > 1.5e7 && range < 3.0e7)) return "range outside 15 000..30 000 km: p0, the time or the ephemeris is off";
    const double lx = sr[0] - p0[0], ly = sr[1] - p0[1], lz = sr[2] - p0[2];
    const double ex = -kOEDot * p0[1], ey = kOEDot * p0[0];
    const double lrr = ((lx / range) * (ex - sr[4])) + ((ly / range) * (ey - sr[5])) + ((lz / range) * (0.0 - sr[6]));   // = -range rate
    const double fi = kFL1 * (lrr / kC + sr[7]) / dopplerSign;
    double frac = std::fmod(range / kC - sr[3], kTCA);
    if (frac < 0.0) frac += kTCA;
    double delay0 = frac * fs;
    if (delay0 >= (double)M) delay0 -= (double)M;
    if (delay0 < 0.0) delay0 = 0.0;
    out.prn = prn;
    out.row = row;
    out.sat[0] = sr[0]; out.sat[1] = sr[1]; out.sat[2] = sr[2];
    out.delay0 = delay0;
    out.bin0 = (fi - binStartHz) / binStepHz;
    out.range0 = range;
    out.dopplerHz = fi;
    return nullptr;
}

// The parameter block of one update.  bin = round_half_even(bin0) (std::nearbyint in the default rounding mode).
inline CdArgs cd_args(const dpe_cd_config &c, const CdPlan &pl, const double *p0, const double *R, int K, const dpe_cd_sv *sv)
{
    CdArgs a{};
    for (int k = 0; k < K; ++k) {
        CdSv &d = a.sv[k];
        d.sx = sv[k].sat[0]; d.sy = sv[k].sat[1]; d.sz = sv[k].sat[2];
        const double lx = d.sx - p0[0], ly = d.sy - p0[1], lz = d.sz - p0[2];
        d.range0 = std::sqrt(lx * lx + ly * ly + lz * lz);
        d.delay0 = sv[k].delay0;
        d.row = sv[k].row;
        d.bin = (int32_t)std::nearbyint(sv[k].bin0);
    }
    for (int i = 0; i < 3; ++i) a.p0[i] = p0[i];
    for (int i = 0; i < 9; ++i) a.R[i] = R[i];
    a.fs = c.samplingFrequency;
    a.K = K; a.M = c.M; a.nBins = c.nBins; a.J = c.driftHalfWidth; a.P = c.nPoints;
    a.pitch = pl.pitch; a.nRuns = pl.nRuns;
    return a;
}

}  // namespace dpe
