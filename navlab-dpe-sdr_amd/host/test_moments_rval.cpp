// test_moments_rval -- dpe_bcm_moments_rval on its edge inputs, as a stand-alone host program (its own main, nothing but the C header)
// so that it can be built with -fsanitize=address,undefined together with the host code it calls:
//     g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined -O1 -g -std=c++17 -DDPE_MOMENTS_RVAL_STANDALONE \
//         host/test_moments_rval.cpp -o test_moments_rval_san && ./test_moments_rval_san
// (the define compiles csrc/dpe_bcm_moments_cov.h's function into this program behind the export's name: no library, no GPU), or against
// libdpe_hip.so without it:  g++ -std=c++17 host/test_moments_rval.cpp -I../include -L. -ldpe_hip -Wl,-rpath,'$ORIGIN'
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#ifdef DPE_MOMENTS_RVAL_STANDALONE
#include "../csrc/dpe_bcm_moments_cov.h"
extern "C" int dpe_bcm_moments_rval(const double sums[2][15], const double enu2ecef[9], const double floorVar[2][4], double R[64], int32_t *fallback)
{
    if (!sums || !enu2ecef || !floorVar || !R || !fallback) return -1;
    for (int m = 0; m < 2; ++m)
        for (int c = 0; c < 4; ++c)
            if (!(std::isfinite(floorVar[m][c]) && floorVar[m][c] >= 0.0)) return -1;
    *fallback = dpe::mom_rval(&sums[0][0], enu2ecef, &floorVar[0][0], R);
    return 0;
}
#else
#include "dpe_hip.h"
#endif

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

// the fifteen sums of one point x with weight w
static void one_point(const double x[4], double w, double S[15])
{
    static const int second[4][4] = {{5, 6, 7, 8}, {6, 9, 10, 11}, {7, 10, 12, 13}, {8, 11, 13, 14}};
    S[0] = w;
    for (int a = 0; a < 4; ++a) S[1 + a] = w * x[a];
    for (int a = 0; a < 4; ++a)
        for (int b = a; b < 4; ++b) S[second[a][b]] = (w * x[a]) * x[b];
}

int main()
{
    const double c = std::cos(0.7), s = std::sin(0.7);
    const double Rm[9] = {c, -s, 0, s, c, 0, 0, 0, 1};
    const double fv[2][4] = {{1.0 / 3, 1.0 / 3, 1.0 / 3, 0.0}, {0.02, 0.03, 0.04, 0.0}};
    double sums[2][15], R[64];
    int32_t fb = -1;
    // 1. a single point per manifold: C cancels to 0, the block is the floor; symmetric; off-diagonal blocks 0
    const double x0[4] = {2.0, -4.0, 6.0, 1.5}, x1[4] = {-0.5, 0.25, 0.0, 0.0};
    one_point(x0, 3.25, sums[0]);
    one_point(x1, 0.5, sums[1]);
    EXPECT(dpe_bcm_moments_rval(sums, Rm, fv, R, &fb) == 0 && fb == 0);
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j < 8; ++j) {
            EXPECT(std::memcmp(&R[i * 8 + j], &R[j * 8 + i], sizeof(double)) == 0);
            if ((i < 4) != (j < 4)) EXPECT(R[i * 8 + j] == 0.0);
        }
    EXPECT(R[3 * 8 + 3] == 0.0 && R[7 * 8 + 7] == 0.0);                 // (no spread along t, no floor along t)
    EXPECT(std::fabs(R[0] - 1.0 / 3) < 1e-15 && std::fabs(R[9] - 1.0 / 3) < 1e-15 && R[18] == 1.0 / 3);   // (equal ENU floors: the rotation keeps them)
    // 2. S0 = 0 in either manifold, and in both: the identity block and its bit
    for (int mask = 1; mask < 4; ++mask) {
        one_point(x0, 3.25, sums[0]);
        one_point(x1, 0.5, sums[1]);
        for (int m = 0; m < 2; ++m)
            if (mask >> m & 1) std::memset(sums[m], 0, sizeof(sums[m]));
        EXPECT(dpe_bcm_moments_rval(sums, Rm, fv, R, &fb) == 0 && fb == mask);
        for (int m = 0; m < 2; ++m)
            if (mask >> m & 1)
                for (int a = 0; a < 4; ++a)
                    for (int b = 0; b < 4; ++b) EXPECT(R[(4 * m + a) * 8 + 4 * m + b] == (a == b ? 1.0 : 0.0));
    }
    // 3. sums that are not finite go the way of an empty manifold: no NaN reaches the filter
    one_point(x0, 3.25, sums[0]);
    one_point(x1, 0.5, sums[1]);
    sums[0][0] = NAN;
    sums[1][7] = INFINITY;
    EXPECT(dpe_bcm_moments_rval(sums, Rm, fv, R, &fb) == 0 && fb == 3);
    for (int i = 0; i < 64; ++i) EXPECT(R[i] == (i % 9 == 0 ? 1.0 : 0.0));
    // 4. huge and tiny sums stay finite or fall back, never trap
    one_point(x0, 1e300, sums[0]);
    one_point(x1, 1e-300, sums[1]);
    EXPECT(dpe_bcm_moments_rval(sums, Rm, fv, R, &fb) == 0);
    for (int i = 0; i < 64; ++i) EXPECT(std::isfinite(R[i]));
    // 5. refusals: null arguments, a negative or non-finite floor
    EXPECT(dpe_bcm_moments_rval(nullptr, Rm, fv, R, &fb) != 0);
    EXPECT(dpe_bcm_moments_rval(sums, Rm, fv, R, nullptr) != 0);
    double bad[2][4];
    std::memcpy(bad, fv, sizeof(bad));
    bad[1][3] = -1e-9;
    EXPECT(dpe_bcm_moments_rval(sums, Rm, bad, R, &fb) != 0);
    bad[1][3] = NAN;
    EXPECT(dpe_bcm_moments_rval(sums, Rm, bad, R, &fb) != 0);
    std::printf(fails ? "test_moments_rval: %d checks failed\n" : "test_moments_rval: ok\n", fails);
    return fails ? 1 : 0;
}
