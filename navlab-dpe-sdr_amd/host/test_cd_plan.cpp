// test_cd_plan.cpp -- csrc/dpe_cd_plan.h with a host C++ compiler, no GPU: the launch plan's properties are checked here (exit 1
// with a message on the first that fails), and plans, predictions and refusals are evaluated for the cases of a text file, one answer
// per line, for tests/test_cd_plan_cpu.py to hold against its table and against numpy.  Doubles travel as C99 hex floats.  (The
// header and the orbit arithmetic it takes from dpe_sat.h are plain C++: no HIP header is on the include path.)
//
//   test_cd_plan cases.txt
//     plan M K J P                                   -> run nRuns pitch useLds ldsBytes nJ blocksX pointsPerBlock
//     pred e0 .. e20 prn row x y z t fs b0 db ds M   -> ok delay0 bin0 sx sy sz range0      or: refused <reason>
//     cfg M nBins maxSv J fs b0 db ds far            -> ok                                  or: refused <reason>   (two points: 0 and far east)
//     sv row nRows delay0 bin0 M                     -> ok                                  or: refused <reason>
//     oob J nBins b0 b1 ...                          -> binsOutOfRange
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../csrc/dpe_cd_plan.h"

using namespace dpe;

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            fprintf(stderr, "test_cd_plan: " __VA_ARGS__); \
            fprintf(stderr, "  (%s)\n", #cond);            \
            return 1;                                      \
        }                                                  \
    } while (0)

static int check_plans()
{
    for (int M : {16, 17, 64, 2046, 2500, 4000, 4999, 5000, 16384, 32768})
        for (int K = 1; K <= DPE_CD_MAX_SV; ++K)
            for (int J : {0, 1, 2, 10, 31, 32})
                for (int P : {1, 2, 5, 15, 16, 17, 49, 131, 1024, 1025, 1031, 1681, 65536}) {
                    const CdPlan p = cd_plan(M, K, J, P);
                    CHECK(p.run == kCdRun && p.run % 2 == 1, "run length");
                    CHECK(p.nRuns * p.run >= M && (p.nRuns - 1) * p.run < M, "M = %d: %d runs", M, p.nRuns);
                    CHECK(p.pitch == M + p.run, "M = %d: pitch %d", M, p.pitch);   // a run starting at M - 1 reads run + 1 entries
                    const size_t bytes = (size_t)K * p.pitch * 4;
                    CHECK(p.useLds == (bytes <= kCdLdsMax ? 1 : 0) && p.ldsBytes == (p.useLds ? bytes : 0), "M = %d K = %d: LDS", M, K);
                    CHECK(p.nJ == 2 * J + 1, "J = %d", J);
                    CHECK(p.blocksX >= 1 && p.blocksX <= P, "P = %d J = %d: %d blocks", P, J, p.blocksX);
                    CHECK((long long)p.blocksX * p.nJ <= kCdTargetBlocks, "P = %d J = %d: %d x %d blocks", P, J, p.blocksX, p.nJ);
                    CHECK(p.blocksX == P || (long long)(p.blocksX + 1) * p.nJ > kCdTargetBlocks, "P = %d J = %d: too few blocks", P, J);
                    CHECK((long long)p.pointsPerBlock * p.blocksX >= P && (long long)(p.pointsPerBlock - 1) * p.blocksX < P, "points per block");
                }
    static_assert(sizeof(CdArgs) <= 4096, "the parameter block travels as a kernel argument");
    static_assert(kCdLdsMax <= 160 * 1024 && kCdFlush <= 64, "LDS of a CU; one lane per flushed key");
    return 0;
}

int main(int argc, char **argv)
{
    if (check_plans()) return 1;
    if (argc < 2) return 0;
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "test_cd_plan: cannot open %s\n", argv[1]); return 2; }
    static char line[8192];
    while (fgets(line, sizeof(line), f)) {
        std::vector<std::string> w;
        for (char *t = strtok(line, " \t\r\n"); t; t = strtok(nullptr, " \t\r\n")) w.emplace_back(t);
        if (w.empty()) continue;
        auto D = [&](size_t i) { return strtod(w[i].c_str(), nullptr); };
        auto I = [&](size_t i) { return (int)strtol(w[i].c_str(), nullptr, 10); };
        if (w[0] == "plan" && w.size() == 5) {
            const CdPlan p = cd_plan(I(1), I(2), I(3), I(4));
            printf("%d %d %d %d %zu %d %d %d\n", p.run, p.nRuns, p.pitch, p.useLds, p.ldsBytes, p.nJ, p.blocksX, p.pointsPerBlock);
        } else if (w[0] == "pred" && w.size() == 1 + 21 + 11) {
            double e[21], p0[3];
            for (int i = 0; i < 21; ++i) e[i] = D(1 + i);
            for (int i = 0; i < 3; ++i) p0[i] = D(24 + i);
            dpe_cd_sv s{};
            const char *why = cd_predict_sv(e, I(22), I(23), p0, D(27), D(28), D(29), D(30), D(31), I(32), s);
            if (why) printf("refused %s\n", why);
            else printf("ok %a %a %a %a %a %a\n", s.delay0, s.bin0, s.sat[0], s.sat[1], s.sat[2], s.range0);
        } else if (w[0] == "cfg" && w.size() == 10) {
            const double grid[6] = {0.0, 0.0, 0.0, D(9), 0.0, 0.0};
            dpe_cd_config c{};
            c.M = I(1); c.nBins = I(2); c.maxSv = I(3); c.driftHalfWidth = I(4); c.nPoints = 2; c.enuGrid = grid;
            c.samplingFrequency = D(5); c.binStartHz = D(6); c.binStepHz = D(7); c.dopplerSign = D(8);
            const char *why = cd_config_problem(c);
            printf("%s%s\n", why ? "refused " : "ok", why ? why : "");
        } else if (w[0] == "sv" && w.size() == 6) {
            dpe_cd_sv s{};
            s.row = I(1); s.delay0 = D(3); s.bin0 = D(4);
            const char *why = cd_sv_problem(s, I(5), I(2));
            printf("%s%s\n", why ? "refused " : "ok", why ? why : "");
        } else if (w[0] == "oob" && w.size() >= 4) {
            std::vector<int32_t> b;
            for (size_t i = 3; i < w.size(); ++i) b.push_back(I(i));
            printf("%d\n", cd_bins_out_of_range(b.data(), (int)b.size(), I(1), I(2)));
        } else {
            fprintf(stderr, "test_cd_plan: bad line starting with %s (%zu words)\n", w[0].c_str(), w.size());
            fclose(f);
            return 2;
        }
    }
    fclose(f);
    return 0;
}
