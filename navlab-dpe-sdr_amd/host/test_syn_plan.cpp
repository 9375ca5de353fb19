// test_syn_plan.cpp -- csrc/dpe_syn_plan.h with a plain C++ compiler, no GPU: the launch geometry's properties are checked here
// (exit 1 with a message on the first that fails), and the fp64 mappings are evaluated for the cases of a text file, one answer per
// line, for tests/test_syn_plan_cpu.py to hold against numpy.  Doubles travel as C99 hex floats, so nothing is lost in print.
//
//   test_syn_plan cases.txt
//     flip cpEla cpRef rc fc fs        -> flipAt
//     bits first n fs rc fc cpRef      -> ok bitFirst bitLast
//     chip t fc rc                     -> chip period
//     tw i fs                          -> t (window form)        tr n fs -> t (record form)
//     chan rc fc cpRef prn flipAt S    -> flipAt firstEdge prnRow (the parameter block)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../csrc/dpe_syn_plan.h"

using namespace dpe;

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            fprintf(stderr, "test_syn_plan: " __VA_ARGS__); \
            fprintf(stderr, "  (%s)\n", #cond);           \
            return 1;                                     \
        }                                                 \
    } while (0)

static int check_geometry()
{
    const int sizes[] = {1, 2, 3, 4, 5, 7, 8, 4093, 4095, 4096, 4097, 8191, 12500, 50000, 500000, 1 << 30};
    for (int S : sizes)
        for (int K : {1, 12, 37}) {
            const SynGeom g = syn_geom(S, 5, K);
            CHECK(g.nBlocks == 5LL * g.blocksPerSeg && g.ldsBytes == (size_t)K * 1024, "geometry of S = %d", S);
            for (int align = 0; align < 4; ++align) {
                int next = 0;
                for (int j = 0; j < g.blocksPerSeg; ++j) {
                    int i0, i1;
                    syn_block_range(S, align, j, i0, i1);
                    CHECK(i0 == next || (i0 >= i1 && next == S), "S = %d align %d block %d starts at %d, not %d", S, align, j, i0, next);
                    CHECK(i1 <= S && i1 - i0 <= kSynBlockGroups * kSynLaneSamples, "S = %d align %d block %d ends at %d", S, align, j, i1);
                    CHECK(i0 == 0 || i0 >= i1 || (i0 + align) % kSynLaneSamples == 0, "S = %d align %d block %d: a lane's group is split", S, align, j);
                    if (i1 > i0) next = i1;
                }
                CHECK(next == S, "S = %d align %d: the blocks end at %d", S, align, next);
                CHECK(syn_groups(S, align) <= (long long)g.blocksPerSeg * kSynBlockGroups, "S = %d align %d: groups beyond the blocks", S, align);
            }
        }
    return 0;
}

static int check_floor_div()
{
    const int64_t ms[] = {0, 1, 19, 20, 21, 1022, 1023, 1024, 2045, 2046, 1023LL * 20 - 1, 1023LL * 20, 4294967296LL, 1757000000LL,
                          (1LL << 51) - 1, (1LL << 51) - 1023, 1023LL * 2199023255LL, 1023LL * 2199023255LL - 1};
    for (int64_t m0 : ms)
        for (int sgn : {1, -1})
            for (int d : {20, 1023}) {
                const int64_t m = sgn * m0;
                int64_t q = m / d, r = m % d;
                if (r < 0) { r += d; q -= 1; }
                double rem;
                const double got = syn_floor_div((double)m, (double)d, d == 20 ? 0.05 : 1.0 / 1023.0, rem);
                CHECK((int64_t)got == q && (int64_t)rem == r, "floor division of %" PRId64 " by %d", m, d);
            }
    return 0;
}

int main(int argc, char **argv)
{
    if (check_geometry() || check_floor_div()) return 1;
    if (argc < 2) return 0;
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "test_syn_plan: cannot open %s\n", argv[1]); return 2; }
    char line[512], w[8][64];
    while (fgets(line, sizeof(line), f)) {
        const int n = sscanf(line, "%63s %63s %63s %63s %63s %63s %63s %63s", w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]);
        if (n < 1) continue;
        auto D = [&](int i) { return strtod(w[i], nullptr); };
        auto I = [&](int i) { return strtoll(w[i], nullptr, 10); };
        if (!strcmp(w[0], "flip") && n == 6) {
            printf("%" PRId64 "\n", syn_flip_at((int32_t)I(1), (int32_t)I(2), D(3), D(4), D(5)));
        } else if (!strcmp(w[0], "bits") && n == 7) {
            dpe_chan_start c{};
            c.codePhaseStart = D(4); c.codeFrequency = D(5); c.cpReference = (int32_t)I(6); c.prn = 1;
            int64_t b0 = 0, b1 = 0;
            const bool ok = syn_bit_span(I(1), I(2), D(3), c, b0, b1);
            printf("%d %" PRId64 " %" PRId64 "\n", ok ? 1 : 0, b0, b1);
        } else if (!strcmp(w[0], "chip") && n == 4) {
            double period;
            const int chip = syn_chip(D(1), D(2), D(3), period);
            printf("%d %.0f\n", chip, period);
        } else if (!strcmp(w[0], "tw") && n == 3) {
            printf("%a\n", syn_time_window((int32_t)I(1), D(2)));
        } else if (!strcmp(w[0], "tr") && n == 3) {
            printf("%a\n", syn_time_record(I(1), D(2)));
        } else if (!strcmp(w[0], "chan") && n == 7) {
            dpe_chan_start c{};
            c.codePhaseStart = D(1); c.codeFrequency = D(2); c.cpReference = (int32_t)I(3); c.prn = (int32_t)I(4);
            const SynChan s = syn_chan(c, 1.0, I(5), (int)I(6));
            printf("%d %d %d\n", s.flipAt, s.firstEdge, s.prnRow);
        } else {
            fprintf(stderr, "test_syn_plan: bad line: %s", line);
            fclose(f);
            return 2;
        }
    }
    fclose(f);
    return 0;
}
