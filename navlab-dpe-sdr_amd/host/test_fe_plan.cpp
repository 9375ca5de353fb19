// test_fe_plan.cpp -- csrc/dpe_fe_plan.h with a plain C++ compiler, no GPU: the tile geometry's properties are checked here (exit 1
// with a message on the first that fails), and the mappings are evaluated for the cases of a text file, one answer per line, for
// tests/test_fe_plan_cpu.py to hold against Python integers.  Doubles travel as C99 hex floats.
//
//   test_fe_plan cases.txt
//     delta fIF fs                       -> delta realisedIF
//     phase n delta                      -> (n delta) mod 2^32
//     needed outFirst outCount D T len   -> lo hi
//     geom D T real                      -> tileOut rowLen pitch ldsBytes Q rem
//     owner D T real i                   -> block lane slot
//     tap D T real delta t               -> mode-2 table entry of tap t as four hex floats, for gain 1 and h[t] = 1
//     taps D T mode                      -> the whole table [D][qPitch][4] of mode 0, 1 or 2 as hex floats, for gain 1, delta 0 and h[t] = t + 1
//     cfg fmt out D T fs fIF             -> the refusal of dpe_fe_create's checks, or "ok"
//     conv fmt D T rawFirst rawCount len outFirst outCount rawAlign outAlign -> the refusal of dpe_fe_convert's checks, or "ok"
//     quant re im                        -> the int16 I/Q word of the fp32 pair (dpe_stream_plan.h) and the components it clipped
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../csrc/dpe_fe_plan.h"

using namespace dpe;

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            fprintf(stderr, "test_fe_plan: " __VA_ARGS__); \
            fprintf(stderr, "  (%s)\n", #cond);           \
            return 1;                                     \
        }                                                 \
    } while (0)

// Every output of a call has exactly one owner; the staged tile covers what its outputs read, each staged input lies at its own
// LDS element, every LDS index a lane touches is inside the allocation; sizes stay inside the LDS and 32-bit limits.
static int check_geometry()
{
    const int Ds[] = {1, 2, 3, 4, 5, 7, 10, 16, 31, 63, 64};
    const int Ts[] = {1, 3, 5, 9, 33, 63, 65, 81, 129, 513, 1021, 1023};
    for (int D : Ds)
        for (int T : Ts)
            for (int real = 0; real < 2; ++real) {
                const FeGeom g = fe_geom(D, T, real != 0);
                CHECK(g.tileOut >= kFeRun && g.tileOut % kFeRun == 0 && g.tileOut <= kFeThreads * kFeRun, "D %d T %d: tile of %d outputs", D, T, g.tileOut);
                CHECK(g.ldsBytes <= kFeLdsBytes && g.ldsBytes == g.pitch * D * g.elemBytes, "D %d T %d: %d bytes of LDS", D, T, g.ldsBytes);
                CHECK((g.Q - 1) * D + g.rem == T && g.rem >= 1 && g.rem <= D, "D %d T %d: Q %d rem %d", D, T, g.Q, g.rem);
                CHECK((long long)g.rowLen * D < (1LL << 26), "D %d T %d: staged index beyond the exact range of the division", D, T);
                // owners: the outputs of three and a bit tiles, each exactly once, in order
                const int64_t count = 3LL * g.tileOut + 7;
                CHECK(fe_blocks(g, count) == 4 && fe_blocks(g, g.tileOut) == 1 && fe_blocks(g, g.tileOut + 1) == 2, "D %d T %d: block count", D, T);
                int64_t prev = -1;
                for (int64_t i = 0; i < count; ++i) {
                    int64_t b;
                    int lane, slot;
                    fe_owner(g, i, b, lane, slot);
                    const int64_t back = b * g.tileOut + (int64_t)lane * kFeRun + slot;
                    CHECK(back == i && lane >= 0 && lane < kFeThreads && slot >= 0 && slot < kFeRun && b < fe_blocks(g, count), "D %d T %d: owner of output %" PRId64, D, T, i);
                    CHECK(back == prev + 1, "D %d T %d: output %" PRId64 " owned twice or skipped", D, T, i);
                    prev = back;
                }
                // staging: index i -> (k, p) is the division by D, and distinct inputs get distinct elements inside the allocation
                const int nElem = g.rowLen * D;
                for (int i = 0; i < nElem; ++i) {
                    int k, p;
                    fe_split((uint32_t)i, D, g.magic, k, p);
                    CHECK(k == i / D && p == i % D, "D %d T %d: split of %d", D, T, i);
                    CHECK((long long)(p * g.pitch + k + 1) * g.elemBytes <= g.ldsBytes && k < g.rowLen, "D %d T %d: element of input %d outside the LDS", D, T, i);
                }
                for (int i0 = 0; i0 < kFeThreads && i0 < nElem; i0 += 37) {      // a lane's walk through the tile, as the kernel steps it
                    int k, p;
                    fe_split((uint32_t)i0, D, g.magic, k, p);
                    for (int i = i0 + kFeThreads; i < nElem; i += kFeThreads) {
                        fe_advance(k, p, D, kFeThreads / D, kFeThreads % D);
                        CHECK(k == i / D && p == i % D, "D %d T %d: step to %d", D, T, i);
                    }
                }
                // coverage: output j of the tile and tap t read input j D + t of the tile = element (p, j + q), which is staged;
                // the window's refill reads at most element rowLen of a row (inside the pitch)
                int taps = 0;
                for (int p = 0; p < D; ++p) {
                    const int nq = fe_phase_taps(p, g.Q, g.rem);
                    taps += nq;
                    for (int q = 0; q < nq; ++q) CHECK(q * D + p < T, "D %d T %d: phase %d tap %d beyond T", D, T, p, q);
                    CHECK(nq == 0 || (nq - 1) * D + p < T, "D %d T %d: phase %d", D, T, p);
                    CHECK(nq * D + p >= T, "D %d T %d: phase %d misses a tap", D, T, p);
                    CHECK(g.tileOut - 1 + nq - 1 < g.rowLen || nq == 0, "D %d T %d: phase %d reads beyond the staged row", D, T, p);
                    CHECK(g.tileOut - kFeRun + nq - 1 + kFeRun < g.pitch, "D %d T %d: phase %d refills beyond the pitch", D, T, p);
                }
                CHECK(taps == T, "D %d T %d: the phases hold %d taps", D, T, taps);
                CHECK((g.tileOut - 1) * D + T <= nElem, "D %d T %d: the staged tile ends before its last output's last tap", D, T);
            }
    return 0;
}

// needed range against the definition, and the phase word's additivity the kernel rests on
static int check_ranges()
{
    for (int D : {1, 4, 64})
        for (int T : {1, 33, 1023})
            for (int64_t first : {INT64_C(0), INT64_C(1), INT64_C(999), (INT64_C(1) << 33) + 5, INT64_C(1) << 55})
                for (int64_t count : {INT64_C(1), INT64_C(7), INT64_C(1) << 30})
                    for (int64_t len : {INT64_C(-1), INT64_C(0), INT64_C(100), first * D + 3, INT64_MAX / 2}) {
                        int64_t lo, hi;
                        fe_needed(first, count, D, T, len, lo, hi);
                        const int T0 = (T - 1) / 2;
                        int64_t a = first * D - T0, b = (first + count - 1) * D + T - T0;
                        if (a < 0) a = 0;
                        if (len >= 0 && b > len) b = len;
                        if (b < a) b = a;
                        CHECK(lo == a && hi == b && lo >= 0 && hi >= lo, "needed range of %" PRId64 " + %" PRId64 " D %d T %d", first, count, D, T);
                    }
    for (uint32_t delta : {0u, 1u, 0x40000000u, 0xC0000000u, 0x1F9ADD37u, 0xFFFFFFFFu})
        for (int64_t n : {INT64_C(-511), INT64_C(-1), INT64_C(0), INT64_C(12345), (INT64_C(1) << 33) + 1, (INT64_C(1) << 61) + 3})
            for (int t : {0, 1, 511, 1022})
                CHECK(fe_phase(n + t, delta) == (uint32_t)(fe_phase(n, delta) + fe_phase(t, delta)), "phase word not additive at n %" PRId64 " t %d", n, t);
    double c, s;
    fe_cos_sin(0, c, s);
    CHECK(c == 1.0 && s == 0.0, "cos, sin of word 0");
    fe_cos_sin(0x40000000u, c, s);
    CHECK(c == 0.0 && s == 1.0, "cos, sin of a quarter turn");
    fe_cos_sin(0x80000000u, c, s);
    CHECK(c == -1.0 && s == 0.0, "cos, sin of a half turn");
    fe_cos_sin(0xC0000000u, c, s);
    CHECK(c == 0.0 && s == -1.0, "cos, sin of three quarter turns");
    return 0;
}

static dpe_fe_config config(int fmt, int out, int D, int T, double fs, double fIF)
{
    dpe_fe_config c{};
    c.samplingFrequency = fs;
    c.intermediateFrequency = fIF;
    c.gain = 1.0;
    c.levels[0] = -3; c.levels[1] = -1; c.levels[2] = 1; c.levels[3] = 3;
    c.format = fmt;
    c.outputFormat = out;
    c.decimation = D;
    c.nTaps = T;
    return c;
}

int main(int argc, char **argv)
{
    if (check_geometry() || check_ranges()) return 1;
    if (argc < 2) return 0;
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "test_fe_plan: cannot open %s\n", argv[1]); return 2; }
    char line[512], w[11][64], msg[320];
    static double ones[kFeMaxT + 2];
    for (double &v : ones) v = 1.0;
    while (fgets(line, sizeof(line), f)) {
        const int n = sscanf(line, "%63s %63s %63s %63s %63s %63s %63s %63s %63s %63s %63s", w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9], w[10]);
        if (n < 1) continue;
        auto D = [&](int i) { return strtod(w[i], nullptr); };
        auto I = [&](int i) { return strtoll(w[i], nullptr, 10); };
        if (!strcmp(w[0], "delta") && n == 3) {
            const uint32_t d = fe_delta(D(1), D(2));
            printf("%u %a\n", d, fe_realised_if(d, D(2)));
        } else if (!strcmp(w[0], "phase") && n == 3) {
            printf("%u\n", fe_phase(I(1), (uint32_t)strtoull(w[2], nullptr, 10)));
        } else if (!strcmp(w[0], "needed") && n == 6) {
            int64_t lo, hi;
            fe_needed(I(1), I(2), (int)I(3), (int)I(4), I(5), lo, hi);
            printf("%" PRId64 " %" PRId64 "\n", lo, hi);
        } else if (!strcmp(w[0], "geom") && n == 4) {
            const FeGeom g = fe_geom((int)I(1), (int)I(2), I(3) != 0);
            printf("%d %d %d %d %d %d\n", g.tileOut, g.rowLen, g.pitch, g.ldsBytes, g.Q, g.rem);
        } else if (!strcmp(w[0], "owner") && n == 5) {
            const FeGeom g = fe_geom((int)I(1), (int)I(2), I(3) != 0);
            int64_t b;
            int lane, slot;
            fe_owner(g, I(4), b, lane, slot);
            printf("%" PRId64 " %d %d\n", b, lane, slot);
        } else if (!strcmp(w[0], "tap") && n == 6) {
            const FeGeom g = fe_geom((int)I(1), (int)I(2), I(3) != 0);
            const std::vector<float> tab = fe_taps(g, kFeComplexMix, (uint32_t)strtoull(w[4], nullptr, 10), 1.0, ones);
            const int t = (int)I(5);
            const float *e = tab.data() + ((size_t)(t % g.D) * g.qPitch + t / g.D) * 4;
            printf("%a %a %a %a\n", e[0], e[1], e[2], e[3]);
        } else if (!strcmp(w[0], "taps") && n == 4) {
            static double ramp[kFeMaxT + 2];
            for (int t = 0; t < kFeMaxT + 2; ++t) ramp[t] = t + 1.0;
            const int mode = (int)I(3);
            const FeGeom g = fe_geom((int)I(1), (int)I(2), mode == kFeRealIn);
            const std::vector<float> tab = fe_taps(g, (FeMode)mode, 0u, 1.0, ramp);
            for (size_t i = 0; i < tab.size(); ++i) printf("%s%a", i ? " " : "", tab[i]);
            printf("\n");
        } else if (!strcmp(w[0], "cfg") && n == 7) {
            const dpe_fe_config c = config((int)I(1), (int)I(2), (int)I(3), (int)I(4), D(5), D(6));
            printf("%s\n", fe_config_problem(&c, ones, msg, sizeof(msg)) ? msg : "ok");
        } else if (!strcmp(w[0], "conv") && n == 11) {
            const dpe_fe_config c = config((int)I(1), 0, (int)I(2), (int)I(3), 1.0e7, 0.0);
            printf("%s\n", fe_convert_problem(c, false, false, (unsigned)I(9), (unsigned)I(10), I(4), I(5), I(6), I(7), I(8), msg, sizeof(msg)) ? msg : "ok");
        } else if (!strcmp(w[0], "quant") && n == 3) {
            unsigned clipped = 0;
            const int word = stream_quantise((float)D(1), (float)D(2), clipped);
            printf("%u %u\n", (unsigned)word, clipped);
        } else {
            fprintf(stderr, "test_fe_plan: bad line: %s", line);
            fclose(f);
            return 2;
        }
    }
    fclose(f);
    return 0;
}
