// test_ix_plan.cpp -- csrc/dpe_ix_plan.h with a plain C++ compiler, no GPU: the launch plan's properties are checked here (exit 1
// with a message on the first that fails), and the mappings are evaluated for the cases of a text file, one answer per line, for
// tests/test_ix_plan_cpu.py to hold against Python integers.  Doubles travel as C99 hex floats.
//
//   test_ix_plan cases.txt
//     needed outFirst outCount N len          -> lo hi
//     frames frameFirst frameCount N len      -> lo hi
//     launch outFirst outCount N              -> h0 h1 blocks countedFrames
//     owner n outFirst N                      -> block ha hb (the owner of output n and its hops, in a call that ends at n)
//     lds N                                   -> frame perBin detected hist select counts bytes
//     tables N m i                            -> tw[m] (two hex floats) and w[i]
//     blank power                             -> the blanker's 32-bit word
//     cfg N kappa guard blank gain in out     -> the refusal of dpe_ix_create's checks, or "ok"
//     proc N in out xFirst xCount len outFirst outCount xAlign outAlign -> the refusal of dpe_ix_process's checks, or "ok"
//     ana N xFirst xCount len frameFirst frameCount -> the refusal of dpe_ix_analyse's checks, or "ok"
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../csrc/dpe_ix_plan.h"

using namespace dpe;

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            fprintf(stderr, "test_ix_plan: " __VA_ARGS__); \
            fprintf(stderr, "  (%s)\n", #cond);           \
            return 1;                                     \
        }                                                 \
    } while (0)

// Every output of a call has exactly one owner, whose frames are the two the output is made of; what the owner's frames read lies
// inside the call's needed range; the frames counted over the blocks are the multiples of H among the outputs.
static int check_ownership()
{
    for (int N : {64, 128, 1024, 4096}) {
        const int64_t H = N / 2;
        for (int64_t first : {INT64_C(0), INT64_C(1), H - 1, H, 3 * H + 5, INT64_C(1000003), (INT64_C(1) << 55) - 40 * H - 7})
            for (int64_t count : {INT64_C(1), INT64_C(2), H, H + 1, 16 * H, 16 * H + 1, 17 * H + 9, 40 * H + 7}) {
                const IxLaunch l = ix_launch(first, count, N);
                int64_t lo, hi;
                ix_needed(first, count, N, -1, lo, hi);
                CHECK(l.blocks >= 1 && l.h0 == first / H && l.h1 == (first + count - 1) / H, "N %d: hops of %" PRId64 " + %" PRId64, N, first, count);
                int64_t nextHop = l.h0, counted = 0;
                for (int64_t b = 0; b < l.blocks; ++b) {
                    int64_t ha, hb;
                    ix_block_hops(l.h0, l.h1, b, ha, hb);
                    CHECK(ha == nextHop && hb >= ha && hb - ha < kIxHopsPerBlock && hb <= l.h1, "N %d: block %" PRId64 " owns %" PRId64 "..%" PRId64, N, b, ha, hb);
                    nextHop = hb + 1;
                    // its frames ha .. hb + 1 read the samples (ha - 1) H .. (hb + 2) H - 1; below 0 they are zeros
                    CHECK((ha - 1) * H >= lo || (ha - 1) * H < 0, "N %d: block %" PRId64 " reads before the needed range", N, b);
                    CHECK((hb + 2) * H <= hi, "N %d: block %" PRId64 " reads beyond the needed range", N, b);
                    for (int64_t k = ha; k <= hb; ++k) counted += ix_counted(k, H, first, count);
                }
                CHECK(nextHop == l.h1 + 1, "N %d: the blocks end at hop %" PRId64 ", the call at %" PRId64, N, nextHop - 1, l.h1);
                CHECK(counted == ix_counted_frames(first, count, N), "N %d: %" PRId64 " frames counted over the blocks", N, counted);
                for (int64_t n : {first, first + count / 2, first + count - 1}) {
                    const int64_t b = ix_owner(n, l.h0, N);
                    int64_t ha, hb;
                    ix_block_hops(l.h0, l.h1, b, ha, hb);
                    CHECK(b >= 0 && b < l.blocks && n / H >= ha && n / H <= hb, "N %d: owner of output %" PRId64, N, n);
                }
                // counted frames over a split sum to those of one call
                for (int64_t cut : {INT64_C(1), count / 3, count / 2, count - 1}) {
                    if (cut < 1 || cut >= count) continue;
                    CHECK(ix_counted_frames(first, cut, N) + ix_counted_frames(first + cut, count - cut, N) == ix_counted_frames(first, count, N),
                          "N %d: counted frames of %" PRId64 " + %" PRId64 " cut at %" PRId64, N, first, count, cut);
                }
            }
    }
    return 0;
}

// The LDS regions follow one another without overlap, aligned to their elements; every pass of the transform touches each element
// of the frame exactly once, inside the frame, with twiddle indices below N / 2; the bit reversal is a permutation of the bins.
static int check_lds_and_transform()
{
    for (int N : {64, 128, 256, 512, 1024, 2048, 4096}) {
        const IxLds l = ix_lds(N);
        CHECK(l.frame == 0 && l.perBin == 8 * N && l.detected - l.perBin == 4 * N && l.hist - l.detected == N && l.select - l.hist == 1024 &&
                  l.counts - l.select == 8 && l.bytes - l.counts == 16, "N %d: regions", N);
        CHECK(l.perBin % 8 == 0 && l.hist % 4 == 0 && l.select % 4 == 0 && l.counts % 4 == 0, "N %d: alignment", N);
        CHECK(2 * l.bytes <= 160 * 1024 && l.bytes <= 64 * 1024, "N %d: %d bytes of LDS", N, l.bytes);
        CHECK(N / 2 <= kIxCarry * kIxThreads, "N %d: the carried half does not fit the lanes' registers", N);
        const int logN = ix_log2(N);
        CHECK((1 << logN) == N, "N %d: log2", N);
        std::vector<int> seen((size_t)N);
        int stages = 0;
        for (int hf = N >> 1;; hf >>= 2) {                      // the forward passes; the backward ones use the same indices
            if (hf >= 2) {
                const int q = hf >> 1, mA = N / (2 * hf), mB = N / hf;
                std::fill(seen.begin(), seen.end(), 0);
                for (int u = 0; u < N / 4; ++u) {
                    int base, j;
                    ix_pair_index(u, q, base, j);
                    CHECK(base >= 0 && base + 3 * q < N && j >= 0 && j < q, "N %d q %d: element %d", N, q, u);
                    CHECK((j + q) * mA < N / 2 && j * mB < N / 2, "N %d q %d: twiddle of element %d", N, q, u);
                    for (int e = 0; e < 4; ++e) ++seen[(size_t)(base + e * q)];
                }
                for (int i = 0; i < N; ++i) CHECK(seen[(size_t)i] == 1, "N %d q %d: index %d touched %d times", N, q, i, seen[(size_t)i]);
                stages += 2;
                continue;
            }
            if (hf == 1) {
                std::fill(seen.begin(), seen.end(), 0);
                for (int t = 0; t < N / 2; ++t) {
                    int i0, j;
                    ix_single_index(t, 1, i0, j);
                    CHECK(i0 >= 0 && i0 + 1 < N && j == 0, "N %d: single stage element %d", N, t);
                    ++seen[(size_t)i0];
                    ++seen[(size_t)i0 + 1];
                }
                for (int i = 0; i < N; ++i) CHECK(seen[(size_t)i] == 1, "N %d: single stage index %d", N, i);
                stages += 1;
            }
            break;
        }
        CHECK(stages == logN, "N %d: %d stages", N, stages);
        std::fill(seen.begin(), seen.end(), 0);
        for (int p = 0; p < N; ++p) {
            const int f = ix_bitrev(p, logN);
            CHECK(f >= 0 && f < N && ix_bitrev(f, logN) == p, "N %d: bit reversal of %d", N, p);
            ++seen[(size_t)f];
        }
        for (int i = 0; i < N; ++i) CHECK(seen[(size_t)i] == 1, "N %d: bin %d", N, i);
        const std::vector<float> tw = ix_twiddles(N), w = ix_window(N);
        CHECK(tw[0] == 1.f && tw[1] == 0.f && tw[2 * (size_t)(N / 4)] == 0.f && tw[2 * (size_t)(N / 4) + 1] == -1.f, "N %d: twiddles on the axes", N);
        CHECK(tw[2 * (size_t)(N / 8)] == -tw[2 * (size_t)(N / 8) + 1], "N %d: the eighth turn", N);
        for (int i = 0; i < N / 2; ++i) {
            const double s = (double)w[(size_t)i] * w[(size_t)i] + (double)w[(size_t)(i + N / 2)] * w[(size_t)(i + N / 2)];
            CHECK(std::fabs(s - 1.0) < 3e-7 && w[(size_t)i] == w[(size_t)(N - 1 - i)], "N %d: window at %d", N, i);
        }
    }
    return 0;
}

static dpe_ix_config config(int N, double kappa, int guard, double blank, double gain, int in, int out)
{
    dpe_ix_config c{};
    c.threshold = kappa;
    c.blankPower = blank;
    c.gain = gain;
    c.frameLength = N;
    c.guard = guard;
    c.inputFormat = in;
    c.outputFormat = out;
    return c;
}

int main(int argc, char **argv)
{
    if (check_ownership() || check_lds_and_transform()) return 1;
    if (argc < 2) return 0;
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "test_ix_plan: cannot open %s\n", argv[1]); return 2; }
    char line[512], w[11][64], msg[320];
    while (fgets(line, sizeof(line), f)) {
        const int n = sscanf(line, "%63s %63s %63s %63s %63s %63s %63s %63s %63s %63s %63s", w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9], w[10]);
        if (n < 1) continue;
        auto D = [&](int i) { return strtod(w[i], nullptr); };
        auto I = [&](int i) { return strtoll(w[i], nullptr, 10); };
        int64_t lo, hi;
        if (!strcmp(w[0], "needed") && n == 5) {
            ix_needed(I(1), I(2), (int)I(3), I(4), lo, hi);
            printf("%" PRId64 " %" PRId64 "\n", lo, hi);
        } else if (!strcmp(w[0], "frames") && n == 5) {
            ix_needed_frames(I(1), I(2), (int)I(3), I(4), lo, hi);
            printf("%" PRId64 " %" PRId64 "\n", lo, hi);
        } else if (!strcmp(w[0], "launch") && n == 4) {
            const IxLaunch l = ix_launch(I(1), I(2), (int)I(3));
            printf("%" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", l.h0, l.h1, l.blocks, ix_counted_frames(I(1), I(2), (int)I(3)));
        } else if (!strcmp(w[0], "owner") && n == 4) {
            const IxLaunch l = ix_launch(I(2), I(1) - I(2) + 1, (int)I(3));
            const int64_t b = ix_owner(I(1), l.h0, (int)I(3));
            int64_t ha, hb;
            ix_block_hops(l.h0, l.h1, b, ha, hb);
            printf("%" PRId64 " %" PRId64 " %" PRId64 "\n", b, ha, hb);
        } else if (!strcmp(w[0], "lds") && n == 2) {
            const IxLds l = ix_lds((int)I(1));
            printf("%d %d %d %d %d %d %d\n", l.frame, l.perBin, l.detected, l.hist, l.select, l.counts, l.bytes);
        } else if (!strcmp(w[0], "tables") && n == 4) {
            const std::vector<float> tw = ix_twiddles((int)I(1)), win = ix_window((int)I(1));
            printf("%a %a %a\n", tw[2 * (size_t)I(2)], tw[2 * (size_t)I(2) + 1], win[(size_t)I(3)]);
        } else if (!strcmp(w[0], "blank") && n == 2) {
            printf("%u\n", ix_blank_word(D(1)));
        } else if (!strcmp(w[0], "cfg") && n == 8) {
            const dpe_ix_config c = config((int)I(1), D(2), (int)I(3), D(4), D(5), (int)I(6), (int)I(7));
            printf("%s\n", ix_config_problem(&c, msg, sizeof(msg)) ? msg : "ok");
        } else if (!strcmp(w[0], "proc") && n == 11) {
            const dpe_ix_config c = config((int)I(1), 10.0, 1, 0.0, 1.0, (int)I(2), (int)I(3));
            printf("%s\n", ix_process_problem(c, false, false, (unsigned)I(9), (unsigned)I(10), I(4), I(5), I(6), I(7), I(8), msg, sizeof(msg)) ? msg : "ok");
        } else if (!strcmp(w[0], "ana") && n == 7) {
            const dpe_ix_config c = config((int)I(1), 10.0, 1, 0.0, 1.0, 0, 0);
            printf("%s\n", ix_analyse_problem(c, false, 0u, I(2), I(3), I(4), I(5), I(6), 0u, 0u, msg, sizeof(msg)) ? msg : "ok");
        } else {
            fprintf(stderr, "test_ix_plan: bad line: %s", line);
            fclose(f);
            return 2;
        }
    }
    fclose(f);
    return 0;
}
