// test_arr_plan.cpp -- csrc/dpe_arr_plan.h with a plain C++ compiler, no GPU: the launch plan's properties are checked here (exit 1
// with a message on the first that fails), and the mappings are evaluated for the cases of a text file, one answer per line, for
// tests/test_arr_plan_cpu.py to hold against Python integers.  Doubles travel as C99 hex floats.
//
//   test_arr_plan cases.txt
//     needed outFirst outCount L len          -> lo hi
//     blocks blockFirst blockCount L len      -> lo hi
//     launch outFirst outCount L len          -> k0 k1 units countedBlocks
//     owner n outFirst L                      -> unit ka kb (the owner of output n and its blocks, in a call that ends at n)
//     samples k L len                         -> the samples of block k inside the record
//     lds M L                                 -> cov part applied fallback counts bytes
//     apply M v.. x..                         -> re im of arr_apply (M pairs of v, M pairs of x, hex floats)
//     cfg M L B lambda gain out ref cons      -> the refusal of dpe_arr_create's checks, or "ok" (cons: none, ok, zero, nan)
//     proc M L B out xFirst xCount len outFirst outCount xAddr0 xStride outAddr0 outStride -> dpe_arr_process's checks (address 0: NULL)
//     ana M L xFirst xCount len blockFirst blockCount -> the refusal of dpe_arr_analyse's checks, or "ok"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <vector>

#include "../csrc/dpe_arr_plan.h"

using namespace dpe;

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            fprintf(stderr, "test_arr_plan: " __VA_ARGS__); \
            fprintf(stderr, "  (%s)\n", #cond);            \
            return 1;                                      \
        }                                                  \
    } while (0)

// Every output of a call has exactly one owner, whose blocks hold it; what the owner's blocks read lies inside the call's needed
// range; the blocks counted over the units are the multiples of L among the outputs inside the record, and add over splits.
static int check_ownership()
{
    for (int L : {256, 1024, 4096, 65536}) {
        const int ub = arr_unit_blocks(L);
        CHECK(ub >= 1 && ub <= kArrMaxUnitBlocks && (L >= kArrUnitSamples ? ub == 1 : ub * L == kArrUnitSamples), "L %d: %d blocks per unit", L, ub);
        for (int64_t first : {INT64_C(0), INT64_C(1), (int64_t)L - 1, (int64_t)L, 3 * (int64_t)L + 5, INT64_C(1000003), (INT64_C(1) << 55) - 40 * (int64_t)L - 7})
            for (int64_t count : {INT64_C(1), INT64_C(2), (int64_t)L, (int64_t)L + 1, 16 * (int64_t)L, 16 * (int64_t)L + 1, 17 * (int64_t)L + 9, 40 * (int64_t)L + 7})
                for (int64_t len : {INT64_C(-1), first + count / 2, first + count + 5 * L}) {
                    const ArrLaunch l = arr_launch(first, count, L);
                    int64_t lo, hi;
                    arr_needed(first, count, L, -1, lo, hi);
                    CHECK(l.units >= 1 && l.k0 == first / L && l.k1 == (first + count - 1) / L, "L %d: blocks of %" PRId64 " + %" PRId64, L, first, count);
                    int64_t next = l.k0, counted = 0;
                    for (int64_t u = 0; u < l.units; ++u) {
                        int64_t ka, kb;
                        arr_unit_range(l.k0, l.k1, u, L, ka, kb);
                        CHECK(ka == next && kb >= ka && kb - ka < ub && kb <= l.k1, "L %d: unit %" PRId64 " owns %" PRId64 "..%" PRId64, L, u, ka, kb);
                        next = kb + 1;
                        CHECK(ka * L >= lo && (kb + 1) * L <= hi, "L %d: unit %" PRId64 " reads outside the needed range", L, u);
                        for (int64_t k = ka; k <= kb; ++k) counted += arr_counted(k, L, first, count, len);
                    }
                    CHECK(next == l.k1 + 1, "L %d: the units end at block %" PRId64 ", the call at %" PRId64, L, next - 1, l.k1);
                    CHECK(counted == arr_counted_blocks(first, count, L, len), "L %d: %" PRId64 " blocks counted over the units", L, counted);
                    for (int64_t n : {first, first + count / 2, first + count - 1}) {
                        const int64_t u = arr_owner(n, l.k0, L);
                        int64_t ka, kb;
                        arr_unit_range(l.k0, l.k1, u, L, ka, kb);
                        CHECK(u >= 0 && u < l.units && n / L >= ka && n / L <= kb, "L %d: owner of output %" PRId64, L, n);
                    }
                    for (int64_t cut : {INT64_C(1), count / 3, count / 2, count - 1}) {
                        if (cut < 1 || cut >= count) continue;
                        CHECK(arr_counted_blocks(first, cut, L, len) + arr_counted_blocks(first + cut, count - cut, L, len) == arr_counted_blocks(first, count, L, len),
                              "L %d: counted blocks of %" PRId64 " + %" PRId64 " cut at %" PRId64, L, first, count, cut);
                    }
                }
    }
    return 0;
}

// The LDS regions follow one another without overlap, aligned to their elements, and two workgroups fit a CU; the packed
// covariance gives every entry of the Hermitian matrix back; the padded size is the power of two the wave's fold needs.
static int check_lds_and_packing()
{
    for (int M = kArrMinM; M <= kArrMaxM; ++M) {
        const int vp = arr_padded(M);
        CHECK(vp >= M * M && vp <= 64 && (vp & (vp - 1)) == 0 && (vp == 4 || vp / 2 < M * M), "M %d: padded to %d", M, vp);
        for (int L = kArrMinL; L <= kArrMaxL; L *= 2) {
            const ArrLds l = arr_lds(M, L);
            const int ub = arr_unit_blocks(L);
            CHECK(l.cov == 0 && l.part - l.cov == 8 * ub * M * M && l.applied - l.part == 16 * kArrWaves * vp && l.fallback - l.applied == 8 * ub * kArrMaxB * M &&
                      l.counts - l.fallback == 4 * ub && l.bytes - l.counts == 16, "M %d L %d: regions", M, L);
            CHECK(l.part % 8 == 0 && l.applied % 8 == 0 && l.fallback % 4 == 0 && l.counts % 4 == 0, "M %d L %d: alignment", M, L);
            CHECK(2 * l.bytes <= 160 * 1024 && l.bytes <= 64 * 1024, "M %d L %d: %d bytes of LDS", M, L, l.bytes);
            CHECK(ub * kArrMaxB <= 64, "L %d: the solve's lanes do not fit one wave", L);
        }
        std::vector<int64_t> p((size_t)(M * M));
        for (int i = 0; i < M * M; ++i) p[(size_t)i] = 1000 + i;
        for (int a = 0; a < M; ++a)
            for (int b = 0; b < M; ++b) {
                int64_t re, im, re2, im2;
                arr_cov_entry(p.data(), M, a, b, re, im);
                arr_cov_entry(p.data(), M, b, a, re2, im2);
                CHECK(re == re2 && im == -im2 && (a != b || im == 0), "M %d: entry %d %d is not the conjugate of %d %d", M, a, b, b, a);
                CHECK(re == p[(size_t)((a > b ? a : b) * M + (a > b ? b : a))], "M %d: real part of entry %d %d", M, a, b);
            }
    }
    return 0;
}

static dpe_arr_config config(int M, int L, int B, double lambda, double gain, int out, int ref)
{
    dpe_arr_config c{};
    c.loading = lambda;
    c.gain = gain;
    c.nElements = M;
    c.blockLength = L;
    c.nConstraints = B;
    c.reference = ref;
    c.outputFormat = out;
    return c;
}

int main(int argc, char **argv)
{
    if (check_ownership() || check_lds_and_packing()) return 1;
    if (argc < 2) return 0;
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "test_arr_plan: cannot open %s\n", argv[1]); return 2; }
    char line[2048], w[40][48], msg[320];
    while (fgets(line, sizeof(line), f)) {
        int n = 0, used = 0, pos = 0;
        while (n < 40 && sscanf(line + pos, "%47s%n", w[n], &used) == 1) { pos += used; ++n; }
        if (n < 1) continue;
        auto D = [&](int i) { return strtod(w[i], nullptr); };
        auto I = [&](int i) { return strtoll(w[i], nullptr, 10); };
        int64_t lo, hi;
        if (!strcmp(w[0], "needed") && n == 5) {
            arr_needed(I(1), I(2), (int)I(3), I(4), lo, hi);
            printf("%" PRId64 " %" PRId64 "\n", lo, hi);
        } else if (!strcmp(w[0], "blocks") && n == 5) {
            arr_needed_blocks(I(1), I(2), (int)I(3), I(4), lo, hi);
            printf("%" PRId64 " %" PRId64 "\n", lo, hi);
        } else if (!strcmp(w[0], "launch") && n == 5) {
            const ArrLaunch l = arr_launch(I(1), I(2), (int)I(3));
            printf("%" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", l.k0, l.k1, l.units, arr_counted_blocks(I(1), I(2), (int)I(3), I(4)));
        } else if (!strcmp(w[0], "owner") && n == 4) {
            const ArrLaunch l = arr_launch(I(2), I(1) - I(2) + 1, (int)I(3));
            const int64_t u = arr_owner(I(1), l.k0, (int)I(3));
            int64_t ka, kb;
            arr_unit_range(l.k0, l.k1, u, (int)I(3), ka, kb);
            printf("%" PRId64 " %" PRId64 " %" PRId64 "\n", u, ka, kb);
        } else if (!strcmp(w[0], "samples") && n == 4) {
            printf("%" PRId64 "\n", arr_block_samples(I(1), (int)I(2), I(3)));
        } else if (!strcmp(w[0], "lds") && n == 3) {
            const ArrLds l = arr_lds((int)I(1), (int)I(2));
            printf("%d %d %d %d %d %d\n", l.cov, l.part, l.applied, l.fallback, l.counts, l.bytes);
        } else if (!strcmp(w[0], "apply") && n >= 2 && n == 2 + 4 * (int)I(1)) {
            const int M = (int)I(1);
            float vr[kArrMaxM], vi[kArrMaxM], xi[kArrMaxM], xq[kArrMaxM], re, im;
            for (int a = 0; a < M; ++a) {
                vr[a] = (float)D(2 + 2 * a);
                vi[a] = (float)D(3 + 2 * a);
                xi[a] = (float)D(2 + 2 * M + 2 * a);
                xq[a] = (float)D(3 + 2 * M + 2 * a);
            }
            arr_apply(M, vr, vi, xi, xq, re, im);
            printf("%a %a\n", re, im);
        } else if (!strcmp(w[0], "cfg") && n == 9) {
            const dpe_arr_config c = config((int)I(1), (int)I(2), (int)I(3), D(4), D(5), (int)I(6), (int)I(7));
            std::vector<double> cons((size_t)(2 * kArrMaxM * kArrMaxB), 1.0);
            if (!strcmp(w[8], "zero")) for (int i = 0; i < 2 * c.nElements; ++i) cons[(size_t)(2 * c.nElements * (c.nConstraints - 1) + i)] = 0.0;
            if (!strcmp(w[8], "nan")) cons[3] = std::numeric_limits<double>::quiet_NaN();
            printf("%s\n", arr_config_problem(&c, strcmp(w[8], "none") ? cons.data() : nullptr, msg, sizeof(msg)) ? msg : "ok");
        } else if (!strcmp(w[0], "proc") && n == 14) {
            const dpe_arr_config c = config((int)I(1), (int)I(2), (int)I(3), 1e-3, 1.0, (int)I(4), 0);
            uint64_t xa[kArrMaxM], oa[kArrMaxB];
            for (int a = 0; a < kArrMaxM; ++a) xa[a] = (uint64_t)I(10) + (uint64_t)a * (uint64_t)I(11);
            for (int b = 0; b < kArrMaxB; ++b) oa[b] = (uint64_t)I(12) + (uint64_t)b * (uint64_t)I(13);
            if (I(11) < 0) xa[c.nElements - 1] = 0;       // a negative stride: the last element's pointer is NULL
            printf("%s\n", arr_process_problem(c, xa, oa, I(5), I(6), I(7), I(8), I(9), msg, sizeof(msg)) ? msg : "ok");
        } else if (!strcmp(w[0], "ana") && n == 8) {
            const dpe_arr_config c = config((int)I(1), (int)I(2), 1, 1e-3, 1.0, 0, 0);
            uint64_t xa[kArrMaxM];
            for (int a = 0; a < kArrMaxM; ++a) xa[a] = 4096u * (uint64_t)(a + 1);
            printf("%s\n", arr_analyse_problem(c, xa, I(3), I(4), I(5), I(6), I(7), 0u, 0u, 0u, msg, sizeof(msg)) ? msg : "ok");
        } else {
            fprintf(stderr, "test_arr_plan: bad line: %s", line);
            fclose(f);
            return 2;
        }
    }
    fclose(f);
    return 0;
}
