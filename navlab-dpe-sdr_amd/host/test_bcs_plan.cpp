// test_bcs_plan.cpp -- stage 1's launch plan (csrc/dpe_bcs_plan.h) with a plain C++ compiler and no GPU: reads a table of rows
// (tests/golden/bcs_plan_parent.json: per row the inputs of bcs_shape / bcs_plan and the plan as the library chose it before the plan
// became a header), prints this build's shape and plan per row as one JSON object per line; tests/test_bcs_plan_cpu.py compares them
// field by field.  Also holds bcs_chan_facts to a few hand-made channel blocks (exit status 1 when one of them fails).
//   g++ -std=c++17 -ffp-contract=off test_bcs_plan.cpp -o test_bcs_plan && ./test_bcs_plan table.json
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../csrc/dpe_bcs_plan.h"

// ---- just enough JSON to read the table: objects, arrays, strings without escapes, numbers, true / false / null
struct Json {
    enum Kind { Null, Num, Str, Arr, Obj } kind = Null;
    double num = 0.0;
    std::string str;
    std::vector<Json> arr;
    std::map<std::string, Json> obj;
    const Json &at(const char *k) const
    {
        const auto it = obj.find(k);
        if (it == obj.end()) { std::fprintf(stderr, "table: key %s missing\n", k); std::exit(2); }
        return it->second;
    }
    int i(const char *k) const { return (int)at(k).num; }
    bool b(const char *k) const { return at(k).num != 0.0; }
    double d(const char *k) const { return at(k).num; }
};

struct Parser {
    const char *p;
    void ws() { while (*p == ' ' || *p == '\n' || *p == '\t' || *p == '\r') ++p; }
    [[noreturn]] void fail(const char *what) { std::fprintf(stderr, "table: %s at ...%.30s\n", what, p); std::exit(2); }
    std::string string()
    {
        if (*p != '"') fail("string expected");
        const char *e = std::strchr(++p, '"');
        if (!e) fail("unterminated string");
        std::string s(p, e);
        p = e + 1;
        return s;
    }
    Json value()
    {
        ws();
        Json j;
        if (*p == '{') {
            j.kind = Json::Obj;
            ++p; ws();
            while (*p != '}') {
                ws();
                const std::string k = string();
                ws();
                if (*p++ != ':') fail("':' expected");
                j.obj[k] = value();
                ws();
                if (*p == ',') ++p;
                else if (*p != '}') fail("',' or '}' expected");
            }
            ++p;
        } else if (*p == '[') {
            j.kind = Json::Arr;
            ++p; ws();
            while (*p != ']') {
                j.arr.push_back(value());
                ws();
                if (*p == ',') ++p;
                else if (*p != ']') fail("',' or ']' expected");
            }
            ++p;
        } else if (*p == '"') {
            j.kind = Json::Str;
            j.str = string();
        } else if (!std::strncmp(p, "true", 4)) { j.kind = Json::Num; j.num = 1.0; p += 4; }
        else if (!std::strncmp(p, "false", 5)) { j.kind = Json::Num; j.num = 0.0; p += 5; }
        else if (!std::strncmp(p, "null", 4)) { p += 4; }
        else {
            char *e = nullptr;
            j.kind = Json::Num;
            j.num = std::strtod(p, &e);   // (correctly rounded: the table's doubles are printed with 17 digits)
            if (e == p) fail("value expected");
            p = e;
        }
        return j;
    }
};

// ---- bcs_chan_facts on hand-made channel blocks: the seven fields it reads, nothing of dpe_prep.h
struct Chan {
    double rc, codeStep, fc, fi, invStep;
    int idxNext, hasFlip;
};
static Chan nominal(double fs, double fc = dpe::kFCA)
{
    return {100.25, fc / fs, fc, 1500.0, fs / fc, 0, 0};
}
static int check_facts()
{
    using namespace dpe;
    int bad = 0;
    const auto expect = [&](const char *what, bool ok) { if (!ok) { std::fprintf(stderr, "bcs_chan_facts: %s\n", what); ++bad; } };
    const double fs = 25e6;
    Chan c[3] = {nominal(fs), nominal(fs, kFCA * (1.0 + 3e-6)), nominal(fs, kFCA * (1.0 - 3e-6))};
    BcsChanFacts f = bcs_chan_facts(c, 3, true);
    expect("nominal channels take both chip forms", f.chip && f.chip2 && f.l1 == 24 && f.stepMax == c[1].codeStep);
    f = bcs_chan_facts(c, 3, false);
    expect("chip2 switched off", f.chip && !f.chip2 && f.l1 == 0 && f.stepMax == 0.0);
    c[2].fi = 0.25 * c[2].fc / 6.283185307179586 * 1.0001;
    f = bcs_chan_facts(c, 3, true);
    expect("a carrier beyond the closed-form DC term's range", !f.chip && !f.chip2);
    c[2] = nominal(20e6);   // 19 samples per chip beside 24
    f = bcs_chan_facts(c, 3, true);
    expect("chips of different lengths", f.chip && !f.chip2 && f.l1 == 24);
    Chan lo = nominal(15e6), hi = nominal(26e6);   // 14 and 25 samples per chip
    expect("chips shorter than k2MinL1", bcs_chan_facts(&lo, 1, true).chip && !bcs_chan_facts(&lo, 1, true).chip2);
    expect("chips longer than k2MaxL1 + 1", bcs_chan_facts(&hi, 1, true).chip && !bcs_chan_facts(&hi, 1, true).chip2);
    // nav-bit boundary: on a chip boundary of the replica (sample idxNext starts a new chip) or inside a chip
    Chan b = nominal(fs);
    b.rc = 0.5; b.hasFlip = 1;
    b.idxNext = (int)(std::floor((40.0 - b.rc) * b.invStep) + 1);   // the first sample of chip 40
    expect("boundary on a chip boundary", bcs_chan_facts(&b, 1, true).chip2);
    b.idxNext += 5;
    expect("boundary inside a chip", bcs_chan_facts(&b, 1, true).chip && !bcs_chan_facts(&b, 1, true).chip2);
    b.hasFlip = 0;
    expect("no boundary in the window", bcs_chan_facts(&b, 1, true).chip2);
    return bad;
}

static void print_shape(const dpe::BcsShape &s)
{
    std::printf("\"shape\":{\"C\":%lld,\"nMom\":%d,\"fftMode\":%d,\"useTable\":%d,\"LH\":%d,\"nSub\":%d,\"tilesPerBlock\":%d,\"nBlk\":%d,\"nPassChip\":%d,"
                "\"chipTpbMax\":%d,\"chipOK\":%d,\"nBlkAlloc\":%d,\"resident16\":%d,\"chipResident\":%d,\"chip2Resident\":%d}",
                s.C, s.nMom, (int)s.fftMode, (int)s.useTable, s.LH, s.nSub, s.tilesPerBlock, s.nBlk, s.nPassChip, s.chipTpbMax, (int)s.chipOK, s.nBlkAlloc,
                s.resident16, s.chipResident, s.chip2Resident);
}

static void print_plan(const dpe::BcsPlan &p)
{
    if (p.form == dpe::BcsForm::Fft) {   // the FFT form takes the kernel name and the DC-sum blocks from the plan, nothing else
        std::printf("\"plan\":{\"kernel\":\"%s\",\"sumBlocks\":%d,\"sumSlotsUsed\":%d}", p.kernel, p.sumBlocks, p.sumSlotsUsed);
        return;
    }
    std::printf("\"plan\":{\"kernel\":\"%s\",\"chip\":%d,\"nTiles\":%d,\"tpb\":%d,\"nBlk\":%d,\"chipNMom\":%d,\"c2Lt\":%d,\"c2nBlk\":%d,\"c2NMom\":%d,\"c2L1\":%d,"
                "\"fuse\":%d,\"coRide\":%d,\"inl\":%d,\"upInSum\":%d,\"useGraph\":%d,\"ride\":%d,\"rideF\":%d,\"rideSB\":%d,\"rideGS\":%d,\"sumBlocks\":%d,"
                "\"sumSlotsUsed\":%d,\"sumLaunch\":%d,\"chunkLags\":%d,\"nSideChunks\":%d,\"nBinBlk\":%d,\"fatFinalize\":%d,\"chunks\":[",
                p.kernel, (int)p.chip, p.nTiles, p.tpb, p.nBlk, p.chipNMom, p.c2Lt, p.c2nBlk, p.c2NMom, p.c2L1, (int)p.fuse, (int)p.coRide, (int)p.inl,
                (int)p.upInSum, (int)p.useGraph, (int)p.ride, p.rideF, p.rideSB, p.rideGS, p.sumBlocks, p.sumSlotsUsed, (int)p.sumLaunch, p.chunkLags,
                p.nSideChunks, p.nBinBlk, (int)p.fatFinalize);
    for (int i = 0; i < p.nChunks; ++i) {
        const dpe::BcsChunk &c = p.chunk[i];
        std::printf("%s{\"lagShift\":%d,\"c2\":%d,\"nMomUse\":%d,\"nBlkUse\":%d,\"momLenUse\":%d}", i ? "," : "", c.lagShift, (int)c.c2, c.nMomUse, c.nBlkUse,
                    c.momLenUse);
    }
    std::printf("]}");
}

int main(int argc, char **argv)
{
    using namespace dpe;
    if (argc != 2) { std::fprintf(stderr, "usage: %s table.json\n", argv[0]); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    std::string text;
    char buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, n);
    std::fclose(f);
    Parser ps{text.c_str()};
    const Json table = ps.value();
    for (const Json &row : table.arr) {
        const Json &in = row.at("in"), &sw = in.at("sw");
        dpe_bcs_config cfg{};
        cfg.samplesPerWindow = in.i("S"); cfg.lagHalfWidth = in.i("L"); cfg.binHalfWidth = in.i("B");
        cfg.maxWindows = in.i("maxWindows"); cfg.maxChannels = in.i("maxChannels");
        cfg.samplingFrequency = in.d("fs");
        BcsSwitches s;
        s.forceFft = sw.b("forceFft"); s.noWide = sw.b("noWide"); s.noBank16 = sw.b("noBank16"); s.noFuse = sw.b("noFuse");
        s.noChip = sw.b("noChip"); s.noChip2 = sw.b("noChip2"); s.noSumRide = sw.b("noSumRide");
        s.sumRideMin = sw.i("rideMinW"); s.rideLA = sw.i("rideLA");
        s.chip2P = sw.i("chip2P"); s.chipTpb = sw.i("chipTpb"); s.tpb16 = sw.i("tpb16"); s.fat = sw.i("fat");
        BcsShape shape = bcs_shape(cfg, s, in.i("cus"));
        if (shape.chipOK) bcs_shape_residency(shape, in.i("chipResident") / in.i("cus"), in.i("chip2Resident") / in.i("cus"));
        BcsChanFacts facts;
        facts.chip = in.b("factChip"); facts.chip2 = in.b("factChip2"); facts.l1 = in.i("factL1"); facts.stepMax = in.d("factStepMax");
        BcsCall call;
        call.dev = in.b("dev"); call.graphEnabled = in.b("graphEnabled"); call.capturing = in.b("capturing"); call.vecOK = in.b("vecOK");
        call.rerun = in.b("rerun"); call.coPending = in.b("coPending"); call.profiler = in.b("profiler");
        const BcsPlan plan = bcs_plan(shape, facts, in.i("nWindows"), in.i("nChan"), call);
        std::printf("{\"name\":\"%s\",", row.at("name").str.c_str());
        print_shape(shape);
        std::printf(",");
        print_plan(plan);
        std::printf("}\n");
    }
    return check_facts() ? 1 : 0;
}
