// test_acq_plan.cpp -- the acquisition search's plan (csrc/dpe_acq_plan.h) with a plain C++ compiler and no GPU: reads a table of rows
// (tests/golden/acq_plan_parent.json: per row the configuration, the switches, the device's answers, and the shape and launch list as
// the library chose them before the plan became a header), prints this build's shape and launches per row as one JSON object per line;
// tests/test_acq_plan_cpu.py compares them field by field.
//   g++ -std=c++17 -ffp-contract=off test_acq_plan.cpp -o test_acq_plan && ./test_acq_plan table.json
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../csrc/dpe_acq_plan.h"

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
        const Json &in = row.at("in"), &jsw = in.at("sw"), &jdev = in.at("dev");
        dpe_acq_config cfg{};
        cfg.samplesPerWindow = in.i("S"); cfg.nCodePeriods = in.i("N"); cfg.nBins = in.i("B"); cfg.nPrn = in.i("P");
        cfg.mode = in.i("mode"); cfg.prnChunk = in.i("prnChunk"); cfg.samplingFrequency = in.d("fs");
        AcqSwitches sw;
        sw.noFused = jsw.b("noFused"); sw.noPack = jsw.b("noPack"); sw.noFwdPack = jsw.b("noFwdPack");
        sw.noFusedFwd = jsw.b("noFusedFwd"); sw.statsLds = jsw.b("statsLds");
        AcqDevice dev;
        dev.cus = jdev.i("cus"); dev.packLds = jdev.b("packLds"); dev.mixedLds = jdev.b("mixedLds");
        const AcqShape s = acq_shape(cfg, sw, dev);
        std::printf("{\"name\":\"%s\",\"createOk\":%d,\"launches\":[", row.at("name").str.c_str(), (int)acq_create_ok(s, dev));
        int n = 0;
        acq_for_each_launch(s, [&](const AcqLaunch &l) {
            std::printf("%s{\"kernel\":\"%s\",\"gx\":%u,\"gy\":%u,\"gz\":%u,\"block\":%u,\"lds\":%zu,\"bpb\":%d,\"nSeg\":%d,\"p0\":%d,\"pc\":%d,\"order\":%d,\"coherent\":%d}",
                        n++ ? "," : "", acq_kernel_name(l.kernel), l.gx, l.gy, l.gz, l.block, l.lds, l.bpb, l.nSeg, l.p0, l.pc, l.order, l.coherent);
            return true;
        });
        std::printf("],\"shape\":{\"S\":%d,\"N\":%d,\"M\":%d,\"B\":%d,\"P\":%d,\"len\":%d,\"SX\":%d,\"chunk\":%d,\"corr\":\"%s\",\"fwd\":\"%s\","
                    "\"nX\":%zu,\"nRc\":%zu,\"nY\":%zu,\"nSurf\":%zu,\"nMp\":%zu,\"nRcq\":%zu,\"nTw\":%zu,\"nTw25k\":%zu,\"nTw2\":%zu,"
                    "\"fwdLen\":%d,\"fwdBatch\":%d,\"invLen\":%d,\"invBatch\":%d,\"mixedOptIn\":%d,\"cus\":%d,"
                    "\"iLo\":%d,\"iHi\":%d,\"maskS\":%d,\"rowInLds\":%d,\"fLo\":%.17g,\"fHi\":%.17g,\"statsSmall\":%d}}\n",
                    s.S, s.N, s.M, s.B, s.P, s.len, s.SX, s.chunk, acq_corr_name(s.corr), acq_fwd_name(s.fwd), s.nX, s.nRc, s.nY, s.nSurf, s.nMp, s.nRcq, s.nTw,
                    s.nTw25k, s.nTw2, s.fwdLen, s.fwdBatch, s.invLen, s.invBatch, (int)s.mixedOptIn, s.cus, s.iLo, s.iHi, s.maskS, s.rowInLds, s.fLo, s.fHi,
                    (int)s.statsSmall);
    }
    return 0;
}
