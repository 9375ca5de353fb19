// dpe_nav.hip -- scalar navigation for MI355X (gfx950): the stage that turns a tracked record into the handoff the DPE loop starts
// from, and the per-epoch scalar fix a DPE receiver is compared against.  Only the reference's Python twin has it:
//   parse_ephemerides                     libgnss/dataparser.py:10-70     preamble search, bits by majority, words, subframes
//   Word / Subframe / Ephemerides         libgnss/ephemeris.py:16-297     parity, HOW, subframes 1-3 -> ephemeris fields, timestamp
//   calculate_nav_soln                    scalar/naveng.py:10-88          transmit times, satellite states, pseudoranges, ECI
//   perform_least_sqrs                    scalar/naveng.py:132-224        <= 10 Gauss-Newton position steps, one velocity step
// The decode is host code on integers and fp64 (every scaling an integer times a power of two, then at most one product with pi, in
// the twin's order, so the doubles are the twin's).  The solution's arithmetic is dpe_nav_dev.h; dpe_nav_solve runs it on the host for
// one epoch, nav_solve_log_kernel for every logged epoch of a tracker in one launch: one 64-lane wave per epoch, lane k owns the k-th
// selected channel -- its log row, Kepler solves, clock correction and rotation to ECI, all fp64 -- and the 4-unknown least squares is
// a row-by-row Givens triangularisation that every lane runs on the rows in channel order (each row fetched from its lane), so the
// result is wave-uniform without a broadcast and depends on neither the launch shape nor on which lanes the channels occupy.
// No LDS, no barrier; every write to memory is a plain vector store from lane 0.
#include <algorithm>
#include <cstdlib>

#include "dpe_common.h"
#include "dpe_nav_dev.h"
#include "dpe_trk_log.h"

namespace dpe {

// ---------------------------------------------------------------------------------------------------------------- decode (host)
static const signed char kPreamble[8] = {-1, 1, 1, 1, -1, 1, -1, -1};                       // dataparser.py:7
static const unsigned char kParityMat[6][24] = {                                            // ephemeris.py:9-14
    {1, 1, 1, 0, 1, 1, 0, 0, 0, 1, 1, 1, 1, 1, 0, 0, 1, 1, 0, 1, 0, 0, 1, 0}, {0, 1, 1, 1, 0, 1, 1, 0, 0, 0, 1, 1, 1, 1, 1, 0, 0, 1, 1, 0, 1, 0, 0, 1},
    {1, 0, 1, 1, 1, 0, 1, 1, 0, 0, 0, 1, 1, 1, 1, 1, 0, 0, 1, 1, 0, 1, 0, 0}, {0, 1, 0, 1, 1, 1, 0, 1, 1, 0, 0, 0, 1, 1, 1, 1, 1, 0, 0, 1, 1, 0, 1, 0},
    {1, 0, 1, 0, 1, 1, 1, 0, 1, 1, 0, 0, 0, 1, 1, 1, 1, 1, 0, 0, 1, 1, 0, 1}, {0, 0, 1, 0, 1, 1, 0, 1, 1, 1, 1, 0, 1, 0, 1, 0, 0, 0, 1, 0, 0, 1, 1, 1}};
constexpr int kPreambleLen = 160, kPreambleThreshold = 153, kSubframeCp = 6000, kBitCp = 20;

static inline int sgn(int v) { return (v > 0) - (v < 0); }

// preamble_correlations[i] (np.correlate 'valid'): sum over the 160 entries from i
static inline int preamble_corr(const int8_t *s, int64_t i)
{
    int acc = 0;
    for (int b = 0; b < 8; ++b) {
        int t = 0;
        for (int j = 0; j < kBitCp; ++j) t += s[i + b * kBitCp + j];
        acc += kPreamble[b] * t;
    }
    return acc;
}
// sign of the sum of 20 entries: one navigation bit in the twin's +-1 form (0 on a tie)
static inline int nav_bit(const int8_t *s, int64_t i)
{
    int t = 0;
    for (int j = 0; j < kBitCp; ++j) t += s[i + j];
    return sgn(t);
}

// ephemeris.py Word: bits[30] in +-1 form, d29 / d30 of the word before.  ok: paritypass; b[24]: the data bits as 0 / 1 (bitstring)
struct NavWord {
    int d29, d30, ok;
    unsigned data;   // 24 data bits, the first one in bit 23
};
static NavWord make_word(int polarity, int d29s, int d30s, const int *bits)
{
    NavWord w;
    w.d29 = bits[28];
    w.d30 = bits[29];
    const int dStar[6] = {d29s, d30s, d29s, d30s, d30s, d29s};
    bool pass = true;
    for (int i = 0; i < 6; ++i) {
        int prod = 1;
        for (int j = 0; j < 24; ++j) {
            const int p = d30s * (int)kParityMat[i][j] * bits[j];
            if (p != 0) prod *= p;
        }
        if (prod * dStar[i] != bits[24 + i]) pass = false;
    }
    w.ok = pass ? 1 : 0;
    w.data = 0u;
    for (int j = 0; j < 24; ++j) w.data = (w.data << 1) | (polarity * bits[j] == -1 ? 1u : 0u);
    return w;
}
// bitstring[a:b] of a word (or of two words joined) as an unsigned integer
static inline unsigned long long wbits(const NavWord &w, int a, int b) { return (w.data >> (24 - b)) & ((1ull << (b - a)) - 1ull); }
static inline long long twos(unsigned long long v, int len) { return (v >> (len - 1)) & 1ull ? (long long)v - (1ll << len) : (long long)v; }
static inline unsigned long long join(unsigned long long hi, unsigned long long lo, int loLen) { return (hi << loLen) | lo; }

enum { F_SQRTA, F_E, F_I0, F_OMG0, F_OMG, F_M0, F_DELN, F_OMGD, F_IDOT, F_CRC, F_CRS, F_CUC, F_CUS, F_CIC, F_CIS, F_TOE, F_TOC, F_AF0, F_AF1, F_AF2, F_TGD };

// ten words from 300 bits, polarity chained through d30 (dataparser.py:54-64).  Returns the words' parity flags; *mismatch: the first
// word's polarity is not the d30 handed in (the twin's assertion)
static void make_subframe(const int *bits300, int polarity, int &d29, int &d30, NavWord w[10], bool *mismatch)
{
    *mismatch = polarity != d30;
    w[0] = make_word(polarity, d29, d30, bits300);
    for (int i = 1; i < 10; ++i) w[i] = make_word(w[i - 1].d30, w[i - 1].d29, w[i - 1].d30, bits300 + 30 * i);
    d29 = w[9].d29;
    d30 = w[9].d30;
}

static void decode_full(const int8_t *s, int64_t n, int64_t cpFirst, dpe_nav_decoded &o)
{
    const double p2m5 = std::ldexp(1.0, -5), p2m19 = std::ldexp(1.0, -19), p2m29 = std::ldexp(1.0, -29), p2m31 = std::ldexp(1.0, -31),
                 p2m33 = std::ldexp(1.0, -33), p2m43 = std::ldexp(1.0, -43), p2m55 = std::ldexp(1.0, -55);
    const int64_t nCorr = n - kPreambleLen + 1;
    std::vector<unsigned char> hit((size_t)std::max<int64_t>(nCorr, 0), 0);
    for (int64_t i = 0; i < nCorr; ++i)
        if (std::abs(preamble_corr(s, i)) > kPreambleThreshold) { hit[(size_t)i] = 1; ++o.nPreambleHits; }
    int64_t loc0 = -1;
    for (int64_t i = 0; i + 4 * kSubframeCp < nCorr; ++i)
        if (hit[(size_t)i] && hit[(size_t)(i + kSubframeCp)] && hit[(size_t)(i + 2 * kSubframeCp)] && hit[(size_t)(i + 3 * kSubframeCp)] && hit[(size_t)(i + 4 * kSubframeCp)]) {
            loc0 = i;
            break;
        }
    if (loc0 < 0 || loc0 + 5 * kSubframeCp > n) { o.status |= DPE_NAV_DEC_FEW_PREAMBLES; return; }
    if (loc0 < 2 * kBitCp) { o.status |= DPE_NAV_DEC_NO_HISTORY; return; }
    bool allP = true, allN = true;
    for (int f = 0; f < 5; ++f) {
        o.polarity[f] = sgn(preamble_corr(s, loc0 + (int64_t)f * kSubframeCp));
        o.subframeCp[f] = loc0 + (int64_t)f * kSubframeCp + cpFirst;
        allP = allP && o.polarity[f] == 1;
        allN = allN && o.polarity[f] == -1;
    }
    if (!allP && !allN) o.status |= DPE_NAV_DEC_POLARITY_FLIP;
    std::vector<int> bits(1500);
    for (int b = 0; b < 1500; ++b) bits[b] = nav_bit(s, loc0 + (int64_t)b * kBitCp);
    int d29 = nav_bit(s, loc0 - 2 * kBitCp), d30 = nav_bit(s, loc0 - kBitCp);
    int iodeFirst = -1, nFields = 0;
    for (int f = 0; f < 5; ++f) {
        NavWord w[10];
        bool mismatch;
        make_subframe(bits.data() + 300 * f, o.polarity[f], d29, d30, w, &mismatch);
        bool allOk = true;
        for (int i = 0; i < 10; ++i) { o.parity[f * 10 + i] = w[i].ok; allOk = allOk && w[i].ok; }
        if (mismatch) o.status |= DPE_NAV_DEC_POLARITY_D30;
        if (!allOk) o.status |= DPE_NAV_DEC_PARITY;
        if (mismatch || !allOk) continue;   // (the twin raises here: a failed word has no bit string)
        const int id = (int)wbits(w[1], 19, 22);
        o.subframeId[f] = id;
        if (id < 1 || id > 3) continue;
        const int tow = (int)wbits(w[1], 0, 17) * 6 - 6;
        const int iode = id == 1 ? (int)wbits(w[7], 0, 8) : id == 2 ? (int)wbits(w[2], 0, 8) : (int)wbits(w[9], 0, 8);
        if (iodeFirst < 0) iodeFirst = iode;
        o.iode = iodeFirst;
        if (id == 1 && o.iodc < 0) o.iodc = (int)join(wbits(w[2], 22, 24), wbits(w[7], 0, 8), 8);
        if (iode != iodeFirst) { o.status |= DPE_NAV_DEC_IODE; continue; }
        // Ephemerides.add: a field already present stays
        if (o.cp < 0) { o.tow = tow; o.cp = o.subframeCp[f]; }
        auto put = [&](int idx, double v) { if (std::isnan(o.eph[idx])) { o.eph[idx] = v; ++nFields; } };
        if (id == 1) {
            if (o.week < 0) o.week = (int)wbits(w[2], 0, 10) + 1024;
            if (o.accuracy < 0) o.accuracy = (int)wbits(w[2], 12, 16);
            if (o.health < 0) o.health = (int)wbits(w[2], 16, 17);
            put(F_TGD, (double)twos(wbits(w[6], 16, 24), 8) * p2m31);
            put(F_TOC, (double)((long long)wbits(w[7], 8, 24) * 16));
            put(F_AF2, (double)twos(wbits(w[8], 0, 8), 8) * p2m55);
            put(F_AF1, (double)twos(wbits(w[8], 8, 24), 16) * p2m43);
            put(F_AF0, (double)twos(wbits(w[9], 0, 22), 22) * p2m31);
        } else if (id == 2) {
            put(F_CRS, (double)twos(wbits(w[2], 8, 24), 16) * p2m5);
            put(F_DELN, (double)twos(wbits(w[3], 0, 16), 16) * p2m43 * kPi);
            put(F_M0, (double)twos(join(wbits(w[3], 16, 24), wbits(w[4], 0, 24), 24), 32) * p2m31 * kPi);
            put(F_CUC, (double)twos(wbits(w[5], 0, 16), 16) * p2m29);
            put(F_E, (double)join(wbits(w[5], 16, 24), wbits(w[6], 0, 24), 24) * p2m33);
            put(F_CUS, (double)twos(wbits(w[7], 0, 16), 16) * p2m29);
            put(F_SQRTA, (double)join(wbits(w[7], 16, 24), wbits(w[8], 0, 24), 24) * p2m19);
            put(F_TOE, (double)((long long)wbits(w[9], 0, 16) * 16));
        } else {
            put(F_IDOT, (double)twos(wbits(w[9], 8, 22), 14) * p2m43 * kPi);
            put(F_CIC, (double)twos(wbits(w[2], 0, 16), 16) * p2m29);
            put(F_OMG0, (double)twos(join(wbits(w[2], 16, 24), wbits(w[3], 0, 24), 24), 32) * p2m31 * kPi);
            put(F_CIS, (double)twos(wbits(w[4], 0, 16), 16) * p2m29);
            put(F_I0, (double)twos(join(wbits(w[4], 16, 24), wbits(w[5], 0, 24), 24), 32) * p2m31 * kPi);
            put(F_CRC, (double)twos(wbits(w[6], 0, 16), 16) * p2m5);
            put(F_OMG, (double)twos(join(wbits(w[6], 16, 24), wbits(w[7], 0, 24), 24), 32) * p2m31 * kPi);
            put(F_OMGD, (double)twos(wbits(w[8], 0, 24), 24) * p2m43 * kPi);
        }
    }
    if (nFields != DPE_NAV_EPH_DOUBLES || o.cp < 0) o.status |= DPE_NAV_DEC_INCOMPLETE;
}

// TLM and HOW of the subframe whose preamble starts at entry i; false: a parity failure, or the polarity contradicts d30
static bool tlm_how(const int8_t *s, int64_t i, int *howCount, int *id)
{
    int bits[60];
    for (int b = 0; b < 60; ++b) bits[b] = nav_bit(s, i + (int64_t)b * kBitCp);
    const int d29 = nav_bit(s, i - 2 * kBitCp), d30 = nav_bit(s, i - kBitCp);
    const int pol = sgn(preamble_corr(s, i));
    if (pol != d30) return false;
    const NavWord w0 = make_word(pol, d29, d30, bits);
    const NavWord w1 = make_word(w0.d30, w0.d29, w0.d30, bits + 30);
    if (!w0.ok || !w1.ok) return false;
    *howCount = (int)wbits(w1, 0, 17);
    *id = (int)wbits(w1, 19, 22);
    return true;
}

static void decode_assisted(const int8_t *s, int64_t n, int64_t cpFirst, dpe_nav_decoded &o)
{
    const int64_t nCorr = n - kPreambleLen + 1;
    const int64_t need = kSubframeCp + 60 * kBitCp;   // the second subframe's TLM and HOW
    bool found = false;
    for (int64_t i = 0; i < nCorr; ++i) {
        if (std::abs(preamble_corr(s, i)) <= kPreambleThreshold) continue;
        ++o.nPreambleHits;
        if (found || i < 2 * kBitCp || i + need > n) continue;
        if (std::abs(preamble_corr(s, i + kSubframeCp)) <= kPreambleThreshold) continue;
        int how0, how1, id0, id1;
        if (!tlm_how(s, i, &how0, &id0) || !tlm_how(s, i + kSubframeCp, &how1, &id1)) continue;
        if (how1 * 6 != how0 * 6 + 6) continue;
        found = true;
        // the twin's convention: the stamp is the start of the first of subframes 1-3 from here on (ephemeris.py:255-262) -- behind a
        // subframe 4 or 5 that is the same instant counted on, 6 s and 6000 code periods per subframe
        const int skip = id0 == 4 ? 2 : id0 == 5 ? 1 : 0;
        o.tow = how0 * 6 - 6 + 6 * skip;
        o.cp = i + cpFirst + (int64_t)skip * kSubframeCp;
        o.subframeId[0] = id0;
        o.subframeId[1] = id1;
        o.polarity[0] = sgn(preamble_corr(s, i));
        o.polarity[1] = sgn(preamble_corr(s, i + kSubframeCp));
        o.subframeCp[0] = i + cpFirst;
        o.subframeCp[1] = i + cpFirst + kSubframeCp;
        o.parity[0] = o.parity[1] = o.parity[10] = o.parity[11] = 1;
    }
    if (!found) o.status |= DPE_NAV_DEC_FEW_PREAMBLES;
}

// ---------------------------------------------------------------------------------------------------------------- solve (device)
constexpr int kNavWaves = 4;   // epochs per block

struct NavLogArgs {
    const double *log;        // the tracker's ring
    long long logCap, firstWindow;
    int K, nEpochs, stride, n;
    double ds, rxTime0, rxTimeStep;
    const NavChan *chan;      // [nChan]
    dpe_nav_fix *out;         // [nEpochs]
    int sel[DPE_MAX_CHAN];    // the selected channels in ascending order
};

__device__ __forceinline__ double nav_wave_max(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

__global__ __launch_bounds__(kNavWaves * 64) void nav_solve_log_kernel(NavLogArgs a)
{
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * kNavWaves + (threadIdx.x >> 6);
    if (e >= a.nEpochs) return;   // (wave-uniform; the kernel has no barrier)
    const bool active = lane < a.n;
    const long long slot = (a.firstWindow + (long long)e * a.stride) % a.logCap;
    double tt = -INFINITY, fi = 0.0, sat[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int bad = 0;
    if (active) {
        const int ch = a.sel[lane];
        const double *rec = a.log + ((size_t)slot * a.K + ch) * DPE_TRK_LOG_DOUBLES;
        const double cp = rec[0], rc = rec[1];
        fi = rec[4];
        const NavChan c = a.chan[ch];
        if (nav_transmit(c, cp, rc, tt, sat)) bad = DPE_NAV_SOL_KEPLER;
    }
    int status = __any(bad) ? DPE_NAV_SOL_KEPLER : 0;
    const double rxTime = a.rxTime0 == a.rxTime0 ? a.rxTime0 + (double)e * a.rxTimeStep : nav_wave_max(tt) + 0.068;
    double o[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (active) nav_observe(sat, tt, fi, a.ds, rxTime, o);
    dpe_nav_fix f;
    nav_solve_core(a.n, [&](int k, double r[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) r[i] = __shfl(o[i], k, 64);
    }, rxTime, f, status);
    if (lane == 0) a.out[e] = f;
}

}  // namespace dpe

struct dpe_nav {
    int K = 0;
    double ds = 1.0;
    int status = 0;
    std::vector<dpe::NavChan> chan;
    dpe::NavChan *chan_d = nullptr;
    bool chanDirty = true;
    dpe_nav_fix *out_d = nullptr;
    long long outCap = 0;
};

static int nav_select(const dpe_nav *h, uint64_t mask, int sel[DPE_MAX_CHAN])
{
    int n = 0;
    for (int k = 0; k < h->K; ++k)
        if (mask == 0 || ((mask >> k) & 1ull)) sel[n++] = k;
    return n;
}

extern "C" {

int dpe_nav_create(int32_t nChan, double dopplerSign, dpe_nav **out)
{
    DPE_REQUIRE(out, "[ScalarNavigator] create: null argument");
    DPE_REQUIRE(nChan >= 1 && nChan <= DPE_MAX_CHAN, "[ScalarNavigator] create: nChan out of range");
    dpe_nav *h = new dpe_nav();
    h->K = nChan;
    h->ds = dopplerSign != 0.0 ? dopplerSign : 1.0;
    h->chan.resize(nChan);
    for (auto &c : h->chan) std::memset(&c, 0, sizeof(c));
    *out = h;
    return 0;
}

int dpe_nav_destroy(dpe_nav *h)
{
    if (!h) return 0;
    if (h->chan_d) (void)hipFree(h->chan_d);
    if (h->out_d) (void)hipFree(h->out_d);
    delete h;
    return 0;
}

int dpe_nav_decode(dpe_nav *h, int32_t chan, const int8_t *signs, int64_t n, int64_t cpFirst, int32_t mode, const double *cpLog,
                   int64_t nCpLog, dpe_nav_decoded *out)
{
    using namespace dpe;
    DPE_REQUIRE(h && signs && out, "[ScalarNavigator] decode: null argument");
    DPE_REQUIRE(chan >= 0 && chan < h->K, "[ScalarNavigator] decode: channel %d out of range", chan);
    DPE_REQUIRE(n >= 0 && cpFirst >= 0, "[ScalarNavigator] decode: negative length or code-period count");
    DPE_REQUIRE(mode == DPE_NAV_MODE_FULL || mode == DPE_NAV_MODE_ASSISTED, "[ScalarNavigator] decode: unknown mode %d", mode);
    dpe_nav_decoded &o = *out;
    std::memset(&o, 0, sizeof(o));
    for (double &v : o.eph) v = std::nan("");
    o.week = o.accuracy = o.health = o.iode = o.iodc = -1;
    o.tow = -1;
    o.cp = -1;
    for (int f = 0; f < 5; ++f) { o.subframeId[f] = -1; o.subframeCp[f] = -1; }
    for (int &p : o.parity) p = -1;
    if (cpLog)
        for (int64_t i = 1; i < nCpLog; ++i)
            if (cpLog[i] - cpLog[i - 1] != 1.0) { o.status |= DPE_NAV_DEC_CP_SLIP; break; }   // dataparser.py:15
    if (mode == DPE_NAV_MODE_FULL) decode_full(signs, n, cpFirst, o);
    else decode_assisted(signs, n, cpFirst, o);
    NavChan &c = h->chan[chan];
    if (mode == DPE_NAV_MODE_FULL && !(o.status & (DPE_NAV_DEC_INCOMPLETE | DPE_NAV_DEC_FEW_PREAMBLES | DPE_NAV_DEC_NO_HISTORY))) {
        std::memcpy(&c.eph, o.eph, sizeof(double) * DPE_NAV_EPH_DOUBLES);
        c.haveEph = 1;
    }
    if (o.cp >= 0) {
        c.tow = (double)o.tow;
        c.cp = (double)o.cp;
        c.haveTime = 1;
    }
    h->chanDirty = true;
    return 0;
}

int dpe_nav_set_ephemerides(dpe_nav *h, const double *eph, const int32_t *tow, const int64_t *cp)
{
    DPE_REQUIRE(h, "[ScalarNavigator] set_ephemerides: null argument");
    DPE_REQUIRE((tow == nullptr) == (cp == nullptr), "[ScalarNavigator] set_ephemerides: a timestamp is TOW and cp together");
    for (int k = 0; k < h->K; ++k) {
        dpe::NavChan &c = h->chan[k];
        if (eph) {
            std::memcpy(&c.eph, eph + (size_t)k * DPE_NAV_EPH_DOUBLES, sizeof(double) * DPE_NAV_EPH_DOUBLES);
            c.haveEph = 1;
        }
        if (tow) {
            c.tow = (double)tow[k];
            c.cp = (double)cp[k];
            c.haveTime = 1;
        }
    }
    h->chanDirty = true;
    return 0;
}

int dpe_nav_solve(dpe_nav *h, const double *cp, const double *rc, const double *fi, uint64_t chanMask, double rxTime0, dpe_nav_fix *out)
{
    using namespace dpe;
    DPE_REQUIRE(h && cp && rc && fi && out, "[ScalarNavigator] solve: null argument");
    int sel[DPE_MAX_CHAN];
    const int n = nav_select(h, chanMask, sel);
    int status = 0;
    double tt[DPE_MAX_CHAN], sat[DPE_MAX_CHAN][8], obs[DPE_MAX_CHAN][8];
    double tmax = -INFINITY;
    for (int i = 0; i < n; ++i) {
        const NavChan &c = h->chan[sel[i]];
        DPE_REQUIRE(c.haveEph && c.haveTime, "[ScalarNavigator] solve: channel %d has no ephemerides or no timestamp", sel[i]);
        if (nav_transmit(c, cp[sel[i]], rc[sel[i]], tt[i], sat[i])) status |= DPE_NAV_SOL_KEPLER;
        tmax = std::fmax(tmax, tt[i]);
    }
    const double rxTime = rxTime0 == rxTime0 ? rxTime0 : tmax + 0.068;
    for (int i = 0; i < n; ++i) nav_observe(sat[i], tt[i], fi[sel[i]], h->ds, rxTime, obs[i]);
    nav_solve_core(n, [&](int k, double r[8]) { for (int i = 0; i < 8; ++i) r[i] = obs[k][i]; }, rxTime, *out, status);
    h->status |= out->status;
    return 0;
}

int dpe_nav_solve_log(dpe_nav *h, dpe_trk *trk, int64_t firstWindow, int32_t nEpochs, int32_t stride, uint64_t chanMask, double rxTime0,
                      double rxTimeStep, dpe_nav_fix *out, dpe_stream_t stream_)
{
    using namespace dpe;
    DPE_REQUIRE(h && trk && out, "[ScalarNavigator] solve_log: null argument");
    TrkLogView v;
    if (trk_log_view(trk, &v)) return -1;
    DPE_REQUIRE(v.K == h->K, "[ScalarNavigator] solve_log: the tracker has %d channels, the navigator %d", v.K, h->K);
    DPE_REQUIRE(nEpochs >= 1 && stride >= 1, "[ScalarNavigator] solve_log: nEpochs and stride must be positive");
    const long long last = firstWindow + (long long)(nEpochs - 1) * stride;
    DPE_REQUIRE(firstWindow >= 0 && last < v.nWindows, "[ScalarNavigator] solve_log: windows [%lld, %lld] have not been tracked",
                (long long)firstWindow, last);
    DPE_REQUIRE(firstWindow >= v.nWindows - v.logCap, "[ScalarNavigator] solve_log: window %lld has left the log (capacity %lld)",
                (long long)firstWindow, v.logCap);
    NavLogArgs a;
    a.n = nav_select(h, chanMask, a.sel);
    for (int i = a.n; i < DPE_MAX_CHAN; ++i) a.sel[i] = 0;
    for (int i = 0; i < a.n; ++i)
        DPE_REQUIRE(h->chan[a.sel[i]].haveEph && h->chan[a.sel[i]].haveTime, "[ScalarNavigator] solve_log: channel %d has no ephemerides or no timestamp",
                    a.sel[i]);
    hipStream_t st = (hipStream_t)stream_;
    if (!h->chan_d) {
        h->chan_d = dev_alloc<NavChan>(h->K);
        DPE_REQUIRE(h->chan_d, "[ScalarNavigator] solve_log: device allocation failed");
        h->chanDirty = true;
    }
    if (h->chanDirty) {   // ephemerides and timestamps go up once, not per call
        DPE_CHECK_HIP(hipStreamSynchronize(st));
        DPE_CHECK_HIP(hipMemcpy(h->chan_d, h->chan.data(), sizeof(NavChan) * h->K, hipMemcpyHostToDevice));
        h->chanDirty = false;
    }
    if (h->outCap < nEpochs) {
        DPE_CHECK_HIP(hipStreamSynchronize(st));
        if (h->out_d) (void)hipFree(h->out_d);
        h->outCap = 0;
        h->out_d = dev_alloc<dpe_nav_fix>((size_t)nEpochs);
        DPE_REQUIRE(h->out_d, "[ScalarNavigator] solve_log: device allocation failed");
        h->outCap = nEpochs;
    }
    a.log = v.log; a.logCap = v.logCap; a.firstWindow = firstWindow;
    a.K = v.K; a.nEpochs = nEpochs; a.stride = stride;
    a.ds = h->ds; a.rxTime0 = rxTime0; a.rxTimeStep = rxTimeStep;
    a.chan = h->chan_d; a.out = h->out_d;
    const int blocks = (nEpochs + kNavWaves - 1) / kNavWaves;
    hipLaunchKernelGGL(nav_solve_log_kernel, dim3(blocks), dim3(kNavWaves * 64), 0, st, a);
    DPE_CHECK_HIP(hipGetLastError());
    DPE_CHECK_HIP(hipMemcpyAsync(out, h->out_d, sizeof(dpe_nav_fix) * (size_t)nEpochs, hipMemcpyDeviceToHost, st));
    DPE_CHECK_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < nEpochs; ++i) h->status |= out[i].status;
    return 0;
}

int dpe_nav_load_log(dpe_trk *trk, int32_t nWindows, const double *rows, dpe_stream_t stream_)
{
    return dpe::trk_log_load(trk, nWindows, rows, (hipStream_t)stream_);
}

int dpe_nav_status(dpe_nav *h, int32_t *status)
{
    DPE_REQUIRE(h && status, "[ScalarNavigator] status: null argument");
    *status = h->status;
    return 0;
}

}  // extern "C"
