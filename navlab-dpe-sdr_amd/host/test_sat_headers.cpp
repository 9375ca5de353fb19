// test_sat_headers.cpp -- the orbit and channel-manager arithmetic headers with a host C++ compiler alone, no HIP header on the
// include path.  SAT_HEADERS chooses what is included:
//   1  dpe_sat.h alone
//   2  dpe_chm_arith.h alone
//   3  dpe_cd_plan.h, then dpe_sat.h, then dpe_chm_arith.h
// Each form evaluates one ephemeris and prints every double as a C99 hex float, one call per line; tests/test_sat_headers_cpu.py
// holds the forms to each other and to tests/golden/sat_headers_parent.txt, string for string.
//
//   test_sat_headers e0 .. e20 tx tau  cpElaEnd cpRef cpRefTOW rcEnd riEnd fc fi  x0 .. x7 rxTime T dopplerSign
//     sat_state       8 doubles     sat_state(e, tx)
//     sat_state_floor 8 doubles     sat_state_t(e, tx, ModFloor())
//     rotate_state    8 doubles     rotate_state(the first state, tau)
//     propagate       status, then fi fc rcStart rcEnd riStart riEnd txTime, cpElaStart cpElaEnd, sat[8]      (forms 2 and 3)
#include <cstdio>
#include <cstdlib>

#if SAT_HEADERS == 1
#include "../csrc/dpe_sat.h"
#elif SAT_HEADERS == 2
#include "../csrc/dpe_chm_arith.h"
#elif SAT_HEADERS == 3
#include "../csrc/dpe_cd_plan.h"
#include "../csrc/dpe_sat.h"
#include "../csrc/dpe_chm_arith.h"
#else
#error "SAT_HEADERS must be 1, 2 or 3"
#endif

using namespace dpe;

static void put(const char *name, const double *v, int n)
{
    printf("%s", name);
    for (int i = 0; i < n; ++i) printf(" %a", v[i]);
    printf("\n");
}

int main(int argc, char **argv)
{
    if (argc != 1 + 21 + 2 + 7 + 8 + 3) {
        fprintf(stderr, "test_sat_headers: %d arguments, 41 expected\n", argc - 1);
        return 2;
    }
    double a[41];
    for (int i = 0; i < 41; ++i) a[i] = strtod(argv[1 + i], nullptr);
    Eph e;
    double *ep = &e.sqrtA;
    for (int i = 0; i < 21; ++i) ep[i] = a[i];
    const double tx = a[21], tau = a[22];
    double s[8], sf[8], sr[8];
    if (sat_state(e, tx, s) || sat_state_t(e, tx, sf, ModFloor())) {
        fprintf(stderr, "test_sat_headers: Kepler's equation did not converge\n");
        return 1;
    }
    rotate_state(s, tau, sr);
    put("sat_state", s, 8);
    put("sat_state_floor", sf, 8);
    put("rotate_state", sr, 8);
#if SAT_HEADERS != 1
    Chan c{};
    c.prn = 1;
    c.cpElaEnd = (int)a[23]; c.cpRef = (int)a[24]; c.cpRefTOW = (int)a[25];
    c.rcEnd = a[26]; c.riEnd = a[27]; c.fc = a[28]; c.fi = a[29];
    c.eph = e;
    c.txTime = tx_of(c, c.cpElaEnd, c.rcEnd);
    if (sat_state(c.eph, c.txTime, c.sat)) return 1;
    const int status = propagate(c, a + 30, a[38], a[39], (int)a[40], SatDirect());
    const double f[7] = {c.fi, c.fc, c.rcStart, c.rcEnd, c.riStart, c.riEnd, c.txTime};
    printf("propagate %d", status);
    for (int i = 0; i < 7; ++i) printf(" %a", f[i]);
    printf(" %d %d", c.cpElaStart, c.cpElaEnd);
    for (int i = 0; i < 8; ++i) printf(" %a", c.sat[i]);
    printf("\n");
#endif
    return 0;
}
