// dpe_trk_log.h -- the scalar tracker's device-resident log as the other translation units may read it (dpe_nav.hip solves the logged
// epochs without the log coming back to the host).  Defined in dpe_trk.hip.
#pragma once
#include "dpe_common.h"

namespace dpe {

struct TrkLogView {
    const double *log;    // [logCap][K][DPE_TRK_LOG_DOUBLES], a ring over the windows since dpe_trk_set_params
    long long logCap, nWindows;
    int K;
    const int *prn;       // host, [K]
};
int trk_log_view(dpe_trk *h, TrkLogView *out);
// rows [nWindows][K][DPE_TRK_LOG_DOUBLES] (host) become the log's windows [0, nWindows).  This ends the record the tracker was on: its
// window count becomes nWindows and dpe_trk_track refuses to go on until dpe_trk_set_params (a log carries no loop state)
int trk_log_load(dpe_trk *h, int nWindows, const double *rows, hipStream_t st);

}  // namespace dpe
