#!/usr/bin/env python3
"""Timing behind profiles/nav_scalar.txt: dpe_nav_solve_log over 36 000 epochs x 8 SVs (HIP events, 3 warm-ups, median of 10), the
host form over the same epochs on one thread with the cost of the 36 000 calls through ctypes measured separately, and
dpe_trk_track for a record of the same length (one second of synthetic signal, repeated: the tracker's time does not depend on
what it tracks).  Needs a GPU:  python scripts/nav_scalar_time.py"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import navlab_dpe_sdr_amd as dpe  # noqa: E402

N, K, FS, S = 36000, 8, 2.5e6, 2500
ho = dpe.handoff.read_handoff(dpe.workload.HANDOFF_CSV)
t = np.arange(N) * 1e-3
chips = ho["rc"][None, :] + ho["fc"][None, :] * t[:, None]
cp = ho["cp"][None, :] + np.floor(chips / 1023.0)
rc = chips - 1023.0 * np.floor(chips / 1023.0)
fi = np.repeat(ho["fi"][None, :], N, axis=0)
trk = dpe.ScalarTracker(FS, ho["prn_list"], log_capacity_windows=N)
nav = dpe.ScalarNavigator(ho["prn_list"])
nav.set_ephemerides(ho["eph"], ho["TOW"], ho["cp_timestamp"])
tm = dpe.engine.HipEventTimer()

# the tracker on a record of N windows
ch = dpe.synth.random_channels(3, K, prns=ho["prn_list"])
ch["cp_ref"] = ch["cp_ref"] % 20
iq, _ = dpe.synth.gen_iq_record(5, FS, 1000 * S, ch, amp=90.0)
iq_d = torch.from_numpy(iq).to("cuda:0").repeat(N // 1000)
init = [dict(prn=int(p), rc=ch["rc"][k], ri=ch["ri"][k], fc=ch["fc"][k], fi=ch["fi"][k]) for k, p in enumerate(ho["prn_list"])]
ms = []
for i in range(13):
    trk.set_params(init)
    tm.start(); trk.track(iq_d, N); tm.stop()
    ms.append(tm.elapsed_ms())
print("dpe_trk_track %d windows x %d channels: median %.2f ms (frozen: %d)" % (N, K, np.median(ms[3:]), trk.dev_status()))

trk.load_log(dict(cp=cp, rc=rc, fi=fi))
ms = []
for i in range(13):
    tm.start(); out = nav.solve_log(trk); tm.stop()
    ms.append(tm.elapsed_ms())
print("dpe_nav_solve_log %d x %d: median %.3f ms (min %.3f max %.3f), status %d, iterations <= %d"
      % (N, K, np.median(ms[3:]), min(ms[3:]), max(ms[3:]), int(np.bitwise_or.reduce(out["status"])), out["iterations"].max()))
hs, cs = [], []
for i in range(3):
    t0 = time.perf_counter()
    host = [nav.solve(cp[m], rc[m], fi[m], chans=[0, 1, 2]) for m in range(N)]     # three rows: the call, the set-up, almost no arithmetic
    cs.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    host = [nav.solve(cp[m], rc[m], fi[m]) for m in range(N)]
    hs.append((time.perf_counter() - t0) * 1e3)
print("dpe_nav_solve, one thread, %d calls: median %.1f ms; the same calls on three channels (rank-deficient: three satellite states, one "
      "sweep, no iteration): %.1f ms" % (N, np.median(hs), np.median(cs)))
hx = np.array([h["X_ECEF"] for h in host])
print("device - host: position %.3e m, velocity %.3e m/s" % (np.abs(out["X_ECEF"][:, :4] - hx[:, :4]).max(), np.abs(out["X_ECEF"][:, 4:] - hx[:, 4:]).max()))
