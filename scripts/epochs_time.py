#!/usr/bin/env python3
"""Timing behind profiles/epochs.txt: the multi-epoch scan (engine.EpochManifold, dpe_bcm_update_epochs) at config R's shape
-- two 25^4-point grids, 8 SVs, 256 windows -- as 16 groups of 16 windows and as 256 groups of 1, beside dpe_bcm_update on
the same 256 windows with scores written (the single-window scan: the yardstick), and the 16 x 16 case again with the pairs
of a pass capped so that a group takes 4 passes (the price of a pass: one row read and write, one LDS refill).  HIP events
around the C entry point, 3 warm-ups, median of 10.  The banks hold noise: the scan's time does not depend on their values
(bank half-widths of config R, wide enough for every index).  Needs a GPU:  python scripts/epochs_time.py [output file]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import navlab_dpe_sdr_amd as dpe  # noqa: E402

K, W, G, N = 8, 256, 390625, 16
cfg = dpe.workload.CONFIG_R
FS, S = cfg["fs"], cfg["S"]
Cf = dpe.engine.carr_fft_len(S)
pos = dpe.synth.rand_grid(3, G)
vel = dpe.synth.rand_grid(4, G, half=(6.0, 6.0, 6.0, 3.0))
L, B = dpe.pipeline.bank_half_widths(pos, vel, FS, Cf)
ho = dpe.handoff.read_handoff(dpe.workload.HANDOFF_CSV)
dev = torch.device("cuda:0")

X = np.array(ho["X_ECEF"], dtype=np.float64)
cm = dpe.engine.ChanMgr.from_handoff(ho, S / FS, K)
ce, bw = np.zeros((W, K), dtype=dpe.engine.CHAN_END_DTYPE), np.zeros(W, dtype=dpe.engine.BCM_WINDOW_DTYPE)
for w in range(W):
    (cm.Start if w == 0 else cm.Update)(X, X, (0.0,))
    _s, e, win = cm.outputs()
    ce[w], bw[w] = e, win[0]
cm.Stop()
g = torch.Generator(device=dev).manual_seed(0)
code = torch.randn((W, K, 2 * L + 1, 2), device=dev, generator=g)
carr = torch.randn((W, K, 2 * B + 1, 2), device=dev, generator=g)
tm = dpe.engine.HipEventTimer()


def timed(fn):
    ms = []
    for _ in range(13):
        tm.start(); fn(); tm.stop()
        ms.append(tm.elapsed_ms())
    return float(np.median(ms[3:])), min(ms[3:]), max(ms[3:])


def epochs(n, pairs_per_pass=0):
    h = dpe.EpochManifold(FS, S, Cf, pos, vel, n, pairs_per_pass, lag_half_width=L, bin_half_width=B, max_windows=W, max_channels=K)
    h.Start()
    t = timed(lambda: h.Update(code, carr, bw, ce, n))
    res = h.results()
    h.Stop()
    return t, res


lines = []
single = dpe.BatchCorrManifold(FS, S, Cf, pos, vel, lag_half_width=L, bin_half_width=B, max_windows=W, max_channels=K, write_scores=True)
single.Start()
ts = timed(lambda: single.Update(code, carr, bw, ce))
sres = single.results()
single.Stop()
lines.append("dpe_bcm_update, 256 windows, scores written (the single-window scan): median %.3f ms (min %.3f, max %.3f)" % ts)
t16, r16 = epochs(N)
lines.append("dpe_bcm_update_epochs, 16 groups x 16 windows, automatic passes (%d per group): median %.3f ms (min %.3f, max %.3f)"
             % ((r16[0]["nPasses"],) + t16))
t1, r1 = epochs(1)
lines.append("dpe_bcm_update_epochs, 256 groups x 1 window (%d pass): median %.3f ms (min %.3f, max %.3f)" % ((r1[0]["nPasses"],) + t1))
t4, r4 = epochs(N, 4 * K)
lines.append("dpe_bcm_update_epochs, 16 groups x 16 windows, pairsPerPass %d (%d passes per group): median %.3f ms (min %.3f, max %.3f)"
             % ((4 * K, r4[0]["nPasses"]) + t4))
t1p, r1p = epochs(N, N * K)
lines.append("dpe_bcm_update_epochs, 16 groups x 16 windows, pairsPerPass %d (%d passes per group): median %.3f ms (min %.3f, max %.3f)"
             % ((N * K, r1p[0]["nPasses"]) + t1p))
lines.append("16 x 16 / single-window scan of the same 256 windows: %.2f;  256 x 1 / single-window scan: %.2f" % (t16[0] / ts[0], t1[0] / ts[0]))
lines.append("a pass costs (4 passes against %d): %.3f ms per extra pass over the 16 groups" % (r16[0]["nPasses"], (t4[0] - t16[0]) / max(1, r4[0]["nPasses"] - r16[0]["nPasses"])))
same = sum(int(r1[w]["posIndex"] == sres[w]["posIndex"] and r1[w]["velIndex"] == sres[w]["velIndex"]) for w in range(W))
lines.append("256 x 1 against dpe_bcm_update, windows with the same arg-max pair: %d of %d;  16 x 16 in 4 passes against automatic, groups with "
             "the same keys: %d of 16" % (same, W, sum(int(a["posIndex"] == b["posIndex"] and a["posScore"] == b["posScore"] and
                                                             a["velIndex"] == b["velIndex"] and a["velScore"] == b["velScore"])
                                                         for a, b in zip(r16, r4))))
hdr = "%s: %d SVs, grids %d + %d points, %d windows, L = %d, B = %d (LDS budget: %d pairs per pass)" % (
    dpe.engine.device_info()[0], K, G, G, W, L, B, (150 * 1024) // ((2 * max(L, B) + 1) * 16 + 32))
text = "\n".join([hdr] + lines)
print(text)
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "epochs.txt")
with open(out, "w") as f:
    f.write("Multi-epoch scan against the single-window scan of the same windows (scripts/epochs_time.py: HIP events around the\n"
            "C entry point, 3 warm-ups, median of 10)\n\n" + text + "\n")
