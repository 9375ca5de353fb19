#!/usr/bin/env python3
"""Timing behind profiles/subsets_scan.txt: the subsets scan (engine.SubsetManifold, dpe_bcm_update_subsets) at config R's shape
-- two 25^4-point grids, 8 SVs, 256 windows -- with the 8 leave-one-out masks (a), beside the way to the same nine fixes
without it: nine dpe_bcm_update calls, one on all 8 channels and eight on 7 (b), and beside one plain dpe_bcm_update (c), all
on the same box in the same run with scores written.  HIP events around the C entry points, 3 warm-ups, median of 10.  The
banks hold noise: the scan's time does not depend on their values (bank half-widths of config R, wide enough for every index);
the 7-channel calls of (b) read the first 7 rows of each window, which costs what any 7 rows cost.  (b) leaves out the eight
gathers of 7 bank rows or the eight stage-1 calls a real caller also pays.
Needs a GPU:  python scripts/subsets_time.py [output file]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import navlab_dpe_sdr_amd as dpe  # noqa: E402

K, W, G = 8, 256, 390625
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
masks = dpe.engine.leave_one_out_masks(K)


def timed(fn):
    ms = []
    for _ in range(13):
        tm.start(); fn(); tm.stop()
        ms.append(tm.elapsed_ms())
    return float(np.median(ms[3:])), min(ms[3:]), max(ms[3:])


kw = dict(lag_half_width=L, bin_half_width=B, max_windows=W, max_channels=K)
sub = dpe.SubsetManifold(FS, S, Cf, pos, vel, K, **kw)
sub.Start()
ta = timed(lambda: sub.Update(code, carr, bw, ce, masks))
ra = sub.results()
t0 = timed(lambda: sub.Update(code, carr, bw, ce, None))
split = sub.last_split()
sub.Stop()

plain = dpe.BatchCorrManifold(FS, S, Cf, pos, vel, write_scores=True, **kw)
plain.Start()
tc = timed(lambda: plain.Update(code, carr, bw, ce))
rc = plain.results()
ce7 = [np.ascontiguousarray(ce[:, [k for k in range(K) if k != j]]) for j in range(K)]


def nine():
    plain.Update(code, carr, bw, ce)
    for j in range(K):
        plain.Update(code, carr, bw, ce7[j])


tb = timed(nine)
plain.Stop()

same = sum(int(ra[w]["posIndex"] == rc[w]["posIndex"] and ra[w]["velIndex"] == rc[w]["velIndex"]) for w in range(W))
n_ent = 2 * max(L, B) + 1
lds = K * n_ent * 16
lines = [
    "(a) dpe_bcm_update_subsets, 256 windows, 8 leave-one-out masks: median %.3f ms (min %.3f, max %.3f)" % ta,
    "(b) nine dpe_bcm_update calls (8 channels, then 8 x 7 channels):  median %.3f ms (min %.3f, max %.3f)" % tb,
    "(c) one dpe_bcm_update, 8 channels:                              median %.3f ms (min %.3f, max %.3f)" % tc,
    "    dpe_bcm_update_subsets with nSubsets = 0 (the plain variant): median %.3f ms (min %.3f, max %.3f)" % t0,
    "(a) / (b) = %.2f;  (a) / (c) = %.2f;  nSubsets = 0 / (c) = %.2f" % (ta[0] / tb[0], ta[0] / tc[0], t0[0] / tc[0]),
    "blocks per window (position, velocity): %s;  dynamic LDS per block %d B (K x (2 max(L, B) + 1) x 16)" % (split, lds),
    "full set's arg-max pair against dpe_bcm_update's: the same on %d of %d windows" % (same, W),
]
hdr = "%s: %d SVs, grids %d + %d points, %d windows, L = %d, B = %d" % (dpe.engine.device_info()[0], K, G, G, W, L, B)
text = "\n".join([hdr] + lines)
print(text)
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "subsets_scan.txt")
with open(out, "w") as f:
    f.write("Subsets scan with the leave-one-out masks against nine plain scans and against one (scripts/subsets_time.py: HIP events\n"
            "around the C entry points, 3 warm-ups, median of 10)\n\n" + text + "\n")
