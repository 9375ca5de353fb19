#!/usr/bin/env python3
"""Timing behind profiles/refine_scan.txt: the coarse-to-fine scan (engine.RefineManifold, dpe_bcm_update_refine) on one MI355X.

(1) Refine against one axes Update, at config R's stage shape (256 windows, 8 SVs): two levels of 25^4 axes through the refine
    handle against ONE Update of a dpe_bcm_create_axes handle on one 25^4 grid, Update + results each, the two handles
    alternating in one process.  Expectation: 2x (the same arithmetic per level, one more launch), within 10 % for the centre
    decode and the per-tile adds.
(2) Refine against the dense grid, one window: levels 7^4 -> 13^4 against the dense 31^4 axes grid of equal resolution and
    reach (tests/refine_world.py's grids).  The capability's own comparison; recorded, not gated.
Wall clock around Update + results (the results call waits for the stream), 5 warm-ups, median of 20.  The banks hold noise (the
scan's time does not depend on their values), with half-widths from pipeline.bank_half_widths_refine for the levels of each
case, the same for both handles of a case.
Needs a GPU:  python scripts/refine_time.py [output file]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import navlab_dpe_sdr_amd as dpe  # noqa: E402

K = 8
cfg = dpe.workload.CONFIG_R
FS, S = cfg["fs"], cfg["S"]
Cf = dpe.engine.carr_fft_len(S)
ho = dpe.handoff.read_handoff(dpe.workload.HANDOFF_CSV)
dev = torch.device("cuda:0")
X = np.array(ho["X_ECEF"], dtype=np.float64)


def records(W):
    cm = dpe.engine.ChanMgr.from_handoff(ho, S / FS, K)
    ce, bw = np.zeros((W, K), dtype=dpe.engine.CHAN_END_DTYPE), np.zeros(W, dtype=dpe.engine.BCM_WINDOW_DTYPE)
    for w in range(W):
        (cm.Start if w == 0 else cm.Update)(X, X, (0.0,))
        _s, e, win = cm.outputs()
        ce[w], bw[w] = e, win[0]
    cm.Stop()
    return ce, bw


def case(W, levels, single, write_scores):
    """Median (min, max) ms of Update + results for the refine handle on `levels` and the axes handle on `single`, alternating."""
    L, B = dpe.pipeline.bank_half_widths_refine(levels, FS, Cf)
    L1, B1 = dpe.pipeline.bank_half_widths_refine([single], FS, Cf)
    L, B = max(L, L1), max(B, B1)
    ce, bw = records(W)
    g = torch.Generator(device=dev).manual_seed(0)
    code = torch.randn((W, K, 2 * L + 1, 2), device=dev, generator=g)
    carr = torch.randn((W, K, 2 * B + 1, 2), device=dev, generator=g)
    kw = dict(lag_half_width=L, bin_half_width=B, max_windows=W, max_channels=K, write_scores=write_scores)
    ref = dpe.RefineManifold(FS, S, Cf, levels, **kw)
    one = dpe.BatchCorrManifold(FS, S, Cf, single[0], single[1], **kw)
    ref.Start(); one.Start()
    t = {"refine": [], "axes": []}
    for _ in range(25):
        for name, h in (("refine", ref), ("axes", one)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h.Update(code, carr, bw, ce)
            h.results()
            t[name].append((time.perf_counter() - t0) * 1e3)
    splits = (ref.last_split(), one.last_split())
    ref.Stop(); one.Stop()
    stat = {k: (float(np.median(v[5:])), min(v[5:]), max(v[5:])) for k, v in t.items()}
    return stat, (L, B), splits


u25 = (dpe.GridAxes.uniform(25, 1.0), dpe.GridAxes.uniform(25, 0.5))
f25 = (dpe.GridAxes.uniform(25, 1.0 / 12), dpe.GridAxes.uniform(25, 0.5 / 12))
s1, lb1, sp1 = case(256, [u25, f25], u25, True)


def uniform(n, step, shift=(0.0, 0.0, 0.0, 0.0)):
    return dpe.GridAxes(*[step * (np.arange(n) - (n - 1) // 2) + s for s in shift])


coarse = (uniform(7, 40.0), uniform(7, 12.0))
fine = (uniform(13, 40.0 / 3), uniform(13, 4.0))
dense = (uniform(31, 40.0 / 3), uniform(31, 4.0))
s2, lb2, sp2 = case(1, [coarse, fine], dense, True)

lines = [
    "(1) 256 windows, %d SVs, L = %d, B = %d, scores written" % ((K,) + lb1),
    "    refine, two levels of 25^4, Update + results: median %.3f ms (min %.3f, max %.3f)" % s1["refine"],
    "    axes handle, one 25^4 grid, Update + results:  median %.3f ms (min %.3f, max %.3f)" % s1["axes"],
    "    ratio %.2f (expected 2, margin 10 %%); blocks per window: refine last level %s, axes %s" % ((s1["refine"][0] / s1["axes"][0],) + sp1),
    "(2) 1 window, %d SVs, L = %d, B = %d, scores written" % ((K,) + lb2),
    "    refine, 7^4 -> 13^4 (30 962 points per manifold), Update + results: median %.3f ms (min %.3f, max %.3f)" % s2["refine"],
    "    axes handle, dense 31^4 (923 521 points per manifold), Update + results: median %.3f ms (min %.3f, max %.3f)" % s2["axes"],
    "    ratio %.3f; blocks per window: refine last level %s, axes %s" % ((s2["refine"][0] / s2["axes"][0],) + sp2),
]
text = "\n".join([dpe.engine.device_info()[0]] + lines)
print(text)
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "refine_scan.txt")
with open(out, "w") as f:
    f.write("Coarse-to-fine scan against one axes Update and against the dense grid (scripts/refine_time.py: wall clock around\n"
            "Update + results, the two handles alternating, 5 warm-ups, median of 20)\n\n" + text + "\n")
