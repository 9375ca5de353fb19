#!/usr/bin/env python3
"""Timing behind profiles/collective.txt: one collective-detection update (engine.CollectiveDetector, dpe_cd_update) on one MI355X
at a user shape -- by default K = 8 SVs, M = 2 500 delays, 41 bins, drift half-width J = 10, a 41 x 41 horizontal lattice
(P = 1 681): 8.8e7 hypotheses, 7.06e8 hypothesis x SV terms.

HIP events around a window of REPEAT back-to-back updates on one stream (the update is asynchronous; nothing is read back inside
the window), 3 warm-up windows, then 7 timed ones: median, min and max per update.  The surface holds uniform noise (the scan's
time does not depend on the values); delays and bins are drawn so that every (SV, j) stays inside the raster, the worst case for
time.  Beside the time goes the LDS-read bound of the chosen tile shape: a lane reads run + 1 = 6 dwords for run = 5 terms with
ds_read_b32, which the LDS serves at 128 B per clock and CU (256 CUs, 2.4 GHz); where K rows do not fit a block's LDS the rows are
read from L2 and the bound does not apply (printed as such).  The residual against the fp64 specification (tests/cd_ref.py) is
measured on the parity cases of tests/cd_world.py and printed as a fraction of the tests' tolerance.
Needs a GPU:  python scripts/collective_time.py [--K 8 --M 2500 --bins 41 --J 10 --side 41 --step 150] [--out file]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import navlab_dpe_sdr_amd as dpe  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--K", type=int, default=8)
ap.add_argument("--M", type=int, default=2500)
ap.add_argument("--bins", type=int, default=41)
ap.add_argument("--J", type=int, default=10)
ap.add_argument("--side", type=int, default=41, help="points per side of the square horizontal lattice")
ap.add_argument("--step", type=float, default=150.0, help="lattice spacing, m")
ap.add_argument("--repeat", type=int, default=200)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collective.txt"))
a = ap.parse_args()
assert a.bins >= 2 * a.J + 1, "the raster has to hold every drift hypothesis of a centred SV"

FS, BIN_STEP = 2.5e6, 100.0
RUN, LDS_MAX, CUS, CLOCK, LDS_B_PER_CLK = 5, 155 * 1024, 256, 2.4e9, 128.0      # csrc/dpe_cd_plan.h; MI355X: ds_read_b32
rng = np.random.Generator(np.random.PCG64(0))
ax = a.step * (np.arange(a.side) - (a.side - 1) // 2)
E, N = np.meshgrid(ax, ax, indexing="ij")
grid = np.stack([E.ravel(), N.ravel(), np.zeros(E.size)], axis=1)
P = grid.shape[0]
p0 = dpe.handoff.read_handoff(dpe.workload.HANDOFF_CSV)["X_ECEF"][:3].copy()
R = dpe.synth.enu2ecef_matrix(p0)
sv = []
for k in range(a.K):
    az, el, rg = rng.uniform(0, 2 * np.pi), np.radians(rng.uniform(10.0, 90.0)), rng.uniform(2.0e7, 2.5e7)
    d = rg * np.array([np.cos(el) * np.sin(az), np.cos(el) * np.cos(az), np.sin(el)])
    sv.append(dict(prn=k + 1, row=k, sat=p0 + R @ d, delay0=float(rng.uniform(0, a.M)), bin0=float(rng.uniform(a.J, a.bins - 1 - a.J))))
bins = BIN_STEP * (np.arange(a.bins) - (a.bins - 1) // 2)
dev = torch.device("cuda:0")
surf = torch.rand((a.K, a.bins, a.M), device=dev, generator=torch.Generator(device=dev).manual_seed(0))
cd = dpe.CollectiveDetector(FS, a.M, bins, grid, drift_half_width=a.J, max_sv=a.K)
arr = cd.sv_array(sv)
timer = dpe.engine.HipEventTimer()
times = []
for it in range(10):
    timer.start()
    for _ in range(a.repeat):
        cd.update(surf, arr, p0, R)
    timer.stop()
    times.append(timer.elapsed_ms() / a.repeat)
fix, _ = cd.results()
cd.close()
t = np.array(times[3:])
nJ = 2 * a.J + 1
terms = float(P) * nJ * a.M * a.K
n_runs = (a.M + RUN - 1) // RUN
in_lds = a.K * (a.M + RUN) * 4 <= LDS_MAX
bound_ms = float(P) * nJ * a.K * n_runs * (RUN + 1) * 4.0 / (LDS_B_PER_CLK * CUS * CLOCK) * 1e3

lines = [
    "K = %d SVs, M = %d, %d bins, J = %d, P = %d points (%d x %d, %.0f m): %.3g hypotheses, %.3g hypothesis x SV terms"
    % (a.K, a.M, a.bins, a.J, P, a.side, a.side, a.step, float(P) * nJ * a.M, terms),
    "update (tau, scan, finalize: three launches), HIP events around %d back-to-back updates, 3 warm-up windows, 7 timed:" % a.repeat,
    "    median %.4f ms (min %.4f, max %.4f) per update = %.3g hypothesis x SV per second" % (float(np.median(t)), t.min(), t.max(),
                                                                                             terms / (float(np.median(t)) * 1e-3)),
]
if in_lds:
    lines.append("    LDS-read bound of the tile shape (%d dword reads per %d terms, %d B/clk/CU, %d CUs, %.1f GHz): %.4f ms -> the update "
                 "runs at %.2f of it" % (RUN + 1, RUN, int(LDS_B_PER_CLK), CUS, CLOCK / 1e9, bound_ms, bound_ms / float(np.median(t))))
else:
    lines.append("    K rows of M + %d floats exceed a block's %d KB of LDS: rows are read from L2, the LDS-read bound does not apply" % (RUN, LDS_MAX // 1024))
lines.append("    arg-max of the noise surface: point %d, j %d, m %d, score %.6f" % (fix["point"], fix["j"], fix["m"], fix["score"]))

# residual against the fp64 specification, on the tests' parity cases
try:
    from tests import cd_world
    worst = 0.0
    for name in cd_world.RANDOM_CASES:
        c = cd_world.random_case(name)
        h = dpe.CollectiveDetector(c["fs"], c["M"], c["bins"], c["grid"], drift_half_width=c["J"], max_sv=c["K"])
        h.update(torch.from_numpy(c["surface"]).to(dev), c["sv"], c["p0"], c["R"])
        h.results()
        score, _ = h.read_map()
        h.close()
        r = float((np.abs(score.astype(np.float64) - c["ref"]["map_score"]) / cd_world.tolerance(c["ref"])).max())
        rel = float((np.abs(score.astype(np.float64) - c["ref"]["map_score"]) / np.maximum(c["ref"]["map_score"], c["ref"]["row_max"])).max())
        worst = max(worst, r)
        lines.append("    residual, case %-22s largest |GPU - fp64 specification| = %.2e of max(score, row maximum) = %.3f of the tolerance 2e-6"
                     % (name + ":", rel, r))
    lines.append("    largest residual over the cases: %.3f of the tolerance" % worst)
except ImportError as e:
    lines.append("    residual not measured: tests/cd_world.py not importable (%s)" % e)

text = "\n".join([dpe.engine.device_info()[0]] + lines)
print(text)
with open(a.out, "w") as f:
    f.write("Collective detection: one update at a user shape, and the residual against the fp64 specification\n"
            "(scripts/collective_time.py)\n\n" + text + "\n")
