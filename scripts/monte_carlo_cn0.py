#!/usr/bin/env python3
"""RMSE against C/N0 over noise realisations made on the device (pipeline.run_monte_carlo): how DPE work is usually reported, and
the reference's own manual check (cudarecv/src/main.cu:105-280) with the noise, not only the initial offset, varied.  Config R's
shape: 2.5 Msps x 20 ms windows, 8 SVs.  Every level draws `realisations` windows from the device synthesiser (engine.Synthesizer:
no host synthesis, no host-to-device copy), and one stage-1 and one manifold update run over the batch.

The grids: the manifold interpolates the sample-rate correlation linearly, so the ML fix can only move between nodes
(scripts/monte_carlo.py) -- a +-12 m grid sees one node.  Here the position grid is PyGNSS' spread grid (+-110 m, 25^4 points,
receiver.py:995-1026) and the grid centre is offset from the truth by `offset` metres east, so the truth is not the centre.

    python scripts/monte_carlo_cn0.py [realisations=64] [offset_m=35] [seed=1]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import navlab_dpe_sdr_amd as dpe  # noqa: E402


def main():
    n_real = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    offset = float(sys.argv[2]) if len(sys.argv) > 2 else 35.0
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    cfg = dpe.workload.CONFIG_R
    fs, S, K = cfg["fs"], cfg["S"], cfg["K"]
    ho = dpe.handoff.read_handoff(dpe.workload.HANDOFF_CSV)
    pos, vel = dpe.synth.spread_grid()
    X = ho["X_ECEF"]
    up = X[:3] / np.linalg.norm(X[:3])
    east = np.cross([0.0, 0.0, 1.0], up)
    east /= np.linalg.norm(east)
    levels = np.arange(50.0, 19.0, -3.0)
    rows = dpe.pipeline.run_monte_carlo(ho, fs, S, K, pos, vel, levels, n_real, seed, init_delta=offset * east, weighted_mean=True)
    print("%s: S = %d, K = %d, grids %d + %d points, %d realisations per level, centre %.1f m east of the truth, sigma = 300"
          % (dpe.engine.device_info()[0], S, K, pos.shape[0], vel.shape[0], n_real, offset))
    print("C/N0    amp     ML: E      N      U     3-D   clock   vel 3-D  drift  |  mean: 3-D   clock   | out of window")
    for r in rows:
        print("%4.1f  %6.2f  %7.2f %6.2f %6.2f  %6.2f  %6.2f   %6.3f %6.3f  |      %6.2f  %6.2f   | %d"
              % (r["cn0_dbhz"], r["amp"], r["rmse_enu"][0], r["rmse_enu"][1], r["rmse_enu"][2], r["rmse_3d"], r["rmse_clock"], r["rmse_vel"],
                 r["rmse_drift"], r["mean_rmse_3d"], r["mean_rmse_clock"], int(r["pos_out_of_window"].max() + r["vel_out_of_window"].max())))


if __name__ == "__main__":
    main()
