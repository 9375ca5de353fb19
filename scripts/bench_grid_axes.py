"""Throughput of the grid-axes scan against the point-list scan on the same tensor grids (dpe_bcm_create_axes vs dpe_bcm_create).

Config R's stage shape (2.5 Msps x 20 ms, 8 SVs, 256 windows, L / B as bench.py) on the reference's default grids (Uniform 25^4
at 1 m for both manifolds, dpeflow.cpp:83-87) and on PyGNSS' spread grids; both handles score the SAME banks, alternating, after
warm-up.  Scan times are device events around the fused scan launch (dpe_bcm_profile); step times are host clocks around one
Update + results.  Then one 1.04e8-point arg-max-only window, which only the axes form can hold, and the closed loop of
dpe_flow --device-loop with and without --grid-axes.  One JSON document on stdout
(and in --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import navlab_dpe_sdr_amd as dpe  # noqa: E402


def med(x):
    return float(np.median(np.asarray(x)))


def device_loop_us(W, repeats):
    """dpe_flow --device-loop (one window per Update, cuChanMgr on the device) on the reference's default 25^4 grids, us per
    window with and without --grid-axes, alternating; the fixes of the two forms are compared too."""
    import re
    import subprocess
    import tempfile
    fs, S, K = 2.5e6, 50000, 8
    iq, _, _, _ = dpe.workload.build_windows(W, fs, S, K, seed=5, amp=200.0)
    d = tempfile.mkdtemp()
    dat = os.path.join(d, "s.dat")
    iq.tofile(dat)
    ho_path = os.path.join(d, "handoff.csv")
    with open(dpe.workload.HANDOFF_CSV) as f, open(ho_path, "w") as g:
        for line in f:
            g.write("bytes_read,0\n" if line.startswith("bytes_read") else line)
    exe = os.path.join(os.path.dirname(dpe.engine.LIB_PATH), "dpe_flow")
    us = {"points": [], "axes": []}
    rows = {}
    for _ in range(repeats):
        for k, extra in (("points", []), ("axes", ["--grid-axes"])):
            xo = os.path.join(d, "X_%s.csv" % k)
            r = subprocess.run([exe, "--samples", dat, "--handoff", ho_path, "--out", xo, "--iters", str(W), "--grid-dim", "25",
                                "--spacing", "1.0", "--device-loop"] + extra, capture_output=True, text=True, timeout=300, check=True)
            m = re.search(r"iterations, ([0-9.eE+-]+) us per iteration", r.stderr)
            us[k].append(float(m.group(1)))
            rows[k] = np.loadtxt(xo, delimiter=",")
    return dict(windows=W, repeats=repeats, us_per_window={k: med(v) for k, v in us.items()}, runs=us,
                max_fix_difference_m=float(np.abs(rows["axes"] - rows["points"]).max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--loop-windows", type=int, default=500)
    ap.add_argument("--loop-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    cfg = dpe.workload.CONFIG_R
    fs, S, K, L, B = cfg["fs"], cfg["S"], cfg["K"], cfg["L"], cfg["B"]
    W = a.windows
    iq, cs, ce, bw = dpe.workload.build_windows(a.distinct, fs, S, K, seed=0, amp=cfg["amp"])
    rep = (W + a.distinct - 1) // a.distinct
    iq, cs, ce, bw = (np.concatenate([x] * rep)[:W] for x in (iq, cs, ce, bw))
    bcs = dpe.BatchCorrScores(fs, samples_per_window=S, lag_half_width=L, bin_half_width=B, max_windows=W, max_channels=K)
    bcs.Start()
    bcs.Update(torch.from_numpy(iq).to("cuda:0"), cs)
    torch.cuda.synchronize()
    out = dict(config="R stage shape: %g sps x %d samples, %d SVs, %d windows, L=%d, B=%d" % (fs, S, K, W, L, B), steps=a.steps,
               device=dpe.engine.device_info()[0], grids={})

    def handle(pos, vel, W_, write_scores=True):
        m = dpe.BatchCorrManifold(fs, S, bcs.NumFFTPoints, pos, vel, lag_half_width=L, bin_half_width=B, max_windows=W_,
                                  max_channels=K, write_scores=write_scores)
        m.Start()
        return m

    grids = {"uniform25_1m": (dpe.GridAxes.uniform(25, 1.0), dpe.GridAxes.uniform(25, 1.0)),
             "pygnss_spread": dpe.GridAxes.pygnss_spread()}
    for name, (pa, va) in grids.items():
        hs = {"points": handle(pa.points(), va.points(), W), "axes": handle(pa, va, W)}
        scan = {k: [] for k in hs}
        step = {k: [] for k in hs}
        same = True
        for it in range(a.warmup + a.steps):
            res = {}
            for k, m in hs.items():          # alternating, same banks
                m.profile(True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.Update(bcs.CodeScores, bcs.CarrScores, bw, ce)
                res[k] = m.results()
                t1 = time.perf_counter()
                ms, n = m.profile(True)["bcm_scan"]
                if it >= a.warmup:
                    scan[k].append(ms / max(n, 1))
                    step[k].append((t1 - t0) * 1e3)
            same &= all(r["posIndex"] == q["posIndex"] and r["velIndex"] == q["velIndex"] for r, q in zip(res["points"], res["axes"]))
        out["grids"][name] = dict(points=pa.size, scan_ms={k: med(v) for k, v in scan.items()},
                                  update_results_ms={k: med(v) for k, v in step.items()},
                                  scan_ms_spread={k: [float(min(v)), float(max(v))] for k, v in scan.items()},
                                  argmax_indices_equal=bool(same))
        for m in hs.values():
            m.Stop()
    # one arg-max-only window on 101^4 = 1.04e8 points (as a point list: 1.6 GB on the device, 3.3 GB fp64 on the host)
    pa, va = dpe.GridAxes.uniform(101, 1.0), dpe.GridAxes.uniform(25, 1.0)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    m = handle(pa, va, 1, write_scores=False)
    torch.cuda.synchronize()
    grew = free0 - torch.cuda.mem_get_info()[0]
    t = []
    for it in range(a.warmup + a.steps):
        m.profile(True)
        m.Update(bcs.CodeScores, bcs.CarrScores, bw[:1], ce[:1])
        r = m.results()[0]
        ms, n = m.profile(True)["bcm_scan"]
        if it >= a.warmup:
            t.append(ms / max(n, 1))
    m.Stop()
    out["wide_window"] = dict(points=pa.size, create_device_bytes=int(grew), scan_ms=med(t), points_per_s=pa.size / (med(t) * 1e-3),
                              posIndex=int(r["posIndex"]), posScore=float(r["posScore"]))
    bcs.Stop()
    out["device_loop"] = device_loop_us(a.loop_windows, a.loop_repeats)
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
