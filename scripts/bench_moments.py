"""Time of the manifold-moments stage (dpe_bcm_moments) behind the scan at config R's shape: 256 windows, Uniform 25^4 grids
at 1 m for both manifolds (point lists), 8 SVs, L / B as bench.py.  Four timings between HIP events (dpe_event_*) on the launch
stream, median of --steps after --warmup:
  (a) Update alone            (b) Update + moments at rho = 0            (c) Update + moments at rho = 0.99            (d) moments alone
(d) is taken at both rho.  The stage's algorithmic traffic is the 4-byte scores, 4 G W 2 bytes; it is printed over (d) next to
the measured copy / triad ceiling (dpe_hbm_ceiling).
--update-only times (a) alone and binds no moments symbol: with DPE_LIB_PATH pointing at the parent commit's library it is the
yardstick for (a) in the same session."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import navlab_dpe_sdr_amd as dpe  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--update-only", action="store_true")
    a = ap.parse_args()
    eng = dpe.engine
    if a.update_only:
        eng.EXPORTS = [e for e in eng.EXPORTS if not e.startswith("dpe_bcm_moments")]
    import torch
    torch.cuda.set_device(0)
    cfg = dpe.workload.CONFIG_R
    fs, S, K, L, B, W = cfg["fs"], cfg["S"], cfg["K"], cfg["L"], cfg["B"], a.windows
    iq, cs, ce, bw = dpe.workload.build_windows(a.distinct, fs, S, K, seed=0, amp=cfg["amp"])
    rep = (W + a.distinct - 1) // a.distinct
    iq, cs, ce, bw = (np.concatenate([x] * rep)[:W] for x in (iq, cs, ce, bw))
    bcs = dpe.BatchCorrScores(fs, samples_per_window=S, lag_half_width=L, bin_half_width=B, max_windows=W, max_channels=K)
    bcs.Start()
    bcs.Update(torch.from_numpy(iq).to("cuda:0"), cs)
    grid = dpe.GridAxes.uniform(25, 1.0).points()
    m = dpe.BatchCorrManifold(fs, S, bcs.NumFFTPoints, grid, grid, lag_half_width=L, bin_half_width=B, max_windows=W, max_channels=K)
    m.Start()
    torch.cuda.synchronize()
    G = grid.shape[0]
    timer = eng.HipEventTimer()
    stream = eng._stream(None)

    def update():
        m.Update(bcs.CodeScores, bcs.CarrScores, bw, ce)

    def moments(rho):
        c = eng.BcmMomentsConfig((C.c_double * 2)(rho, rho), None, None, None, 0, 0, 0, 0)
        eng._check(eng.lib().dpe_bcm_moments(m._h, C.byref(c), stream))

    def timed(*calls):
        t = []
        for it in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            timer.start()
            for f in calls:
                f()
            timer.stop()
            ms = timer.elapsed_ms()
            if it >= a.warmup:
                t.append(ms)
        return float(np.median(t)), float(min(t)), float(max(t))

    print("device %s; config R stage shape: %d windows, 2 x %d points, %d SVs, L=%d B=%d; median [min, max] of %d after %d, ms"
          % (eng.device_info()[0], W, G, K, L, B, a.steps, a.warmup))
    print("library %s" % os.path.basename(eng.LIB_PATH))
    print("(a) Update alone                  %.4f [%.4f, %.4f]" % timed(update))
    if not a.update_only:
        print("(b) Update + moments rho = 0      %.4f [%.4f, %.4f]" % timed(update, lambda: moments(0.0)))
        print("(c) Update + moments rho = 0.99   %.4f [%.4f, %.4f]" % timed(update, lambda: moments(0.99)))
        update()
        nbytes = 4.0 * G * W * 2
        for rho in (0.0, 0.99):
            d = timed(lambda: moments(rho))
            r = m.moments(rho)
            print("(d) moments alone, rho = %-4g     %.4f [%.4f, %.4f]   %.0f MB of scores -> %.0f GB/s; nAbove of window 0: %s"
                  % ((rho,) + d + (nbytes / 1e6, nbytes / d[0] / 1e6, list(r[0]["nAbove"]))))
        copy, triad = eng.hbm_ceiling()
        print("dpe_hbm_ceiling: copy %.0f GB/s, triad %.0f GB/s" % (copy, triad))
    m.Stop()
    bcs.Stop()


if __name__ == "__main__":
    main()
