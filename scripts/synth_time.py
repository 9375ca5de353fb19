#!/usr/bin/env python3
"""Timing behind profiles/synth.txt: the device synthesiser (engine.Synthesizer.windows, dpe_syn_windows) at config R's batch --
256 windows x 50 000 samples x 8 SVs -- and at config H's shape -- 128 x 500 000 x 12 -- beside dpe_sampleblock_upload of the same
bytes from pinned host memory (what a host-made batch costs to bring over) and one host synth.gen_iq window of R's shape.  One
process; every shape warmed up 3 times; HIP events on one stream around the C entry point, median of 10 (the host window: wall
clock, median of 3).  Noise on (sigma = 300): the full model.  Needs a GPU:  python scripts/synth_time.py [output file]"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import navlab_dpe_sdr_amd as dpe  # noqa: E402

assert torch.cuda.is_available(), "synth_time.py measures on a GPU: there is none"
ho = dpe.workload.extend_handoff(dpe.handoff.read_handoff(dpe.workload.HANDOFF_CSV), 12)
tm = dpe.engine.HipEventTimer()
lib = dpe.engine.lib()


def timed(fn):
    ms = []
    for _ in range(13):
        tm.start(); fn(); tm.stop()
        ms.append(tm.elapsed_ms())
    return float(np.median(ms[3:])), min(ms[3:]), max(ms[3:])


def chan_starts(cfg, W):
    X = np.array(ho["X_ECEF"], dtype=np.float64)
    cm = dpe.engine.ChanMgr.from_handoff(ho, cfg["S"] / cfg["fs"], cfg["K"])
    cs = np.zeros((W, cfg["K"]), dtype=dpe.engine.CHAN_START_DTYPE)
    for w in range(W):
        (cm.Start if w == 0 else cm.Update)(X, X, (0.0,))
        cs[w] = cm.outputs()[0]
    cm.Stop()
    return cs


lines = []
for name, cfg, W in (("R", dpe.workload.CONFIG_R, 256), ("H", dpe.workload.CONFIG_H, 128)):
    fs, S, K = cfg["fs"], cfg["S"], cfg["K"]
    cs = chan_starts(cfg, W)
    syn = dpe.Synthesizer(fs, max_segments=W, max_channels=K)
    out = torch.empty((W, 2 * S), dtype=torch.int16, device="cuda")
    flips = np.ones((W, K), dtype=bool)
    t = timed(lambda: syn.windows(S, cs, amp=cfg["amp"], sigma=300.0, flip=flips, seed=1, first_stream=0, out=out))
    t0 = timed(lambda: syn.windows(S, cs, amp=cfg["amp"], sigma=0.0, flip=flips, seed=1, first_stream=0, out=out))
    syn.close()
    n = W * S
    lines.append("%s  Synthesizer.windows %d x %d samples x %d SVs: median %.3f ms (min %.3f, max %.3f) = %.2f Gsample/s, %.1f GB/s written, "
                 "%.2f ps per sample and SV;  without noise (sigma = 0): %.3f ms" % (name, W, S, K, t[0], t[1], t[2], n / t[0] * 1e-6,
                                                                                   4 * n / t[0] * 1e-6, t[0] * 1e9 / (n * K), t0[0]))
    host = torch.empty((W, 2 * S), dtype=torch.int16).pin_memory()
    host.copy_(out)
    dst = torch.empty_like(out)
    up = timed(lambda: dpe.engine._check(lib.dpe_sampleblock_upload(C.c_void_p(dst.data_ptr()), C.c_void_p(host.data_ptr()), C.c_int64(n),
                                                                    dpe.engine._stream(None))))
    torch.cuda.synchronize()
    assert torch.equal(dst, out)
    lines.append("%s  dpe_sampleblock_upload of the same %d bytes (pinned): median %.3f ms (min %.3f, max %.3f) = %.1f GB/s;  generation / upload = %.2f"
                 % (name, 4 * n, up[0], up[1], up[2], 4 * n / up[0] * 1e-6, t[0] / up[0]))
    del host, dst, out
cfg = dpe.workload.CONFIG_R
ch = dpe.synth.random_channels(1, cfg["K"])
hs = []
for _ in range(3):
    a = time.perf_counter()
    dpe.synth.gen_iq(1, cfg["fs"], cfg["S"], ch, amp=cfg["amp"])
    hs.append((time.perf_counter() - a) * 1e3)
lines.append("host synth.gen_iq, ONE window of R's shape (%d samples x %d SVs, numpy, one thread): median %.2f ms, i.e. %.0f ms per 256 windows"
             % (cfg["S"], cfg["K"], float(np.median(hs)), 256 * float(np.median(hs))))
text = "\n".join([dpe.engine.device_info()[0]] + lines)
print(text)
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "synth.txt")
with open(out_path, "w") as f:
    f.write("Device synthesiser against the upload of the same bytes and the host generator (scripts/synth_time.py: HIP events on one\n"
            "stream around the C entry point, 3 warm-ups, median of 10)\n\n" + text + "\n")
