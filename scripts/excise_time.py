#!/usr/bin/env python3
"""Timing behind profiles/excise.txt: the excisor (engine.Excisor, dpe_ix_process) on one MI355X, one call over a record of 2^26
complex samples, int16 in and out, at the frame lengths N = 256, 1024 and 4096 (threshold 10, guard 1).  The record is noise
within +-2047 under a tone of amplitude 6000, so that every frame excises something.

HIP events around a window of REPEAT back-to-back calls on one stream (the call is asynchronous; nothing is read back inside the
window), 3 warm-up windows, then 7 timed ones: median, min and max per call.  Beside the time: samples per second, and the ratio
of the stream-copy bound (bytes in + bytes out) / 6.2 TB/s to the time.  For scale, the fp64 numpy specification (tests/ix_ref.py)
on one host thread over 2^20 samples of the same record, scaled to the record.
Needs a GPU:  python scripts/excise_time.py [--log2n 26 --repeat 5] [--out file]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):      # the host figure is for ONE thread: set before numpy loads
    os.environ[_v] = "1"
import numpy as np  # noqa: E402
import torch  # noqa: E402
import navlab_dpe_sdr_amd as dpe  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2n", type=int, default=26)
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "excise.txt"))
a = ap.parse_args()

COPY_BPS = 6.2e12
S = 1 << a.log2n
dev = torch.device("cuda:0")
gen = torch.Generator(device=dev).manual_seed(0)
n = torch.arange(S, device=dev, dtype=torch.float64)
x = torch.randint(-2047, 2048, (S, 2), device=dev, generator=gen, dtype=torch.int16).to(torch.float64)
ang = 2.0 * np.pi * torch.remainder(0.1837 * n, 1.0)
x[:, 0] += torch.round(6000.0 * torch.cos(ang))
x[:, 1] += torch.round(6000.0 * torch.sin(ang))
x = x.to(torch.int16).reshape(-1).contiguous()
del n, ang
out = torch.empty(2 * S, dtype=torch.int16, device=dev)
timer = dpe.engine.HipEventTimer()
lines = []
for N in (256, 1024, 4096):
    ix = dpe.Excisor(N, 10.0, guard=1)
    times = []
    for it in range(10):
        timer.start()
        for _ in range(a.repeat):
            ix.process(x, 0, 0, S, record_length=S, out=out)
        timer.stop()
        times.append(timer.elapsed_ms() / a.repeat)
    st = ix.stats()
    t = np.array(times[3:])
    med = float(np.median(t))
    bound_ms = 8.0 * S / COPY_BPS * 1e3
    lines.append("N = %d, hop %d, %d hops per block, %d B of LDS, 2^%d samples (%.0f MB in, %.0f MB out):" % (N, ix.hop, ix.hops_per_block, ix.lds_bytes,
                                                                                                        a.log2n, 4.0 * S / 1e6, 4.0 * S / 1e6))
    lines.append("    median %.4f ms (min %.4f, max %.4f) per call = %.3g samples per second; stream-copy bound %.4f ms = %.3f of the time"
                 % (med, t.min(), t.max(), S / (med * 1e-3), bound_ms, bound_ms / med))
    lines.append("    %d frames counted, %.2f %% of their bins excised, %d components clipped" % (st["frames"], 100.0 * st["excisedBins"] / (st["frames"] * N),
                                                                                              st["clipped"]))
    try:
        from tests import ix_ref
        n_h = min(S, 1 << 20)
        xh = ix_ref.from_i16(x[: 2 * n_h].cpu().numpy())
        t0 = time.perf_counter()
        y = ix_ref.quantise(ix_ref.interleave(ix_ref.excise(xh, 0, n_h, 0, n_h - N, N, 10.0, 1)))
        dt = time.perf_counter() - t0
        got = out[: y.size].cpu().numpy()
        off = int(np.abs(got.astype(np.int32) - y).max())
        frac = float((got != y).mean())
        lines.append("    host numpy specification, one thread: %.2f s for 2^20 samples = %.3g samples per second (%.0f x the device's time per sample); "
                     "device against it over those outputs: at most %d apart, %.4f %% of the components differ (undecided bins)"
                     % (dt, n_h / dt, (dt / n_h) / (med * 1e-3 / S), off, 100.0 * frac))
    except ImportError as e:
        lines.append("    host time not measured: tests/ix_ref.py not importable (%s)" % e)
    ix.close()

text = "\n".join([dpe.engine.device_info()[0]] + lines)
print(text)
with open(a.out, "w") as f:
    f.write("Interference excision: int16 I/Q to int16 I/Q, one call over the record per frame length (scripts/excise_time.py)\n\n" + text + "\n")
