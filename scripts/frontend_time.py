#!/usr/bin/env python3
"""Timing behind profiles/frontend.txt: the front end (engine.FrontEnd, dpe_fe_convert) on one MI355X, one call over a record of
2^26 input samples per case:

    I16C  25 Msps -> 2.5 Msps   D = 10, T = 81, zero IF          (and the same with a 1 MHz IF: complex taps)
    I8R   D = 4, T = 33, IF fs / 4
    P2R   D = 4, T = 33, IF fs / 4

HIP events around a window of REPEAT back-to-back calls on one stream (the call is asynchronous; nothing is read back inside the
window), 3 warm-up windows, then 7 timed ones: median, min and max per call.  Beside the time: input samples per second, and the
ratio of the stream-copy bound (bytes in + bytes out) / 6.2 TB/s (README, round 1) to the time.  For scale, the fp64 numpy
specification (tests/fe_ref.py) on one host thread over 2^22 samples of the same case, scaled to the record.  The residual against
the specification is measured on the parity table of tests/fe_world.py and printed as a fraction of the tests' tolerance.
Needs a GPU:  python scripts/frontend_time.py [--log2n 26 --repeat 20] [--out file]"""
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
from navlab_dpe_sdr_amd import frontend  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2n", type=int, default=26)
ap.add_argument("--repeat", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontend.txt"))
a = ap.parse_args()

COPY_BPS = 6.2e12
N = 1 << a.log2n
CASES = (("I16C", 25e6, 10, 0.0, 0.5), ("I16C", 25e6, 10, 1.0e6, 0.5), ("I8R", 10e6, 4, 2.5e6, 1.0), ("P2R", 10e6, 4, 2.5e6, 20.0))
dev = torch.device("cuda:0")
gen = torch.Generator(device=dev).manual_seed(0)
timer = dpe.engine.HipEventTimer()
lines = []
for fmt, fs, D, f_if, gain in CASES:
    h = frontend.design_lowpass(D)
    fe = dpe.FrontEnd(fs, fmt, D, h, gain=gain, f_if=f_if)
    n_bytes = N * fe.bytes_num // fe.bytes_den
    if fmt == "I16C":
        raw = torch.randint(-2047, 2048, (2 * N,), device=dev, generator=gen, dtype=torch.int16)
    else:
        raw = torch.randint(0, 256, (n_bytes,), device=dev, generator=gen, dtype=torch.uint8)
    n_out = N // D
    out = torch.empty(2 * n_out, dtype=torch.int16, device=dev)
    times = []
    for it in range(10):
        timer.start()
        for _ in range(a.repeat):
            fe.convert(raw, 0, 0, n_out, record_length=N, raw_count=N, out=out)
        timer.stop()
        times.append(timer.elapsed_ms() / a.repeat)
    clipped = fe.clipped()
    t = np.array(times[3:])
    med = float(np.median(t))
    bound_ms = (n_bytes + 4.0 * n_out) / COPY_BPS * 1e3
    lines.append("%-5s fs %.1f Msps, D = %d, T = %d, IF %.2f MHz, 2^%d input samples (%.0f MB in, %.0f MB out), tile %d outputs, %d B of LDS:"
                 % (fmt, fs / 1e6, D, h.size, f_if / 1e6, a.log2n, n_bytes / 1e6, 4.0 * n_out / 1e6, fe.tile_outputs, fe.lds_bytes))
    lines.append("    median %.4f ms (min %.4f, max %.4f) per call = %.3g input samples per second; stream-copy bound %.4f ms = %.3f of the time"
                 % (med, t.min(), t.max(), N / (med * 1e-3), bound_ms, bound_ms / med))
    # the host's fp64 specification on one thread, 2^22 samples of this case
    try:
        from tests import fe_ref
        n_h = min(N, 1 << 22)
        raw_h = raw[: n_h * fe.bytes_num // fe.bytes_den // raw.element_size()].cpu().numpy().view(np.uint8)
        t0 = time.perf_counter()
        x = fe_ref.decode(fmt, raw_h, 0, n_h)
        y = fe_ref.quantise(fe_ref.convert(x, 0, n_h, 0, n_h // D, D, h, gain, fe.delta))
        dt = time.perf_counter() - t0
        got = out[: 2 * (n_h // D - h.size)].cpu().numpy()
        off = int(np.abs(got.astype(np.int32) - y[: got.size]).max())
        lines.append("    host numpy specification, one thread: %.2f s for 2^22 samples = %.3g samples per second (%.0f x the device's time per sample); "
                     "device against it over those outputs: at most %d apart; %d components clipped"
                     % (dt, n_h / dt, (dt / n_h) / (med * 1e-3 / N), off, clipped))
    except ImportError as e:
        lines.append("    host time not measured: tests/fe_ref.py not importable (%s)" % e)
    fe.close()
    del raw, out

# residual against the fp64 specification, on the tests' parity table
try:
    from tests import fe_ref, fe_world
    worst, where = 0.0, None
    for i in range(len(fe_world.PARITY)):
        c = fe_world.parity_case(i)
        fe = dpe.FrontEnd(fe_world.FS, c["fmt"], c["D"], c["h"], gain=c["gain"], f_if=c["f_if"], out_f32=True)
        raw = torch.from_numpy(c["raw"].copy()).to(dev)
        got = fe.convert(raw, c["raw_first"], c["out_first"], c["out_count"], raw_count=c["raw_count"]).cpu().numpy().astype(np.float64)
        fe.close()
        r = float(np.abs(got - fe_ref.interleave(c["y"])).max() / c["tol"])
        if r > worst:
            worst, where = r, fe_world.PARITY[i]
    lines.append("residual of the fp32 output against the fp64 specification over the %d parity cases: at most %.3f of the tolerance "
                 "(2 T + 16) 2^-24 gain sum|h| max|x|, at %s" % (len(fe_world.PARITY), worst, (where,)))
except ImportError as e:
    lines.append("residual not measured: tests/fe_world.py not importable (%s)" % e)

text = "\n".join([dpe.engine.device_info()[0]] + lines)
print(text)
with open(a.out, "w") as f:
    f.write("Front end: raw record bytes to baseband int16 I/Q, one call per case, and the residual against the fp64 specification\n"
            "(scripts/frontend_time.py)\n\n" + text + "\n")
