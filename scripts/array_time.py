#!/usr/bin/env python3
"""Timing behind profiles/array.txt: the array combiner (engine.ArrayCombiner, dpe_arr_process) on one MI355X, one call over a
record of 2^26 complex samples per element, int16 in and out, power inversion (one constraint, reference element 0, loading 1e-3),
for M = 4 and 8 elements at the block lengths L = 256, 1024 and 16384.  Each element is noise within +-2047 plus one common
wide-band interferer of sigma 6000 per component with a phase per element.

HIP events around a window of REPEAT back-to-back calls on one stream (the call is asynchronous; nothing is read back inside the
window), 3 warm-up windows, then 7 timed ones: median, min and max per call.  Beside the time: samples per second, and the ratio
of the stream-copy bound (M + B) 4 bytes 2^26 / 6.2 TB/s to the time.  To tell the three parts of the kernel apart the same record
is also timed through dpe_arr_analyse with no result buffer (pass 1 and the solve, no pass 2).
Needs a GPU:  python scripts/array_time.py [--log2n 26 --repeat 5] [--out file]"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import navlab_dpe_sdr_amd as dpe  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2n", type=int, default=26)
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "array.txt"))
a = ap.parse_args()

COPY_BPS = 6.2e12
S = 1 << a.log2n
dev = torch.device("cuda:0")
gen = torch.Generator(device=dev).manual_seed(0)
jam = 6000.0 * torch.randn((S, 2), device=dev, generator=gen, dtype=torch.float32)
rows = []
for e in range(8):
    ph = 2.0 * np.pi * 0.37 * e + 0.2 * e * e
    c, s = float(np.cos(ph)), float(np.sin(ph))
    x = torch.randint(-2047, 2048, (S, 2), device=dev, generator=gen, dtype=torch.int16).to(torch.float32)
    x[:, 0] += c * jam[:, 0] - s * jam[:, 1]
    x[:, 1] += s * jam[:, 0] + c * jam[:, 1]
    rows.append(torch.clamp(torch.round(x), -32768, 32767).to(torch.int16).reshape(-1).contiguous())
    del x
del jam
out = [torch.empty(2 * S, dtype=torch.int16, device=dev)]
timer = dpe.engine.HipEventTimer()
lib = dpe.engine.lib()


def timed(call):
    times = []
    for it in range(10):
        timer.start()
        for _ in range(a.repeat):
            call()
        timer.stop()
        times.append(timer.elapsed_ms() / a.repeat)
    return np.array(times[3:])


lines = []
for M in (4, 8):
    for L in (256, 1024, 16384):
        arr = dpe.ArrayCombiner(M, L)
        t = timed(lambda: arr.process(rows[:M], 0, 0, S, record_length=S, out=out))
        st = arr.stats()
        ptrs = (C.c_void_p * M)(*[r.data_ptr() for r in rows[:M]])
        stream = dpe.engine._stream(None)

        def solve_only():
            dpe.engine._check(lib.dpe_arr_analyse(arr._h, ptrs, C.c_int64(0), C.c_int64(S), C.c_int64(S), C.c_int64(0), C.c_int64(min(S // L, 1 << 24)),
                                                  None, None, None, stream))
        part = S / (min(S // L, 1 << 24) * L)                    # an analyse call takes 2^24 blocks at most
        t1 = timed(solve_only) * part
        med, med1 = float(np.median(t)), float(np.median(t1))
        bound_ms = (M + 1) * 4.0 * S / COPY_BPS * 1e3
        rms = float(torch.sqrt(2.0 * torch.mean(out[0][: 1 << 22].double() ** 2)))
        lines.append("M = %d, L = %d, %d blocks per workgroup, %d B of LDS, 2^%d samples per element (%.0f MB in, %.0f MB out):"
                     % (M, L, arr.blocks_per_unit, arr.lds_bytes, a.log2n, M * 4.0 * S / 1e6, 4.0 * S / 1e6))
        lines.append("    median %.4f ms (min %.4f, max %.4f) per call = %.3g samples per second; stream-copy bound %.4f ms = %.3f of the time"
                     % (med, t.min(), t.max(), S / (med * 1e-3), bound_ms, bound_ms / med))
        lines.append("    covariance and solve alone (analyse, nothing written): median %.4f ms = %.2f of the call" % (med1, med1 / med))
        lines.append("    %d blocks counted, %d fallback, %d components clipped; output rms %.0f" % (st["blocks"], st["fallbackBlocks"], st["clipped"], rms))
        arr.close()

text = "\n".join([dpe.engine.device_info()[0]] + lines)
print(text)
with open(a.out, "w") as f:
    f.write("Array combiner: M element streams of int16 I/Q to one, power inversion, one call over the record (scripts/array_time.py)\n\n" + text + "\n")
