#!/usr/bin/env python3
"""Timing behind profiles/joint_scan.txt: the joint scan of four receivers x 8 SVs over the two 25^4-point grids, 256 windows
(engine.JointManifold, one launch), against the composed form the single-receiver entry points allow: four dpe_bcm_update calls
with writeScores = 1, then a sum over the four rows and an arg-max per manifold.  HIP events, 3 warm-ups, median of 10.  The
banks hold noise: the scan's time does not depend on their values (bank half-widths of config R, wide enough for every index).
Writes profiles/joint_scan.txt, with the register figures of the scan kernels read from the compiler's own remarks
(hipcc --offload-arch=gfx950 -O3 -std=c++17 -Rpass-analysis=kernel-resource-usage -c csrc/dpe_bcm.hip, device pass only).
Needs a GPU and hipcc:  python scripts/joint_scan_time.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import navlab_dpe_sdr_amd as dpe  # noqa: E402

N, K, W, G = 4, 8, 256, 390625
cfg = dpe.workload.CONFIG_R
FS, S = cfg["fs"], cfg["S"]
Cf = dpe.engine.carr_fft_len(S)
pos = dpe.synth.rand_grid(3, G)
vel = dpe.synth.rand_grid(4, G, half=(6.0, 6.0, 6.0, 3.0))
L, B = dpe.pipeline.bank_half_widths(pos, vel, FS, Cf)
ho = dpe.handoff.read_handoff(dpe.workload.HANDOFF_CSV)


class DevView:
    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = dict(shape=shape, typestr="<f4", data=(int(ptr), False), version=2)


dev = torch.device("cuda:0")
ce, bw, code, carr = [], [], [], []
for r in range(N):
    X = np.array(ho["X_ECEF"], dtype=np.float64)
    X[:3] += 0.7 * r
    cm = dpe.engine.ChanMgr.from_handoff(ho, S / FS, K)
    e_all, w_all = np.zeros((W, K), dtype=dpe.engine.CHAN_END_DTYPE), np.zeros(W, dtype=dpe.engine.BCM_WINDOW_DTYPE)
    for w in range(W):
        (cm.Start if w == 0 else cm.Update)(X, X, (0.0,))
        _s, e, win = cm.outputs()
        e_all[w], w_all[w] = e, win[0]
    cm.Stop()
    if r:
        w_all["enu2ecef"] = bw[0]["enu2ecef"]
    ce.append(e_all)
    bw.append(w_all)
    g = torch.Generator(device=dev).manual_seed(r)
    code.append(torch.randn((W, K, 2 * L + 1, 2), device=dev, generator=g))
    carr.append(torch.randn((W, K, 2 * B + 1, 2), device=dev, generator=g))

joint = dpe.JointManifold(FS, S, Cf, pos, vel, N, N * K, lag_half_width=L, bin_half_width=B, max_windows=W, max_channels=K)
joint.Start()
rx = joint.pack([[dict(code=code[r][w].data_ptr(), carr=carr[r][w].data_ptr(), win=bw[r][w], chan=ce[r][w]) for r in range(N)] for w in range(W)])   # packed once: the timed call is the C entry point
singles = []
for r in range(N):
    h = dpe.BatchCorrManifold(FS, S, Cf, pos, vel, lag_half_width=L, bin_half_width=B, max_windows=W, max_channels=K)
    h.Start()
    singles.append(h)
rows = [(torch.as_tensor(DevView(h.PosScores, (W, h.PosScoresPitch)), device=dev), torch.as_tensor(DevView(h.VelScores, (W, h.VelScoresPitch)), device=dev))
        for h in singles]
tm = dpe.engine.HipEventTimer()


def run_joint():
    joint.Update(rx)


def run_composed():
    for r, h in enumerate(singles):
        h.Update(code[r], carr[r], bw[r], ce[r])
    out = []
    for m in range(2):
        s = rows[0][m] + rows[1][m]
        s += rows[2][m]
        s += rows[3][m]
        out.append(torch.argmax(s[:, :G], dim=1))
    return out


def timed(fn):
    ms = []
    for _ in range(13):
        tm.start(); fn(); tm.stop()
        ms.append(tm.elapsed_ms())
    return float(np.median(ms[3:])), min(ms[3:]), max(ms[3:])


lines = []
for own in (True, False):
    joint.set_own_keys(own)
    t = timed(run_joint)
    lines.append("joint launch, own keys %s: median %.3f ms (min %.3f, max %.3f)" % ("on" if own else "off", *t))
    if own:
        tj = t[0]
tc = timed(run_composed)
lines.append("composed (4 x dpe_bcm_update with writeScores, sum of 4 rows, arg-max, both manifolds): median %.3f ms (min %.3f, max %.3f)" % tc)
lines.append("composed / joint (own keys on): %.2f" % (tc[0] / tj))
# the two forms agree on the arg-max
joint.set_own_keys(True)
run_joint()
res = joint.results()
am = run_composed()
torch.cuda.synchronize()
same = sum(int(res[w]["posIndex"] == int(am[0][w]) and res[w]["velIndex"] == int(am[1][w])) for w in range(W))
lines.append("windows on which the two forms give the same arg-max pair: %d of %d" % (same, W))
hdr = "%s: %d receivers x %d SVs, grids %d + %d points, %d windows, L = %d, B = %d" % (dpe.engine.device_info()[0], N, K, G, G, W, L, B)


def register_figures():
    """VGPRs / SGPRs / scratch / waves per SIMD of the LP = 1 scan kernels, from the compiler's resource-usage remarks."""
    import re
    import subprocess
    pkg = os.path.dirname(dpe.engine.LIB_PATH)
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-Wno-pass-failed", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", "csrc/dpe_bcm.hip", "-o", os.devnull]
    err = subprocess.run(cmd, cwd=pkg, capture_output=True, text=True).stderr
    out = ["registers: " + " ".join(cmd[1:])]
    for blk in re.split(r"(?=remark: Function Name: )", err):
        m = re.search(r"Function Name: (\S+)", blk)
        if not m:
            continue
        for tag, label in (("bcm_scan_joint_kernelILi1ELb1ELb1ELb1E", "bcm_scan_joint_kernel<1, clamp, clamp, OWN>"),
                           ("bcm_scan_joint_kernelILi1ELb1ELb1ELb0E", "bcm_scan_joint_kernel<1, clamp, clamp, no OWN>"),
                           ("bcm_scan_joint_kernelILi1ELb0ELb0ELb1E", "bcm_scan_joint_kernel<1, no clamp, no clamp, OWN>"),
                           ("bcm_scan_joint_kernelILi1ELb0ELb0ELb0E", "bcm_scan_joint_kernel<1, no clamp, no clamp, no OWN>"),
                           ("bcm_scan_kernelILi1ELb1ELb1ELb0ELb0E", "bcm_scan_kernel<1, clamp, clamp>"),
                           ("bcm_scan_kernelILi1ELb0ELb0ELb0ELb0E", "bcm_scan_kernel<1, no clamp, no clamp>")):
            if tag in m.group(1):
                f = {k: re.search(k + r": (\d+)", blk) for k in ("VGPRs", "SGPRs", r"ScratchSize \[bytes/lane\]", r"Occupancy \[waves/SIMD\]")}
                out.append("  %-52s %s VGPRs, %s SGPRs, scratch %s B/lane, %s waves per SIMD" % ((label,) + tuple(v.group(1) if v else "?" for v in f.values())))
    return out


text = "\n".join([hdr] + lines + ["this shape runs the unclamped variants (every index provably inside the banks)"] + register_figures())
print(text)
prof = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "joint_scan.txt")
with open(prof, "w") as f:
    f.write("Joint scan of several receivers against the composed single-receiver form (scripts/joint_scan_time.py: HIP events around the\n"
            "C entry points, 3 warm-ups, median of 10; banks hold noise, the receiver array is packed once outside the timed call).\n\n" + text + "\n")
