"""Closed-loop latency of the C++ flow (host/dpe_flow): one window per Update, fix fed back to the channel
manager, on a synthetic sample file.  Prints us per iteration for a 9^4 and the reference-default 25^4 grid: host-driven
loop (cuChanMgr / cuEKF on the host, the fix read back every window), the same with hipGraph replay, and --device-loop
(cuChanMgr on the device, nothing read back; rows must equal the host-driven loop's); with the filter, and with the filter's R from
the manifold moments (--measurement-cov 0.9,0.99), the device loop in both forms of that stage: the measurement kernel adding the
moments' block partials itself (the form kept) and bcm_moments_finish_kernel as a launch of its own in front (DPE_CHM_COV_TWO_LAUNCH=1).
DPE_LAT_ROWS=ekf runs the 25^4 filter rows alone; DPE_LAT_FLOW names another dpe_flow (a parent commit's build, which knows no
--measurement-cov: give it DPE_LAT_ROWS=ekf-plain)."""
import sys, os, subprocess, numpy as np, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import navlab_dpe_sdr_amd as dpe
W, fs, S, K = int(os.environ.get("DPE_LAT_WINDOWS", "200")), 2.5e6, 50000, 8
iq, _, _, _ = dpe.workload.build_windows(W, fs, S, K, seed=5, amp=200.0)
d = tempfile.mkdtemp()
dat = os.path.join(d, "s.dat"); iq.tofile(dat)
ho_path = os.path.join(d, "handoff.csv")
with open(dpe.workload.HANDOFF_CSV) as f, open(ho_path, "w") as g:
    for line in f:
        g.write("bytes_read,0\n" if line.startswith("bytes_read") else line)
exe = os.environ.get("DPE_LAT_FLOW") or os.path.join(os.path.dirname(dpe.engine.LIB_PATH), "dpe_flow")
COV = ["--measurement-cov", "0.9,0.99"]
plain = [(25, ["--ekf"], {}), (25, ["--device-loop", "--ekf"], {})]      # EnableEKF = true: the filter on the host / inside the measurement kernel
cov = [(25, ["--ekf"] + COV, {}), (25, ["--device-loop", "--ekf"] + COV, {}), (25, ["--device-loop", "--ekf"] + COV, {"DPE_CHM_COV_TWO_LAUNCH": "1"})]
rows_of = {"": [(9, [], {}), (9, ["--device-loop"], {}), (9, ["--graph"], {}), (25, [], {}), (25, ["--device-loop"], {}),
                (25, ["--device-loop", "--fix-lag", "2"], {}), (25, ["--graph"], {})] + plain + cov,
           "ekf": plain + cov, "ekf-plain": plain}[os.environ.get("DPE_LAT_ROWS", "")]
base = {}
for dim, extra, env in rows_of:
    r = subprocess.run([exe, "--samples", dat, "--handoff", ho_path, "--out", os.path.join(d, "X.csv"), "--iters", str(W), "--grid-dim", str(dim), "--spacing", "1.0"] + extra,
                       capture_output=True, text=True, timeout=120, env=dict(os.environ, **env))
    print(dim, extra, env or "", [l for l in r.stderr.splitlines() if "iterations" in l or "LoadFlow" in l or "second half" in l])
    rows = np.loadtxt(os.path.join(d, "X.csv"), delimiter=",")
    ho = dpe.handoff.read_handoff(ho_path)
    print("  max |fix - truth| m:", np.abs(rows[:, :3] - ho["X_ECEF"][:3]).max(), "rows", rows.shape)
    key = (dim, "--ekf" in extra, "--measurement-cov" in extra)
    if "--device-loop" not in extra and "--graph" not in extra:
        base[key] = rows
    elif extra[0] == "--device-loop":
        print("  max |fix - host-driven loop| m:", np.abs(rows - base[key]).max())
