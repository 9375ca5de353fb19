"""Collective detection's host-side planning (csrc/dpe_cd_plan.h) without a GPU: host/test_cd_plan.cpp, built with the host
compiler, checks the launch plan's properties itself (runs cover a row exactly once, the wrap pad covers what a run may read, the LDS
form is chosen exactly where K rows fit, the grid of blocks covers every point) and evaluates plans, predictions and refusals for
the cases written here: plans are held to the table below, predictions to tests/cd_ref.py's numpy restatement on oracle.sat_pos
(delay0 to 1e-6 sample, bin0 to 1e-6 bin), refusals to their messages."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import cd_ref, cd_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "navlab-dpe-sdr_amd", "host", "test_cd_plan.cpp")

# (M, K, J, P) -> run, runs per row, pitch, rows in LDS, LDS bytes, nJ, blocks per j, points per block
PLAN_TABLE = {
    (2500, 8, 10, 1681): (5, 500, 2505, 1, 80160, 21, 48, 36),       # the shape scripts/collective_time.py times: two blocks per CU
    (2500, 8, 2, 49): (5, 500, 2505, 1, 80160, 5, 49, 1),
    (2500, 15, 0, 1): (5, 500, 2505, 1, 150300, 1, 1, 1),
    (2500, 16, 2, 1): (5, 500, 2505, 0, 0, 5, 1, 1),                 # 160 320 B: over a block's 155 KB, rows from L2
    (5000, 7, 0, 49): (5, 1000, 5005, 1, 140140, 1, 49, 1),
    (5000, 8, 2, 5): (5, 1000, 5005, 0, 0, 5, 5, 1),
    (5000, 16, 0, 49): (5, 1000, 5005, 0, 0, 1, 49, 1),
    (2046, 4, 32, 131): (5, 410, 2051, 1, 32816, 65, 15, 9),         # 2 046 = 409 runs and one of a single delay
    (2046, 1, 0, 1031): (5, 410, 2051, 1, 8204, 1, 1024, 2),
    (4000, 9, 32, 65536): (5, 800, 4005, 1, 144180, 65, 15, 4370),
    (16, 16, 0, 3): (5, 4, 21, 1, 1344, 1, 3, 1),
}


def _cxx():
    for c in ("g++", "c++", "clang++"):
        if shutil.which(c):
            return shutil.which(c)
    return None


def _build(tmp_path):
    if _cxx() is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "test_cd_plan")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", SRC, "-o", exe], check=True)
    return exe


THREADS, FLUSH, LDS_MAX = 512, 8, 155 * 1024       # kCdThreads, kCdFlush, kCdLdsMax

# What each shape of tests/cd_world.py's second table is there to reach, in cd_plan's own values.
# name -> (rows in LDS, LDS bytes, runs per row, blocks per j, points per block)
NEW_CASE_PLANS = {
    "k3": (1, 3060, 50, 9, 1), "k5": (1, 5100, 50, 9, 1), "k7": (1, 7140, 50, 9, 1), "k13": (1, 13260, 50, 9, 1),
    "lds-4092-k2": (1, 32776, 819, 5, 1),            # LDS form, 819 runs: lanes 0..306 take a second run
    "lds-32768-k1": (1, 131092, 6554, 3, 1),         # the M maximum: 13 passes (12 full ones and 410 runs)
    "lds-2475-k16": (1, 158720, 495, 3, 1),          # the limit itself ...
    "l2-2476-k16": (0, 0, 496, 3, 1),                # ... and 64 B over it
    "lds-4955-k8": (1, 158720, 991, 3, 1),
    "runs-512": (1, 20520, 512, 5, 1),
    "runs-513": (1, 20528, 513, 5, 1),
    "m-16": (1, 168, 4, 9, 1),
    "walk-20": (1, 552, 13, 15, 20),
    "walk-64": (1, 84, 4, 1024, 64),
    "repeat-2046-k4-j32": (1, 32816, 410, 15, 4),
    "tie-2561-ones": (1, 30792, 513, 15, 3),
    "interior-l2-5000-k8": (0, 0, 1000, 5, 1),
    "plant-minus-l2-2500-k16": (0, 0, 500, 3, 1),
}


def test_new_cases_reach_what_they_are_named_for(tmp_path):
    exe = _build(tmp_path)
    names = list(NEW_CASE_PLANS)
    path = tmp_path / "plans.txt"
    shapes = [cd_world.NEW_CASES[n][0] for n in names]                              # (M, K, P, J, seed)
    path.write_text("".join("plan %d %d %d %d\n" % (M, K, J, P) for M, K, P, J, _ in shapes))
    got = subprocess.run([exe, str(path)], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    assert len(got) == len(names)
    plan = {}
    for n, line in zip(names, got):
        run, n_runs, pitch, use_lds, lds_bytes, n_j, blocks_x, per_block = (int(v) for v in line.split())
        assert (use_lds, lds_bytes, n_runs, blocks_x, per_block) == NEW_CASE_PLANS[n], (n, line)
        M, K, P, J, _ = cd_world.NEW_CASES[n][0]
        plan[n] = dict(lds=use_lds, bytes=lds_bytes, need=K * pitch * 4, passes=-(-n_runs // THREADS), runs=n_runs, blocks=blocks_x,
                       per_block=per_block, short=blocks_x * per_block - P)
    assert sorted(cd_world.NEW_CASES[n][0][1] % 4 for n in ("k3", "k5", "k7", "k13", "runs-512")) == [1, 1, 2, 3, 3]
    assert plan["lds-4092-k2"]["lds"] and plan["lds-4092-k2"]["passes"] == 2
    assert plan["lds-32768-k1"]["lds"] and plan["lds-32768-k1"]["passes"] == 13 and cd_world.NEW_CASES["lds-32768-k1"][0][0] == 32768
    assert plan["lds-2475-k16"]["bytes"] == LDS_MAX == plan["lds-4955-k8"]["bytes"]
    assert not plan["l2-2476-k16"]["lds"] and plan["l2-2476-k16"]["need"] == LDS_MAX + 64
    assert plan["runs-512"]["runs"] == THREADS and plan["runs-513"]["runs"] == THREADS + 1 and plan["runs-513"]["passes"] == 2
    assert plan["m-16"]["runs"] == 4 and cd_world.NEW_CASES["m-16"][0][0] == 16
    # a flush slot is reused more than once, and the blocks' point counts differ (19 and 20)
    assert plan["walk-20"]["per_block"] > 2 * FLUSH and 0 < plan["walk-20"]["short"] < plan["walk-20"]["blocks"]
    assert plan["walk-64"]["per_block"] == 8 * FLUSH and cd_world.NEW_CASES["walk-64"][0][2] == 65536 and plan["walk-64"]["short"] == 0
    # the repeated offsets p, p + 20, p + 40 fall to different blocks (20 and 40 are no multiples of 15) and to different slots
    assert 20 % plan["repeat-2046-k4-j32"]["blocks"] and 40 % plan["repeat-2046-k4-j32"]["blocks"]
    assert plan["tie-2561-ones"]["per_block"] == 3 and plan["tie-2561-ones"]["passes"] == 2
    assert not plan["interior-l2-5000-k8"]["lds"] and not plan["plant-minus-l2-2500-k16"]["lds"]


def test_plan_predictions_and_refusals(tmp_path, oracle):
    exe = _build(tmp_path)
    h = float.hex
    g = cd_world.geometry()
    b = cd_world.bins()
    lines, want = [], []
    for key, val in PLAN_TABLE.items():
        lines.append("plan %d %d %d %d" % key)
        want.append(" ".join(str(v) for v in val))
    preds = []
    for ds in (1.0, -1.0):
        for p, t in ((g["truth"], g["rx_time"]), (g["p0"], g["rx_time"] + 0.5)):
            ref = cd_ref.predict(oracle, g["eph"], g["prns"], range(len(g["prns"])), p, t, cd_world.FS, cd_world.M, float(b[0]), 100.0, ds=ds)
            for k, r in enumerate(ref):
                lines.append("pred %s %d %d %s %s %s %s %s %s %d" % (" ".join(h(float(v)) for v in g["eph"][k]), r["prn"], k,
                             " ".join(h(float(v)) for v in p), h(t), h(cd_world.FS), h(float(b[0])), h(100.0), h(ds), cd_world.M))
                want.append(None)
                preds.append((len(lines) - 1, r))
    e0 = " ".join(h(float(v)) for v in g["eph"][0])
    tail = "%s %s %s %s %s %s %d" % (" ".join(h(float(v)) for v in g["p0"]), h(g["rx_time"]), h(2.5e6), h(-6200.0), h(100.0), h(1.0), 2500)
    for line, msg in (("pred %s 38 0 %s" % (e0, tail), "refused PRN outside 1..37"), ("pred %s 2 -1 %s" % (e0, tail), "refused negative surface row"),
                      ("pred %s 2 0 %s" % (e0.replace(h(float(g["eph"][0][0])), h(10.0)), tail), "refused ephemeris is not a GPS orbit (sqrt_A, e)"),
                      ("pred %s 2 0 %s" % (e0, tail.replace(h(float(g["p0"][0])), h(9.0e7))), "refused range outside 15 000..30 000 km: p0, the time or the ephemeris is off")):
        lines.append(line)
        want.append(msg)
    far = 0.5 * 100.0 / cd_ref.DOPPLER_HZ_PER_KM * 1000.0           # 45 454.5 m at 100 Hz bins; 227 272.7 m at 500 Hz
    for args, msg in (((2500, 125, 8, 2, 2.5e6, -6200.0, 100.0, 1.0, far * 0.999), "ok"),
                      ((2500, 125, 8, 2, 2.5e6, -6200.0, 100.0, 1.0, far * 1.001), "refused the grid reaches farther"),
                      ((2500, 25, 8, 2, 2.5e6, -6000.0, 500.0, 1.0, far * 4.999), "ok"),
                      ((2500, 25, 8, 2, 2.5e6, -6000.0, -500.0, -1.0, far * 5.001), "refused the grid reaches farther"),
                      ((15, 125, 8, 2, 2.5e6, 0.0, 100.0, 1.0, 0.0), "refused M outside 16..32768"),
                      ((2500, 0, 8, 2, 2.5e6, 0.0, 100.0, 1.0, 0.0), "refused nBins outside 1..65536"),
                      ((2500, 125, 17, 2, 2.5e6, 0.0, 100.0, 1.0, 0.0), "refused maxSv outside 1..16"),
                      ((2500, 125, 8, 33, 2.5e6, 0.0, 100.0, 1.0, 0.0), "refused driftHalfWidth outside 0..32"),
                      ((2500, 125, 8, 2, -1.0, 0.0, 100.0, 1.0, 0.0), "refused sampling frequency not positive"),
                      ((2500, 125, 8, 2, 2.5e6, 0.0, 0.0, 1.0, 0.0), "refused bin raster not finite, or a zero bin step"),
                      ((2500, 125, 8, 2, 2.5e6, 0.0, 100.0, 2.0, 0.0), "refused dopplerSign is neither +1 nor -1"),
                      ((2500, 125, 8, 2, 2.5e6, 0.0, 100.0, 1.0, float("nan")), "refused a grid point is not finite")):
        lines.append("cfg %d %d %d %d %s %s %s %s %s" % (args[:4] + tuple(h(float(v)) for v in args[4:])))
        want.append(msg)
    for args, msg in (((0, 1, 0.0, 3.5, 2500), "ok"), ((1, 1, 0.0, 3.5, 2500), "refused surface row outside the surface"),
                      ((-1, 4, 0.0, 3.5, 2500), "refused surface row outside the surface"), ((0, 1, 2500.0, 3.5, 2500), "refused delay0 outside [0, M)"),
                      ((0, 1, -1e-9, 3.5, 2500), "refused delay0 outside [0, M)"), ((0, 1, 2499.999, 3.5, 2500), "ok"),
                      ((0, 1, 1.0, float("inf"), 2500), "refused bin0 not finite or beyond 1e6 bins")):
        lines.append("sv %d %d %s %s %d" % (args[0], args[1], h(args[2]), h(args[3]), args[4]))
        want.append(msg)
    for J, n_bins, bins, n in ((0, 9, (0, 8, 4), 0), (2, 9, (0, 8, 2, 4), 4), (32, 73, (0, 72, 2, 40), 94), (1, 5, (-3, 7), 6)):
        lines.append("oob %d %d %s" % (J, n_bins, " ".join(str(v) for v in bins)))
        want.append(str(n))
    path = tmp_path / "cases.txt"
    path.write_text("".join(line + "\n" for line in lines))
    p = subprocess.run([exe, str(path)], check=True, stdout=subprocess.PIPE, text=True)     # (exit 1: a property failed, message on stderr)
    got = p.stdout.splitlines()
    assert len(got) == len(lines)
    for line, w, have in zip(lines, want, got):
        if w is not None:
            assert have == w or (w.endswith("farther") and have.startswith(w)), (line[:60], have)
    for i, r in preds:
        f = got[i].split()
        assert f[0] == "ok", got[i]
        v = [float.fromhex(x) for x in f[1:]]
        d = abs(v[0] - r["delay0"])
        assert min(d, cd_world.M - d) < 1e-6 and abs(v[1] - r["bin0"]) < 1e-6
        assert np.abs(np.array(v[2:5]) - r["sat"]).max() < 1e-4 and abs(v[5] - r["range0"]) < 1e-4
