"""Grids given by their axes (dpe_bcm_create_axes, GridAxes) on the device: parity with the oracle on the materialised grid,
agreement with a point-list handle on the same grid, shards that cut rows, the pipe, and a 1.04e8-point grid that only fits as
axes.  The runner is this file's own: helpers.run_gpu takes point lists."""
import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import helpers

pytestmark = pytest.mark.gpu


def _banks(case, L, B):
    """BatchCorrScores on the case's windows: (handle, window array, chan_end array) for the manifold handles."""
    import torch
    iq, cs, ce, bw = helpers.pack_gpu_inputs(case)
    W, K = cs.shape
    bcs = dpe.BatchCorrScores(case["fs"], samples_per_window=case["S"], lag_half_width=L, bin_half_width=B, max_windows=W,
                              max_channels=K)
    bcs.Start()
    bcs.Update(torch.from_numpy(iq).to("cuda:0"), cs)
    return bcs, bw, ce


def _manifold(case, bcs, pos, vel, L, B, W, K, lpower=1, write_scores=True, weighted_mean=True):
    m = dpe.BatchCorrManifold(case["fs"], case["S"], bcs.NumFFTPoints, pos, vel, LPower=lpower, lag_half_width=L, bin_half_width=B,
                              max_windows=W, max_channels=K, write_scores=write_scores, weighted_mean=weighted_mean)
    m.Start()
    return m


def _scan(m, bcs, bw, ce):
    m.Update(bcs.CodeScores, bcs.CarrScores, bw, ce)
    out = dict(res=m.results())
    if m.write_scores:
        out["pos"], out["vel"] = m.read_scores()
    return out


def run_axes(case, pos_ax, vel_ax, L, B, lpower=1, write_scores=True, weighted_mean=True):
    """The axes handle and a point-list handle on the same banks; the output dict of helpers.run_gpu for the axes handle."""
    bcs, bw, ce = _banks(case, L, B)
    W, K = ce.shape
    ma = _manifold(case, bcs, pos_ax, vel_ax, L, B, W, K, lpower, write_scores, weighted_mean)
    mp = _manifold(case, bcs, case["pos"], case["vel"], L, B, W, K, lpower, write_scores, weighted_mean)
    ax, pl = _scan(ma, bcs, bw, ce), _scan(mp, bcs, bw, ce)
    code, carr = bcs.read_banks()
    idx_next, no_flip, mean = bcs.read_info()
    ax.update(code=list(code), carr=list(carr), idx_next=idx_next, no_flip=no_flip, mean=mean)
    for d in (ax, pl):
        if write_scores:
            d["pos"], d["vel"] = list(d["pos"]), list(d["vel"])
    ma.Stop(); mp.Stop(); bcs.Stop()
    return ax, pl


def assert_matches_point_list(ax, pl, write_scores):
    for w, (ra, rp) in enumerate(zip(ax["res"], pl["res"])):
        for name, key, sk in (("pos", "posIndex", "posScore"), ("vel", "velIndex", "velScore")):
            if write_scores:
                a, p = ax[name][w], pl[name][w]
                assert np.abs(a - p).max() <= 2e-6 * p.max(), "%s scores window %d" % (name, w)
                if ra[key] != rp[key]:   # an fp32 tie only
                    assert abs(p[ra[key]] - p[rp[key]]) <= 2e-6 * p.max(), "%s arg-max window %d" % (name, w)
            elif ra[key] != rp[key]:
                assert abs(ra[sk] - rp[sk]) <= 2e-6 * rp[sk], "%s arg-max window %d" % (name, w)
        if ra["posIndex"] == rp["posIndex"] and ra["velIndex"] == rp["velIndex"]:
            assert np.array_equal(ra["zVal"], rp["zVal"])


def _case(grid, W=2, seed=11, S=50000, K=8, center_offset=None):
    """A case on the handoff geometry whose grids are the given GridAxes, materialised for the oracle."""
    pos_ax, vel_ax = grid
    case = helpers.make_case(seed=seed, fs=2.5e6, S=S, K=K, G=64, amp=200.0, W=W, center_offset=center_offset)
    case["pos"], case["vel"] = pos_ax.points(), vel_ax.points()
    return case


GRIDS = {
    "uniform25": lambda: (dpe.GridAxes.uniform(25, 1.0), dpe.GridAxes.uniform(25, 1.0)),
    "arthur25": lambda: (dpe.GridAxes.arthur_basis(25, 1.0), dpe.GridAxes.uniform(25, 1.0)),
    "spread": lambda: dpe.GridAxes.pygnss_spread(),
    "odd_3_5_7_1": lambda: (dpe.GridAxes.uniform((3, 5, 7, 1), (4.0, 3.0, 2.0, 1.0)), dpe.GridAxes.uniform((5, 3, 1, 7), 0.5)),
    "odd_4_4_4_33": lambda: (dpe.GridAxes.uniform((4, 4, 4, 33), (3.0, 3.0, 3.0, 0.7)), dpe.GridAxes.uniform((4, 4, 4, 33), 0.4)),
}


@pytest.mark.parametrize("grid,lpower,L,B,wm,ws", [
    ("uniform25", 1, 4, 20, True, True),      # the reference's default configuration at config R's stage shape
    ("arthur25", 2, 4, 20, False, True),
    ("spread", 3, 4, 20, True, True),
    ("spread", 1, 2, 6, True, True),          # narrow banks: both clamp variants, out-of-window pairs
    ("odd_3_5_7_1", 1, 1, 2, True, True),
    ("odd_4_4_4_33", 2, 2, 3, False, False),
    ("odd_4_4_4_33", 1, 8, 20, True, True),
])
def test_axes_vs_oracle_and_point_list(grid, lpower, L, B, wm, ws):
    pos_ax, vel_ax = GRIDS[grid]()
    case = _case((pos_ax, vel_ax), W=2 if grid in ("uniform25", "arthur25") else 3)
    ax, pl = run_axes(case, pos_ax, vel_ax, L, B, lpower=lpower, write_scores=ws, weighted_mean=wm)
    ref = helpers.run_oracle(case, L, B, lpower=lpower)
    helpers.assert_parity(ax, ref, tol=2e-6 if lpower != 3 else 1e-5, check_scores=ws)   # (test_gpu_parity.py's)
    assert_matches_point_list(ax, pl, ws)
    if L <= 2:
        assert sum(r["posOutOfWindow"] + r["velOutOfWindow"] for r in ax["res"]) > 0


@pytest.mark.parametrize("world", [3, 5, 7])   # (3 and 7 cut rows of 25 points; 5 ranks split 25^4 on row boundaries)
def test_shards_cut_rows(world):
    pos_ax, vel_ax = dpe.GridAxes.uniform(25, 1.0), dpe.GridAxes.uniform(25, 1.0)
    case = _case((pos_ax, vel_ax), W=2, seed=4)
    L, B = 4, 20
    bcs, bw, ce = _banks(case, L, B)
    W, K = ce.shape
    whole = _manifold(case, bcs, pos_ax, vel_ax, L, B, W, K)
    full = _scan(whole, bcs, bw, ce)
    full_keys = np.array(dpe.engine.d2h(whole.Keys, 16 * W, np.uint64)).reshape(W, 2)
    keys, ps, vs = [], [], []
    for r in range(world):
        pb, pe = dpe.sharding.shard_range(pos_ax.size, r, world)
        vb, ve = dpe.sharding.shard_range(vel_ax.size, r, world)
        m = _manifold(case, bcs, pos_ax.shard(pb, pe), vel_ax.shard(vb, ve), L, B, W, K)
        out = _scan(m, bcs, bw, ce)
        ps.append(out["pos"]); vs.append(out["vel"])
        keys.append(np.array(dpe.engine.d2h(m.Keys, 16 * W, np.uint64)).reshape(W, 2))
        if r == world - 1:
            last = m
        else:
            m.Stop()
    assert np.array_equal(np.concatenate(ps, axis=1), full["pos"]) and np.array_equal(np.concatenate(vs, axis=1), full["vel"])
    reduced = np.max(np.stack(keys), axis=0)
    assert np.array_equal(reduced, full_keys)
    dec = last.results_from_keys(reduced)        # NULL global grids: decoded from the axes
    for w in range(W):
        assert dec[w]["posIndex"] == full["res"][w]["posIndex"] and dec[w]["velIndex"] == full["res"][w]["velIndex"]
        assert np.array_equal(dec[w]["zVal"], full["res"][w]["zVal"])
    last.Stop(); whole.Stop(); bcs.Stop()


def test_pipe_lanes_equal_a_lone_handle():
    import torch
    pos_ax, vel_ax = dpe.GridAxes.pygnss_spread()
    case = _case((pos_ax, vel_ax), W=2, seed=8)
    L, B = 4, 20
    iq, cs, ce, bw = helpers.pack_gpu_inputs(case)
    W, K = cs.shape
    bcs, _, _ = _banks(case, L, B)
    lone = _manifold(case, bcs, pos_ax, vel_ax, L, B, W, K, weighted_mean=False)
    want = _scan(lone, bcs, bw, ce)
    pipe = dpe.Pipe(case["fs"], case["S"], pos_ax, vel_ax, lag_half_width=L, bin_half_width=B, max_windows=W, max_channels=K,
                    in_flight=2)
    iq_d = torch.from_numpy(iq).to("cuda:0")
    tickets = [pipe.submit(iq_d, cs, bw, ce) for _ in range(2)]
    for t in tickets:
        got = pipe.results(t)
        for g, r in zip(got, want["res"]):
            assert (g["posIndex"], g["velIndex"], g["posScore"], g["velScore"]) == (r["posIndex"], r["velIndex"], r["posScore"], r["velScore"])
            assert np.array_equal(g["zVal"], r["zVal"])
        _, m, _ = pipe.lane(t)
        ps, vs = m.read_scores()
        assert np.array_equal(ps, want["pos"]) and np.array_equal(vs, want["vel"])
    pipe.close(); lone.Stop(); bcs.Stop()


def test_hundred_million_points_as_axes():
    import torch
    pos_ax, vel_ax = dpe.GridAxes.uniform(101, 1.0), dpe.GridAxes.uniform(9, 1.0)
    assert pos_ax.size == 101 ** 4
    case = _case((dpe.GridAxes.uniform(3, 1.0), vel_ax), W=1, seed=21, center_offset=(7.0, -5.0, 3.0, 11.0))
    L, B = 4, 20
    bcs, bw, ce = _banks(case, L, B)
    K = ce.shape[1]
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    m = _manifold(case, bcs, pos_ax, vel_ax, L, B, 1, K, write_scores=False, weighted_mean=False)
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info()[0] < 64 << 20
    res = _scan(m, bcs, bw, ce)["res"][0]
    m.Stop()
    # the 9^4 block of the grid around the reported point, as a point list on the same banks
    ix = np.unravel_index(res["posIndex"], pos_ax.dim)
    sl = [np.arange(max(0, i - 4), min(101, i + 5)) for i in ix]
    blk = np.stack(np.meshgrid(*[pos_ax.axes[c][sl[c]] for c in range(4)], indexing="ij"), axis=-1).reshape(-1, 4)
    mp = _manifold(case, bcs, blk, vel_ax.points(), L, B, 1, K, write_scores=True, weighted_mean=False)
    out = _scan(mp, bcs, bw, ce)
    mp.Stop(); bcs.Stop()
    j = out["res"][0]["posIndex"]
    assert np.array_equal(blk[j], pos_ax.global_point(res["posIndex"])) or \
        abs(out["pos"][0][j] - res["posScore"]) <= 2e-6 * res["posScore"]
    assert abs(out["pos"][0].max() - res["posScore"]) <= 2e-6 * res["posScore"]


def test_update_dev_and_prepared_match_update(golden, oracle):
    """dpe_bcm_update_dev on an axes handle (the channel parameters as device port arrays, O7 state) against dpe_bcm_update with
    the host form of the same inputs; dpe_bcm_update_prepared runs inside the device-resident loop (test_flow_grid_axes)."""
    import torch
    g = golden("o7_dp_iteration")
    ho = dpe.handoff.read_handoff(helpers.HANDOFF)
    K, fs, S = 8, float(g["fs"]), int(g["S"])
    cm = oracle.ChanMgr(ho["prn_list"], ho["rc"], ho["ri"], ho["fc"], ho["fi"], ho["cp"], ho["cp_timestamp"],
                        ho["TOW"], ho["eph"], ho["rxTime"], 0.02)
    pos_ax, vel_ax = dpe.GridAxes.pygnss_spread()
    tg = pos_ax.axes[3]
    X = ho["X_ECEF"]
    batch, R = cm.start(X, X, tg)
    L, B = 8, 48
    dev = torch.device("cuda:0")
    iq_d = torch.from_numpy(g["iq"]).to(dev)
    bcs = dpe.BatchCorrScores(fs, samples_per_window=S, lag_half_width=L, bin_half_width=B, max_windows=1, max_channels=K)
    bcs.Start()
    cs = dpe.engine.chan_start_array(ho["prn_list"], cm.rcStart, cm.riStart, cm.fc, cm.fi, cm.cpElaStart, cm.cpRef)
    ce = dpe.engine.chan_end_array(batch[:, tg.size // 2], cm.rcEnd, cm.fc, cm.fi, cm.cpRefTOW, cm.cpElaEnd, cm.cpRef)
    bw = dpe.engine.bcm_window_array(X[None, :], R[None, :], [cm.rxTime])
    bcs.Update(iq_d, cs)

    def d(a, dt):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=dt)).to(dev)
    ports = dict(xCurrkk1=d(X, np.float64), enu2ecef=d(np.asarray(R).ravel(), np.float64), satStates=d(batch, np.float64),
                 codePhaseEnd=d(cm.rcEnd, np.float64), codeFrequency=d(cm.fc, np.float64), carrierFrequency=d(cm.fi, np.float64),
                 cpRefTOW=d(cm.cpRefTOW, np.int32), cpElapsedEnd=d(cm.cpElaEnd, np.int32), cpRef=d(cm.cpRef, np.int32),
                 dopplerSign=d([1], np.int32))
    out = []
    for form in ("host", "dev"):
        m = dpe.BatchCorrManifold(fs, S, bcs.NumFFTPoints, pos_ax, vel_ax, lag_half_width=L, bin_half_width=B, max_channels=K)
        m.Start()
        if form == "host":
            m.Update(bcs.CodeScores, bcs.CarrScores, bw, ce)
        else:
            m.UpdateDev(bcs.CodeScores, bcs.CarrScores, K, ports, tg.size, cm.rxTime)
        out.append((m.results()[0],) + m.read_scores())
        m.Stop()
    bcs.Stop()
    (r0, p0, v0), (r1, p1, v1) = out
    # the device prep forms the centre index as a compensated fp64 sum where the host uses long double: scores within fp32 rounding
    assert np.abs(p1 - p0).max() <= 2e-6 * p0.max() and np.abs(v1 - v0).max() <= 2e-6 * v0.max()
    for key, sc in (("posIndex", p0[0]), ("velIndex", v0[0])):
        if r1[key] != r0[key]:
            assert abs(sc[r1[key]] - sc[r0[key]]) <= 2e-6 * sc.max()
    if r1["posIndex"] == r0["posIndex"] and r1["velIndex"] == r0["velIndex"]:
        assert np.abs(r1["zVal"] - r0["zVal"]).max() < 1e-6
        assert np.array_equal(pos_ax.global_point(r0["posIndex"]), pos_ax.points()[r0["posIndex"]])


@pytest.mark.parametrize("mode", [[], ["--device-loop"], ["--device-loop", "--ekf"]])
def test_flow_grid_axes(tmp_path, mode):
    """dpe_flow --grid-axes (BatchCorrManifold's GridAxes parameter: the built 25^4 grids go to the engine as axes) against
    dpe_flow with point lists, over 24 closed-loop windows: the same fixes.  --device-loop reaches dpe_bcm_update_prepared and the
    measurement kernel's decoding of the arg-max from the axes."""
    import os
    import subprocess
    W, fs, S, K = 24, 2.5e6, 50000, 8
    iq, _, _, _ = dpe.workload.build_windows(W, fs, S, K, seed=6, amp=200.0)
    dat = str(tmp_path / "synthetic_2500kHz.dat")
    iq.tofile(dat)
    ho_path = str(tmp_path / "handoff.csv")
    with open(dpe.workload.HANDOFF_CSV) as f, open(ho_path, "w") as g:
        for line in f:
            g.write("bytes_read,0\n" if line.startswith("bytes_read") else line)
    exe = os.path.join(os.path.dirname(dpe.engine.LIB_PATH), "dpe_flow")
    rows = {}
    for axes in (False, True):
        out = str(tmp_path / ("X_axes.csv" if axes else "X.csv"))
        subprocess.check_call([exe, "--samples", dat, "--handoff", ho_path, "--out", out, "--iters", str(W), "--grid-dim", "25",
                               "--spacing", "1.0"] + mode + (["--grid-axes"] if axes else []), timeout=600)
        rows[axes] = np.loadtxt(out, delimiter=",")
    assert rows[True].shape == rows[False].shape and rows[False].shape[0] >= 20
    assert np.abs(rows[True] - rows[False]).max() < 1e-6
