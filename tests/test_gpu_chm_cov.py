"""The device-resident loop's filter fed the manifold moments' covariance (dpe_chm_dev_set_measurement_cov; chm_k1_cov_kernel,
csrc/dpe_chm_dev.h): per window, what the measurement kernel left in its ring -- sums, counts, thresholds, R -- against
dpe_bcm_moments on the same handle and dpe_bcm_moments_rval in the frame the window was scored in, and the device filter against
the host filter (csrc/dpe_ekf.hip) fed the device's measurement and that R.  All BIT FOR BIT.  The loop is the shape of
tests/test_gpu_chm_filter.py: FS = 2.5e6, S = 8192, K = 6, 6 windows, its seeds.  Position grid 7^4 at 2 m (2 401 points: three
1 024-point blocks to fold in block order), velocity grid 5^4 at 0.5 m/s (one block): the two splits differ."""
import os
import re
import subprocess

import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import chm_world as cw

pytestmark = pytest.mark.gpu

FS, S, K, W = 2.5e6, 8192, 6, 6
RHO = (0.9, 0.99)


@pytest.fixture(scope="module")
def windows():
    iq, _, _, _ = dpe.workload.build_windows(W, FS, S, K, seed=11, amp=200.0, velocity=np.array([4.0, -3.0, 2.0]))
    return np.ascontiguousarray(iq)


def point_grids():
    return dpe.synth.uniform_grid(7, 2.0), dpe.synth.uniform_grid(5, 0.5)


def axes_grids():
    return dpe.grid_axes.GridAxes.uniform(7, 2.0), dpe.grid_axes.GridAxes.uniform(5, 0.5)


class Loop:
    """The attached device loop with the filter; rho = None: no set_measurement_cov (R = I)."""

    def __init__(self, iq, couple, rho, grids=point_grids, two_launch=False):
        import torch
        ho = dpe.handoff.read_handoff(dpe.workload.HANDOFF_CSV)
        gp, gv = grids()
        lp, lv = dpe.synth.uniform_grid(7, 2.0), dpe.synth.uniform_grid(5, 0.5)     # (the bank widths take point lists)
        L, B = dpe.pipeline.bank_half_widths(lp, lv, FS, dpe.engine.carr_fft_len(S))
        self.floors = np.array([dpe.pipeline.quantisation_floor(gp), dpe.pipeline.quantisation_floor(gv)])
        self.bcs = dpe.engine.BatchCorrScores(FS, samples_per_window=S, lag_half_width=L, bin_half_width=B, max_channels=K)
        self.bcs.Start()
        self.bcm = dpe.engine.BatchCorrManifold(FS, S, self.bcs.NumFFTPoints, gp, gv, LPower=1, lag_half_width=L, bin_half_width=B, max_channels=K)
        self.bcm.Start()
        self.G = (len(lp), len(lv))
        self.cm = dpe.engine.ChanMgrDev.from_handoff(ho, S / FS, K, (0.0,))
        self.cm.attach(self.bcs, self.bcm, 32)
        x = np.array(ho["X_ECEF"], dtype=np.float64).copy()
        self.cm.set_ekf(S / FS, x, couple_velocity=couple)
        self.rho = rho
        if rho is not None:
            if two_launch:      # (bcm_moments_finish_kernel in front of the measurement kernel: the form kept for comparison)
                os.environ["DPE_CHM_COV_TWO_LAUNCH"] = "1"
            try:
                self.cm.set_measurement_cov(rho, self.floors[0], self.floors[1])
            finally:
                os.environ.pop("DPE_CHM_COV_TWO_LAUNCH", None)
        self.host = dpe.engine.cuEKF(x, SampleLength=S / FS, EnableEKF=True, couple_velocity=couple)
        self.z_dev = self.cm.ports()[5]
        self.iq_d = torch.from_numpy(iq).to("cuda:0")
        self.cm.Start(x)
        self.w = 0

    def step(self):
        """One window: -> (fix record, the measurement the filter consumed, the frame the window was scored in)."""
        frame = self.cm.outputs()[2]["enu2ecef"][0].copy()
        self.bcs.UpdatePrepared(self.iq_d[self.w], K)
        self.bcm.UpdatePrepared(self.bcs.CodeScores, self.bcs.CarrScores, K)
        self.cm.step()
        r = self.cm.fix(self.w)
        self.w += 1
        return r, dpe.engine.d2h(self.z_dev, 64, np.float64), frame

    def assert_equal(self, tag):
        d, h = self.cm.ekf_state(), self.host.state()
        for k in cw.EKF_KEYS:
            assert d[k].tobytes() == h[k].tobytes(), (tag, k, np.abs(d[k] - h[k]).max())

    def checked_window(self):
        """One window with the three equalities of the suite; -> (fix, rval record, moments of the host path, K of the host filter)."""
        w = self.w
        r, z, frame = self.step()
        rv = self.cm.rval(w)
        mom = self.bcm.moments(self.rho)[0]                   # the same handle, before the next Update
        for k in ("sums", "nAbove", "threshold"):
            assert rv[k].tobytes() == mom[k].tobytes(), (w, k, rv[k], mom[k])
        R, fb = dpe.engine.moments_rval(rv["sums"], frame, self.floors)
        assert rv["R"].tobytes() == R.tobytes(), (w, np.abs(rv["R"] - R).max())
        assert rv["fallback"] == fb and bool(r["status"] & 128) == bool(fb)
        self.host.Update(z, R)
        assert r["zVal"].tobytes() == self.host.xCurrk1k1.tobytes(), w
        self.assert_equal(w)
        return r, rv, mom, self.host.state()["K"].copy()

    def close(self):
        self.host.Stop(); self.cm.Stop(); self.bcm.Stop(); self.bcs.Stop()


def identity_run_gains(iq, couple, grids=point_grids):
    """K per window of the same loop with R = I (no set_measurement_cov), the device filter's own."""
    lp = Loop(iq, couple, None, grids)
    out = []
    for w in range(W):
        lp.step()
        out.append(lp.cm.ekf_state()["K"].copy())
    lp.close()
    return out


@pytest.mark.parametrize("two_launch", [False, True], ids=["folded", "two_launch"])
@pytest.mark.parametrize("couple", [True, False], ids=["coupled", "uncoupled"])
def test_bit_for_bit_with_the_host_path(windows, couple, two_launch):
    """6a.  rho = (0.9, 0.99): sums, counts and thresholds equal dpe_bcm_moments', R equals dpe_bcm_moments_rval's, the filter equals the
    host filter's in every member, in every window -- in the folded form and with bcm_moments_finish_kernel in front (the same bits).
    At least one window per manifold has two or more points above the threshold (C != 0 is exercised), and K differs from the R = I run."""
    lp = Loop(windows, couple, RHO, two_launch=two_launch)
    above, gains = np.zeros(2, dtype=np.int64), []
    for w in range(W):
        r, rv, mom, Kh = lp.checked_window()
        assert r["status"] == 0 and rv["fallback"] == 0, (w, r["status"])
        print("window %d nAbove %s threshold %s diag R %s" % (w, rv["nAbove"], rv["threshold"], np.diag(rv["R"])))
        above = np.maximum(above, rv["nAbove"])
        gains.append(Kh)
    lp.close()
    assert (above >= 2).all(), above
    ident = identity_run_gains(windows, couple)
    assert any(a.tobytes() != b.tobytes() for a, b in zip(gains, ident))


def test_raw_score_weights_take_every_point(windows):
    """6b.  rho = (0, 0): every point of both grids is above the threshold (all scores positive), all three blocks of the position row
    carry weight; the same three equalities."""
    lp = Loop(windows, True, (0.0, 0.0))
    for w in range(W):
        r, rv, mom, _ = lp.checked_window()
        assert tuple(rv["nAbove"]) == lp.G and (rv["threshold"] == 0).all(), (w, rv["nAbove"])
        assert r["status"] == 0
    lp.close()


@pytest.mark.parametrize("rho", [RHO, (0.0, 0.0)], ids=["thresholded", "raw"])
def test_grid_axes_handle(windows, rho):
    """6b.  A GridAxes handle (posAx / velAx set: bcm_moments_kernel<true>, the measurement decoded from the axes): the same equalities,
    and the same R as the point-list handle of the same grids gives."""
    lp = Loop(windows, True, rho, axes_grids)
    ref = Loop(windows, True, rho, point_grids)
    for w in range(W):
        r, rv, mom, _ = lp.checked_window()
        r2, rv2, _, _ = ref.checked_window()
        assert r["status"] == 0
        assert rv["nAbove"].tobytes() == rv2["nAbove"].tobytes() and rv["threshold"].tobytes() == rv2["threshold"].tobytes()
        assert r["zVal"].tobytes() == r2["zVal"].tobytes()
    lp.close(); ref.close()


@pytest.mark.parametrize("couple", [True, False], ids=["coupled", "uncoupled"])
def test_off_is_off(windows, couple):
    """6c.  set_ekf and no set_measurement_cov: fixes and filter members equal the host filter fed R = I, as before; rval is refused."""
    lp = Loop(windows, couple, None)
    for w in range(W):
        r, z, _ = lp.step()
        lp.host.Update(z, np.eye(8))
        assert r["zVal"].tobytes() == lp.host.xCurrk1k1.tobytes(), w
        assert r["status"] == 0
        lp.assert_equal(w)
    with pytest.raises(dpe.DpeError, match=r"rval: no measurement covariance \(dpe_chm_dev_set_measurement_cov\)"):
        lp.cm.rval(0)
    lp.close()


def test_rval_ring_refuses_windows_it_does_not_hold(windows):
    lp = Loop(windows, True, RHO)
    with pytest.raises(dpe.DpeError, match="rval: window 0 not enqueued yet"):
        lp.cm.rval(0)
    lp.step()
    assert lp.cm.rval(0)["R"].shape == (8, 8)
    with pytest.raises(dpe.DpeError, match="rval: window 1 not enqueued yet"):
        lp.cm.rval(1)
    with pytest.raises(dpe.DpeError, match="rval: window -1 not enqueued yet"):
        lp.cm.rval(-1)
    lp.close()


def test_refusals(windows, tmp_path):
    """6d.  Every refusal of dpe_chm_dev_set_measurement_cov, each by its message."""
    ho = dpe.handoff.read_handoff(dpe.workload.HANDOFF_CSV)
    gp, gv = point_grids()
    L, B = dpe.pipeline.bank_half_widths(gp, gv, FS, dpe.engine.carr_fft_len(S))
    fl = np.array([dpe.pipeline.quantisation_floor(gp), dpe.pipeline.quantisation_floor(gv)])
    x = np.array(ho["X_ECEF"], dtype=np.float64).copy()
    bcs = dpe.engine.BatchCorrScores(FS, samples_per_window=S, lag_half_width=L, bin_half_width=B, max_channels=K)
    bcs.Start()

    def manifold(cls=dpe.engine.BatchCorrManifold, **kw):
        m = cls(FS, S, bcs.NumFFTPoints, gp, gv, lag_half_width=L, bin_half_width=B, max_channels=K, **kw)
        m.Start()
        return m

    def manager():
        return dpe.engine.ChanMgrDev.from_handoff(ho, S / FS, K, (0.0,))

    bcm = manifold()
    # no manifold handle attached
    cm = manager()
    with pytest.raises(dpe.DpeError, match="set_measurement_cov: attach a BatchCorrManifold first"):
        cm.set_measurement_cov(RHO, fl[0], fl[1])
    # no filter: the pass-through ignores R
    cm.attach(bcs, bcm, 8)
    with pytest.raises(dpe.DpeError, match="set_measurement_cov: no filter .*the pass-through ignores R"):
        cm.set_measurement_cov(RHO, fl[0], fl[1])
    cm.set_ekf(S / FS, x)
    # rho outside [0, 1) or not finite; a floor negative or not finite
    for bad in ((1.0, 0.5), (0.5, -0.01), (float("nan"), 0.5), (0.5, float("inf"))):
        with pytest.raises(dpe.DpeError, match=r"set_measurement_cov: rho\[[01]\] = .* outside \[0, 1\)"):
            cm.set_measurement_cov(bad, fl[0], fl[1])
    for m, name in ((0, "posFloorVar"), (1, "velFloorVar")):
        for bad in (-1e-3, float("nan"), float("inf")):
            f = fl.copy()
            f[m, 2] = bad
            with pytest.raises(dpe.DpeError, match=r"set_measurement_cov: %s\[2\] = .* is negative or not finite" % name):
                cm.set_measurement_cov(RHO, f[0], f[1])
    # a sharded loop
    comm = dpe.engine.Comm(0, 1, str(tmp_path), dpe.engine.Comm.HOSTFILES)
    cm.set_shard(comm, gp, gv)
    with pytest.raises(dpe.DpeError, match=r"set_measurement_cov: a sharded loop \(dpe_chm_dev_set_shard\) is not supported"):
        cm.set_measurement_cov(RHO, fl[0], fl[1])
    cm.Stop()
    comm.close()
    # ... and the other way round: a loop that takes its R from the moments cannot be sharded afterwards
    cm = manager()
    cm.attach(bcs, bcm, 8)
    cm.set_ekf(S / FS, x)
    cm.set_measurement_cov(RHO, fl[0], fl[1])
    os.makedirs(str(tmp_path / "b"))
    comm = dpe.engine.Comm(0, 1, str(tmp_path / "b"), dpe.engine.Comm.HOSTFILES)
    with pytest.raises(dpe.DpeError, match="set_shard: the loop takes its R from the manifold moments"):
        cm.set_shard(comm, gp, gv)
    # Start has already run
    cm.Start(x)
    with pytest.raises(dpe.DpeError, match="set_measurement_cov: before Start"):
        cm.set_measurement_cov(RHO, fl[0], fl[1])
    cm.Stop()
    comm.close()
    bcm.Stop()
    # the attached handle has writeScores = 0
    bcm = manifold(write_scores=False)
    cm = manager()
    cm.attach(bcs, bcm, 8)
    cm.set_ekf(S / FS, x)
    with pytest.raises(dpe.DpeError, match="moments: created with writeScores=0"):
        cm.set_measurement_cov(RHO, fl[0], fl[1])
    cm.Stop()
    bcm.Stop()
    # a family dpe_bcm_moments refuses cannot be attached in the first place (the hook's own refusal), so the call finds no manifold
    bcm = dpe.engine.EpochManifold(FS, S, bcs.NumFFTPoints, gp, gv, 1, lag_half_width=L, bin_half_width=B, max_channels=K)
    bcm.Start()
    cm = manager()
    with pytest.raises(dpe.DpeError, match="an epochs handle .* cannot serve the device-resident loop"):
        cm.attach(bcs, bcm, 8)
    with pytest.raises(dpe.DpeError, match="set_measurement_cov: attach a BatchCorrManifold first"):
        cm.set_measurement_cov(RHO, fl[0], fl[1])
    cm.Stop()
    bcm.Stop()
    bcs.Stop()


def test_pipeline_switch(windows):
    """pipeline.run_device_loop(measurement_cov=...): the result dicts carry RVal, sums, nAbove, and RVal is dpe_bcm_moments_rval of
    those sums with quantisation_floor's floors in the frame the window was scored in (`inputs`, kept with keep_scores); without
    the filter the switch is refused.  (At this window length the arg-max sits on the grid centre in every window, the innovation is 0
    and the fixes do not show the gain: K is compared in test_bit_for_bit_with_the_host_path.)"""
    ho = dpe.handoff.read_handoff(dpe.workload.HANDOFF_CSV)
    gp, gv = point_grids()
    floors = np.array([dpe.pipeline.quantisation_floor(gp), dpe.pipeline.quantisation_floor(gv)])
    fx, res, status = dpe.pipeline.run_device_loop(windows, ho, FS, gp, gv, K=K, enable_ekf=True, ring_depth=4, measurement_cov=RHO,
                                                   keep_scores=True)
    assert status == 0 and len(res) == W and np.isfinite(fx).all()
    for r in res:
        assert r["RVal"].shape == (8, 8) and r["sums"].shape == (2, 15) and r["nAbove"].shape == (2,) and r["fallback"] == 0
        R, fb = dpe.engine.moments_rval(r["sums"], r["inputs"][2]["enu2ecef"][0], floors)
        assert r["RVal"].tobytes() == R.tobytes() and fb == 0
        assert (np.linalg.eigvalsh(r["RVal"]) > 0).all() and not np.array_equal(r["RVal"], np.eye(8))
    with pytest.raises(dpe.DpeError, match="no filter"):
        dpe.pipeline.run_device_loop(windows[:1], ho, FS, gp, gv, K=K, measurement_cov=RHO)


def test_cpp_flow_measurement_cov_host_and_device_loop_agree(tmp_path):
    """6e.  dpe_flow --ekf --measurement-cov 0.9,0.99, host-driven (dpe_bcm_moments -> dpe_bcm_moments_rval -> dpe_ekf_step_update) and
    --device-loop --fix-lag 3 (dpe_chm_dev_set_measurement_cov): identical X-file rows, which differ from the rows without the switch.
    The set-up of test_cpp_flow_device_loop_with_the_filter_matches_the_host_driven_filter: W = 30, 9^4 grids.  And the refusals."""
    Wf, fs, Sf, Kf = 30, 2.5e6, 50000, 8
    iq, _, _, _ = dpe.workload.build_windows(Wf, fs, Sf, Kf, seed=5, amp=200.0, velocity=np.array([4.0, -2.0, 1.0]))
    dat = str(tmp_path / "synthetic_2500kHz.dat")
    iq.tofile(dat)
    ho_path = str(tmp_path / "handoff.csv")
    with open(dpe.workload.HANDOFF_CSV) as f, open(ho_path, "w") as g:
        for line in f:
            g.write("bytes_read,0\n" if line.startswith("bytes_read") else line)
    exe = os.path.join(os.path.dirname(dpe.engine.LIB_PATH), "dpe_flow")
    base = [exe, "--samples", dat, "--handoff", ho_path, "--iters", str(Wf), "--grid-dim", "9", "--spacing", "1.0", "--init-delta", "2", "-1", "1", "3"]
    cov = ["--measurement-cov", "0.9,0.99"]
    rows = {}
    for name, extra in (("host", ["--ekf"] + cov), ("dev", ["--device-loop", "--ekf", "--fix-lag", "3"] + cov), ("plain", ["--ekf"])):
        out = str(tmp_path / ("X_%s.csv" % name))
        subprocess.check_call(base + ["--out", out] + extra)
        rows[name] = np.loadtxt(out, delimiter=",")
        assert rows[name].shape == (Wf, 8)
    assert np.array_equal(rows["dev"], rows["host"])
    assert not np.array_equal(rows["host"], rows["plain"])
    for extra, msg in ((cov, "needs --ekf"), (["--ekf", "--graph"] + cov, "not available with"),
                       (["--ekf", "--ranks", "2", "--rank", "0", "--rendezvous", str(tmp_path)] + cov, "not available with"),
                       (["--ekf", "--measurement-cov", "1.0,0.5"], r"rho outside \[0, 1\)")):
        p = subprocess.run(base + ["--out", str(tmp_path / "X_refused.csv")] + extra, stderr=subprocess.PIPE, text=True)
        assert p.returncode == 2 and re.search(msg, p.stderr), (extra, p.stderr)
