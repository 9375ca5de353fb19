"""The device-resident channel manager (chm_k1, csrc/dpe_chm_dev.h; chm_k2 / chm_k3, csrc/dpe_chm_k2.h) on the worlds of tests/chm_world.py -- week
crossovers, eccentric orbits, four other sites, a wide and even time grid, 37 channels, a Kepler failure, long runs at 1 and 5 ms --
against the host form, port by port, at the bounds of tests/test_gpu_chm_dev.py (chm_world.compare; the one derived change: the
satellite-state and fc bounds of an e = 0.3 channel times 1 / (1 - e)).  Then the attached loop replayed port by port by a host
manager fed the device's own fixes, and the measurement hold (status bit 4) with and without the filter.  What each world reaches
is proven on the CPU by tests/test_chm_world_cpu.py."""
import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import chm_world as cw

pytestmark = pytest.mark.gpu

SHORT_WORLDS = [n for n in cw.WORLDS if not n.startswith("long_") and n != "kepler_fail"]


def _dev_x(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to("cuda:0")


@pytest.mark.parametrize("name", SHORT_WORLDS)
def test_device_form_matches_the_host_form_on_every_world(name):
    """Start + 5 Updates with the moving fix of test_device_channel_manager_matches_the_host_form: every port and all K x dimT batch
    rows.  `wide_tg`: rows 0, 1, 6, 7 take the direct evaluation, rows 2, 3, 5 the first-order one, row 4 = dimT / 2 is the mid entry
    (an even grid: (dimT - 1) / 2 would be row 3, whose time differs).  `full`: 333 batch entries, the strided loop's second trip."""
    wd = cw.world(name)
    ho, T, tg = wd["ho"], wd["T"], wd["tg"]
    K = len(ho["prn_list"])
    scale = 1.0 / (1.0 - np.where(wd["ecc"] == 0.3, 0.3, 0.0)) if name == "ecc" else None
    host = dpe.engine.ChanMgr.from_handoff(ho, T)
    dev = dpe.engine.ChanMgrDev.from_handoff(ho, T, None, tg)
    x = np.array(ho["X_ECEF"], dtype=np.float64).copy()
    host.Start(x, x, tg)
    dev.Start(x)
    worst = cw.compare(dev.outputs(with_batch=True), host.outputs(with_batch=True), scale=scale)
    for x1, xk in cw.moving_fixes(x, 5):
        host.Update(x1, xk, tg)
        dev.Update(_dev_x(x1), _dev_x(xk))
        d, h = dev.outputs(with_batch=True), host.outputs(with_batch=True)
        cw.merge_worst(worst, cw.compare(d, h, scale=scale))
        assert d[3].shape == (K, len(tg), 8) and np.array_equal(d[1]["satState"], d[3][:, len(tg) // 2])
        assert dev.status == 0, dev.status
    print("world %s: worst deviation / bound over Start + 5 Updates:" % name, {k: float("%.3g" % v) for k, v in worst.items()})
    dev.Stop(); host.Stop()


def test_kepler_failure_is_flagged_and_leaves_the_other_channels_alone():
    """K = 5, channel 2 at e = 0.99 with a mean anomaly that misses the 10-iteration cap (by a margin, see chm_world): status bit 1
    after Start and still after every Update (sticky); channels 0, 1, 3, 4 of every port and batch row equal a host manager built
    from those four alone; the state port, the ENU matrix and rxTime are exact.  Nothing is asserted about channel 2."""
    wd = cw.world("kepler_fail")
    ho, T, tg, good = wd["ho"], wd["T"], wd["tg"], [0, 1, 3, 4]
    host = dpe.engine.ChanMgr.from_handoff(wd["good"], T)
    dev = dpe.engine.ChanMgrDev.from_handoff(ho, T, None, tg)
    x = np.array(ho["X_ECEF"], dtype=np.float64).copy()
    host.Start(x, x, tg)
    dev.Start(x)
    worst = cw.compare(dev.outputs(with_batch=True), host.outputs(with_batch=True), dev_chans=good)
    assert dev.status & 1, dev.status
    for x1, xk in cw.moving_fixes(x, 5):
        host.Update(x1, xk, tg)
        dev.Update(_dev_x(x1), _dev_x(xk))
        cw.merge_worst(worst, cw.compare(dev.outputs(with_batch=True), host.outputs(with_batch=True), dev_chans=good))
        assert dev.status & 1 and not dev.status & ~1, dev.status
    print("world kepler_fail: worst deviation / bound, good channels:", {k: float("%.3g" % v) for k, v in worst.items()})
    dev.Stop(); host.Stop()


@pytest.mark.parametrize("name", ["long_1ms", "long_5ms"])
def test_device_form_over_long_runs_at_1_and_5_ms(name):
    """T = 0.001 / 0.005, 200 / 150 windows of an accelerating receiver with a noisy fix (the recipe of
    test_chanmgr_long_runs_random_subsets), device against host at every step, both fed the same states: integers exactly equal
    (the seeds keep rcEnd 1e-3 chips clear of the code-period edges, test_chm_world_cpu.py), cp x 1023 + rc within 1e-4 chips,
    carrier phase on the circle, everything else at compare's bounds; no status bit at the end."""
    wd = cw.world(name)
    ho, T, tg = wd["ho"], wd["T"], wd["tg"]
    host = dpe.engine.ChanMgr.from_handoff(ho, T)
    dev = dpe.engine.ChanMgrDev.from_handoff(ho, T, None, tg)
    worst = {}
    for it, (xk, centre) in enumerate(cw.long_run_fixes(ho["X_ECEF"], T, wd["n"], wd["seed"])):
        if it == 0:
            host.Start(centre, centre, tg)      # (the device form's Start takes one state for both ports)
            dev.Start(centre)
        else:
            host.Update(xk, centre, tg)
            dev.Update(_dev_x(xk), _dev_x(centre))
        (sd, ed, wdv, bd), (sh, eh, wh, bh) = dev.outputs(with_batch=True), host.outputs(with_batch=True)
        for f in ("cpElapsedStart", "cpReference", "prn"):
            assert np.array_equal(sd[f], sh[f]), (it, f)
        for f in ("cpRefTOW", "cpElapsedEnd", "cpRef"):
            assert np.array_equal(ed[f], eh[f]), (it, f)
        chips = np.abs((ed["cpElapsedEnd"] * 1023.0 + ed["codePhaseEnd"]) - (eh["cpElapsedEnd"] * 1023.0 + eh["codePhaseEnd"])).max()
        chips0 = np.abs((sd["cpElapsedStart"] * 1023.0 + sd["codePhaseStart"]) - (sh["cpElapsedStart"] * 1023.0 + sh["codePhaseStart"])).max()
        assert chips <= 1e-4 and chips0 <= 1e-4, (it, chips, chips0)
        dp = np.abs(sd["carrierPhaseStart"] - sh["carrierPhaseStart"])
        dp = np.minimum(dp, 1.0 - dp).max()
        assert dp <= 1e-9, (it, dp)
        # the carrier phase has been compared on the circle: hand compare() the host's, so that a wrap at 1.0 is not a difference
        sd = sd.copy()
        sd["carrierPhaseStart"] = sh["carrierPhaseStart"]
        cw.merge_worst(worst, cw.compare((sd, ed, wdv, bd), (sh, eh, wh, bh)))
        worst["riCircle"] = max(worst.get("riCircle", 0.0), dp / 1e-9)
    assert dev.status == 0, dev.status
    print("world %s: worst deviation / bound over %d steps:" % (name, wd["n"]), {k: float("%.3g" % v) for k, v in worst.items()})
    dev.Stop(); host.Stop()


# ---------------------------------------------------------------------------------------------------------------------------------
# the attached loop (measurement from the scan's keys, chm_k2 riding in the stage-1 launch beside chm_k3), port by port

FS, S, K6, W12 = 2.5e6, 8192, 6, 12
# At a few m/s the 3.3 ms windows' scores are flat over the 5^4 grids and every fix is the grid centre -- the loop would be fed one
# constant state.  At this speed the velocity fix moves by ~2 m/s per window and the position / clock fix by ~2 m: every window's
# Update gets a new state, and the transmit time chm_k3 predicted is off by a real fix correction.
V_FAST = np.array([300.0, -200.0, 100.0])


def _with_batch(inputs):
    """run_device_loop keeps ChanMgrDev.outputs() without the batch rows; with a one-entry time grid the batch IS the end port's state."""
    s, e, win = inputs
    return s, e, win, e["satState"][:, None, :].copy()


def test_attached_loop_replayed_port_by_port_by_the_host_form():
    """12 windows, S = 8192, K = 6, 5^4 uniform grids, a fast receiver (V_FAST above: the fix has to move).  A host ChanMgr started on the same state gets
    Update(z_w, z_w) with z_w the DEVICE's own fix of window w (bit-identical input; the pass-through puts z on both state ports); its
    outputs equal the device manager's outputs before window w + 1 at compare's bounds, for every w.  From window 2 on chm_k2 has,
    by the code, a speculation to take: chm_k3 rode the previous stage-1 launch, and the transmit time it predicted is off by the fix
    correction / c ~ 1e-7 s < 1e-5 s.  The test cannot observe which branch ran and does not claim to; it holds whichever ran to the
    host form's ports."""
    iq, _, _, _ = dpe.workload.build_windows(W12, FS, S, K6, seed=11, amp=200.0, velocity=V_FAST)
    ho = dpe.handoff.read_handoff(dpe.workload.HANDOFF_CSV)
    g = dpe.synth.uniform_grid(5, 1.0)
    tg = np.zeros(1)
    fixes, res, status = dpe.pipeline.run_device_loop(iq, ho, FS, g, g, time_grid=tg, K=K6, ring_depth=8, keep_scores=True)
    assert status == 0 and np.isfinite(fixes).all()
    host = dpe.engine.ChanMgr.from_handoff(ho, S / FS, K6)
    x = np.array(ho["X_ECEF"], dtype=np.float64)
    host.Start(x, x, tg)
    worst = cw.compare(_with_batch(res[0]["inputs"]), host.outputs(with_batch=True))
    for w in range(W12 - 1):
        host.Update(fixes[w], fixes[w], tg)
        cw.merge_worst(worst, cw.compare(_with_batch(res[w + 1]["inputs"]), host.outputs(with_batch=True)))
    moved = np.abs(np.diff(fixes, axis=0))
    assert moved[:, :3].max() >= 1.0 and moved[:, 4:7].max() >= 1.0      # the fix moved, position and velocity: the replay was fed something
    print("attached loop: largest fix step %.1f m, %.1f m/s; clock %.1f m" % (moved[:, :3].max(), moved[:, 4:7].max(), moved[:, 3].max()))
    print("attached loop, 12 windows: worst deviation / bound:", {k: float("%.3g" % v) for k, v in worst.items()})
    host.Stop()


@pytest.mark.parametrize("ekf", [False, True], ids=["pass-through", "filter"])
def test_measurement_hold_on_a_window_without_a_score(ekf):
    """Window 5's scan is given all-NaN banks: no arg-max key.  That window's fix carries status bit 4, its zVal is the x_k|k-1 port
    before the window bit for bit, posIndex / velIndex are the grid offsets (0); the host manager fed the held state matches the
    next window's ports; windows 6 .. 11 go on with finite fixes and keep bit 4 (sticky).  With the filter (set_ekf) the host cuEKF,
    which skips the held window's Update, reproduces every x_k|k bit for bit, before and after."""
    import torch
    iq, _, _, _ = dpe.workload.build_windows(W12, FS, S, K6, seed=11, amp=200.0, velocity=V_FAST)
    ho = dpe.handoff.read_handoff(dpe.workload.HANDOFF_CSV)
    g = dpe.synth.uniform_grid(5, 1.0)
    tg = np.zeros(1)
    L, B = dpe.pipeline.bank_half_widths(g, g, FS, dpe.engine.carr_fft_len(S))
    bcs = dpe.engine.BatchCorrScores(FS, samples_per_window=S, lag_half_width=L, bin_half_width=B, max_channels=K6)
    bcs.Start()
    bcm = dpe.engine.BatchCorrManifold(FS, S, bcs.NumFFTPoints, g, g, LPower=1, lag_half_width=L, bin_half_width=B, max_channels=K6)
    bcm.Start()
    cm = dpe.engine.ChanMgrDev.from_handoff(ho, S / FS, K6, tg)
    cm.attach(bcs, bcm, 16)
    x = np.array(ho["X_ECEF"], dtype=np.float64).copy()
    filt = None
    if ekf:
        cm.set_ekf(S / FS, x)
        filt = dpe.engine.cuEKF(x, SampleLength=S / FS, EnableEKF=True)
    z_dev = cm.ports()[5]
    nan_code = torch.full((K6, 2 * L + 1, 2), float("nan"), dtype=torch.float32, device="cuda:0")
    nan_carr = torch.full((K6, 2 * B + 1, 2), float("nan"), dtype=torch.float32, device="cuda:0")
    iq_d = torch.from_numpy(np.ascontiguousarray(iq)).to("cuda:0")
    cm.Start(x)
    host = dpe.engine.ChanMgr.from_handoff(ho, S / FS, K6)
    host.Start(x, x, tg)
    for w in range(W12):
        before = cm.outputs(with_batch=True)
        cw.compare(before, host.outputs(with_batch=True))
        bcs.UpdatePrepared(iq_d[w], K6)
        if w == 5:
            bcm.UpdatePrepared(nan_code.data_ptr(), nan_carr.data_ptr(), K6)
        else:
            bcm.UpdatePrepared(bcs.CodeScores, bcs.CarrScores, K6)
        cm.step()
        r = cm.fix(w)
        assert np.isfinite(r["zVal"]).all(), w
        assert r["status"] == (4 if w >= 5 else 0), (w, r["status"])
        z = dpe.engine.d2h(z_dev, 64, np.float64)
        if w == 5:
            assert r["zVal"].tobytes() == before[2]["xCurrkk1"][0].tobytes()
            assert z.tobytes() == before[2]["xCurrkk1"][0].tobytes()
            assert r["posIndex"] == 0 and r["velIndex"] == 0
        elif ekf:
            filt.Update(z, np.eye(8))
            assert filt.xCurrk1k1.tobytes() == r["zVal"].tobytes(), (w, np.abs(filt.xCurrk1k1 - r["zVal"]).max())
        else:
            assert z.tobytes() == r["zVal"].tobytes(), w
        if ekf:
            st = cm.ekf_state()
            x1, xk = st["xk1k1"], st["xkk1"]
            if w == 5:
                x1 = xk = before[2]["xCurrkk1"][0]       # the ports hold the predicted state; the filter's members are untouched
                assert st["xkk1"].tobytes() == xk.tobytes()
            else:
                assert x1.tobytes() == r["zVal"].tobytes()
            host.Update(x1, xk, tg)
        else:
            host.Update(r["zVal"], r["zVal"], tg)
    cw.compare(cm.outputs(with_batch=True), host.outputs(with_batch=True))
    assert cm.status == 4
    if filt is not None:
        filt.Stop()
    host.Stop(); cm.Stop(); bcm.Stop(); bcs.Stop()
