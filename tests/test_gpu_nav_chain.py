"""GPU: the chain from samples to a DPE fix without the twin.  A synthetic world (tests/nav_world.py) whose geometry is exact at
the handoff epoch -> Acquisition.scalar_acquisition -> ScalarTracker.track -> assisted decode -> solve_log -> handoff at the last
epoch -> pipeline.run_closed_loop / run_device_loop on the next windows of the same continuous record."""
import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import helpers, nav_world

pytestmark = pytest.mark.gpu

FS, S, M, W = 2.5e6, 2500, 9000, 6              # 9 s tracked in 1 ms windows, then six 20 ms windows for the DPE loop
CHANS = [0, 1, 2, 3, 4, 6]                      # rows of the shipped handoff
C = 299792458.0


def test_chain_samples_to_dpe_fix(oracle, capsys):
    import torch
    import __graft_entry__ as ge
    ge.build()
    ho = dpe.handoff.read_handoff(helpers.HANDOFF)
    n_e = M * S
    world = nav_world.build(oracle, ho, CHANS, FS, n_e, seed=4, t_epoch=ho["rxTime"] + 2.0)     # sample 0 leaves ~1 s before a subframe edge
    ch, truth = world["ch"], world["truth"]
    K, prns = len(CHANS), [int(p) for p in ch["prn"]]
    n_all = n_e + W * 50000
    iq = np.empty(2 * n_all, dtype=np.int16)                     # 91 MB: a 9 s record is assembled whole; the pieces matter for longer ones
    at = 0
    for piece in dpe.synth.gen_iq_record_chunks(41, FS, n_all, ch, world["nav_bits"], amp=90.0, sigma=300.0):
        iq[at:at + piece.size] = piece
        at += piece.size
    assert at == iq.size
    iq_d = torch.from_numpy(iq[:2 * n_e]).to("cuda:0")
    acq = dpe.Acquisition(FS, 10 * S, prns, np.arange(-62, 63) * 100.0, mode="coherent")
    init = acq.scalar_acquisition(iq_d, iq_d[2 * 10 * S:])
    acq.close()
    assert all(r["found"] for r in init)
    trk = dpe.ScalarTracker(FS, prns, log_capacity_windows=M)
    trk.set_params(init)
    trk.track(iq_d, M)
    st = trk.state()
    assert trk.dev_status() == 0 and all(s["lock"] == 1 and s["frozen"] == 0 for s in st)       # every channel locked, status 0
    nav = dpe.ScalarNavigator(prns)
    nav.set_ephemerides(eph=truth["eph"])                        # assisted: the ephemerides are the caller's
    for k in range(K):
        d = nav.decode(k, trk.read_cp_signs(k), cp_first=0, mode="assisted")
        want = nav_world.expected_timestamp(world, k)
        assert d["status"] == 0 and (d["timestamp"]["TOW"], d["timestamp"]["cp"]) == want, (k, d["timestamp"], want)
    X_true = truth["X_ECEF"]
    R = oracle.enu2ecef(oracle.ecef2ll(X_true)).reshape(3, 3)    # ENU -> ECEF

    def enu_err(x, rx_a, t_true_a):
        return np.concatenate([R.T @ (np.asarray(x[:3]) - X_true[:3]), [C * (rx_a - t_true_a)]])
    # the per-epoch scalar fixes over the locked part (reported, not bounded): one per 20 ms from 1 s on
    first, stride = 1000, 20
    fixes = nav.solve_log(trk, first=first, n_epochs=(M - first) // stride, stride=stride)
    assert np.all(fixes["status"] == 0)
    t_of = truth["rxTime_a"] - (n_e - (first + stride * np.arange(fixes.size)) * S) / FS          # true GPS time of each epoch
    err = np.array([enu_err(f["X_ECEF"], f["rxTime_a"], t) for f, t in zip(fixes, t_of)])
    e_last = err[-1]                                             # the last logged epoch's device fix lies in the loop's pull-in range too
    assert np.all(np.abs(e_last[:3]) <= 110.0) and abs(e_last[3]) <= 132.0, e_last
    # the handoff at the last epoch: the tracker's state after the record = the parameters at sample n_e.  That state is the row the
    # NEXT window would log, not a logged epoch, so its fix is the host form's (dpe_nav_solve), not a solve_log record
    cp, rc, ri, fc, fi = (np.array([s[n] for s in st], dtype=np.float64) for n in ("cp", "rc", "ri", "fc", "fi"))
    fix = nav.solve(cp, rc, fi)
    assert fix["status"] == 0 and nav.status() == 0
    ho_nav = nav.handoff(fix, rc, ri, fc, fi, cp, bytes_read=4 * n_e)
    e_ho = enu_err(fix["X_ECEF"], fix["rxTime_a"], truth["rxTime_a"])
    # the DPE loop on the next windows of the same record, from the handoff and from the true state
    windows = iq[2 * n_e:].reshape(W, 100000)
    pos, vel = dpe.synth.spread_grid()
    f_nav, _ = dpe.pipeline.run_closed_loop(windows, ho_nav, FS, pos, vel)
    f_true, _ = dpe.pipeline.run_closed_loop(windows, truth, FS, pos, vel)
    f_dev, _, dev_status = dpe.pipeline.run_device_loop(windows, ho_nav, FS, pos, vel)
    own = np.linalg.norm(f_true[-1][:3] - X_true[:3])
    apart = np.linalg.norm(f_nav[-1][:3] - f_true[-1][:3])
    clk_own = abs(f_true[-1][3] - X_true[3])
    clk_apart = abs((f_nav[-1][3] - f_true[-1][3]) - C * (ho_nav["rxTime"] - truth["rxTime"]))
    dev_apart = np.abs(f_dev[-1][:4] - f_nav[-1][:4]).max()
    with capsys.disabled():
        print("\nchain: %d PRNs, %.1f s tracked, %d scalar fixes" % (K, n_e / FS, fixes.size))
        print("  scalar fixes E N U c.dt (m): mean %s  rms %s" % (np.round(err.mean(axis=0), 2), np.round(np.sqrt((err ** 2).mean(axis=0)), 2)))
        print("  handoff error E N U c.dt (m): %s   (bounds 110 110 110 132)" % np.round(e_ho, 2))
        print("  closed loop, final fix: true-start own error %.2f m (clock %.2f m); handoff-start apart from it %.2f m (clock %.2f m); "
              "bound own + 5 m" % (own, clk_own, apart, clk_apart))
        print("  device loop apart from the host loop %.3g m, status %d" % (dev_apart, dev_status))
    assert np.all(np.abs(e_ho[:3]) <= 110.0) and abs(e_ho[3]) <= 132.0, e_ho        # the pull-in range of the loop the handoff feeds
    assert apart <= own + 5.0 and clk_apart <= clk_own + 5.0, (apart, own, clk_apart, clk_own)
    assert dev_status == 0 and np.isfinite(f_dev).all() and dev_apart <= 5.0
    trk.close()
    nav.close()
