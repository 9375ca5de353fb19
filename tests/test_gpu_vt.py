"""GPU: vector tracking (dpe_vt_*, csrc/dpe_vt.hip) on the synthetic world of tests/vt_world.py against tests/vt_ref.py.

Bounds and where they come from:
  * teacher-forced correlations: 2e-6 of the channel's prompt peak, the bound tests/test_gpu_trk.py holds dpe_trk_correlate to;
    boundary case and completed periods equal;
  * closed loop: per logged quantity 4 x the largest deviation from vt_ref of vt_ref re-run with its E / P / L rounded to fp32 at
    every window (the rule of DESIGN.md 7c); included masks and status equal;
  * truth: the final position error against X_true below the RMS of the single-epoch least-squares fixes on the same record."""
import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import helpers, vt_ref, vt_world
from tests.test_vt_ref_cpu import N_EPOCHS, N_SAMPLES, OUT_CH, OUT_FIRST, OUT_LEN, ls_rms, outage_profile

pytestmark = pytest.mark.gpu
TOL = 2e-6
NAMES = ("X", "diag", "rxTime0") + vt_ref.CHAN_NAMES
WRAP = {"rc": 1023.0, "ri": 1.0}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return dpe.engine.lib()


def to_dev(iq):
    import torch
    return torch.from_numpy(iq).to("cuda:0")


def make_vt(w, cfg, X0, n_epochs, **kw):
    s = w["start"]
    vt = dpe.VectorTracker(cfg.fs, cfg.prns, T=cfg.T, N=cfg.N, ds=cfg.ds, num_prev=cfg.num_prev, log_capacity_epochs=max(n_epochs, 1), **kw)
    vt.set_ephemerides(s["eph"], s["tow"], s["cps"])
    vt.init(X0, vt_world.sigma0(), s["rxTime0"], s["chan"])
    return vt


def deviation(a, b, name):
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    if name in WRAP:
        d = np.minimum(d, WRAP[name] - d)
    return float(d.max())


def hold_to_yardstick(dev, ref_t, rnd_t, label, capsys):
    """dev: VectorTracker.read_log; ref_t / rnd_t: vt_ref.table of the fp64 and the fp32-rounded restatement."""
    lines, bad = [], []
    for n in NAMES:
        yard, got = deviation(rnd_t[n], ref_t[n], n), deviation(dev[n], ref_t[n], n)
        lines.append("  %-8s device %.3e   yardstick %.3e   ratio %s" % (n, got, yard, "%.2f" % (got / yard) if yard else "-"))
        if got > 4.0 * yard:
            bad.append((n, got, yard))
    with capsys.disabled():
        print("\n%s" % label)
        print("\n".join(lines))
    assert np.array_equal(dev["mask"], ref_t["mask"]) and np.array_equal(dev["status"], ref_t["status"])
    assert not bad, bad


def small_case(oracle, K, T, N, n_epochs, seed=4, ds=1.0):
    """A short world for the shape tests: K channels (synthetic PRNs beyond the handoff's six), T, N; ds: the world's and the loop's
    DopplerSign."""
    ho, chans = None, vt_world.CHANS[:K]
    if K > len(vt_world.CHANS):
        ho, chans = vt_world.synthetic_handoff(dpe.handoff.read_handoff(helpers.HANDOFF), K), list(range(K))
    S = int(round(T * vt_world.FS))
    w = vt_world.build(oracle, n_epochs * N * S, chans=chans, ho=ho, seed=seed, ds=ds)
    iq = vt_world.record(w)
    cfg = vt_ref.Config(vt_world.FS, w["start"]["prns"], T=T, N=N, ds=ds, num_prev=4)
    X0 = vt_world.perturbed(w)
    ref = vt_ref.run(iq, cfg, oracle, w["start"], X0, vt_world.sigma0(), n_epochs)
    rnd = vt_ref.run(iq, cfg, oracle, w["start"], X0, vt_world.sigma0(), n_epochs, round_epl=np.float32)
    return w, iq, cfg, X0, ref, rnd


@pytest.fixture(scope="module")
def nominal(oracle):
    w = vt_world.build(oracle, N_SAMPLES)
    iq = vt_world.record(w)
    cfg = vt_ref.Config(vt_world.FS, w["start"]["prns"])
    X0 = vt_world.perturbed(w)
    ref = vt_ref.run(iq, cfg, oracle, w["start"], X0, vt_world.sigma0(), N_EPOCHS, with_ls=True)
    return w, iq, cfg, X0, ref


@pytest.mark.parametrize("N", [20, 4])
def test_teacher_forced_correlations(built, oracle, nominal, capsys, N):
    w, iq, cfg20, X0, ref20 = nominal
    if N == 20:
        cfg, params, sums, first = cfg20, ref20["params"][7], ref20["sums"][7], 7 * 20 * cfg20.S     # an epoch of the converging loop
    else:
        cfg = vt_ref.Config(vt_world.FS, cfg20.prns, N=4)
        st = vt_ref.new_state(cfg, X0, vt_world.sigma0(), w["start"]["rxTime0"], ref20["params"][3])
        params, first = ref20["params"][3], 3 * 20 * cfg20.S
        sums = vt_ref.correlate_epoch(iq, first, cfg, st)
    vt = dpe.VectorTracker(cfg.fs, cfg.prns, N=N, log_capacity_epochs=1)
    vt.set_ephemerides(w["start"]["eph"], w["start"]["tow"], w["start"]["cps"])
    vt.init(X0, vt_world.sigma0(), w["start"]["rxTime0"] + first / cfg.fs, params)
    vt.track(to_dev(iq[2 * first:2 * (first + N * cfg.S)]), 1)
    got = vt.read_corr()
    vt.close()
    peak = np.hypot(sums[..., 2], sums[..., 3]).max(axis=0)                                       # per channel
    err = np.abs(got[..., :6] - sums[..., :6]).max(axis=(0, 2)) / peak
    with capsys.disabled():
        print("\nteacher-forced, N = %d: worst |sum - vt_ref| / prompt peak per channel %s (bound %.0e)" % (N, np.array2string(err, precision=2), TOL))
    assert np.array_equal(got[..., 6:], sums[..., 6:])                                            # case and completed periods
    assert np.all(err <= TOL), err


def test_closed_loop_40_epochs(built, oracle, nominal, capsys):
    w, iq, cfg, X0, ref = nominal
    rnd = vt_ref.run(iq, cfg, oracle, w["start"], X0, vt_world.sigma0(), N_EPOCHS, round_epl=np.float32)
    vt = make_vt(w, cfg, X0, N_EPOCHS)
    vt.track(to_dev(iq), N_EPOCHS)
    dev = vt.read_log()
    assert vt.dev_status() == 0
    vt.close()
    rms = ls_rms(w, ref)
    err = np.linalg.norm(dev["X"][:, :3] - w["start"]["X"][:3], axis=1)
    with capsys.disabled():
        print("\nclosed loop, 40 epochs of 20 ms from 30 m / 0.5 m/s off: device position error %.2f m -> %.2f m; single-epoch LS RMS %.2f m"
              % (err[0], err[-1], rms))
    hold_to_yardstick(dev, vt_ref.table(ref["recs"]), vt_ref.table(rnd["recs"]), "closed loop vs vt_ref (K = 6, N = 20, T = 1 ms)", capsys)
    assert err[-1] < rms, (err[-1], rms)


def test_outage_record(built, oracle, capsys):
    w = vt_world.build(oracle, N_SAMPLES)
    iq = vt_world.record(w, profile=outage_profile())
    cfg = vt_ref.Config(vt_world.FS, w["start"]["prns"])
    X0 = vt_world.perturbed(w)
    ref = vt_ref.table(vt_ref.run(iq, cfg, oracle, w["start"], X0, vt_world.sigma0(), N_EPOCHS)["recs"])
    vt = make_vt(w, cfg, X0, N_EPOCHS)
    vt.track(to_dev(iq), N_EPOCHS)
    dev = vt.read_log()
    status = vt.dev_status()
    vt.close()
    back = OUT_FIRST + OUT_LEN
    with capsys.disabled():
        print("\noutage of channel %d in epochs %d .. %d: device masks %s; dpc at return %.4f chip (vt_ref %.4f); lock metric there %.1f"
              % (OUT_CH, OUT_FIRST, back - 1, "".join(str((int(m) >> OUT_CH) & 1) for m in dev["mask"]), dev["dpc"][back, OUT_CH],
                 ref["dpc"][back, OUT_CH], dev["lock"][back, OUT_CH]))
    assert np.array_equal(dev["mask"], ref["mask"])
    assert abs(dev["dpc"][back, OUT_CH]) < 0.25
    assert status == 0 and np.all(dev["status"] == 0)


def test_split_calls_and_displaced_record(built, oracle, nominal):
    import torch
    w, iq, cfg, X0, _ = nominal
    iq_d = to_dev(iq)
    per = 2 * cfg.N * cfg.S
    logs = []
    for split in ((N_EPOCHS,), (13, 27)):
        vt = make_vt(w, cfg, X0, N_EPOCHS)
        at = 0
        for n in split:
            vt.track(iq_d[at * per:], n)
            at += n
        logs.append(vt.read_log())
        vt.close()
    for n in NAMES + ("mask", "status"):
        assert np.array_equal(logs[0][n], logs[1][n]), n                                          # track(40) == track(13) + track(27), bit for bit
    buf = torch.empty(iq.size + 2, dtype=torch.int16, device="cuda:0")                            # the same record 4 bytes further on
    buf[2:] = iq_d
    vt = make_vt(w, cfg, X0, N_EPOCHS)
    vt.track(buf[2:], N_EPOCHS)
    moved = vt.read_log()
    vt.close()
    assert buf[2:].data_ptr() % 16 == 4
    for n in NAMES + ("mask", "status"):
        assert np.array_equal(logs[0][n], moved[n]), n


@pytest.mark.parametrize("K,T,N,n_epochs", [(6, 0.5e-3, 20, 12), (4, 1e-3, 20, 6), (16, 1e-3, 20, 6)])
def test_shapes(built, oracle, capsys, K, T, N, n_epochs):
    """S % 4 = 2 (T = 0.5 ms -> S = 1250), the minimum of four channels, and the sixteen the update is built for."""
    w, iq, cfg, X0, ref, rnd = small_case(oracle, K, T, N, n_epochs)
    vt = make_vt(w, cfg, X0, n_epochs)
    vt.track(to_dev(iq), n_epochs)
    dev = vt.read_log()
    vt.close()
    hold_to_yardstick(dev, vt_ref.table(ref["recs"]), vt_ref.table(rnd["recs"]), "K = %d, T = %g ms, N = %d (S = %d), %d epochs" % (K, T * 1e3, N, cfg.S, n_epochs), capsys)


def test_chain_scalar_tracker_to_vector_tracker(built, oracle, nominal, capsys):
    """ScalarTracker.track (0.3 s) -> solve_log at its last window -> dpe_vt_init_from_trk -> 20 epochs on the next samples."""
    w, iq, cfg, _, ref = nominal
    s = w["start"]
    M = 300
    iq_d = to_dev(iq)
    trk = dpe.ScalarTracker(cfg.fs, cfg.prns, log_capacity_windows=M)
    trk.set_params([dict(prn=p, rc=c[0], ri=c[1], fc=c[2], fi=c[3]) for p, c in zip(cfg.prns, s["chan"])])
    trk.track(iq_d, M)
    nav = dpe.ScalarNavigator(cfg.prns)
    nav.set_ephemerides(s["eph"], s["tow"], s["cps"])
    fix = nav.solve_log(trk, first=M - 1, n_epochs=1)[0]
    assert fix["status"] == 0 and trk.dev_status() == 0
    vt = dpe.VectorTracker(cfg.fs, cfg.prns, log_capacity_epochs=20)
    vt.set_ephemerides(s["eph"], s["tow"], s["cps"])
    vt.init_from_tracker(trk, fix)
    vt.track(iq_d[2 * M * cfg.S:], 20)
    dev = vt.read_log()
    status = vt.dev_status()
    ho = vt.handoff(bytes_read=4 * (M * cfg.S + 20 * cfg.N * cfg.S))
    vt.close(); trk.close(); nav.close()
    rms = ls_rms(w, ref)
    e0 = np.linalg.norm(np.asarray(fix["X_ECEF"])[:3] - s["X"][:3])
    err = np.linalg.norm(dev["X"][:, :3] - s["X"][:3], axis=1)
    with capsys.disabled():
        print("\nchain: scalar fix %.2f m off X_true; vector tracking, 20 epochs: %s m; LS RMS bound %.2f m"
              % (e0, np.array2string(err, precision=2), rms))
    assert status == 0 and np.all(dev["mask"] == (1 << cfg.K) - 1)                                # no channel excluded
    assert np.all(err < rms), (err, rms)
    cm = dpe.ChanMgr.from_handoff(ho, 0.02)                                                       # the end state is a handoff the DPE loop accepts
    cm.Stop()


def test_pipeline_entry(built, oracle, nominal):
    """pipeline.run_vector_tracking from a handoff dict equals the tracker driven by hand, bit for bit; from a (tracker, navigator)
    pair it is the chain; both end states are handoffs the channel manager accepts."""
    w, iq, cfg, _, _ = nominal
    s = w["start"]
    iq_d = to_dev(iq)
    n = 5
    ho = dict(rxTime=s["rxTime0"], X_ECEF=s["X"], prn_list=np.array(cfg.prns, dtype=np.int32), rc=s["chan"][:, 0], ri=s["chan"][:, 1], fc=s["chan"][:, 2],
              fi=s["chan"][:, 3], cp=s["chan"][:, 4], cp_timestamp=s["cps"], TOW=s["tow"], eph=s["eph"])
    log, end, status = dpe.pipeline.run_vector_tracking(iq_d, ho, cfg.fs, n_epochs=n)
    vt = make_vt(w, cfg, s["X"], n)
    vt.track(iq_d, n)
    direct = vt.read_log()
    vt.close()
    assert status == 0
    for name in NAMES + ("mask", "status"):
        assert np.array_equal(log[name], direct[name]), name
    assert end["rxTime"] == direct["rxTime0"][-1] and np.array_equal(end["rc"], direct["rc"][-1]) and np.array_equal(end["X_ECEF"], direct["X"][-1])
    dpe.ChanMgr.from_handoff(end, 0.02).Stop()
    M = 200
    trk = dpe.ScalarTracker(cfg.fs, cfg.prns, log_capacity_windows=M)
    trk.set_params([dict(prn=p, rc=c[0], ri=c[1], fc=c[2], fi=c[3]) for p, c in zip(cfg.prns, s["chan"])])
    trk.track(iq_d, M)
    nav = dpe.ScalarNavigator(cfg.prns)
    nav.set_ephemerides(s["eph"], s["tow"], s["cps"])
    log2, end2, status2 = dpe.pipeline.run_vector_tracking(iq_d[2 * M * cfg.S:], (trk, nav), cfg.fs, n_epochs=n)
    trk.close(); nav.close()
    assert status2 == 0 and np.all(log2["mask"] == (1 << cfg.K) - 1)
    assert np.linalg.norm(end2["X_ECEF"][:3] - s["X"][:3]) < 30.0                                 # (the chain test holds the bound; here: it ran on the right samples)
    dpe.ChanMgr.from_handoff(end2, 0.02).Stop()
