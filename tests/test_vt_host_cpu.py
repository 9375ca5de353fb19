"""CPU: dpe_vt_filter_step_host (the host form of vt_filter_kernel's source, csrc/dpe_vt_dev.h) against tests/vt_ref.py for one
epoch's discriminators, gate, W, update, predict and steering.  Inputs are sums the restatement logged on the world of
tests/vt_world.py.  The tolerance is 4 x the spread of the restatement's own result over the order its rows are taken in (measured
here, per quantity, as O15 does for the least squares); W and the lock mask are exact."""
import ctypes as C

import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import helpers, vt_ref, vt_world

N, S = 20, 2500
VT = dpe.engine.VectorTracker
NAMES = ("X", "diag", "rc", "ri", "fc", "fi", "cp", "eR", "eV", "lock", "dpc", "dfi")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return dpe.engine.lib()


def host_state(cfg_ref, st):
    """vt_ref's state dict -> dpe_vt_state_rec"""
    h = dpe.engine.VtStateRec()
    for i in range(8):
        h.X[i] = st["X"][i]
    for i in range(64):
        h.Sigma[i] = st["Sigma"].reshape(-1)[i]
    h.rxTime0, h.rxBase, h.epochs, h.status = st["rxTime0"], st["rxBase"], st["epochs"], 0
    h.satValid = 0 if st["sat"] is None else 1
    for k in range(cfg_ref.K):
        c = h.chan[k]
        c.rc, c.ri, c.fc, c.fi, c.cp = (float(st[n][k]) for n in ("rc", "ri", "fc", "fi", "cp"))
        if st["sat"] is not None:
            for i in range(8):
                c.sat[i] = st["sat"][k][i]
        for i in range(cfg_ref.num_prev):
            c.histRange[i], c.histRate[i] = st["histR"][k, i], st["histV"][k, i]
        c.histN, c.histPos = int(st["histN"][k]), int(st["histPos"][k])
    return h


def copy_state(st):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}


def world_epochs(oracle, K, n_epochs):
    """The restatement's state before and the sums of each of its first n_epochs epochs, for K channels."""
    ho = None
    chans = vt_world.CHANS[:K]
    if K > len(vt_world.CHANS):
        ho = vt_world.synthetic_handoff(dpe.handoff.read_handoff(helpers.HANDOFF), K)
        chans = list(range(K))
    w = vt_world.build(oracle, n_epochs * N * S, chans=chans, ho=ho)
    iq = vt_world.record(w)
    cfg = vt_ref.Config(vt_world.FS, w["start"]["prns"], num_prev=3)      # a short history: the measured W is in use from epoch 4 on
    st = vt_ref.new_state(cfg, vt_world.perturbed(w), vt_world.sigma0(), w["start"]["rxTime0"], w["start"]["chan"])
    steps = []
    for e in range(n_epochs):
        s = vt_ref.correlate_epoch(iq, e * N * S, cfg, st)
        steps.append((copy_state(st), s))
        vt_ref.filter_step(cfg, oracle, w["start"]["eph"], w["start"]["tow"], w["start"]["cps"], st, s)
    return w, cfg, steps


def compare(oracle, w, cfg, before, sums, capsys, label, expect_status=0):
    """One epoch on both sides from the same state.  Returns the host record."""
    eph, tow, cps = w["start"]["eph"], w["start"]["tow"], w["start"]["cps"]
    ref = vt_ref.filter_step(cfg, oracle, eph, tow, cps, copy_state(before), sums)
    rng = np.random.default_rng(7)
    spread = {n: np.zeros_like(np.asarray(ref[n], dtype=np.float64)) for n in NAMES}
    for _ in range(6):                                       # the restatement's own noise: the same epoch, rows in another order
        alt = vt_ref.filter_step(cfg, oracle, eph, tow, cps, copy_state(before), sums, order=list(rng.permutation(cfg.K)))
        for n in NAMES:
            spread[n] = np.maximum(spread[n], np.abs(np.asarray(alt[n]) - np.asarray(ref[n])))
    ccfg = VT.config(cfg.fs, cfg.prns, T=cfg.T, N=cfg.N, num_prev=cfg.num_prev)
    h = host_state(cfg, before)
    got = VT.filter_step_host(ccfg, eph, tow, cps, h, sums)
    assert got["mask"] == ref["mask"] and got["status"] == ref["status"] == expect_status, (got["mask"], ref["mask"], got["status"], ref["status"])
    assert np.array_equal(got["wR"], ref["wR"]) and np.array_equal(got["wV"], ref["wV"])         # W is exact
    assert got["rxTime0"] == ref["rxTime0"] and h.epochs == before["epochs"] + 1
    lines = []
    worst = 0.0
    for n in NAMES:
        d = np.abs(np.asarray(got[n]) - np.asarray(ref[n]))
        tol = 4.0 * spread[n]
        lines.append("  %-5s |host - ref| max %.3g   4 x spread max %.3g" % (n, d.max(), tol.max()))
        worst = max(worst, float((d - tol).max()))
    with capsys.disabled():
        print("\n%s: K = %d" % (label, cfg.K))
        print("\n".join(lines))
    for n in NAMES:
        d = np.abs(np.asarray(got[n]) - np.asarray(ref[n]))
        assert np.all(d <= 4.0 * spread[n]), (n, d, 4.0 * spread[n])
    return got, h


@pytest.mark.parametrize("K", [4, 6, 16])
def test_host_matches_restatement(built, oracle, capsys, K):
    w, cfg, steps = world_epochs(oracle, K, 5)
    for e in (0, 4):                                         # the first epoch (configured W, satellite states computed) and one with measured W
        compare(oracle, w, cfg, steps[e][0], steps[e][1], capsys, "epoch %d" % e)


def test_excluded_channel_and_too_few_channels(built, oracle, capsys):
    w, cfg, steps = world_epochs(oracle, 6, 2)
    before, sums = steps[1]
    s = sums.copy()
    rng = np.random.default_rng(3)
    s[:, 2, :6] = rng.normal(0.0, 15000.0, (N, 6))           # channel 2 sees noise alone: excluded, the others update
    got, _ = compare(oracle, w, cfg, before, s, capsys, "channel 2 without signal")
    assert got["mask"] == 0b111011 and got["n_incl"] == 5
    s[:, 3, :6] = rng.normal(0.0, 15000.0, (N, 6))
    s[:, 4, :6] = rng.normal(0.0, 15000.0, (N, 6))           # three left: predict only, status bit 1
    got, _ = compare(oracle, w, cfg, before, s, capsys, "three channels left", expect_status=VT.NO_UPDATE)
    assert got["n_incl"] == 3


def test_non_positive_pivot(built, oracle, capsys):
    w, cfg, steps = world_epochs(oracle, 6, 1)
    before, sums = steps[0]
    b = copy_state(before)
    b["Sigma"] = np.zeros((8, 8))
    eph, tow, cps = w["start"]["eph"], w["start"]["tow"], w["start"]["cps"]
    # W = 0: a history of three equal residuals and no floor (a configured initial variance of 0 selects the default)
    b2 = copy_state(b)
    b2["histN"][:] = 3
    cfgz = vt_ref.Config(vt_world.FS, cfg.prns, num_prev=3, min_var=(0.0, 0.0))
    ref = vt_ref.filter_step(cfgz, oracle, eph, tow, cps, copy_state(b2), sums)
    ccfg = VT.config(cfg.fs, cfg.prns, num_prev=3, min_var=(-1.0, -1.0))
    h = host_state(cfgz, b2)
    got = VT.filter_step_host(ccfg, eph, tow, cps, h, sums)
    assert ref["status"] == VT.PIVOT and got["status"] == VT.PIVOT and h.status == VT.PIVOT
    assert np.array_equal(got["X"][4:], b2["X"][4:]) and np.all(np.isfinite(got["X"]))            # predict only
    assert np.allclose(got["X"], ref["X"], rtol=0, atol=1e-9)


def test_non_finite_input(built, oracle):
    w, cfg, steps = world_epochs(oracle, 6, 1)
    before, sums = steps[0]
    s = sums.copy()
    s[3, 1, 2] = np.nan
    s[7, 5, 0] = np.inf
    eph, tow, cps = w["start"]["eph"], w["start"]["tow"], w["start"]["cps"]
    ref = vt_ref.filter_step(cfg, oracle, eph, tow, cps, copy_state(before), s)
    h = host_state(cfg, before)
    got = VT.filter_step_host(VT.config(cfg.fs, cfg.prns, num_prev=3), eph, tow, cps, h, s)
    assert got["status"] == VT.BAD_WINDOW == ref["status"] and got["mask"] == ref["mask"] == 0b011101
    for n in NAMES + ("wR", "wV"):
        assert np.all(np.isfinite(got[n])), n
    assert np.all(np.isfinite(np.array(h.Sigma)))
    s[:, 0, 6] = -1.0                                         # a window whose boundary case is -1
    h = host_state(cfg, before)
    got = VT.filter_step_host(VT.config(cfg.fs, cfg.prns, num_prev=3), eph, tow, cps, h, s)
    assert got["status"] == (VT.BAD_WINDOW | VT.NO_UPDATE) and got["mask"] == 0b011100
