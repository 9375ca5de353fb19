"""GPU: DopplerSign = -1 through every stage that takes it -- the manifold scan (host coefficient set-up bcm_expand, device set-up
bcm_prep_one, point lists, axes, and the epochs / subsets / joint / refine entry points), the channel manager in the closed loops,
acquisition, the scalar navigator and the vector tracker.  The inputs are proven on the CPU by tests/test_doppler_sign_cpu.py: they
are self-consistent, the references peak where the world puts the peak, and a wrong sign moves the result by 0.88 of a row's maximum.

No bound here is new.  Each test holds the -1 run to what the +1 test of the same path holds its run to, named in its docstring, and
prints the -1 figure next to the +1 figure of the same run where the path has one."""
import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import helpers, mirror, vt_ref
from tests.test_doppler_sign_cpu import K, NARROW, S, VT_SHAPE, W, WIDE, sign_case
from tests.test_gpu_axes_scan import _run as run_grids
from tests.test_gpu_axes_scan import assert_matches_point_list, assert_own_argmax
from tests.test_gpu_epochs import same_bits
from tests.test_gpu_parity import TOL
from tests.test_nav_cpu import sol_bound

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return dpe.engine.lib()


@pytest.fixture(scope="module")
def cases(built, oracle):
    return {-1: sign_case(-1), 1: sign_case(1)}


def to_dev(a, dt=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a if dt is None else np.asarray(a), dtype=dt)).to("cuda:0")


def fmt(worst):
    return ", ".join("%s %.2e" % (k, v) for k, v in sorted(worst.items()))


# ---- scan parity against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("lpower", [1, 2])
@pytest.mark.parametrize("banks", ["wide", "narrow"])
def test_scan_matches_the_oracle_at_minus_one(cases, capsys, banks, lpower):
    """helpers.run_gpu against helpers.run_oracle through helpers.assert_parity as it is, tol = tests/test_gpu_parity.py's TOL (2e-6 of
    the peak; its LPower = 2 test holds the same).  S = 5000, K = 8, 1025-point grids (two tiles, the second ragged), three windows of
    which two come out of propagate.  wide: L = 8, B = 24, every pair inside; narrow: L = B = 1, the clamped variants.  The wide case
    runs at +1 on the same three windows too: a regression of both signs reads differently from one of -1 alone."""
    L, B = WIDE if banks == "wide" else NARROW
    ref = helpers.run_oracle(cases[-1], L, B, lpower=lpower)
    out = helpers.run_gpu(cases[-1], L, B, lpower=lpower)
    line = "scan vs oracle, %s banks (L = %d, B = %d), LPower %d, worst over 3 windows (bound %.0e; faithful pos %.0e):" % (banks, L, B, lpower, TOL, helpers.POS_REF_NOISE)
    plus = None
    if banks == "wide":
        plus = helpers.assert_parity(helpers.run_gpu(cases[1], L, B, lpower=lpower), helpers.run_oracle(cases[1], L, B, lpower=lpower), tol=TOL)
    else:
        assert all(0 < r["velOutOfWindow"] < K * cases[-1]["vel"].shape[0] for r in ref["res"])
    minus = helpers.assert_parity(out, ref, tol=TOL)
    with capsys.disabled():
        print("\n%s\n  ds = -1: %s%s" % (line, fmt(minus), "\n  ds = +1: %s" % fmt(plus) if plus else ""))
    if banks == "wide":
        assert all(r["posIndex"] == 0 and r["velIndex"] == 0 and r["velOutOfWindow"] == 0 for r in out["res"])


# ---- device ports ------------------------------------------------------------------------------------------------------
def test_device_ports_at_minus_one_and_the_refusal_of_another_sign(cases, capsys):
    """BatchCorrManifold.UpdateDev with dopplerSign = [-1] in device memory (bcm_prep_one) against Update with the host window at -1
    (bcm_expand), window 1 of the wide case: scores to 1e-6 of the row maximum, indices and zVal equal -- the device-form block of
    tests/test_gpu_parity.py.  Then [0] and [2] on the device: results() refuses with a message that names DopplerSign, the score rows
    read back are finite (a bad port value is replaced, every index stays in its table), and [-1] again gives the first
    result again.  The comparison runs at +1 on the same window first, for the figure beside."""
    L, B = WIDE
    w = 1
    for sign in (1, -1):
        case = cases[sign]
        win = case["wins"][w]
        iq, cs, ce, bw = helpers.pack_gpu_inputs(case)
        assert bw["dopplerSign"][w] == sign
        bcs = dpe.BatchCorrScores(case["fs"], samples_per_window=S, lag_half_width=L, bin_half_width=B, max_windows=1, max_channels=K)
        bcs.Start()
        bcs.Update(to_dev(iq[w]), cs[w:w + 1])

        def make():
            h = dpe.BatchCorrManifold(case["fs"], S, bcs.NumFFTPoints, case["pos"], case["vel"], lag_half_width=L, bin_half_width=B, max_channels=K)
            h.Start()
            return h

        host = make()
        host.Update(bcs.CodeScores, bcs.CarrScores, bw[w:w + 1], ce[w:w + 1])
        r0 = host.results()[0]
        ps0, vs0 = host.read_scores()
        host.Stop()
        keep = dict(x=to_dev(win["centre"], np.float64), R=to_dev(np.asarray(win["R"]).ravel(), np.float64), sat=to_dev(win["sat"][:, None, :], np.float64),
                    rcE=to_dev(win["rcEnd"], np.float64), fc=to_dev(win["fc"], np.float64), fi=to_dev(win["fi"], np.float64),
                    tow=to_dev(win["cpRefTOW"], np.int32), elaE=to_dev(win["cpElaEnd"], np.int32), ref=to_dev(win["cpRef"], np.int32),
                    ds=to_dev([sign], np.int32))
        ports = dict(xCurrkk1=keep["x"], enu2ecef=keep["R"], satStates=keep["sat"], codePhaseEnd=keep["rcE"], codeFrequency=keep["fc"],
                     carrierFrequency=keep["fi"], cpRefTOW=keep["tow"], cpElapsedEnd=keep["elaE"], cpRef=keep["ref"], dopplerSign=keep["ds"])
        dev = make()
        try:
            def update():
                dev.UpdateDev(bcs.CodeScores, bcs.CarrScores, K, ports, 1, float(win["rxTime"]))

            update()
            r1 = dev.results()[0]
            ps1, vs1 = dev.read_scores()
            ep, ev = np.abs(ps1[0] - ps0[0]).max() / ps0[0].max(), np.abs(vs1[0] - vs0[0]).max() / vs0[0].max()
            with capsys.disabled():
                print("%sdevice ports at ds = %+d vs the host window: pos %.2e, vel %.2e of the row maximum (bound 1e-6)" % ("\n" if sign == 1 else "", sign, ep, ev))
            assert ep < 1e-6 and ev < 1e-6
            assert r1["posIndex"] == r0["posIndex"] == 0 and r1["velIndex"] == r0["velIndex"] == 0
            assert np.array_equal(r1["zVal"], r0["zVal"]) and r1["posOutOfWindow"] == 0 and r1["velOutOfWindow"] == 0
            for bad in ((0, 2) if sign == -1 else ()):
                keep["ds"][0] = bad
                update()
                with pytest.raises(dpe.DpeError, match="DopplerSign"):
                    dev.results()
                ps, vs = dev.read_scores()
                assert np.isfinite(ps).all() and np.isfinite(vs).all()
                keep["ds"][0] = -1
                update()
                r2 = dev.results()[0]
                ps2, vs2 = dev.read_scores()
                assert same_bits(ps2, ps1) and same_bits(vs2, vs1)
                assert (r2["posIndex"], r2["velIndex"], r2["posOutOfWindow"], r2["velOutOfWindow"]) == (r1["posIndex"], r1["velIndex"], 0, 0)
                assert np.float32(r2["posScore"]).tobytes() == np.float32(r1["posScore"]).tobytes() and np.array_equal(r2["zVal"], r1["zVal"])
        finally:
            dev.Stop()
            bcs.Stop()


# ---- axes scan ---------------------------------------------------------------------------------------------------------
def axes_case(cases, sign=-1):
    grids = (dpe.GridAxes.uniform(5, 1.0), dpe.GridAxes.uniform(5, 1.0))
    case = dict(cases[sign])
    case["pos"], case["vel"] = grids[0].points(), grids[1].points()
    return case, grids


def test_axes_scan_at_minus_one(cases, capsys):
    """The -1 windows on 5^4 tensor-product grids (GridAxes.uniform, as tests/test_gpu_axes_scan.py builds its grids): the axes handle
    against the point-list handle on the same banks to that file's standard (scores within 2e-6 of the maximum, an arg-max difference
    only as an fp32 tie, equal zVal; own arg-max and key exact), and against the oracle at tests/test_gpu_parity.py's tolerances as
    that file does.  The per-axis products the axes scan forms from v.g, v.h, pad0 and pad1 all change sign at -1.  The +1 windows
    run the same way first, for the figures beside."""
    L, B = WIDE
    for sign in (1, -1):
        case, grids = axes_case(cases, sign)
        ax = run_grids(case, grids, L, B)
        pl = run_grids(case, grids, L, B, point_list=True)
        assert_own_argmax(ax)
        assert_matches_point_list(ax, pl)
        worst = helpers.assert_parity(ax, helpers.run_oracle(case, L, B), tol=TOL)
        d = max(np.abs(ax[n][w] - pl[n][w]).max() / pl[n][w].max() for n in ("pos", "vel") for w in range(W))
        with capsys.disabled():
            print("%saxes scan at ds = %+d, 5^4 grids: vs the point-list handle %.2e of the maximum (bound 2e-6); vs the oracle %s (bound %.0e)"
                  % ("\n" if sign == 1 else "", sign, d, fmt(worst), TOL))


# ---- the other scan entry points ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def window0(cases):
    """Stage 1 of the wide -1 case (kept alive: its banks are the scans' inputs) and the base handle's result on window 0."""
    case = cases[-1]
    L, B = WIDE
    iq, cs, ce, bw = helpers.pack_gpu_inputs(case)
    bcs = dpe.BatchCorrScores(case["fs"], samples_per_window=S, lag_half_width=L, bin_half_width=B, max_windows=W, max_channels=K)
    bcs.Start()
    bcs.Update(to_dev(iq), cs)
    kw = dict(lag_half_width=L, bin_half_width=B, max_windows=1, max_channels=K)
    h = dpe.BatchCorrManifold(case["fs"], S, bcs.NumFFTPoints, case["pos"], case["vel"], **kw)
    h.Start()
    h.Update(bcs.CodeScores, bcs.CarrScores, bw[:1], ce[:1])
    base = dict(res=h.results()[0], keys=dpe.engine.d2h(h.Keys, 16, np.uint64).copy())
    base["pos"], base["vel"] = h.read_scores()
    h.Stop()
    assert bw["dopplerSign"][0] == -1 and base["res"]["posIndex"] == 0 and base["res"]["velIndex"] == 0
    yield dict(case=case, bcs=bcs, bw=bw[:1], ce=ce[:1], kw=kw, base=base, args=(case["fs"], S, bcs.NumFFTPoints))
    bcs.Stop()


def assert_is_base(got, rows, keys, base):
    """The relation every entry's own suite asserts for its trivial configuration at +1: the base handle's bits."""
    r = base["res"]
    assert same_bits(rows[0], base["pos"]) and same_bits(rows[1], base["vel"]) and np.array_equal(np.ravel(keys), base["keys"])
    for k in ("posIndex", "velIndex", "posOutOfWindow", "velOutOfWindow"):
        assert got[k] == r[k], k
    for k in ("posScore", "velScore"):
        assert np.float32(got[k]).tobytes() == np.float32(r[k]).tobytes(), k
    assert got["zVal"].tobytes() == r["zVal"].tobytes()


def test_one_epoch_is_the_base_scan_at_minus_one(window0):
    """EpochManifold, n_epochs = 1 (tests/test_gpu_epochs.py::test_one_epoch_is_the_single_window_scan_bit_for_bit)."""
    d = window0
    h = dpe.EpochManifold(*d["args"], d["case"]["pos"], d["case"]["vel"], 1, **d["kw"])
    h.Start()
    try:
        h.Update(d["bcs"].CodeScores, d["bcs"].CarrScores, d["bw"], d["ce"], 1)
        res = h.results()[0]
        assert_is_base(res, h.read_scores(), h.read_keys(), d["base"])
        assert res["nPasses"] == 1
    finally:
        h.Stop()


def test_the_full_mask_is_the_base_scan_at_minus_one(window0):
    """SubsetManifold with the full mask as its one subset (tests/test_gpu_subsets.py: the full set's rows, keys and fix are
    dpe_bcm_update's, and a subset's fix is dpe_bcm_update's on its channels -- here all of them)."""
    d = window0
    h = dpe.SubsetManifold(*d["args"], d["case"]["pos"], d["case"]["vel"], 1, **d["kw"])
    h.Start()
    try:
        h.Update(d["bcs"].CodeScores, d["bcs"].CarrScores, d["bw"], d["ce"], np.array([(1 << K) - 1], dtype=np.uint64))
        res = h.results()[0]
        assert_is_base(res, h.read_scores(), h.read_keys(), d["base"])
        sub, r = res["subs"][0], d["base"]["res"]
        for k in ("posIndex", "velIndex", "posOutOfWindow", "velOutOfWindow"):
            assert sub[k] == r[k], k
        assert np.float32(sub["posScore"]).tobytes() == np.float32(r["posScore"]).tobytes()
        assert np.float32(sub["velScore"]).tobytes() == np.float32(r["velScore"]).tobytes()
        assert sub["zVal"].tobytes() == r["zVal"].tobytes() and not res["oobPerSv"].any()
    finally:
        h.Stop()


def test_one_receiver_is_the_base_scan_at_minus_one(window0):
    """JointManifold with one receiver (tests/test_gpu_joint.py::test_one_receiver_is_the_single_receiver_scan_bit_for_bit)."""
    d = window0
    h = dpe.JointManifold(*d["args"], d["case"]["pos"], d["case"]["vel"], 1, K, **d["kw"])
    h.Start()
    try:
        code, carr = dpe.engine.bank_rows(d["bcs"], 0)
        h.Update([dict(code=code, carr=carr, win=d["bw"][0], chan=d["ce"][0])])
        res = h.results()[0]
        r = d["base"]["res"]
        ps, vs = h.read_scores()
        assert same_bits(ps, d["base"]["pos"]) and same_bits(vs, d["base"]["vel"]) and np.array_equal(h.read_keys()[0], d["base"]["keys"])
        assert np.array_equal(res["rx"][0]["zVal"], r["zVal"])
        assert res["posIndex"] == r["posIndex"] == res["rx"][0]["posIndex"] and res["velIndex"] == r["velIndex"] == res["rx"][0]["velIndex"]
        assert res["posOutOfWindow"] == 0 and res["velOutOfWindow"] == 0
    finally:
        h.Stop()


def test_one_level_is_the_axes_scan_at_minus_one(window0, cases):
    """RefineManifold with one level against the axes handle of the 5^4 grids on the same banks
    (tests/test_gpu_refine.py::test_refusals_and_one_level: rows, keys, zVal and indices are the axes handle's bits)."""
    d = window0
    _, (pa, va) = axes_case(cases)
    ax = dpe.BatchCorrManifold(*d["args"], pa, va, **d["kw"])
    ax.Start()
    h = dpe.RefineManifold(*d["args"], [(pa, va)], **d["kw"])
    h.Start()
    try:
        args = (d["bcs"].CodeScores, d["bcs"].CarrScores, d["bw"], d["ce"])
        ax.Update(*args)
        want, (ps, vs) = ax.results()[0], ax.read_scores()
        wk = dpe.engine.d2h(ax.Keys, 16, np.uint64)
        h.Update(*args)
        got, rows = h.results()[0], h.read_scores(0)
        assert same_bits(rows[0], ps) and same_bits(rows[1], vs) and np.array_equal(h.read_keys(0)[0], wk)
        assert got["zVal"].tobytes() == want["zVal"].tobytes()
        assert got["posIndex"][0] == want["posIndex"] and got["velIndex"][0] == want["velIndex"]
        assert got["posOutOfWindow"][0] == want["posOutOfWindow"] == 0 and got["velOutOfWindow"][0] == want["velOutOfWindow"] == 0
    finally:
        h.Stop()
        ax.Stop()


# ---- closed loops ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def moving(built):
    """24 windows of a receiver moving at (5, -3, 2) m/s, the record and the handoff of a +1 receiver and their mirror images."""
    fs, S_, K_, W_ = 2.5e6, 50000, 8, 24
    v = np.array([5.0, -3.0, 2.0])
    iq, _, _, _ = dpe.workload.build_windows(W_, fs, S_, K_, seed=71, amp=200.0, velocity=v)
    ho = dpe.workload.extend_handoff(dpe.handoff.read_handoff(dpe.workload.HANDOFF_CSV), K_)
    pos, vel = dpe.synth.uniform_grid(9, 1.0), dpe.synth.uniform_grid(9, 2.0)
    return dict(fs=fs, K=K_, W=W_, v=v, iq=iq, ho=ho, iq_m=mirror.mirror_iq(iq), ho_m=mirror.mirror_handoff(ho), pos=pos, vel=vel,
                tg=np.unique(pos[:, 3]))


@pytest.mark.parametrize("enable_ekf", [False, True])
def test_closed_loops_at_minus_one(moving, capsys, enable_ekf):
    """run_closed_loop and run_device_loop (ring_depth = 8) at doppler_sign = -1 on the mirrored record from the mirrored handoff, held
    to tests/test_gpu_chm_dev.py::test_device_closed_loop_matches_the_host_driven_loop: equal indices and out-of-window counts per
    window, scores within 2e-6, fixes within 1e-8, status 0; against truth the velocity error above 5 m/s in the first window and below
    2 m/s from window 15 on.  enable_ekf: cuEKF's filter in both loops, held to the same 1e-8 (that file feeds its device filter's
    measurements to the host filter and finds the bits; the two loops as wholes it reports at ~1e-15, their ENU matrices differing in
    the last bit).  The -1 loops put no pair outside the banks from window 5 on
    (tests/test_gpu_parity.py::test_closed_loop_with_a_moving_receiver's criterion).  The sign is not ignored: the same record with the
    loop left at +1 puts velocity pairs outside the banks in window 0 (the handoff's fi against the Doppler of the geometry: centre
    indices 2 fi C / fs off, hundreds of bins), and from window 1 on -- propagate has replaced fi by the geometry's, the wrong one for
    this record -- wipes the carrier off 2 fi away: seven of the eight channels then correlate to noise (1 % of the peak at this
    amplitude), so the velocity score stays below half the right loop's.  Reported, not asserted: in how many windows the -1 loop picks the grid points of the +1 loop on the record as it
    was -- the same mathematics with mirrored carrier banks, where fp32 ties may fall differently."""
    m = moving
    kw = dict(time_grid=m["tg"], K=m["K"], enable_ekf=enable_ekf)
    fixes_h, res_h = dpe.pipeline.run_closed_loop(m["iq_m"], m["ho_m"], m["fs"], m["pos"], m["vel"], doppler_sign=-1, **kw)
    fixes_d, res_d, status = dpe.pipeline.run_device_loop(m["iq_m"], m["ho_m"], m["fs"], m["pos"], m["vel"], ring_depth=8, doppler_sign=-1, **kw)
    fixes_p, res_p, status_p = dpe.pipeline.run_device_loop(m["iq"], m["ho"], m["fs"], m["pos"], m["vel"], ring_depth=8, **kw)
    fixes_hp, res_hp = dpe.pipeline.run_closed_loop(m["iq"], m["ho"], m["fs"], m["pos"], m["vel"], **kw)
    score_p = max(abs(a["posScore"] - b["posScore"]) / b["posScore"] for a, b in zip(res_p, res_hp))
    same = sum(1 for a, b in zip(res_d, res_p) if (a["posIndex"], a["velIndex"]) == (b["posIndex"], b["velIndex"]))
    verr, verr_p = np.linalg.norm(fixes_d[:, 4:7] - m["v"], axis=1), np.linalg.norm(fixes_p[:, 4:7] - m["v"], axis=1)
    score = max(abs(a["posScore"] - b["posScore"]) / b["posScore"] for a, b in zip(res_d, res_h))
    with capsys.disabled():
        print("\nclosed loops at ds = -1, %s, %d windows: device loop vs host-driven loop: fixes %.2e m (bound 1e-8), scores %.2e (bound 2e-6)"
              % ("filter" if enable_ekf else "pass-through", m["W"], np.abs(fixes_d - fixes_h).max(), score))
        print("  ds = +1 on the record as it was, the same two loops: fixes %.2e m, scores %.2e" % (np.abs(fixes_p - fixes_hp).max(), score_p))
        print("  velocity error vs truth: window 0 %.2f m/s, worst from window 15 on %.2f m/s (ds = +1 on the record as it was: %.2f, %.2f)"
              % (verr[0], verr[15:].max(), verr_p[0], verr_p[15:].max()))
        print("  windows whose grid points equal the +1 loop's: %d of %d; largest fix difference %.2e" % (same, m["W"], np.abs(fixes_d - fixes_p).max()))
    assert status == 0 and status_p == 0
    for w in range(m["W"]):
        assert res_d[w]["posIndex"] == res_h[w]["posIndex"] and res_d[w]["velIndex"] == res_h[w]["velIndex"], w
        assert res_d[w]["posOutOfWindow"] == res_h[w]["posOutOfWindow"] and res_d[w]["velOutOfWindow"] == res_h[w]["velOutOfWindow"]
        assert abs(res_d[w]["posScore"] - res_h[w]["posScore"]) <= 2e-6 * res_h[w]["posScore"]
    assert np.abs(fixes_d - fixes_h).max() < 1e-8
    assert verr[0] > 5.0 and verr[15:].max() < 2.0, verr
    assert all(r["posOutOfWindow"] == 0 and r["velOutOfWindow"] == 0 for r in res_d[5:])
    if not enable_ekf:
        _, res_w, _ = dpe.pipeline.run_device_loop(m["iq_m"], m["ho_m"], m["fs"], m["pos"], m["vel"], ring_depth=8, **kw)
        with capsys.disabled():
            print("  the loop left at +1 on this record: window 0 velOutOfWindow %d; velocity score / the -1 loop's, windows 1 on: at most %.3f"
                  % (res_w[0]["velOutOfWindow"], max(a["velScore"] / b["velScore"] for a, b in zip(res_w[1:], res_d[1:]))))
        assert res_w[0]["velOutOfWindow"] > 0
        assert all(a["velScore"] < 0.5 * b["velScore"] for a, b in zip(res_w[1:], res_d[1:]))


# ---- acquisition -------------------------------------------------------------------------------------------------------
def test_acquisition_at_minus_one(golden, oracle, capsys):
    """Fixture O9's two-window record mirrored, through Acquisition(ds = -1): search_signal and the two-window driver against
    oracle.search_signal / oracle.scalar_acquisition(doppler_sign = -1) at the bounds of
    tests/test_gpu_acq.py::test_o9_fine_frequency_and_two_window_driver (same coarse cell and fine FFT bin; rc 1e-9, fi 1e-9, fc 1e-6,
    ri 2e-5 cycles, statistics 2e-4; final rc 1e-6).  The fi found is the +1 run's negated, and fc follows F_CA - (F_CA / F_L1) fi: the
    +1 run's fc."""
    g = golden("o9_scalar_acquisition")
    fs, S_ = float(g["fs"]), int(g["S"])
    prns = [int(p) for p in g["prn_list"]]
    assert np.array_equal(g["bins"], oracle.acq_bins(True))
    iq = np.ascontiguousarray(g["iq"])
    iq_m = mirror.mirror_iq(iq)
    wins, final = oracle.scalar_acquisition(iq_m, fs, prns, doppler_sign=-1.0)
    wins_p, _ = oracle.scalar_acquisition(iq, fs, prns)
    got = {}
    for ds, rec in ((1.0, iq), (-1.0, iq_m)):
        d = to_dev(rec)
        acq = dpe.Acquisition(fs, S_, prns, g["bins"], mode="coherent", ds=ds)
        got[ds] = ([acq.search_signal(d[:2 * S_]), acq.search_signal(d[2 * S_:])], acq.scalar_acquisition(d[:2 * S_], d[2 * S_:]))
        acq.close()
    worst, worst_p = dict(rc=0.0, fi=0.0, fc=0.0, ri=0.0), dict(rc=0.0, fi=0.0, fc=0.0, ri=0.0)
    for w in range(2):
        for p, ref in zip(got[1.0][0][w], wins_p[w]):
            d = abs(p["ri"] - ref["ri"])
            for n, e in (("rc", abs(p["rc"] - ref["rc"])), ("fi", abs(p["fi"] - ref["fi"])), ("fc", abs(p["fc"] - ref["fc"])), ("ri", min(d, 1.0 - d))):
                worst_p[n] = max(worst_p[n], e)
        for i, (r, ref, p) in enumerate(zip(got[-1.0][0][w], wins[w], got[1.0][0][w])):
            assert r["found"] == ref["found"] == p["found"]
            assert (r["max_code_idx"], r["max_dopp_idx"], r["max_carr_idx"]) == (ref["max_code_idx"], ref["max_dopp_idx"], ref["max_carr_idx"])
            d = abs(r["ri"] - ref["ri"])
            for n, e in (("rc", abs(r["rc"] - ref["rc"])), ("fi", abs(r["fi"] - ref["fi"])), ("fc", abs(r["fc"] - ref["fc"])), ("ri", min(d, 1.0 - d))):
                worst[n] = max(worst[n], e)
            assert abs(r["rc"] - ref["rc"]) < 1e-9 and abs(r["fi"] - ref["fi"]) < 1e-9 and abs(r["fc"] - ref["fc"]) < 1e-6
            assert min(d, 1.0 - d) < 2e-5
            assert abs(r["cppr"] / ref["cppr"] - 1) < 2e-4 and abs(r["cppm"] / ref["cppm"] - 1) < 2e-4
            assert abs(r["fi"] + p["fi"]) < 1e-9 and abs(r["fi"]) > 0
            assert abs(r["fc"] - (1.023e6 - (1.023e6 / 1.57542e9) * r["fi"])) < 1e-6 and abs(r["fc"] - p["fc"]) < 1e-6
    for i, (r, p) in enumerate(zip(got[-1.0][1], got[1.0][1])):
        assert r["from_second_window"] == bool(wins[1][i]["cppm"] > wins[0][i]["cppm"])
        assert abs(r["rc"] - final[i, 0]) < 1e-6 and abs(r["fc"] - final[i, 2]) < 1e-6 and abs(r["fi"] - final[i, 3]) < 1e-9
        d = abs(r["ri"] - final[i, 1])
        assert min(d, 1.0 - d) < 2e-5
        assert abs(r["fi"] + p["fi"]) < 1e-9 and abs(r["fc"] - p["fc"]) < 1e-6
    with capsys.disabled():
        print("\nacquisition at ds = -1 on O9 mirrored, vs the oracle at -1: %s (bounds rc 1e-9, fi 1e-9, fc 1e-6, ri 2e-5)" % fmt(worst))
        print("  ds = +1 on O9 as it is, vs the oracle at +1:            %s" % fmt(worst_p))


# ---- scalar navigator --------------------------------------------------------------------------------------------------
def test_solve_log_at_minus_one_is_the_plus_one_result(built, golden, capsys):
    """ScalarNavigator(ds = -1).solve_log on a tracker loaded with O15's rows mirrored: the bytes of solve_log at +1 on the rows as they
    are (the sign enters as fi * ds alone), and so within tests/test_nav_cpu.py's sol_bound of the twin."""
    g = golden("o15_scalar_nav")
    log = dict(cp=g["sol_cp"], rc=g["sol_rc"], fi=g["sol_fi"])
    out = {}
    for ds, rows in ((1.0, log), (-1.0, mirror.mirror_log(log))):
        trk = dpe.ScalarTracker(2.5e6, g["sol_prn"], log_capacity_windows=64, ds=ds)
        trk.load_log(rows)
        nav = dpe.ScalarNavigator(g["sol_prn"], ds=ds)
        nav.set_ephemerides(g["sol_eph"], g["sol_tow"], g["sol_cp_timestamp"])
        out[ds] = nav.solve_log(trk)
        assert nav.status() == 0
        trk.close(); nav.close()
    assert out[-1.0].tobytes() == out[1.0].tobytes() and np.all(out[-1.0]["status"] == 0)
    rows = np.concatenate([out[-1.0]["rxTime_a"][:, None], out[-1.0]["rxTime"][:, None], out[-1.0]["X_ECEF"]], axis=1)
    err, bound = np.abs(rows - g["sol_twin"]).max(axis=0), sol_bound(g)
    with capsys.disabled():
        print("\nsolve_log at ds = -1 on O15 mirrored: the +1 bytes; worst |ours - twin| / bound over the outputs %.3f" % np.max(err[bound > 0] / bound[bound > 0]))
    assert np.all(err <= bound), (err, bound)


# ---- vector tracker ----------------------------------------------------------------------------------------------------
def test_vector_tracker_at_minus_one(built, oracle, capsys):
    """K = 6, T = 1 ms, N = 20, 8 epochs from 30 m off, num_prev = 4, the world and the loop at ds = -1: tests/test_gpu_vt.py's
    hold_to_yardstick as it is (4 x the fp32-rounded reference's own deviation, masks and status equal) and dev_status() == 0."""
    from tests import test_gpu_vt as tv
    s = VT_SHAPE
    w, iq, cfg, X0, ref, rnd = tv.small_case(oracle, s["K"], s["T"], s["N"], s["n_epochs"], ds=-1.0)
    assert cfg.ds == -1.0 and np.all(w["start"]["chan"][:, 3] == w["ch"]["fi"])
    vt = tv.make_vt(w, cfg, X0, s["n_epochs"])
    assert vt.cfg.dopplerSign == -1.0
    vt.track(tv.to_dev(iq), s["n_epochs"])
    dev = vt.read_log()
    status = vt.dev_status()
    vt.close()
    err = np.linalg.norm(dev["X"][:, :3] - w["start"]["X"][:3], axis=1)
    with capsys.disabled():
        print("\nvector tracker at ds = -1: device position error by epoch (m) %s, masks %s" % (np.round(err, 1), [int(v) for v in dev["mask"]]))
    tv.hold_to_yardstick(dev, vt_ref.table(ref["recs"]), vt_ref.table(rnd["recs"]), "ds = -1, K = 6, T = 1 ms, N = 20, 8 epochs", capsys)
    assert status == 0 and np.all(dev["mask"] == (1 << cfg.K) - 1)
    # the same shape at +1, for the figures beside (tests/test_gpu_vt.py::test_shapes' check)
    w, iq, cfg, X0, ref, rnd = tv.small_case(oracle, s["K"], s["T"], s["N"], s["n_epochs"])
    vt = tv.make_vt(w, cfg, X0, s["n_epochs"])
    vt.track(tv.to_dev(iq), s["n_epochs"])
    dev = vt.read_log()
    vt.close()
    tv.hold_to_yardstick(dev, vt_ref.table(ref["recs"]), vt_ref.table(rnd["recs"]), "ds = +1, the same shape", capsys)
