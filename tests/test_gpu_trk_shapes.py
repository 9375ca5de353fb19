"""GPU: the scalar tracker (csrc/dpe_trk.hip) and the navigator's log reader (csrc/dpe_nav.hip) where tests/test_gpu_trk.py and
tests/test_gpu_nav.py hold their inputs constant: window lengths that are no multiple of 4 samples (unaligned windows, a partial
quad at every window's end), T of 0.5 and 1.5 ms (boundary cases 0 and 2 in every second window), ds = -1, hand-made
parameters at the ends of the code phase and on either side of the case decision, the fourth branch (a frozen channel) and log /
sign rings that wrap.  Inputs: tests/trk_shapes.py, proven on the CPU by tests/test_trk_shapes_cpu.py.

Reference and bounds are those of tests/test_gpu_trk.py, imported from there: tests/trk_ref.py in fp64; closed loop within
4 x the yardstick (trk_ref with fp32 E / P / L) per logged quantity and equal where the yardstick is 0; teacher-forced sums within
TOL = 2e-6 of the channel's prompt peak; everything integer, and every invariance, bit for bit.
Each figure is printed before it is asserted (run with -s to see them).

Measured (MI355X): largest device / yardstick ratio 1.48, 0.97, 0.76 and 1.04 at the four closed-loop shapes, no sign left out;
teacher-forced E / P / L and segment sums within 1.9e-8 of the prompt peak over all rows; every invariance bit for bit."""
import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import trk_ref, trk_shapes as ts
from tests.test_gpu_trk import TOL, _bits, _compare, _init, _yardstick
from tests.test_nav_cpu import o15_navigator

pytestmark = pytest.mark.gpu
NAMES = dpe.ScalarTracker.LOG_NAMES


def _dev(iq, offset=0):
    """The record on the device, `offset` int16 values (2 bytes each) past a 16-byte boundary."""
    import torch
    buf = torch.empty(iq.size + 8, dtype=torch.int16, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    d = buf[offset:offset + iq.size]
    d.copy_(torch.from_numpy(np.array(iq)))
    assert d.data_ptr() % 16 == 2 * offset
    return d


def _run(r, iq_d, pieces, chans=None, cap=None):
    """Track sum(pieces) windows of record r in len(pieces) launches.  Returns (log, signs, state)."""
    sel = list(range(len(ts.PRNS))) if chans is None else list(chans)
    prns = [ts.PRNS[k] for k in sel]
    trk = dpe.ScalarTracker(r["fs"], prns, T=r["T"], log_capacity_windows=sum(pieces) if cap is None else cap, ds=r["ds"])
    trk.set_params(_init(prns, r["start"][sel]))
    assert trk.S == r["S"]
    done = 0
    for n in pieces:
        trk.track(iq_d[2 * r["S"] * done:], n)
        done += n
    log = trk.read_log()
    signs = [trk.read_cp_signs(k) for k in range(len(sel))]
    st = trk.state()
    assert trk.dev_status() == 0
    trk.close()
    return log, signs, st


def _same(a, b, what):
    (la, sa, ta), (lb, sb, tb) = a, b
    for n in NAMES:
        assert np.array_equal(_bits(la[n]), _bits(lb[n])), (what, n)
    assert len(sa) == len(sb) and all(np.array_equal(x, y) for x, y in zip(sa, sb)), what
    assert ta == tb, what


@pytest.mark.parametrize("shape", ts.SHAPES, ids=ts.SHAPE_IDS)
def test_closed_loop_at_shape(shape):
    fs, T, M, ds = shape
    r, x = ts.record(*shape), ts.reference(*shape)
    ref, g, label = x["ref"], x["g"], ts.SHAPE_IDS[ts.SHAPES.index(shape)]
    yard = _yardstick(g, ref, x["rounded"], M)
    iq_d = _dev(r["iq"])
    dev, signs, st = one = _run(r, iq_d, [M])
    assert np.array_equal(dev["case"].astype(np.int64), x["case"])
    assert np.array_equal(dev["cp_compl"][:-1], np.diff(dev["cp"], axis=0)) and np.array_equal(dev["cp_compl"], np.maximum(x["case"], 0))
    for k in range(2):
        n = x["signs"][k].size
        med = np.median(np.hypot(ref["iP"][:M, k], ref["qP"][:M, k]))
        keep = np.abs(x["ps"][k]) >= 0.01 * med
        print("%s cp_sign ch %d: %d signs, %d left out, %d differ" % (label, k, n, n - keep.sum(), (signs[k] != x["signs"][k]).sum()))
        assert st[k]["nSigns"] == n == signs[k].size and st[k]["cp"] == n == dev["cp"][M - 1, k] + dev["cp_compl"][M - 1, k]
        assert keep.mean() >= 0.99 and np.array_equal(signs[k][keep], x["signs"][k][keep].astype(np.int8))
        assert st[k]["frozen"] == 0 and st[k]["nWindows"] == M
        for n_ in ("rc", "ri", "fc", "fi"):                       # the state holds the NEXT window's parameters: the log's row M
            y = np.abs(x["rounded"][n_][:M + 1] - ref[n_][:M + 1]).max()
            assert abs(st[k][n_] - ref[n_][M, k]) <= 4.0 * y, (n_, k)
    _compare(g, dev, ref, yard, M, label)
    # invariances, bit for bit.  Two launches cut at an odd window: the second starts on a window 8 bytes off a 16-byte boundary
    # where S % 4 == 2.  (Each window keeps its address whatever the cut, so what flips every window between the 16-byte and the
    # 4-byte loads is the same record 4, 8 and 12 bytes further on.)
    a = M // 2 - 1
    assert a % 2 == 1 and (r["S"] % 4 == 0 or (4 * r["S"] * a) % 16 == 8)
    _same(one, _run(r, iq_d, [a, M - a]), "track(%d) then track(%d)" % (a, M - a))
    for off in (2, 4, 6):
        _same(one, _run(r, _dev(r["iq"], off), [M]), "record %d bytes off" % (2 * off))
    for k in range(2):                                            # K = 2 in one launch == each channel alone
        d, sd, td = _run(r, iq_d, [M], chans=[k])
        for n in NAMES:
            assert np.array_equal(_bits(dev[n][:, k]), _bits(d[n][:, 0])), (n, k)
        assert np.array_equal(signs[k], sd[0]) and st[k] == td[0]


@pytest.mark.parametrize("fs,T", [(2.5e6, 1e-3), (2.5e6, 0.5e-3)], ids=["S2500", "S1250"])
def test_teacher_forced_correlator_at_edge_parameters(fs, T):
    S, M = int(round(T * fs)), ts.N_EDGE
    p, clean = ts.edge_params(fs, T)
    r = ts.record(fs, T, M, 1.0)
    ref = ts.correlate_ref(r["iq"], fs, S, p)
    iq_d = _dev(r["iq"])
    trk = dpe.ScalarTracker(fs, ts.PRNS, T=T, log_capacity_windows=8)
    base = trk.correlate(iq_d, clean)
    assert trk.dev_status() == 0 and (base["case"] >= 0).all()
    out = trk.correlate(iq_d, p)
    assert trk.dev_status() & 1                                   # the fourth branch: a status bit in ordinary arithmetic
    trk.set_params(_init(ts.PRNS, r["start"]))
    assert trk.dev_status() == 0
    trk.close()
    bad = ref["case"] < 0
    assert bad.sum() == 2 and np.array_equal(out["case"], ref["case"]) and np.array_equal(out["cp_compl"], ref["cp_compl"])
    ok = np.isfinite(p).all(axis=2)
    assert np.array_equal(out["idxs1"][ok], ref["idxs1"][ok]) and np.array_equal(out["idxs2"][ok], ref["idxs2"][ok])
    for n in ("seg", "epl", "signs"):                             # zero outputs for the fourth branch ...
        assert (out[n][bad] == 0).all(), n
        assert np.array_equal(out[n][~bad], base[n][~bad]) if n == "signs" else \
            np.array_equal(_bits(out[n][~bad].view(np.float64)), _bits(base[n][~bad].view(np.float64))), n   # ... neighbours unchanged
    for n in ("case", "cp_compl", "idxs1", "idxs2"):
        assert np.array_equal(out[n][~bad], base[n][~bad]), n
    for k in range(2):
        peak = np.abs(ref["epl"][:, k, 1]).max()
        decided = np.abs(ref["ps"][:, k]) >= 0.01 * peak
        print("S = %d ch %d: %d signs, %d decided on >= 1 %% of the prompt peak" % (S, k, ref["cp_compl"][:, k].sum(), decided.sum()))
        assert np.array_equal(out["signs"][:, k][decided], ref["signs"][:, k][decided])
        assert (out["signs"][:, k][np.arange(2) >= ref["cp_compl"][:, k, None]] == 0).all()
        for m, name in enumerate(ts.EDGE_ROWS):
            e = np.abs(out["epl"][m, k] - ref["epl"][m, k]).max() / peak
            s = np.abs(out["seg"][m, k] - ref["seg"][m, k]).max() / peak
            print("S = %d ch %d %-13s case %2d  e/p/l %.3e  segment sums %.3e of the prompt peak" % (S, k, name, ref["case"][m, k], e, s))
        assert np.abs(out["epl"][:, k] - ref["epl"][:, k]).max() / peak < TOL
        assert np.abs(out["seg"][:, k] - ref["seg"][:, k]).max() / peak < TOL


def test_frozen_channel_in_the_closed_loop():
    """Three channels, the middle one started with fc = -1.023e6: the twin's "EXTREME ERROR" as a status bit and a frozen channel."""
    fs, T, M, ds = ts.RING_SHAPE
    M = 40
    r = ts.record(fs, T, ts.RING_SHAPE[2], ds, extra=ts.RING_EXTRA + 1)
    iq_d = _dev(r["iq"])
    S = r["S"]
    prns = [ts.PRNS[0], 15, ts.PRNS[1]]
    bad = np.array([511.25, 0.4, ts.BAD_FC, 300.0])
    start = np.stack([r["start"][0], bad, r["start"][1]])
    trk = dpe.ScalarTracker(fs, prns, T=T, log_capacity_windows=2 * M)
    two = dpe.ScalarTracker(fs, ts.PRNS, T=T, log_capacity_windows=2 * M)
    trk.set_params(_init(prns, start))
    two.set_params(_init(ts.PRNS, r["start"]))
    for call in range(2):                                         # the second call keeps it frozen and sets no further state
        trk.track(iq_d[2 * S * M * call:], M)
        two.track(iq_d[2 * S * M * call:], M)
        n = M * (call + 1)
        assert trk.dev_status() == 1 and two.dev_status() == 0
        st, log, ref = trk.state(), trk.read_log(), two.read_log()
        f = st[1]
        assert f["frozen"] == 1 and f["cp"] == 0 and f["nSigns"] == 0 and f["lock"] == 0 and f["nWindows"] == n
        assert [f["rc"], f["ri"], f["fc"], f["fi"]] == list(bad) and f["paRe"] == 0.0 and f["paIm"] == 0.0
        assert f["fi_bias"] == bad[3] and f["fc_bias"] == bad[2] - trk_ref.F_CA - 1.0 * trk_ref.F_CA / trk_ref.F_L1 * bad[3]
        assert trk.read_cp_signs(1).size == 0
        assert (log["case"][:, 1] == -1).all() and (log["cp_compl"][:, 1] == 0).all() and (log["cp"][:, 1] == 0).all()
        for j, name in enumerate(("rc", "ri", "fc", "fi")):
            assert (log[name][:, 1] == bad[j]).all(), name
        assert (log["fc_bias"][:, 1] == f["fc_bias"]).all() and (log["fi_bias"][:, 1] == bad[3]).all() and (log["lock"][:, 1] == 0).all()
        for name in NAMES:
            if name not in ("cp", "rc", "ri", "fc", "fi", "fc_bias", "fi_bias", "lock", "case", "cp_compl"):
                assert np.isnan(log[name][:, 1]).all(), name      # the correlations among them
        for k3, k2 in ((0, 0), (2, 1)):                           # the neighbours: as if it were not there
            for name in NAMES:
                assert log[name].shape == (n, 3) and np.array_equal(_bits(log[name][:, k3]), _bits(ref[name][:, k2])), (name, k3)
            assert np.array_equal(trk.read_cp_signs(k3), two.read_cp_signs(k2))
            assert st[k3] == two.state()[k2] and st[k3]["frozen"] == 0
    trk.set_params(_init(prns, np.stack([r["start"][0], [511.25, 0.4, trk_ref.F_CA, 300.0], r["start"][1]])))
    assert trk.dev_status() == 0 and all(s["frozen"] == 0 and s["nWindows"] == 0 for s in trk.state())
    trk.track(iq_d, 3)                                            # and the channel runs again
    assert trk.dev_status() == 0 and (trk.read_log()["case"] >= 0).all()
    trk.close()
    two.close()


def test_log_and_sign_rings_wrap():
    """A 24-window log (a 50-entry sign ring) tracked as 37 + 63 windows against a 100-window log tracked in one call; then 7
    more windows, after which the 50 newest signs lie across the sign ring's end as well."""
    fs, T, M, ds = ts.RING_SHAPE
    E = ts.RING_EXTRA
    r = ts.record(fs, T, M, ds, extra=E + 1)
    iq_d = _dev(r["iq"])
    S, CAP, SCAP = r["S"], 24, 50

    def tracker(cap):
        t = dpe.ScalarTracker(fs, ts.PRNS, T=T, log_capacity_windows=cap)
        t.set_params(_init(ts.PRNS, r["start"]))
        return t

    def check(A, B, n, a_first):
        """B's ring against A, which holds the windows from a_first on in order"""
        full = A.read_log(first=a_first)
        assert A.state() == B.state() and A.dev_status() == 0 and B.dev_status() == 0
        reads = [(n - CAP, CAP), (n - 20, 15), (n - 10, 10)] + [(f, 6) for f in range(n - CAP, n - 6) if f % CAP == CAP - 3]
        assert any(f % CAP + c > CAP for f, c in reads) and any(f % CAP + c <= CAP for f, c in reads)
        for f, c in reads:
            got = B.read_log(first=f, n=c)
            for name in NAMES:
                assert got[name].shape == (c, 2) and np.array_equal(_bits(got[name]), _bits(full[name][f - a_first:f - a_first + c])), (name, f, c)
        for f, c in [(n - CAP - 1, 1), (n - CAP - 1, 5), (n, 1), (n - 3, 4), (0, 1)]:
            with pytest.raises(dpe.DpeError):
                B.read_log(first=f, n=c)
        wrapped = False
        for k in range(2):
            ns = B.state()[k]["nSigns"]
            sa = A.read_cp_signs(k)
            assert sa.size == ns and set(sa) <= {-1, 1}
            edge = ns - ns % SCAP                                 # the sign ring's end among the newest SCAP entries
            reads = [(ns - SCAP, SCAP), (ns - 20, 20), (ns - 31, 17)] + ([(edge - 3, 6)] if 3 <= ns % SCAP <= SCAP - 3 else [])
            for f, c in reads:
                wrapped |= f % SCAP + c > SCAP
                assert np.array_equal(B.read_cp_signs(k, first=f, n=c), sa[f:f + c]), (k, f, c)
            for f, c in [(ns - SCAP - 1, 1), (ns - SCAP - 1, 10), (ns, 1), (ns - 2, 3)]:
                with pytest.raises(dpe.DpeError):
                    B.read_cp_signs(k, first=f, n=c)
        return wrapped

    A, B = tracker(M), tracker(CAP)
    A.track(iq_d, M)
    B.track(iq_d, 37)                                             # the wrap falls inside a launch (24 < 37) ...
    B.track(iq_d[2 * S * 37:], 63)                                # ... and between launches
    check(A, B, M, 0)                                             # reads (76, 24), (80, 15), (90, 10): the last straddles the ring's end
    A.close()
    A = tracker(M + E)
    A.track(iq_d, M + E)
    B.track(iq_d[2 * S * M:], E)
    assert check(A, B, M + E, 0)                                  # the newest 50 signs now wrap too
    A.close()
    B.close()


def test_navigator_reads_a_wrapped_log(golden):
    """nav_solve_log_kernel's slot (firstWindow + e stride) % logCap: a 16-window log after 40 windows against the same rows loaded
    into the windows 0 .. 15 of another tracker.  Same inputs, other slots: the fixes are equal bit for bit."""
    import torch
    g = golden("o15_scalar_nav")
    prns = [int(p) for p in g["sol_prn"]]
    K, fs, S, CAP, M = len(prns), 2.5e6, 2500, 16, 40
    rng = np.random.Generator(np.random.PCG64(40))
    iq_d = torch.from_numpy(np.rint(300.0 * rng.standard_normal(2 * S * (M + 1))).astype(np.int16)).to("cuda:0")
    fi = g["sol_fi"][0]
    start = np.stack([g["sol_rc"][0], np.linspace(0.05, 0.9, K), ts.fc_of(fi), fi], axis=1)
    nav = o15_navigator(g)
    Ct, Dt = dpe.ScalarTracker(fs, prns, log_capacity_windows=CAP), dpe.ScalarTracker(fs, prns, log_capacity_windows=CAP)
    Ct.set_params(_init(prns, start))
    Ct.track(iq_d, 13)
    Ct.track(iq_d[2 * S * 13:], M - 13)
    assert Ct.dev_status() == 0
    rows = Ct.read_log(first=M - CAP, n=CAP)
    assert all(not np.isnan(rows[n]).any() for n in ("cp", "rc", "fi")) and len(np.unique(rows["rc"])) == CAP * K
    Dt.load_log(rows)
    back = Dt.read_log()
    for n in NAMES:
        assert np.array_equal(_bits(back[n]), _bits(rows[n])), n
    for first, stride in ((M - CAP, 1), (M - CAP + 1, 3), (M - 1, 1), (M - CAP + 5, 2)):
        n = (M - first + stride - 1) // stride
        c = nav.solve_log(Ct, first=first, n_epochs=n, stride=stride)
        d = nav.solve_log(Dt, first=first - (M - CAP), n_epochs=n, stride=stride)
        print("solve_log first %d stride %d: %d epochs, %d with finite fixes" % (first, stride, n, np.isfinite(c["X_ECEF"]).all(axis=1).sum()))
        assert c.shape == (n,) and c.tobytes() == d.tobytes(), (first, stride)
    one = nav.solve_log(Ct, first=M - CAP, n_epochs=CAP)
    assert len({one[i:i + 1].tobytes() for i in range(CAP)}) == CAP          # every epoch its own fix: a wrong slot would show
    for first, n in ((M - CAP - 1, 1), (M - CAP - 1, CAP), (M - 1, 2), (M, 1)):
        with pytest.raises(dpe.DpeError):
            nav.solve_log(Ct, first=first, n_epochs=n)
    for t in (Ct, Dt, nav):
        t.close()
