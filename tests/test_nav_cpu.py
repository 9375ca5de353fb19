"""CPU: the scalar navigation stage's host forms (dpe_nav_decode, dpe_nav_solve, handoff.write_handoff) against fixture O15 --
the reference twin's parse_ephemerides and calculate_nav_soln (tests/golden/make_golden_o15.py) -- and against the test-side
subframe encoder (tests/nav_synth.py)."""
import os

import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import helpers, nav_synth as ns

OUT_NAMES = ("rxTime_a", "rxTime", "x", "y", "z", "c dt", "vx", "vy", "vz", "c dt'")
MARGIN, POS_FLOOR = 4.0, 1e-7    # the margin the tracker's tests give an fp64-rounding yardstick; the twin's own convergence threshold (m)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return dpe.engine.lib()


def sol_bound(o15):
    b = MARGIN * o15["sol_yardstick"].copy()
    b[2:5] += POS_FLOOR
    return b


def fix_row(f):
    return np.concatenate([[f["rxTime_a"], f["rxTime"]], f["X_ECEF"]])


def o15_navigator(o15):
    nav = dpe.ScalarNavigator(o15["sol_prn"])
    nav.set_ephemerides(o15["sol_eph"], o15["sol_tow"], o15["sol_cp_timestamp"])
    return nav


def test_struct_layouts(built):
    import ctypes as C
    assert C.sizeof(dpe.engine.NavDecoded) == 488 and C.sizeof(dpe.engine.NavFix) == 96


@pytest.mark.parametrize("i", range(5))
def test_decode_matches_twin(built, golden, i):
    """Full mode on O15's streams: integers, flags, polarities, status and every decoded double exactly the twin's."""
    g = golden("o15_scalar_nav")
    s = g["dec_streams"][i, :g["dec_n"][i]]
    nav = dpe.ScalarNavigator([1])
    d = nav.decode(0, s, cp_first=int(g["dec_cp0"][i]), mode="full", cp_log=np.arange(g["dec_cp0"][i], g["dec_cp0"][i] + 50.0))
    assert d["status"] == 0
    assert np.array_equal(d["eph"], g["dec_eph"][i])                       # bit for bit
    assert [d["weeknumber"], d["accuracy"], d["health"], d["IODE"], d["IODC"]] == list(g["dec_ints"][i])
    assert [d["timestamp"]["TOW"], d["timestamp"]["cp"]] == list(g["dec_timestamp"][i])
    assert np.array_equal(d["parity"], g["dec_parity"][i]) and np.array_equal(d["polarity"], g["dec_polarity"][i])
    assert np.array_equal(d["subframe_id"], g["dec_ids"][i]) and np.array_equal(d["subframe_cp"], g["dec_subframe_cp"][i])
    assert np.array_equal(nav.eph[0], g["dec_eph"][i])


def test_decode_corrupted_bit_and_few_preambles(built, golden):
    g = golden("o15_scalar_nav")
    N = dpe.ScalarNavigator
    names = list(g["dec_names"])
    i = names.index("corrupt")
    nav = N([1])
    d = nav.decode(0, g["dec_streams"][i, :g["dec_n"][i]], cp_first=int(g["dec_cp0"][i]))
    assert g["dec_raised"][i] == 1                                          # the twin gives up at the failed word
    formed = g["dec_parity"][i][:, 0] >= 0
    assert formed.sum() >= 2 and np.array_equal(d["parity"][formed], g["dec_parity"][i][formed])
    # beyond the subframe the twin raised in there is no reference: that the decoder forms the later subframes too, leaves the one with
    # the failed word out and says so in the status word is this project's own convention
    assert d["parity"].sum() == 49 and d["parity"][1, 5] == 0
    assert d["status"] == N.DEC_PARITY | N.DEC_INCOMPLETE
    assert np.array_equal(d["polarity"][formed], g["dec_polarity"][i][formed])
    assert np.isnan(nav.eph).all()                                          # nothing incomplete is kept
    i = names.index("short")
    d = N([1]).decode(0, g["dec_streams"][i, :g["dec_n"][i]], cp_first=int(g["dec_cp0"][i]))
    assert g["dec_found"][i] == 0 and d["status"] == N.DEC_FEW_PREAMBLES and d["timestamp"] is None
    # a slip in the supplied code-period counts is reported, as the twin warns
    d = N([1]).decode(0, g["dec_streams"][0, :g["dec_n"][0]], cp_first=int(g["dec_cp0"][0]), cp_log=[10.0, 11.0, 13.0])
    assert d["status"] == N.DEC_CP_SLIP


@pytest.mark.parametrize("pol", [1, -1])
def test_encoder_decoder_round_trip(built, pol):
    """Quantised ephemerides through the encoder and back: exact.  Assisted mode: the same timestamp from 7.3 s of signs."""
    ho = dpe.handoff.read_handoff(helpers.HANDOFF)
    rng = np.random.default_rng(5)
    for k in range(ho["prn_list"].size):
        q = ns.quantise(ns.eph_row_to_dict(ho["eph"][k]))
        q["a_f2"], q["IDOT"] = int(rng.integers(-128, 128)), -int(rng.integers(1, 8192))      # fields the recording leaves at 0 / small
        want = ns.dequantise(q)
        tow0, lead, cp0 = 86400 * 3 + 6 * int(rng.integers(0, 100)), 40 + int(rng.integers(0, 5000)), int(rng.integers(0, 10 ** 6))
        bits = ns.encode_bits([5, 1, 2, 3, 4, 5, 1], tow0 - 6, q, week=2100, accuracy=3, health=1, iode=17 + k, iodc=512 + 17 + k)
        s = ns.sign_stream(bits, pol)[6000 - lead:]
        nav = dpe.ScalarNavigator([int(ho["prn_list"][k])])
        d = nav.decode(0, s, cp_first=cp0)
        assert d["status"] == 0 and d["timestamp"] == dict(TOW=tow0, cp=cp0 + lead)
        assert all(d[n] == want[n] for n in ns.EPH_FIELDS), [(n, d[n], want[n]) for n in ns.EPH_FIELDS if d[n] != want[n]]
        assert (d["weeknumber"], d["accuracy"], d["health"], d["IODE"], d["IODC"]) == (1024 + 2100 % 1024, 3, 1, 17 + k, 512 + 17 + k)
        assert np.all(d["polarity"] == pol)
        a = dpe.ScalarNavigator([1]).decode(0, s[:lead + 7300], cp_first=cp0, mode="assisted")
        assert a["status"] == 0 and a["timestamp"] == d["timestamp"]
        short = dpe.ScalarNavigator([1]).decode(0, s[:lead + 7100], cp_first=cp0, mode="assisted")
        assert short["status"] == dpe.ScalarNavigator.DEC_FEW_PREAMBLES


def test_assisted_equals_full_on_o15(built, golden):
    g = golden("o15_scalar_nav")
    for i in range(5):
        s = g["dec_streams"][i, :g["dec_n"][i]]
        a = dpe.ScalarNavigator([1]).decode(0, s, cp_first=int(g["dec_cp0"][i]), mode="assisted")
        ts = g["dec_timestamp"][i]
        assert a["status"] == 0 and a["timestamp"] == dict(TOW=int(ts[0]), cp=int(ts[1]))     # also where the stream starts in subframe 4 or 5


def test_solve_matches_twin(built, golden, capsys):
    """dpe_nav_solve on every O15 epoch against calculate_nav_soln: within 4 x the spread of the twin's own result over the
    satellite orders (+ 1e-7 m on the position, the twin's convergence threshold)."""
    g = golden("o15_scalar_nav")
    nav = o15_navigator(g)
    M = g["sol_cp"].shape[0]
    assert M >= 20 and g["sol_orders"].shape[0] >= 7
    got = np.array([fix_row(nav.solve(g["sol_cp"][m], g["sol_rc"][m], g["sol_fi"][m])) for m in range(M)])
    err = np.abs(got - g["sol_twin"]).max(axis=0)
    bound = sol_bound(g)
    with capsys.disabled():
        print("\nO15 host solve: max |ours - twin| over %d epochs, the yardstick, and their ratio to the bound" % M)
        for n, e, y, b in zip(OUT_NAMES, err, g["sol_yardstick"], bound):
            print("  %-9s err %.3e  yardstick %.3e  err / bound %s" % (n, e, y, "%.3f" % (e / b) if b > 0 else ("0 / 0" if e == 0 else "inf")))
    assert np.all(err <= bound), (err, bound)
    assert nav.status() == 0
    # the rxTime0 schedule (receiver.py:561-569)
    t0, dt = float(g["sol_sched_rxTime0"]), float(g["sol_sched_step"])
    got = np.array([fix_row(nav.solve(g["sol_cp"][m], g["sol_rc"][m], g["sol_fi"][m], rx_time0=t0 + m * dt)) for m in range(M)])
    assert np.all(np.abs(got - g["sol_sched"]).max(axis=0) <= bound)


def test_solve_subsets_and_rank_deficiency(built, golden):
    g = golden("o15_scalar_nav")
    nav = o15_navigator(g)
    cp, rc, fi = g["sol_cp"][3], g["sol_rc"][3], g["sol_fi"][3]
    sel = [0, 2, 3, 5, 7]
    sub = dpe.ScalarNavigator(g["sol_prn"][sel])
    sub.set_ephemerides(g["sol_eph"][sel], g["sol_tow"][sel], g["sol_cp_timestamp"][sel])
    a, b = nav.solve(cp, rc, fi, chans=sel), sub.solve(cp[sel], rc[sel], fi[sel])
    assert np.array_equal(fix_row(a), fix_row(b)) and a["status"] == 0          # a mask and a smaller handle: the same bits
    assert np.abs(a["X_ECEF"][:3] - g["sol_twin"][3, 2:5]).max() < 100.0
    f = nav.solve(cp, rc, fi, chans=[0, 1, 2])                                   # three satellites: no fix, a status bit, no NaN
    assert f["status"] & dpe.ScalarNavigator.SOL_RANK_POS and np.isfinite(fix_row(f)).all()
    twice = dpe.ScalarNavigator(g["sol_prn"][[0, 0, 0, 0, 1]])                   # five rows, rank two
    twice.set_ephemerides(g["sol_eph"][[0, 0, 0, 0, 1]], g["sol_tow"][[0, 0, 0, 0, 1]], g["sol_cp_timestamp"][[0, 0, 0, 0, 1]])
    f = twice.solve(cp[[0, 0, 0, 0, 1]], rc[[0, 0, 0, 0, 1]], fi[[0, 0, 0, 0, 1]])
    assert f["status"] & dpe.ScalarNavigator.SOL_RANK_POS and np.isfinite(fix_row(f)).all()
    with pytest.raises(dpe.DpeError):
        dpe.ScalarNavigator([1, 2, 3, 4]).solve(cp[:4], rc[:4], fi[:4])         # no ephemerides


def test_handoff_round_trip(built, golden, tmp_path):
    ho = dpe.handoff.read_handoff(helpers.HANDOFF)
    p = dpe.handoff.write_handoff(str(tmp_path / "a.csv"), ho)
    back = dpe.handoff.read_handoff(p)
    assert set(back) == set(ho)
    for k in ho:
        assert np.array_equal(np.asarray(back[k]), np.asarray(ho[k])) and np.asarray(back[k]).dtype == np.asarray(ho[k]).dtype, k
    # the rows both files hold are the same text
    shipped = dict(l.split(",", 1) for l in open(helpers.HANDOFF).read().splitlines() if l)
    ours = dict(l.split(",", 1) for l in open(p).read().splitlines() if l)
    assert list(ours)[:12] == list(shipped)[:12] and all(ours[k] == shipped[k] for k in ours)
    # a handoff built in memory from a solution
    g = golden("o15_scalar_nav")
    nav = o15_navigator(g)
    m = 7
    fix = nav.solve(g["sol_cp"][m], g["sol_rc"][m], g["sol_fi"][m])
    h2 = nav.handoff(fix, g["sol_rc"][m], np.linspace(0.1, 0.9, 8), 1.023e6 + g["sol_fi"][m] / 1540.0, g["sol_fi"][m], g["sol_cp"][m], bytes_read=1234)
    back = dpe.handoff.read_handoff(dpe.handoff.write_handoff(str(tmp_path / "b.csv"), h2))
    assert set(back) == set(h2) == set(ho)
    for k in h2:
        assert np.array_equal(np.asarray(back[k]), np.asarray(h2[k])) and np.asarray(back[k]).dtype == np.asarray(ho[k]).dtype, k
    cm = dpe.ChanMgr.from_handoff(back, 0.02)       # the loop's host side takes it as it is
    cm.Stop()
