"""GPU: the joint scan of several receivers over one pair of grids (dpe_bcm_create_joint / engine.JointManifold) against
the fp64 sum over receivers of the oracle's rows, and against the single-receiver scan.

Tolerances are tests/test_gpu_parity.py's, for its reasons, relative to the maximum JOINT score of the window: TOL = 2e-6
against the extended-precision position rows and the velocity rows, helpers.POS_REF_NOISE against the faithful position
rows (the reference's own rxTime - pr / C rounding).  A sum of N rows that each meet a bound relative to their own maximum
meets it relative to the maximum of the sum, because all receivers peak on the same point (tests/test_joint_world_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import helpers, joint_world as jw

pytestmark = pytest.mark.gpu
TOL = 2e-6


class Banks:
    """One BatchCorrScores per receiver, updated with all windows of the world; the handles stay alive (their banks are
    the joint scan's inputs)."""

    def __init__(self, world):
        import torch
        self.world, self.bcs, self.ce, self.bw = world, [], [], []
        for rx in world["rx"]:
            wins = rx["wins"]
            cs = np.stack([dpe.engine.chan_start_array(w["start"]["prn"], w["start"]["rc"], w["start"]["ri"], w["start"]["fc"],
                                                       w["start"]["fi"], w["start"]["cp"], w["start"]["cp_ref"]) for w in wins])
            self.ce.append(np.stack([dpe.engine.chan_end_array(w["sat"], w["rcEnd"], w["fc"], w["fi"], w["cpRefTOW"], w["cpElaEnd"],
                                                               w["cpRef"]) for w in wins]))
            self.bw.append(np.concatenate([dpe.engine.bcm_window_array(w["centre"][None, :], w["R"][None, :], [w["rxTime"]])
                                           for w in wins]))
            b = dpe.BatchCorrScores(world["fs"], samples_per_window=world["S"], lag_half_width=world["L"], bin_half_width=world["B"],
                                    max_windows=world["W"], max_channels=rx["K"])
            b.Start()
            b.Update(torch.from_numpy(np.stack([w["iq"] for w in wins])).to("cuda:0"), cs)
            self.bcs.append(b)

    def rx(self):
        return [[dict(code=dpe.engine.bank_rows(b, w)[0], carr=dpe.engine.bank_rows(b, w)[1], win=self.bw[r][w], chan=self.ce[r][w])
                 for r, b in enumerate(self.bcs)] for w in range(self.world["W"])]

    def close(self):
        for b in self.bcs:
            b.Stop()


def joint_handle(world, lpower=1, own=True, max_total=None, max_rx=None):
    Ks = [rx["K"] for rx in world["rx"]]
    h = dpe.JointManifold(world["fs"], world["S"], world["C"], world["pos"], world["vel"], max_rx or len(Ks), max_total or sum(Ks),
                          LPower=lpower, lag_half_width=world["L"], bin_half_width=world["B"], max_windows=world["W"],
                          max_channels=max(Ks), own_keys=own)
    h.Start()
    return h


def run_joint(world, banks, lpower=1, own=True):
    h = joint_handle(world, lpower, own)
    h.Update(banks.rx())
    res = h.results()
    ps, vs = h.read_scores()
    keys = h.read_keys()
    h.Stop()
    return dict(res=res, pos=ps, vel=vs, keys=keys)


def run_single(world, banks, r, lpower=1):
    """Receiver r alone through dpe_bcm_update on the same banks and inputs."""
    K = world["rx"][r]["K"]
    h = dpe.BatchCorrManifold(world["fs"], world["S"], world["C"], world["pos"], world["vel"], LPower=lpower, lag_half_width=world["L"],
                              bin_half_width=world["B"], max_windows=world["W"], max_channels=K)
    h.Start()
    h.Update(banks.bcs[r].CodeScores, banks.bcs[r].CarrScores, banks.bw[r], banks.ce[r])
    res = h.results()
    ps, vs = h.read_scores()
    keys = dpe.engine.d2h(h.Keys, world["W"] * 16, np.uint64).reshape(-1, 2)
    h.Stop()
    return dict(res=res, pos=ps, vel=vs, keys=keys)


def moved(world, r, w=0):
    """Receiver r's centre moved by the expected grid offset, formed as BCM_MakePosMeas / MakeVelMeas form it."""
    from oracle import oracle as o
    win = world["rx"][r]["wins"][w]
    return o.make_meas(world["pos_at"], world["vel_at"], win["centre"], world["pos"], world["vel"], win["R"])[0]


def check_against_oracle(world, out, ref, w=0, tol=TOL):
    """Scores, arg-max and fixes of window w held to the module's rule; no point is set aside.  Prints the figures first.
    tol: TOL, or 1e-5 for the generic LPower variant (tests/test_gpu_parity.py::test_lpower)."""
    errs = {}
    for name, rname, lim in (("pos", "pos_x", tol), ("pos", "pos", helpers.POS_REF_NOISE), ("vel", "vel", tol)):
        r_, g_ = ref[rname][w], out[name][w]
        errs[rname] = (np.abs(g_ - r_).max() / r_.max(), lim)
    print("joint scan, %d receivers, window %d: " % (len(world["rx"]), w) +
          ", ".join("%s %.3g (bound %.3g)" % (k, v[0], v[1]) for k, v in errs.items()))
    for k, (e, lim) in errs.items():
        assert e < lim, "joint %s row: rel err %.3g" % (k, e)
    j = out["res"][w]
    assert j["posIndex"] == world["pos_at"] == int(np.argmax(ref["pos_x"][w])) and j["velIndex"] == world["vel_at"] == int(np.argmax(ref["vel"][w]))
    assert j["posOutOfWindow"] == 0 and j["velOutOfWindow"] == 0
    assert np.array_equal(j["offset"], world["offset"])
    for r in range(len(world["rx"])):
        z = j["rx"][r]["zVal"]
        assert np.abs(z - moved(world, r, w)).max() < 1e-6          # centre + grid offset (same grid point -> same fix)
        assert np.abs(z - world["rx"][r]["truth"]).max() < 1e-6      # ... which is the truth in this world


@pytest.fixture(scope="module")
def three():
    world = jw.build((5, 8, 4))
    banks = Banks(world)
    yield world, banks
    banks.close()


def test_three_receivers_scores_argmax_own_keys_and_fixes(three, oracle):
    world, banks = three
    ref = jw.oracle_rows(world)
    out = run_joint(world, banks)
    check_against_oracle(world, out, ref)
    for r in range(3):
        single = run_single(world, banks, r)
        own, s = out["res"][0]["rx"][r], single["res"][0]
        for k in ("posIndex", "velIndex", "posOutOfWindow", "velOutOfWindow"):
            assert own[k] == s[k], (r, k)
        assert np.float32(own["posScore"]).tobytes() == np.float32(s["posScore"]).tobytes(), r
        assert np.float32(own["velScore"]).tobytes() == np.float32(s["velScore"]).tobytes(), r
        assert own["posIndex"] == world["pos_at"] and own["velIndex"] == world["vel_at"]


def test_four_receivers_of_ten_svs_beyond_37_channels(oracle):
    world = jw.build((10, 10, 10, 10))
    banks = Banks(world)
    try:
        out = run_joint(world, banks)
        check_against_oracle(world, out, jw.oracle_rows(world))
    finally:
        banks.close()


def test_one_receiver_is_the_single_receiver_scan_bit_for_bit(oracle):
    world = jw.build((6,))
    banks = Banks(world)
    try:
        out, single = run_joint(world, banks), run_single(world, banks, 0)
    finally:
        banks.close()
    assert np.array_equal(out["pos"].view(np.uint32), single["pos"].view(np.uint32))
    assert np.array_equal(out["vel"].view(np.uint32), single["vel"].view(np.uint32))
    assert np.array_equal(out["keys"], single["keys"])
    assert np.array_equal(out["res"][0]["rx"][0]["zVal"], single["res"][0]["zVal"])
    assert out["res"][0]["posIndex"] == single["res"][0]["posIndex"] == out["res"][0]["rx"][0]["posIndex"] == world["pos_at"]


def test_two_windows_lpower_2_own_keys_off_same_joint_bits(oracle):
    world = jw.build((5, 8, 4), seed=1, W=2)
    banks = Banks(world)
    try:
        on, off = run_joint(world, banks, lpower=2, own=True), run_joint(world, banks, lpower=2, own=False)
    finally:
        banks.close()
    assert np.array_equal(on["pos"].view(np.uint32), off["pos"].view(np.uint32))
    assert np.array_equal(on["vel"].view(np.uint32), off["vel"].view(np.uint32))
    assert np.array_equal(on["keys"], off["keys"]) and on["keys"].all()
    ref = jw.oracle_rows(world, lpower=2)
    for w in range(2):
        check_against_oracle(world, on, ref, w)
        for r in range(3):
            assert off["res"][w]["rx"][r]["posIndex"] == -1 and on["res"][w]["rx"][r]["posIndex"] == world["pos_at"]
            assert np.array_equal(off["res"][w]["rx"][r]["zVal"], on["res"][w]["rx"][r]["zVal"])


def test_narrow_banks_clamp_path_counts_per_receiver(oracle):
    """Banks deliberately narrower than the grids reach.  Per-receiver out-of-window counts equal the oracle's (its
    extended-precision count for the position manifold: the faithful one moves a few pairs at the bank edges by its own index
    noise).  Points set aside follow helpers.assert_parity's cap per receiver: against the faithful rows the points where the
    oracle's own two evaluations disagree (at most 16 + pairs / 2000 per receiver), against the extended and the velocity rows
    two points per receiver."""
    world = jw.build((5, 8, 4), widen=False)
    banks = Banks(world)
    try:
        out = run_joint(world, banks)
    finally:
        banks.close()
    ref = jw.oracle_rows(world)
    rows = ref["rx"][0]
    for r, x in enumerate(rows):
        own = out["res"][0]["rx"][r]
        print("receiver %d: out of window pos %d (oracle %d, faithful %d), vel %d (oracle %d)" %
              (r, own["posOutOfWindow"], x["oob_pos_x"], x["oob_pos"], own["velOutOfWindow"], x["oob_vel"]))
    for r, x in enumerate(rows):
        own = out["res"][0]["rx"][r]
        assert own["posOutOfWindow"] == x["oob_pos_x"] and own["velOutOfWindow"] == x["oob_vel"], r
    assert out["res"][0]["posOutOfWindow"] == sum(x["oob_pos_x"] for x in rows)
    assert out["res"][0]["velOutOfWindow"] == sum(x["oob_vel"] for x in rows)
    G = world["pos"].shape[0]
    flips = np.zeros(G, dtype=bool)
    for r, x in enumerate(rows):
        f = np.abs(x["pos"] - x["pos_x"]) > 10 * helpers.POS_REF_NOISE * x["pos"].max()
        f[x["quirks"]] = False          # (the same set tests/test_joint_world_cpu.py counts; empty here: S / 2 is no power of two)
        assert f.sum() <= 16 + G * world["rx"][r]["K"] // 2000
        flips |= f
    for name, rname, lim, aside in (("pos", "pos_x", TOL, 2 * len(rows)), ("pos", "pos", helpers.POS_REF_NOISE, 0),
                                    ("vel", "vel", TOL, 2 * len(rows))):
        r_, g_ = ref[rname][0], out[name][0]
        d = np.abs(g_ - r_) / r_.max()
        if rname == "pos":
            d = d[~flips]
        edge = np.argsort(-d)[:aside]
        edge = edge[d[edge] > 100 * lim]
        keep = np.ones(d.size, dtype=bool)
        keep[edge] = False
        print("narrow banks %s vs %s: rel err %.3g (bound %.3g), %d points set aside" % (name, rname, d[keep].max(), lim, edge.size))
        assert d[keep].max() < lim
    assert out["res"][0]["posIndex"] == int(np.argmax(ref["pos_x"][0])) and out["res"][0]["velIndex"] == int(np.argmax(ref["vel"][0]))


def test_refusals_carry_a_message_and_launch_nothing(three):
    world, banks = three
    h = joint_handle(world, max_total=17, max_rx=3)
    try:
        h.Update(banks.rx())
        before = h.read_keys().copy()
        assert before.all()
        rx, rx0 = banks.rx(), banks.rx()[0]
        bad = banks.bw[2][0].copy()
        bad["enu2ecef"][0] = np.nextafter(bad["enu2ecef"][0], 2.0)
        rx[0][2] = dict(rx[0][2], win=bad)
        with pytest.raises(dpe.DpeError, match="enu2ecef differs"):
            h.Update(rx)
        with pytest.raises(dpe.DpeError, match=r"\(receiver, SV\) pairs, the handle holds 17"):
            h.Update([[rx0[1], rx0[1], rx0[2]]])      # 8 + 8 + 4 pairs
        with pytest.raises(dpe.DpeError, match="use dpe_bcm_update_joint"):
            dpe.engine._check(dpe.engine.lib().dpe_bcm_update(
                h._h, dpe.engine._ptr(banks.bcs[0].CodeScores), dpe.engine._ptr(banks.bcs[0].CarrScores), C.c_int32(1), C.c_int32(5),
                banks.bw[0].ctypes.data_as(C.POINTER(dpe.engine.BcmWindow)), banks.ce[0].ctypes.data_as(C.POINTER(dpe.engine.ChanEnd)),
                dpe.engine._stream(None)))
        ports = dpe.engine.BcmPortsDev(dimT=1, reserved=0)      # (null ports: the joint refusal comes first and nothing is launched)
        with pytest.raises(dpe.DpeError, match="use dpe_bcm_update_joint"):
            dpe.engine._check(dpe.engine.lib().dpe_bcm_update_dev(
                h._h, dpe.engine._ptr(banks.bcs[0].CodeScores), dpe.engine._ptr(banks.bcs[0].CarrScores), C.c_int32(5), C.byref(ports),
                C.c_double(0.0), dpe.engine._stream(None)))
        with pytest.raises(dpe.DpeError, match="use dpe_bcm_update_joint"):
            dpe.engine._check(dpe.engine.lib().dpe_bcm_update_prepared(
                h._h, dpe.engine._ptr(banks.bcs[0].CodeScores), dpe.engine._ptr(banks.bcs[0].CarrScores), C.c_int32(99),
                dpe.engine._stream(None)))
        with pytest.raises(dpe.DpeError, match="use dpe_bcm_update_joint"):      # (also with nChan out of range: the joint refusal first)
            dpe.engine._check(dpe.engine.lib().dpe_bcm_update(
                h._h, dpe.engine._ptr(banks.bcs[0].CodeScores), dpe.engine._ptr(banks.bcs[0].CarrScores), C.c_int32(1), C.c_int32(99),
                banks.bw[0].ctypes.data_as(C.POINTER(dpe.engine.BcmWindow)), banks.ce[0].ctypes.data_as(C.POINTER(dpe.engine.ChanEnd)),
                dpe.engine._stream(None)))
        with pytest.raises(dpe.DpeError, match="use dpe_bcm_results_joint"):
            dpe.BatchCorrManifold.results(h)
        # nothing was launched by the refused calls: the key set of the last good Update is still the current one, unchanged
        keys = C.c_void_p()
        dpe.engine._check(dpe.engine.lib().dpe_bcm_keys(h._h, C.byref(keys)))
        assert keys.value == h.Keys and np.array_equal(h.read_keys(), before)
    finally:
        h.Stop()
    with pytest.raises(dpe.DpeError, match="maxRx 9 out of range"):
        joint_handle(world, max_rx=9)
    with pytest.raises(dpe.DpeError, match="exceeds maxChannelsTotal 4"):       # the bound per receiver (8) above the total
        joint_handle(world, max_total=4)
    with pytest.raises(dpe.DpeError, match="maxChannelsTotal 65 out of range"):
        joint_handle(world, max_total=65)


@pytest.mark.parametrize("start", sorted(jw.LOOP_STARTS))
def test_joint_closed_loop_follows_the_oracle_loop(oracle, start):
    """Three receivers, four windows, every receiver started one grid step off -- in the clock term of a position grid spaced by
    one sample, or in east, north, up and clock at once (joint_world.oracle_loop says why, and why not on the 40 m grid): each
    window's joint arg-max and fixes are those of the same loop driven by the oracle (one oracle channel manager per receiver,
    oracle banks, summed extended-precision rows), and the loop ends on the truth."""
    world = jw.build((5, 8, 4), seed=2, W=4, pos_step=jw.SAMPLE)
    _enu, at1, bound = jw.LOOP_STARTS[start]
    step = jw.loop_step(world, start)
    iqs = [np.stack([w["iq"] for w in rx["wins"]]) for rx in world["rx"]]
    hos = [rx["ho"] for rx in world["rx"]]
    fixes, results = dpe.pipeline.run_joint_closed_loop(iqs, hos, world["fs"], world["pos"], world["vel"], init_delta=step,
                                                        lag_half_width=world["L"], bin_half_width=world["B"])
    ref = jw.oracle_loop(world, step)
    for w in range(4):
        print("window %d: joint arg-max (%d, %d), oracle loop (%d, %d)" % (w, results[w]["posIndex"], results[w]["velIndex"],
                                                                          ref["argmax"][w][0], ref["argmax"][w][1]))
        assert (results[w]["posIndex"], results[w]["velIndex"]) == ref["argmax"][w], w
        assert np.abs(fixes[w] - ref["fixes"][w]).max() < 1e-6
    centre_pt = jw.grid_index((3, 3, 3, 3))
    assert results[1]["posIndex"] == jw.grid_index(at1)      # the one grid step back
    assert results[3]["posIndex"] == centre_pt and results[3]["velIndex"] == centre_pt
    for r in range(3):
        assert np.abs(fixes[3, r] - world["rx"][r]["truth"]).max() < bound
