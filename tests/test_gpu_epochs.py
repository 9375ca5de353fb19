"""GPU: the multi-epoch manifold scan (dpe_bcm_create_epochs / engine.EpochManifold) -- N consecutive windows summed into one
score row and one arg-max -- against the rows dpe_bcm_update gives the same windows, against the fp64 sum of the oracle's
per-window rows, and against itself under other cuts into passes and groups.  Inputs: tests/epoch_world.py, proven on the CPU
by tests/test_epoch_world_cpu.py.

Bounds.  Against the GPU's own per-window rows: the group row is an fp32 sum of N non-negative fp32 terms added in window
order, so it differs from their exact (fp64) sum by at most (N - 1) 2^-24 of the point's sum (each add rounds by at most
half an ulp of a partial sum that never exceeds the total).  Against the oracle: tests/test_gpu_parity.py's scores tolerance
(2e-6 against the extended-precision position rows and the velocity rows, helpers.POS_REF_NOISE against the faithful
position rows), relative to the row maximum, plus that accumulation bound.  Everything else is bit equality."""
import ctypes as C

import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import epoch_world as ew, helpers

pytestmark = pytest.mark.gpu
TOL = ew.ORACLE_TOL


class Banks:
    """Stage 1 over all windows of a world in one call; the handle stays alive (its banks are the scans' inputs)."""

    def __init__(self, world):
        import torch
        self.world = world
        self.cs, self.ce, self.bw, iq = ew.gpu_inputs(world)
        self.bcs = dpe.BatchCorrScores(world["fs"], samples_per_window=world["S"], lag_half_width=world["L"], bin_half_width=world["B"],
                                       max_windows=world["N"], max_channels=world["K"])
        self.bcs.Start()
        self.bcs.Update(torch.from_numpy(iq).to("cuda:0"), self.cs)

    def rows(self, first=0):
        return dpe.engine.bank_rows(self.bcs, first)

    def close(self):
        self.bcs.Stop()


def grids_of(world, cut):
    return (world["pos"], world["vel"]) if cut is None else (world["pos"][:cut[0]], world["vel"][:cut[1]])


def run_epochs(world, banks, n_epochs, first=0, count=None, pairs_per_pass=0, cut=None, lpower=1):
    """Windows first .. first + count - 1 as groups of n_epochs in ONE launch."""
    count = world["N"] - first if count is None else count
    pos, vel = grids_of(world, cut)
    h = dpe.EpochManifold(world["fs"], world["S"], world["C"], pos, vel, n_epochs, pairs_per_pass, LPower=lpower,
                          lag_half_width=world["L"], bin_half_width=world["B"], max_windows=count, max_channels=world["K"])
    h.Start()
    try:
        code, carr = banks.rows(first)
        h.Update(code, carr, banks.bw[first:first + count], banks.ce[first:first + count], n_epochs)
        res = h.results()
        ps, vs = h.read_scores()
        keys = h.read_keys()
    finally:
        h.Stop()
    return dict(res=res, pos=ps, vel=vs, keys=keys)


def run_single(world, banks, cut=None, lpower=1):
    """Every window alone through dpe_bcm_update (one batch) on the same banks and inputs."""
    pos, vel = grids_of(world, cut)
    h = dpe.BatchCorrManifold(world["fs"], world["S"], world["C"], pos, vel, LPower=lpower, lag_half_width=world["L"],
                              bin_half_width=world["B"], max_windows=world["N"], max_channels=world["K"])
    h.Start()
    try:
        h.Update(banks.bcs.CodeScores, banks.bcs.CarrScores, banks.bw, banks.ce)
        res = h.results()
        ps, vs = h.read_scores()
        keys = dpe.engine.d2h(h.Keys, world["N"] * 16, np.uint64).reshape(-1, 2)
    finally:
        h.Stop()
    return dict(res=res, pos=ps, vel=vs, keys=keys)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def key_index(key):
    return 0xFFFFFFFF - int(key & np.uint64(0xFFFFFFFF))


@pytest.fixture(scope="module")
def five():
    world = ew.build(N=5, K=8)
    banks = Banks(world)
    yield world, banks
    banks.close()


@pytest.fixture(scope="module")
def twelve():
    world = ew.build(N=12, K=4, seed=1)
    banks = Banks(world)
    yield world, banks
    banks.close()


def test_group_row_is_the_sum_of_the_window_rows(five, oracle):
    """1.  N = 5, K = 8, one group: both rows against the fp64 sum of dpe_bcm_update's rows and against the oracle's sum; every point."""
    world, banks = five
    N = world["N"]
    out, single, ref = run_epochs(world, banks, N), run_single(world, banks), ew.oracle_rows(world)
    assert out["pos"].shape == (1, 2401) and out["vel"].shape == (1, 2401) and out["res"][0]["nPasses"] == 1
    acc = (N - 1) * 2.0 ** -24
    for name in ("pos", "vel"):
        want = single[name].astype(np.float64).sum(axis=0)
        got = out[name][0].astype(np.float64)
        err = np.abs(got - want)
        print("epochs %s row vs the sum of the GPU's %d window rows: worst %.3g of the point's sum (bound %.3g)"
              % (name, N, (err / want).max(), acc))
        assert np.all(want > 0) and np.all(err <= acc * want)
        # the same fp32 adds in the same order give the same bits
        seq = single[name][0].copy()
        for e in range(1, N):
            seq = seq + single[name][e]
        assert same_bits(out[name][0], seq)
    for name, rname, lim in (("pos", "pos_x", TOL), ("pos", "pos", helpers.POS_REF_NOISE), ("vel", "vel", TOL)):
        r_, g_ = ref[rname], out[name][0].astype(np.float64)
        err = np.abs(g_ - r_)
        print("epochs %s row vs the oracle's summed %s rows: %.3g of the row maximum (bound %.3g + accumulation)"
              % (name, rname, err.max() / r_.max(), lim))
        assert np.all(err <= lim * r_.max() + acc * r_)
    j = out["res"][0]
    assert j["posIndex"] == world["pos_at"] and j["velIndex"] == world["vel_at"]
    assert j["posOutOfWindow"] == 0 and j["velOutOfWindow"] == 0
    assert np.array_equal(j["offset"], world["offset"])
    assert np.abs(j["zVal"] - world["truth"][N - 1]).max() < 1e-6          # the LAST window's centre moved by the offset


def test_one_epoch_is_the_single_window_scan_bit_for_bit(five):
    """2.  n_epochs = 1: three windows as three groups against dpe_bcm_update."""
    world, banks = five
    out, single = run_epochs(world, banks, 1, first=0, count=3), run_single(world, banks)
    assert same_bits(out["pos"], single["pos"][:3]) and same_bits(out["vel"], single["vel"][:3])
    assert np.array_equal(out["keys"], single["keys"][:3])
    for g in range(3):
        a, b = out["res"][g], single["res"][g]
        for k in ("posIndex", "velIndex", "posOutOfWindow", "velOutOfWindow"):
            assert a[k] == b[k], (g, k)
        assert np.float32(a["posScore"]).tobytes() == np.float32(b["posScore"]).tobytes()
        assert np.float32(a["velScore"]).tobytes() == np.float32(b["velScore"]).tobytes()
        assert a["zVal"].tobytes() == b["zVal"].tobytes()
        assert a["nPasses"] == 1


def test_pass_independence(twelve):
    """3.  N = 4, K = 4 in 1, 4 and 2 passes: the same bits."""
    world, banks = twelve
    outs = {}
    for ppp, passes in ((0, 1), (4, 4), (8, 2)):
        outs[ppp] = run_epochs(world, banks, 4, first=0, count=4, pairs_per_pass=ppp)
        assert outs[ppp]["res"][0]["nPasses"] == passes, ppp
    for ppp in (4, 8):
        assert same_bits(outs[ppp]["pos"], outs[0]["pos"]) and same_bits(outs[ppp]["vel"], outs[0]["vel"]), ppp
        assert np.array_equal(outs[ppp]["keys"], outs[0]["keys"]), ppp
    assert outs[0]["res"][0]["posIndex"] == world["pos_at"] and outs[0]["res"][0]["velIndex"] == world["vel_at"]


def test_automatic_pass_choice_at_default_bank_widths():
    """3b.  bin_half_width 48 (the default): a pair costs (2 * 48 + 1) * 16 + 32 = 1584 B of the 150 KB budget, which holds
    floor(153600 / 1584) = 96 pairs = 12 windows of 8 SVs; 13 windows (104 pairs) are just above one LDS fill, so the automatic
    choice takes 2 passes (12 + 1 windows).  Same bits as one window per pass."""
    world = ew.build(N=13, K=8, seed=2, bin_half_width=48)
    n_ent = 2 * max(world["L"], world["B"]) + 1
    budget = (150 * 1024) // (n_ent * 16 + 32)
    assert world["B"] == 48 and budget == 96 and budget // 8 == 12 and 13 * 8 > budget
    banks = Banks(world)
    try:
        auto = run_epochs(world, banks, 13)
        one = run_epochs(world, banks, 13, pairs_per_pass=8)
    finally:
        banks.close()
    assert auto["res"][0]["nPasses"] == -(-13 // (budget // 8)) == 2 and one["res"][0]["nPasses"] == 13
    assert same_bits(auto["pos"], one["pos"]) and same_bits(auto["vel"], one["vel"]) and np.array_equal(auto["keys"], one["keys"])
    assert auto["res"][0]["posIndex"] == world["pos_at"] and auto["res"][0]["velIndex"] == world["vel_at"]


@pytest.mark.parametrize("cut", [None, (1500, 1025)])
def test_group_independence_and_ragged_tiles(twelve, cut):
    """4.  12 windows as 3 groups of 4 in one launch against three launches of one group, in 2 passes each (the load-add-store of
    a partial tile): on the 2401-point grids (two full tiles and a ragged one) and on 1500- / 1025-point cuts of them."""
    world, banks = twelve
    together = run_epochs(world, banks, 4, pairs_per_pass=8, cut=cut)
    assert together["pos"].shape[0] == 3 and together["res"][0]["nPasses"] == 2
    for g in range(3):
        alone = run_epochs(world, banks, 4, first=4 * g, count=4, pairs_per_pass=8, cut=cut)
        assert same_bits(alone["pos"][0], together["pos"][g]) and same_bits(alone["vel"][0], together["vel"][g]), g
        assert np.array_equal(alone["keys"][0], together["keys"][g]), g
        assert alone["res"][0]["zVal"].tobytes() == together["res"][g]["zVal"].tobytes()
    single = run_single(world, banks, cut=cut)
    for g in range(3):      # no point left out, no padded point written: each group row is the ordered fp32 sum of its windows' rows
        for name in ("pos", "vel"):
            seq = single[name][4 * g].copy()
            for e in range(1, 4):
                seq = seq + single[name][4 * g + e]
            assert same_bits(together[name][g], seq), (g, name)


def test_key_is_the_first_maximum_of_the_row_and_the_oracles_argmax(twelve, oracle):
    """5.  Every group's key against np.argmax of the row read back, and against the oracle's arg-max of the fp64 sums."""
    world, banks = twelve
    out = run_epochs(world, banks, 4)
    full = ew.oracle_rows(world)
    for g in range(3):
        for m, name, rname in ((0, "pos", "pos_x"), (1, "vel", "vel")):
            row = out[name][g]
            at = int(np.argmax(row))
            assert key_index(out["keys"][g, m]) == at == out["res"][g]["posIndex" if m == 0 else "velIndex"], (g, name)
            assert np.uint32(int(out["keys"][g, m]) >> 32) == row[at].view(np.uint32)
            want = np.sum([full["win"][4 * g + e][rname] for e in range(4)], axis=0)
            assert at == oracle.argmax_first(want) == (world["pos_at"] if m == 0 else world["vel_at"]), (g, name)


def test_weak_signal_sixteen_epochs_find_the_point_single_windows_do_not(oracle):
    """6.  The capability: at WEAK_AMP the 16-window sum peaks on the true point in both manifolds; most single windows do not."""
    world = ew.weak()
    banks = Banks(world)
    try:
        out, single = run_epochs(world, banks, ew.WEAK_N), run_single(world, banks)
    finally:
        banks.close()
    j = out["res"][0]
    hits = [r["posIndex"] == world["pos_at"] and r["velIndex"] == world["vel_at"] for r in single["res"]]
    hp = sum(r["posIndex"] == world["pos_at"] for r in single["res"])
    hv = sum(r["velIndex"] == world["vel_at"] for r in single["res"])
    print("weak world: epochs arg-max (%d, %d), expected (%d, %d); single windows on the point: position %d, velocity %d, both %d of %d"
          % (j["posIndex"], j["velIndex"], world["pos_at"], world["vel_at"], hp, hv, sum(hits), len(hits)))
    assert j["posIndex"] == world["pos_at"] and j["velIndex"] == world["vel_at"]
    assert len(hits) == ew.WEAK_N and 2 * hp < len(hits) and 2 * hv < len(hits) and 2 * sum(hits) < len(hits)
    assert np.abs(j["zVal"] - world["truth"][-1]).max() < 1e-6


def test_out_of_window_counts_are_the_sum_of_the_windows_counts():
    """7.  Windows 1 and 3 have their centres moved 400 m in the clock term (3.3 samples of the +-5 .. 6 the banks hold): pairs
    leave the banks there.  The group's counts are the sums of dpe_bcm_update's per-window counts, every score stays finite."""
    world = ew.build(N=5, K=8, seed=3, shift=400.0)
    banks = Banks(world)
    try:
        out, single = run_epochs(world, banks, 5, pairs_per_pass=16), run_single(world, banks)
    finally:
        banks.close()
    per = [(r["posOutOfWindow"], r["velOutOfWindow"]) for r in single["res"]]
    print("out-of-window pairs per window (position, velocity):", per, "group:", out["res"][0]["posOutOfWindow"], out["res"][0]["velOutOfWindow"])
    assert per[1][0] > 0 and per[3][0] > 0
    assert out["res"][0]["posOutOfWindow"] == sum(p for p, _ in per) and out["res"][0]["velOutOfWindow"] == sum(v for _, v in per)
    assert np.isfinite(out["pos"]).all() and np.isfinite(out["vel"]).all() and out["res"][0]["nPasses"] == 3
    for name in ("pos", "vel"):
        seq = single[name][0].copy()
        for e in range(1, 5):
            seq = seq + single[name][e]
        assert same_bits(out[name][0], seq), name


def test_refusals_carry_a_message_and_launch_nothing(five):
    """8."""
    world, banks = five
    e, lib = dpe.engine, dpe.engine.lib()
    h = dpe.EpochManifold(world["fs"], world["S"], world["C"], world["pos"], world["vel"], 4, 0, lag_half_width=world["L"],
                          bin_half_width=world["B"], max_windows=5, max_channels=world["K"])
    h.Start()
    plain = dpe.BatchCorrManifold(world["fs"], world["S"], world["C"], world["pos"], world["vel"], lag_half_width=world["L"],
                                  bin_half_width=world["B"], max_windows=5, max_channels=world["K"])
    plain.Start()
    code, carr = banks.rows()
    bwp, cep = banks.bw.ctypes.data_as(C.POINTER(e.BcmWindow)), banks.ce.ctypes.data_as(C.POINTER(e.ChanEnd))
    try:
        h.Update(code, carr, banks.bw[:4], banks.ce[:4], 4)
        before = h.read_keys().copy()
        assert before.all()
        with pytest.raises(dpe.DpeError, match="nEpochs 5 out of range"):          # nEpochs > maxEpochs
            h.Update(code, carr, banks.bw, banks.ce, 5)
        with pytest.raises(dpe.DpeError, match="2 groups of 3 windows out of range"):   # nGroups * nEpochs > maxWindows
            h.Update(code, carr, np.concatenate([banks.bw, banks.bw[:1]]), np.concatenate([banks.ce, banks.ce[:1]]), 3)
        with pytest.raises(dpe.DpeError, match="not whole groups"):
            h.Update(code, carr, banks.bw, banks.ce, 2)
        with pytest.raises(dpe.DpeError, match="use dpe_bcm_update_epochs"):
            e._check(lib.dpe_bcm_update(h._h, e._ptr(code), e._ptr(carr), C.c_int32(1), C.c_int32(8), bwp, cep, e._stream(None)))
        ports = e.BcmPortsDev(dimT=1, reserved=0)      # (null ports: the refusal comes first and nothing is launched)
        with pytest.raises(dpe.DpeError, match="use dpe_bcm_update_epochs"):
            e._check(lib.dpe_bcm_update_dev(h._h, e._ptr(code), e._ptr(carr), C.c_int32(8), C.byref(ports), C.c_double(0.0), e._stream(None)))
        with pytest.raises(dpe.DpeError, match="use dpe_bcm_update_epochs"):
            e._check(lib.dpe_bcm_update_prepared(h._h, e._ptr(code), e._ptr(carr), C.c_int32(8), e._stream(None)))
        with pytest.raises(dpe.DpeError, match="use dpe_bcm_results_epochs"):
            dpe.BatchCorrManifold.results(h)
        with pytest.raises(dpe.DpeError, match="use dpe_bcm_results_epochs"):
            dpe.BatchCorrManifold.results_from_keys(h, before, world["pos"], world["vel"])
        with pytest.raises(dpe.DpeError, match="always launch eagerly"):
            h.set_graph(True)
        comm = e.Comm(0, 1)
        try:
            with pytest.raises(dpe.DpeError, match="sharding is not supported"):
                dpe.BatchCorrManifold.exchange_keys(h, comm)
        finally:
            comm.close()
        cm = e.ChanMgrDev.from_handoff(world["ho"], world["S"] / world["fs"], world["K"])
        try:
            with pytest.raises(dpe.DpeError, match="epochs handle"):
                cm.attach(None, h)
        finally:
            cm.Stop()
        # the joint calls on an epochs handle
        with pytest.raises(dpe.DpeError, match="not made by dpe_bcm_create_joint"):
            e._check(lib.dpe_bcm_update_joint(h._h, C.c_int32(1), C.c_int32(1), (e.BcmJointRx * 1)(), e._stream(None)))
        with pytest.raises(dpe.DpeError, match="no joint update yet"):
            e._check(lib.dpe_bcm_results_joint(h._h, (e.BcmJointResult * 1)(), (e.BcmJointRxResult * 1)(), e._stream(None)))
        with pytest.raises(dpe.DpeError, match="not a handle of dpe_bcm_create_joint"):
            e._check(lib.dpe_bcm_joint_set_own_keys(h._h, C.c_int32(1)))
        # nothing was launched by the refused calls: the key set of the last good Update is still the current one, unchanged
        keys = C.c_void_p()
        e._check(lib.dpe_bcm_keys(h._h, C.byref(keys)))
        assert keys.value == h.Keys and np.array_equal(h.read_keys(), before)
        # the new calls on every other kind of handle
        with pytest.raises(dpe.DpeError, match="not made by dpe_bcm_create_epochs"):
            e._check(lib.dpe_bcm_update_epochs(plain._h, e._ptr(code), e._ptr(carr), C.c_int32(1), C.c_int32(1), C.c_int32(8), bwp, cep,
                                               e._stream(None)))
        with pytest.raises(dpe.DpeError, match="not made by dpe_bcm_create_epochs"):
            e._check(lib.dpe_bcm_results_epochs(plain._h, (e.BcmEpochsResult * 1)(), e._stream(None)))
    finally:
        h.Stop()
        plain.Stop()
    kw = dict(lag_half_width=world["L"], bin_half_width=world["B"], max_windows=5, max_channels=world["K"])
    with pytest.raises(dpe.DpeError, match="pairsPerPass 7 is below maxChannels 8"):
        dpe.EpochManifold(world["fs"], world["S"], world["C"], world["pos"], world["vel"], 4, 7, **kw).Start()
    with pytest.raises(dpe.DpeError, match="maxEpochs 6 out of range"):
        dpe.EpochManifold(world["fs"], world["S"], world["C"], world["pos"], world["vel"], 6, 0, **kw).Start()
    with pytest.raises(dpe.DpeError, match="no 12-byte bank entries"):       # 37 channels x 345 entries: one window does not fit
        dpe.EpochManifold(world["fs"], world["S"], world["C"], world["pos"], world["vel"], 4, 0, lag_half_width=8, bin_half_width=172,
                          max_windows=5, max_channels=37).Start()


def test_closed_loop_of_one_epoch_is_run_closed_loop_bit_for_bit(golden):
    """9a.  Six windows of the O13 closed-loop input."""
    from tests.test_gpu_loop_o13 import _setup
    g = golden("o13_dp_track")
    ho, delta, pos, vel, iq = _setup(g)
    iq = iq[:6]
    assert iq.shape[0] == 6
    tg = np.unique(pos[:, 3])
    want, _ = dpe.pipeline.run_closed_loop(iq, ho, float(g["fs"]), pos, vel, time_grid=tg, init_delta=delta)
    got, res = dpe.pipeline.run_epoch_closed_loop(iq, ho, float(g["fs"]), pos, vel, 1, time_grid=tg, init_delta=delta)
    assert got.shape == want.shape == (6, 8) and got.tobytes() == want.tobytes()
    assert all(r["nPasses"] == 1 for r in res)


def test_closed_loop_of_four_epochs_returns_to_the_trajectory():
    """9b.  The epoch world over eight windows as two groups of four, started one grid step off in the clock term.  The position
    grid is spaced by one sample (joint_world.oracle_loop says why a closed loop on linearly interpolated banks needs that: on
    the 40 m grid every SV prefers the lag it is closest to and no loop moves).  Bound: one grid step (one sample, 119.9 m),
    for the last fix against the truth at the last window.  Measured on an MI355X: 2.9e-11 m after the first group, 0.028 m after the
    second (one window of motion: the next group starts from the last window's fix, unpredicted, as run_closed_loop does)."""
    from tests import joint_world as jw
    world = ew.build(N=8, K=8, seed=4)
    pos, vel = jw.grids(jw.SAMPLE)
    _cs, _ce, _bw, iq = ew.gpu_inputs(world)
    R3 = world["R"].reshape(3, 3)
    step = np.concatenate([R3 @ np.zeros(3), [-jw.SAMPLE]])
    fixes, res = dpe.pipeline.run_epoch_closed_loop(iq, world["ho"], world["fs"], pos, vel, 4, init_delta=step)
    err = np.abs(fixes[:, :4] - world["truth"][[3, 7], :4]).max(axis=1)
    print("epoch closed loop, 2 groups of 4, started %.1f m off in the clock term: position / clock error after group 0 %.3g m, "
          "after group 1 %.3g m; arg-max %s" % (jw.SAMPLE, err[0], err[1], [(r["posIndex"], r["velIndex"]) for r in res]))
    assert fixes.shape == (2, 8) and err[1] < jw.SAMPLE
