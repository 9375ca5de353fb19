"""GPU: bcm_scan_epochs_kernel (csrc/dpe_bcm_epochs.h) where a block walks several tiles -- the shape it is measured at
(profiles/epochs.txt) -- and on the inputs tests/test_gpu_epochs.py holds constant.

tests/test_gpu_epochs.py runs on 7^4 grids (three 1024-point tiles, one per block).  Here 24 blocks walk the 50 and 38 tiles
of 15^4 and 14^4 grids (32 groups), or 128 blocks the 157 tiles of a 20^4 grid (one group), in 1, 2 and 4 passes: every pass
re-issues the block's first tile load, walks the same tiles through the double buffer, and reads the running score of the
earlier passes back from the group's row for every one of its tiles, the ragged one included.  Every test asserts the split
through last_split().  Further: handles with more channels than they are fed (the maxK * nEnt global stride against the
K * nEnt LDS stride), the generic LPower variant, the mixed clamp variants and unequal splits.

Inputs: tests/epoch_world.py on larger grids, proven by the oracle alone in tests/test_epoch_world_cpu.py.  A batch is two
distinct groups dealt round-robin into 32 before stage 1; the oracle is evaluated on the distinct windows only.

Bounds are those stated at the top of tests/test_gpu_epochs.py, unchanged: bit equality with the ordered fp32 sum of
dpe_bcm_update's window rows; against the oracle's fp64 sum TOL = 2e-6 (extended-precision position rows, velocity rows) or
helpers.POS_REF_NOISE (faithful position rows) of the row maximum plus the accumulation bound (N - 1) 2^-24 of the point's sum;
1e-5 in place of TOL for LPower = 3 (tests/test_gpu_parity.py::test_lpower)."""
import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import epoch_world as ew, helpers
from tests.test_gpu_epochs import TOL, key_index, same_bits

pytestmark = pytest.mark.gpu
G32 = 32
TILE = 1024


def tiles(G):
    return -(-G // TILE)


class Banks:
    """Stage 1 over the world's windows, dealt round-robin into `windows` windows BEFORE stage 1 (window w is the world's
    window w % N); max_channels may exceed the world's K (bank rows then keep the handle's channel stride)."""

    def __init__(self, world, windows=None, max_channels=None):
        import torch
        self.world = world
        self.W = world["N"] if windows is None else windows
        self.maxK = world["K"] if max_channels is None else max_channels
        idx = np.arange(self.W) % world["N"]
        cs, ce, bw, iq = ew.gpu_inputs(world)
        self.cs, self.ce, self.bw = (np.ascontiguousarray(a[idx]) for a in (cs, ce, bw))
        self.bcs = dpe.BatchCorrScores(world["fs"], samples_per_window=world["S"], lag_half_width=world["L"], bin_half_width=world["B"],
                                       max_windows=self.W, max_channels=self.maxK)
        self.bcs.Start()
        self.bcs.Update(torch.from_numpy(np.ascontiguousarray(iq[idx])).to("cuda:0"), self.cs)

    def close(self):
        self.bcs.Stop()


def grids_of(world, cut):
    return (world["pos"], world["vel"]) if cut is None else (world["pos"][:cut[0]], world["vel"][:cut[1]])


def run_epochs(world, banks, n_epochs, pairs_per_pass=0, cut=None, lpower=1, split=None, passes=None):
    """All windows of `banks` as groups of n_epochs in ONE launch; split and passes are asserted."""
    pos, vel = grids_of(world, cut)
    h = dpe.EpochManifold(world["fs"], world["S"], world["C"], pos, vel, n_epochs, pairs_per_pass, LPower=lpower,
                          lag_half_width=world["L"], bin_half_width=world["B"], max_windows=banks.W, max_channels=banks.maxK)
    h.Start()
    try:
        h.Update(banks.bcs.CodeScores, banks.bcs.CarrScores, banks.bw, banks.ce, n_epochs)
        got = h.last_split()
        assert split is None or got == split, "scan_split gave %s, the test needs %s" % (got, split)
        res = h.results()
        assert passes is None or all(r["nPasses"] == passes for r in res)
        ps, vs = h.read_scores()
        keys = h.read_keys()
    finally:
        h.Stop()
    return dict(res=res, pos=ps, vel=vs, keys=keys)


def run_single(world, banks, cut=None, lpower=1):
    """Every window alone through dpe_bcm_update (one batch) on the same banks and inputs."""
    pos, vel = grids_of(world, cut)
    h = dpe.BatchCorrManifold(world["fs"], world["S"], world["C"], pos, vel, LPower=lpower, lag_half_width=world["L"],
                              bin_half_width=world["B"], max_windows=banks.W, max_channels=banks.maxK)
    h.Start()
    try:
        h.Update(banks.bcs.CodeScores, banks.bcs.CarrScores, banks.bw, banks.ce)
        res = h.results()
        ps, vs = h.read_scores()
    finally:
        h.Stop()
    return dict(res=res, pos=ps, vel=vs)


def ordered_sum(rows, g, N):
    """Rows g N .. g N + N - 1 added in fp32, in window order, starting from the first."""
    seq = rows[g * N].copy()
    for e in range(1, N):
        seq = seq + rows[g * N + e]
    return seq


def assert_rows_are_ordered_sums(out, single, N, where=""):
    for g in range(out["pos"].shape[0]):
        for name in ("pos", "vel"):
            assert same_bits(out[name][g], ordered_sum(single[name], g, N)), (where, g, name)


def assert_key_is_first_maximum(out, g):
    for m, name, key in ((0, "pos", "posIndex"), (1, "vel", "velIndex")):
        row = out[name][g]
        at = int(np.argmax(row))
        assert key_index(out["keys"][g, m]) == at == out["res"][g][key], (g, name)
        assert np.uint32(int(out["keys"][g, m]) >> 32) == row[at].view(np.uint32), (g, name)


def assert_against_oracle(world, out, g, d, N, tol=TOL, lpower=1, what=""):
    """Group g of `out` (the world's windows d N .. d N + N - 1) against the fp64 sum of the oracle's rows; every point."""
    full = ew.oracle_rows(world, lpower=lpower)
    acc = (N - 1) * 2.0 ** -24
    for name, rname, lim in (("pos", "pos_x", tol), ("pos", "pos", helpers.POS_REF_NOISE), ("vel", "vel", tol)):
        r_ = np.sum([full["win"][d * N + e][rname] for e in range(N)], axis=0)
        err = np.abs(out[name][g].astype(np.float64) - r_)
        print("%sgroup %d, %s row vs the oracle's summed %s rows: %.3g of the row maximum (bound %.3g + accumulation)"
              % (what, g, name, rname, err.max() / r_.max(), lim))
        assert np.all(err <= lim * r_.max() + acc * r_), (g, name, rname)
        if rname != "pos":
            assert int(np.argmax(r_)) == (world["pos_at"] if name == "pos" else world["vel_at"])


WALK = {"15x14": dict(pos_dim=15, vel_dim=14), "14x15": dict(pos_dim=14, vel_dim=15)}
E1_N, E1_K = 4, 4


@pytest.fixture(scope="module", params=sorted(WALK))
def walk(request):
    """K = 4, two distinct groups of N = 4 windows dealt into 32 groups (128 windows); grids 15^4 (50 tiles, blocks 0 and 1
    walk three, block 1 reaches the ragged one by the even path) and 14^4 (38 tiles, block 13 reaches the ragged one as its
    second tile through the bufB -> bufA copy), and swapped.  The per-window rows of dpe_bcm_update are computed once."""
    world = ew.build(N=2 * E1_N, K=E1_K, seed=5, **WALK[request.param])
    assert sorted((tiles(world["pos"].shape[0]), tiles(world["vel"].shape[0]))) == [38, 50]
    banks = Banks(world, G32 * E1_N)
    single = run_single(world, banks)
    yield world, banks, single
    banks.close()


def test_batch_walk_with_passes(walk, oracle):
    """E1."""
    world, banks, single = walk
    outs = {}
    for ppp, passes in ((0, 1), (8, 2), (4, 4)):
        outs[ppp] = run_epochs(world, banks, E1_N, pairs_per_pass=ppp, split=(24, 24), passes=passes)
    one = outs[0]
    assert one["pos"].shape == (G32, world["pos"].shape[0]) and one["vel"].shape == (G32, world["vel"].shape[0])
    assert_rows_are_ordered_sums(one, single, E1_N)
    for ppp in (8, 4):
        assert same_bits(outs[ppp]["pos"], one["pos"]) and same_bits(outs[ppp]["vel"], one["vel"]), ppp
        assert np.array_equal(outs[ppp]["keys"], one["keys"]), ppp
    for g in range(G32):
        assert_key_is_first_maximum(one, g)
        assert one["res"][g]["posIndex"] == world["pos_at"] and one["res"][g]["velIndex"] == world["vel_at"], g
        assert one["res"][g]["posOutOfWindow"] == 0 and one["res"][g]["velOutOfWindow"] == 0
        assert np.abs(one["res"][g]["zVal"] - world["truth"][(g % 2) * E1_N + E1_N - 1]).max() < 1e-6
    for d in range(2):
        assert_against_oracle(world, outs[4], G32 - 2 + d, d, E1_N, what="4 passes, ")


def test_lpower_3_on_the_walk(walk, oracle):
    """E3 (third part).  The generic powf variant on E1's shape, two passes, against the oracle at 1e-5 plus accumulation, and
    against the ordered sums of dpe_bcm_update's rows at the same power."""
    world, banks, _ = walk
    out = run_epochs(world, banks, E1_N, pairs_per_pass=8, lpower=3, split=(24, 24), passes=2)
    assert_rows_are_ordered_sums(out, run_single(world, banks, lpower=3), E1_N)
    for g in range(G32):
        assert_key_is_first_maximum(out, g)
        assert out["res"][g]["posIndex"] == world["pos_at"] and out["res"][g]["velIndex"] == world["vel_at"], g
    for d in range(2):
        assert_against_oracle(world, out, G32 - 2 + d, d, E1_N, tol=1e-5, lpower=3, what="LPower 3, ")


@pytest.fixture(scope="module", params=[True, False], ids=["clean", "narrow"])
def walk_banks(request):
    """E1's 15^4 / 14^4 shape (two distinct groups of 4 windows dealt into 32 groups) with widened banks and with deliberately
    narrow ones (both manifolds clamp and recount)."""
    world = ew.build(N=2 * E1_N, K=E1_K, seed=5, widen=request.param, **WALK["15x14"])
    assert (tiles(world["pos"].shape[0]), tiles(world["vel"].shape[0])) == (50, 38)
    banks = Banks(world, G32 * E1_N)
    yield world, banks, request.param
    banks.close()


@pytest.mark.parametrize("lpower", [1, 2, 3])
def test_walk_every_lpower_clean_and_clamped(walk_banks, lpower):
    """E3 (fourth part).  Every (LPower, clamp) variant on the walk, in two passes: 24 blocks walk 50 and 38 tiles (the ragged
    tile by the even path and through the bufB -> bufA copy), the second pass reads the running score back.  Rows are the
    ordered sums of dpe_bcm_update's rows at the same power, the key the first maximum of the group's row, the counts the sums
    of dpe_bcm_update's per-window counts: non-zero on both manifolds with narrow banks, zero with clean ones."""
    world, banks, widen = walk_banks
    out = run_epochs(world, banks, E1_N, pairs_per_pass=8, lpower=lpower, split=(24, 24), passes=2)
    single = run_single(world, banks, lpower=lpower)
    assert np.isfinite(out["pos"]).all() and np.isfinite(out["vel"]).all()
    assert_rows_are_ordered_sums(out, single, E1_N)
    for g in range(G32):
        assert_key_is_first_maximum(out, g)
        per = single["res"][g * E1_N:(g + 1) * E1_N]
        for k in ("posOutOfWindow", "velOutOfWindow"):
            assert out["res"][g][k] == sum(r[k] for r in per), (g, k)
            assert all((r[k] > 0) == (not widen) for r in per), (g, k)
        if widen:
            assert out["res"][g]["posIndex"] == world["pos_at"] and out["res"][g]["velIndex"] == world["vel_at"], g


@pytest.mark.parametrize("cut", [None, (1500, 1025)])
def test_fewer_channels_than_the_handles_hold(oracle, cut):
    """E2.  BatchCorrScores, EpochManifold and BatchCorrManifold all created for 8 channels and fed K = 5: the banks lie
    maxK * nEnt apart in global memory and K * nEnt apart in the LDS.  N = 4 in 2 passes (10 pairs per pass), on the 7^4
    grids and on the 1500- / 1025-point cuts (a ragged second tile): the bits of the ordered sums of dpe_bcm_update's rows on
    the same banks; on the whole grids also the oracle."""
    world = ew.build(N=4, K=5, seed=6)
    banks = Banks(world, max_channels=8)
    try:
        split = (3, 3) if cut is None else (2, 2)
        out = run_epochs(world, banks, 4, pairs_per_pass=10, cut=cut, split=split, passes=2)
        whole = run_epochs(world, banks, 4, pairs_per_pass=0, cut=cut, split=split, passes=1)
        single = run_single(world, banks, cut=cut)
    finally:
        banks.close()
    assert_rows_are_ordered_sums(out, single, 4)
    assert same_bits(out["pos"], whole["pos"]) and same_bits(out["vel"], whole["vel"]) and np.array_equal(out["keys"], whole["keys"])
    assert_key_is_first_maximum(out, 0)
    assert out["res"][0]["posOutOfWindow"] == 0 and out["res"][0]["velOutOfWindow"] == 0
    if cut is None:
        assert_against_oracle(world, out, 0, 0, 4, what="K 5 of 8, ")
        assert out["res"][0]["posIndex"] == world["pos_at"] and out["res"][0]["velIndex"] == world["vel_at"]


@pytest.mark.parametrize("side", ["L", "B"])
def test_mixed_clamp_and_unequal_splits(oracle, side):
    """E3.  One group of 4 windows in 2 passes on a 20^4 position grid (157 tiles for 128 blocks) and a 7^4 velocity grid (3
    tiles: grid.x is 128 and 125 velocity blocks only take the publish ticket), with only the lag banks narrow (the position
    manifold clamps, <CLAMP_P, !CLAMP_V>), then only the bin banks.  Counts are the sums of dpe_bcm_update's per-window counts
    (the oracle's are printed beside them; the clean side counts nothing), rows the ordered sums, and the clean manifold meets
    the oracle on every point."""
    world = ew.build(N=4, K=4, seed=7, widen=side, pos_dim=20, vel_dim=7)
    assert (tiles(world["pos"].shape[0]), tiles(world["vel"].shape[0])) == (157, 3)
    banks = Banks(world)
    try:
        out = run_epochs(world, banks, 4, pairs_per_pass=8, split=(128, 3), passes=2)
        single = run_single(world, banks)
    finally:
        banks.close()
    per = [(r["posOutOfWindow"], r["velOutOfWindow"]) for r in single["res"]]
    full = ew.oracle_rows(world)
    print("only %s narrow: out-of-window pairs per window (position, velocity) %s, oracle %s; group (%d, %d)"
          % (side, per, [(x["oob_pos_x"], x["oob_vel"]) for x in full["win"]], out["res"][0]["posOutOfWindow"], out["res"][0]["velOutOfWindow"]))
    assert out["res"][0]["posOutOfWindow"] == sum(p for p, _ in per) and out["res"][0]["velOutOfWindow"] == sum(v for _, v in per)
    assert all((p > 0) == (side == "L") and (v > 0) == (side == "B") for p, v in per)
    assert np.isfinite(out["pos"]).all() and np.isfinite(out["vel"]).all()
    assert_rows_are_ordered_sums(out, single, 4)
    assert_key_is_first_maximum(out, 0)
    # the clean manifold against the oracle, every point
    acc = 3 * 2.0 ** -24
    for name, rname, lim in ((("vel", "vel", TOL),) if side == "L" else (("pos", "pos_x", TOL), ("pos", "pos", helpers.POS_REF_NOISE))):
        r_ = full[rname]
        err = np.abs(out[name][0].astype(np.float64) - r_)
        print("clean %s manifold vs the oracle's summed %s rows: %.3g of the row maximum (bound %.3g + accumulation)"
              % (name, rname, err.max() / r_.max(), lim))
        assert np.all(err <= lim * r_.max() + acc * r_)
    assert out["res"][0]["velIndex" if side == "L" else "posIndex"] == world["vel_at" if side == "L" else "pos_at"]
