"""CPU: the inputs of the multi-epoch scan tests (tests/epoch_world.py) are what they claim to be, by the existing oracle
alone.  The group row is formed as the fp64 sum of the oracle's per-window rows.

Strong world: every window alone and the sum peak on the common offset, which is not the grids' centre point; no pair leaves
the widened banks; each centre is the moving truth at its epoch moved back by the offset.
Weak world (WEAK_AMP, WEAK_SEED; found by scanning amplitudes 30 .. 3 with this oracle): fewer than half of the 16 single
windows put their arg-max on the true point, the 16-window sum does, and its margin (best - second best of the fp64 sum) is
at least 10 x the oracle tolerance of the GPU test (2e-6 of the row maximum)."""
import numpy as np
import pytest

from tests import epoch_world as ew, joint_world as jw


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()


@pytest.mark.parametrize("N,K,seed", [(5, 8, 0), (12, 4, 1)])
def test_every_window_alone_and_the_sum_peak_on_the_common_offset(built, oracle, N, K, seed):
    world = ew.build(N=N, K=K, seed=seed)
    ref = ew.oracle_rows(world)
    centre = jw.grid_index((3, 3, 3, 3))
    assert world["pos_at"] != centre and world["vel_at"] != centre
    assert world["pos"].shape[0] == 2401 and world["vel"].shape[0] == 2401      # two full 1024-point tiles and a ragged one
    assert len(ref["win"]) == N
    for e, x in enumerate(ref["win"]):
        assert x["oob_pos"] == 0 and x["oob_pos_x"] == 0 and x["oob_vel"] == 0, e
        assert oracle.argmax_first(x["pos"]) == world["pos_at"], e
        assert oracle.argmax_first(x["pos_x"]) == world["pos_at"], e
        assert oracle.argmax_first(x["vel"]) == world["vel_at"], e
    for name, at in (("pos", world["pos_at"]), ("pos_x", world["pos_at"]), ("vel", world["vel_at"])):
        assert oracle.argmax_first(ref[name]) == at
        assert np.array_equal(ref[name], np.sum([x[name] for x in ref["win"]], axis=0))
    # the truth moves with constant velocity; every centre is the truth of its epoch moved back by the one offset
    R3 = world["R"].reshape(3, 3)
    T = world["S"] / world["fs"]
    d = np.diff(world["truth"], axis=0)
    assert np.abs(d[:, :3] - world["truth"][0, 4:7] * T).max() < 1e-8 and np.linalg.norm(world["truth"][0, 4:7]) > 10.0
    assert np.abs(d[:, 4:]).max() == 0.0
    for e, win in enumerate(world["wins"]):
        moved = win["centre"].copy()
        moved[:3] += R3 @ world["offset"][:3]
        moved[3] += world["offset"][3]
        moved[4:7] += R3 @ world["offset"][4:7]
        moved[7] += world["offset"][7]
        assert np.abs(moved - world["truth"][e]).max() < 1e-8
        if e:
            assert not np.array_equal(win["iq"][:64], world["wins"][0]["iq"][:64]) and win["rxTime"] > world["wins"][e - 1]["rxTime"]


def test_weak_signal_world(built, oracle):
    world = ew.weak()
    ref = ew.oracle_rows(world)
    assert world["N"] == ew.WEAK_N == 16 and len(ref["win"]) == 16
    hp = [oracle.argmax_first(x["pos_x"]) == world["pos_at"] for x in ref["win"]]
    hf = [oracle.argmax_first(x["pos"]) == world["pos_at"] for x in ref["win"]]
    hv = [oracle.argmax_first(x["vel"]) == world["vel_at"] for x in ref["win"]]
    print("weak world: single windows on the point: position %d (faithful %d), velocity %d of 16" % (sum(hp), sum(hf), sum(hv)))
    assert 2 * sum(hp) < 16 and 2 * sum(hf) < 16 and 2 * sum(hv) < 16          # no window is excluded
    for name, at in (("pos_x", world["pos_at"]), ("pos", world["pos_at"]), ("vel", world["vel_at"])):
        row = ref[name]
        assert oracle.argmax_first(row) == at, name
        top = np.sort(row)[-2:]
        margin = (top[1] - top[0]) / row.max()
        print("weak world: %s margin %.3g of the row maximum (needed %.3g)" % (name, margin, 10 * ew.ORACLE_TOL))
        assert margin >= 10 * ew.ORACLE_TOL, name
    assert all(x["oob_pos"] == 0 and x["oob_pos_x"] == 0 and x["oob_vel"] == 0 for x in ref["win"])


def test_shifted_windows_leave_the_banks(built, oracle):
    """The out-of-window world: pairs leave the banks in windows 1 and 3 (at least), and every row stays finite."""
    world = ew.build(N=5, K=8, seed=3, shift=400.0)
    ref = ew.oracle_rows(world)
    assert ref["win"][1]["oob_pos_x"] > 0 and ref["win"][3]["oob_pos_x"] > 0
    assert ref["win"][1]["oob_pos_x"] < 8 * 2401 and np.isfinite(ref["pos_x"]).all() and np.isfinite(ref["vel"]).all()


# the worlds of tests/test_gpu_epochs_walk.py: (arguments of epoch_world.build, windows per group, tiles of the two grids)
WALK_WORLDS = {
    "E1": (dict(N=8, K=4, seed=5, pos_dim=15, vel_dim=14), 4, (50, 38)),
    "E1-swapped": (dict(N=8, K=4, seed=5, pos_dim=14, vel_dim=15), 4, (38, 50)),
    "E2": (dict(N=4, K=5, seed=6), 4, (3, 3)),
    "E3": (dict(N=4, K=4, seed=7, pos_dim=20, vel_dim=7), 4, (157, 3)),
}


@pytest.mark.parametrize("name", sorted(WALK_WORLDS))
def test_walk_worlds_peak_on_the_scaled_offset(built, oracle, name):
    """Every window alone, every group's sum and the sum of all windows peak on the expected point of the larger grids, which
    is neither the centre nor in the first tile; no pair leaves the widened banks."""
    kw, n, want_tiles = WALK_WORLDS[name]
    world = ew.build(**kw)
    ref = ew.oracle_rows(world)
    pd, vd = world["dims"]
    assert (-(-world["pos"].shape[0] // 1024), -(-world["vel"].shape[0] // 1024)) == want_tiles
    assert world["pos_at"] == jw.grid_index(jw.scaled_at(ew.POS_AT, pd), pd) and world["vel_at"] == jw.grid_index(jw.scaled_at(ew.VEL_AT, vd), vd)
    assert world["pos_at"] != jw.grid_index(((pd - 1) // 2,) * 4, pd) and world["vel_at"] != jw.grid_index(((vd - 1) // 2,) * 4, vd)
    assert (pd == 7 or world["pos_at"] >= 1024) and (vd == 7 or world["vel_at"] >= 1024)
    for e, x in enumerate(ref["win"]):
        assert x["oob_pos"] == 0 and x["oob_pos_x"] == 0 and x["oob_vel"] == 0, e
        assert oracle.argmax_first(x["pos"]) == world["pos_at"] and oracle.argmax_first(x["pos_x"]) == world["pos_at"], e
        assert oracle.argmax_first(x["vel"]) == world["vel_at"], e
    for g in range(world["N"] // n):
        for rname, at in (("pos", world["pos_at"]), ("pos_x", world["pos_at"]), ("vel", world["vel_at"])):
            assert oracle.argmax_first(np.sum([ref["win"][g * n + e][rname] for e in range(n)], axis=0)) == at, (g, rname)
    R3 = world["R"].reshape(3, 3)
    for e, win in enumerate(world["wins"]):
        moved = win["centre"].copy()
        moved[:3] += R3 @ world["offset"][:3]
        moved[3] += world["offset"][3]
        moved[4:7] += R3 @ world["offset"][4:7]
        moved[7] += world["offset"][7]
        assert np.abs(moved - world["truth"][e]).max() < 1e-8


@pytest.mark.parametrize("side", ["L", "B"])
def test_walk_world_with_one_side_narrow(built, oracle, side):
    """E3's world: with only the lag (bin) banks narrow, pairs leave the position (velocity) banks in every window and none
    the other side's, whose rows are the widened world's and still peak on the expected point."""
    kw = WALK_WORLDS["E3"][0]
    world, base = ew.build(**dict(kw, widen=side)), ew.build(**kw)
    assert (world["L"], world["B"]) == ((1, base["B"]) if side == "L" else (base["L"], 2))
    ref, clean = ew.oracle_rows(world), ew.oracle_rows(base)
    for e, x in enumerate(ref["win"]):
        assert (x["oob_pos_x"] > 0) == (side == "L") and (x["oob_vel"] > 0) == (side == "B"), e
    same = "vel" if side == "L" else "pos_x"
    assert np.array_equal(ref[same], clean[same]) and np.isfinite(ref["pos_x"]).all() and np.isfinite(ref["vel"]).all()
    assert oracle.argmax_first(ref[same]) == (world["vel_at"] if side == "L" else world["pos_at"])
