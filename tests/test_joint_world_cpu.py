"""CPU: the inputs of the joint-scan tests (tests/joint_world.py) are what they claim to be, by the existing oracle alone:
every receiver ALONE peaks on the expected grid point, no pair leaves the widened banks, and with the deliberately narrow
banks the oracle's own faithful and extended-precision rows stay inside the cap on points set aside that
helpers.assert_parity applies (16 + pairs / 2000 position points per receiver)."""
import numpy as np
import pytest

from tests import helpers, joint_world as jw


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()


@pytest.mark.parametrize("n_sv", [(5, 8, 4), (10, 10, 10, 10), (6,)])
def test_every_receiver_alone_peaks_on_the_common_offset(built, oracle, n_sv):
    world = jw.build(n_sv)
    ref = jw.oracle_rows(world)
    assert world["pos_at"] != jw.grid_index((3, 3, 3, 3)) and world["vel_at"] != jw.grid_index((3, 3, 3, 3))
    assert world["pos"].shape[0] == 2401 and world["vel"].shape[0] == 2401      # two full 1024-point tiles and a ragged one
    for r, x in enumerate(ref["rx"][0]):
        assert x["oob_pos"] == 0 and x["oob_pos_x"] == 0 and x["oob_vel"] == 0, r
        assert oracle.argmax_first(x["pos"]) == world["pos_at"], r
        assert oracle.argmax_first(x["pos_x"]) == world["pos_at"], r
        assert oracle.argmax_first(x["vel"]) == world["vel_at"], r
    assert oracle.argmax_first(ref["pos"][0]) == world["pos_at"] and oracle.argmax_first(ref["vel"][0]) == world["vel_at"]
    # the truth is each centre moved by the common offset, and the baselines are 0.5 .. 3 m
    R3 = world["R"].reshape(3, 3)
    for r, rx in enumerate(world["rx"]):
        moved = rx["centre"].copy()
        moved[:3] += R3 @ world["offset"][:3]
        moved[3] += world["offset"][3]
        moved[4:7] += R3 @ world["offset"][4:7]
        moved[7] += world["offset"][7]
        assert np.abs(moved - rx["truth"]).max() < 1e-8
        if r:
            assert 0.5 <= np.linalg.norm(rx["truth"][:3] - world["rx"][0]["truth"][:3]) <= 3.0 + 1e-9


def test_receivers_differ(built, oracle):
    world = jw.build((5, 8, 4))
    prns = [tuple(rx["prn"]) for rx in world["rx"]]
    assert len(set(prns)) == 3
    assert not np.array_equal(world["rx"][0]["wins"][0]["iq"][:64], world["rx"][1]["wins"][0]["iq"][:64])
    # the code phases were re-derived for each receiver's own position: a shared SV differs between two receivers
    a, b = world["rx"][1], world["rx"][3 - 1]
    shared = set(a["prn"]) & set(b["prn"])
    assert shared
    p = sorted(shared)[0]
    ia, ib = list(a["prn"]).index(p), list(b["prn"]).index(p)
    assert a["ho"]["rc"][ia] != b["ho"]["rc"][ib]


def test_narrow_banks_stay_inside_the_edge_flip_cap(built, oracle):
    """The clamp-path world: pairs do leave the banks, and the oracle's faithful row differs from its extended-precision row
    beyond 10 x POS_REF_NOISE at no more points than assert_parity sets aside, per receiver."""
    world = jw.build((5, 8, 4), widen=False)
    ref = jw.oracle_rows(world)
    for r, x in enumerate(ref["rx"][0]):
        assert x["oob_pos_x"] > 0 and x["oob_vel"] > 0, r
        assert x["pos_x"].max() > 0 and x["vel"].max() > 0
        flips = np.abs(x["pos"] - x["pos_x"]) > 10 * helpers.POS_REF_NOISE * x["pos"].max()
        flips[x["quirks"]] = False
        allowed = 16 + x["pos"].size * world["rx"][r]["K"] // 2000
        print("receiver %d: %d edge flips (cap %d), oob pos %d / %d, vel %d" % (r, flips.sum(), allowed, x["oob_pos"], x["oob_pos_x"],
                                                                             x["oob_vel"]))
        assert flips.sum() <= allowed


@pytest.mark.parametrize("start", sorted(jw.LOOP_STARTS))
def test_oracle_closed_loop_returns_to_the_truth(built, oracle, start):
    """The closed-loop world of tests/test_gpu_joint.py (position grid spaced by one sample; started one grid step off in the
    clock term, or in east, north, up and clock at once; joint_world.oracle_loop says why): the oracle's own joint loop scores
    window 0 with the handoff's channel parameters and stays, steps back by exactly the start offset in window 1, then stays on
    the grids' centre point, and ends on every receiver's true state."""
    world = jw.build((5, 8, 4), seed=2, W=4, pos_step=jw.SAMPLE)
    _enu, at1, bound = jw.LOOP_STARTS[start]
    ref = jw.oracle_loop(world, jw.loop_step(world, start))
    centre = jw.grid_index((3, 3, 3, 3))
    assert ref["argmax"] == [(centre, centre), (jw.grid_index(at1), centre), (centre, centre), (centre, centre)]
    for r, rx in enumerate(world["rx"]):
        assert np.abs(ref["fixes"][0, r] - rx["truth"]).max() > 100.0
        assert np.abs(ref["fixes"][3, r] - rx["truth"]).max() < bound


# the worlds of tests/test_gpu_joint_walk.py: (arguments of joint_world.build, tiles of the position and velocity grids)
WALK_WORLDS = {
    "J1": (dict(n_sv=(5, 8, 4), seed=3, W=2, pos_dim=15, vel_dim=14), (50, 38)),
    "J1-swapped": (dict(n_sv=(5, 8, 4), seed=3, W=2, pos_dim=14, vel_dim=15), (38, 50)),
    "J2": (dict(n_sv=(5, 8, 4), seed=7, W=4), (3, 3)),
    "J3": (dict(n_sv=(8,) * 8, seed=6, W=1, pos_dim=15, vel_dim=14), (50, 38)),
    "J6": (dict(n_sv=(5, 8, 4), seed=5, W=1, pos_dim=13, vel_dim=13), (28, 28)),
    "J7": (dict(n_sv=(5, 8, 4), seed=4, W=2, pos_dim=20, vel_dim=7), (157, 3)),
}


def test_defaults_keep_their_bits():
    """The grid dimension arguments leave the 7^4 worlds what they were."""
    import navlab_dpe_sdr_amd as dpe
    pos, vel = jw.grids()
    assert np.array_equal(pos, dpe.synth.uniform_grid(7, 40.0)) and np.array_equal(vel, dpe.synth.uniform_grid(7, 12.0))
    assert jw.scaled_at(jw.POS_AT, 7) == jw.POS_AT and jw.scaled_at(jw.VEL_AT, 7) == jw.VEL_AT
    assert jw.scaled_step(jw.POS_STEP, 7) == 40.0 and jw.scaled_step(jw.VEL_STEP, 7) == 12.0
    assert np.array_equal(jw.grids(jw.SAMPLE)[0], dpe.synth.uniform_grid(7, jw.SAMPLE))
    for dim in (13, 14, 15, 20):      # the larger grids keep the 7^4 grid's extent and the point leaves the first tile
        p, v = jw.grids(pos_dim=dim, vel_dim=dim)
        assert p.shape == (dim ** 4, 4) and np.abs(p).max() == pytest.approx(120.0) and np.abs(v).max() == pytest.approx(36.0)
        for at in (jw.POS_AT, jw.VEL_AT):
            s = jw.scaled_at(at, dim)
            assert all(0 <= c < dim for c in s) and jw.grid_index(s, dim) >= 1024 and s != ((dim - 1) // 2,) * 4


@pytest.mark.parametrize("name", sorted(WALK_WORLDS))
def test_walk_worlds_peak_on_the_scaled_offset_in_every_window(built, oracle, name):
    """Every receiver alone in every distinct window, and the sum, peak on the expected point of the larger grids, which is
    neither the centre nor in the first tile; no pair leaves the widened banks; the grids have the tile counts the GPU tests
    reason with."""
    kw, want_tiles = WALK_WORLDS[name]
    world = jw.build(**kw)
    ref = jw.oracle_rows(world)
    pd, vd = world["dims"]
    assert (-(-world["pos"].shape[0] // 1024), -(-world["vel"].shape[0] // 1024)) == want_tiles
    assert world["pos_at"] == jw.grid_index(jw.scaled_at(jw.POS_AT, pd), pd) and world["vel_at"] == jw.grid_index(jw.scaled_at(jw.VEL_AT, vd), vd)
    assert world["pos_at"] != jw.grid_index(((pd - 1) // 2,) * 4, pd) and world["vel_at"] != jw.grid_index(((vd - 1) // 2,) * 4, vd)
    if pd != 7:
        assert world["pos_at"] >= 1024
    if vd != 7:
        assert world["vel_at"] >= 1024
    assert len(ref["rx"]) == world["W"]
    for w in range(world["W"]):
        for r, x in enumerate(ref["rx"][w]):
            assert x["oob_pos"] == 0 and x["oob_pos_x"] == 0 and x["oob_vel"] == 0, (w, r)
            assert oracle.argmax_first(x["pos"]) == world["pos_at"], (w, r)
            assert oracle.argmax_first(x["pos_x"]) == world["pos_at"], (w, r)
            assert oracle.argmax_first(x["vel"]) == world["vel_at"], (w, r)
        for rname, at in (("pos", world["pos_at"]), ("pos_x", world["pos_at"]), ("vel", world["vel_at"])):
            assert oracle.argmax_first(ref[rname][w]) == at, (w, rname)
    if world["W"] > 1:
        assert not np.array_equal(world["rx"][0]["wins"][0]["iq"], world["rx"][0]["wins"][1]["iq"])
    if name == "J6":      # the tie test's point list: the first 24 tiles of the grids hold both expected points
        assert 1024 <= world["pos_at"] < 24 * 1024 and 1024 <= world["vel_at"] < 24 * 1024


@pytest.mark.parametrize("name,side", [("J1", "L"), ("J1", "B"), ("J1-swapped", "L"), ("J1-swapped", "B"), ("J2", False), ("J6", False)])
def test_walk_worlds_with_narrow_banks(built, oracle, name, side):
    """The clamp-path variants: with only the lag (bin) banks narrow, pairs of every receiver leave the position (velocity)
    banks in every window and none the other side's, which keeps the widened world's rows; the faithful position row stays
    inside helpers.assert_parity's cap on edge flips per receiver."""
    world = jw.build(**dict(WALK_WORLDS[name][0], widen=side))
    ref = jw.oracle_rows(world)
    if side:
        base = jw.build(**WALK_WORLDS[name][0])
        assert (world["L"], world["B"]) == ((1, base["B"]) if side == "L" else (base["L"], 2))
        clean = jw.oracle_rows(base)
    for w in range(world["W"]):
        for r, x in enumerate(ref["rx"][w]):
            assert (x["oob_pos_x"] > 0) == (side != "B") and (x["oob_vel"] > 0) == (side != "L"), (w, r)
            assert x["pos_x"].max() > 0 and x["vel"].max() > 0
            flips = np.abs(x["pos"] - x["pos_x"]) > 10 * helpers.POS_REF_NOISE * x["pos"].max()
            flips[x["quirks"]] = False
            allowed = 16 + x["pos"].size * world["rx"][r]["K"] // 2000
            print("%s narrow %s, window %d receiver %d: %d edge flips (cap %d), oob pos %d / %d, vel %d"
                  % (name, side, w, r, flips.sum(), allowed, x["oob_pos"], x["oob_pos_x"], x["oob_vel"]))
            assert flips.sum() <= allowed
        if side:
            same = "vel" if side == "L" else "pos_x"
            assert np.array_equal(ref[same][w], clean[same][w])
            assert oracle.argmax_first(ref[same][w]) == (world["vel_at"] if side == "L" else world["pos_at"])
