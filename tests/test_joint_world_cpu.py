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
