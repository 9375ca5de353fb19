"""CPU: the fault worlds of the subsets scan tests (tests/fde_world.py) are what they claim to be, by the existing oracle
alone (extended-precision position rows, the oracle handed only a subset's channels).

Per world (K = 8, seed 0, one 2 ms window, 7^4 grids at 40 m steps), as found when the constants were fixed:

| world | full set's arg-max | without j | without any k != j | smallest margin (of the row maximum) | separations (m) |
| clean | truth | truth | truth | 0.0040 | all 0 |
| j3: bias 200 m, gain 4, LPower 1 | 174.4 m off | truth, margin 0.050 | never truth | full 0.0155, others >= 0.0012 | j: 174.4, others <= 69.3 |
| j0: the same on SV 0 | 149.7 m off | truth, margin 0.043 | never truth | full 0.00085, others >= 0.00058 | j: 149.7, others <= 120.0 |
| j3-lp2: bias 120 m, gain 3, LPower 2 | 174.4 m off | truth, margin 0.094 | never truth | full 0.0188, others >= 0.0062 | j: 174.4, others 0 |

Every row the GPU tests rely on has a margin (best - second best, of the row maximum) of at least 10 x the oracle tolerance of
the GPU tests (2e-6), so a GPU row within tolerance has the same arg-max.  pipeline.solution_separation on the oracle's fixes
names j in the fault worlds and -1 in the clean one, at a threshold of one position step (40 m)."""
import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import epoch_world as ew, fde_world as fw

NEED = 10 * ew.ORACLE_TOL
# name -> (distance of the full set's arg-max from the truth (m), largest separation of a k != j exclusion (m))
EXPECT = {"clean": (0.0, 0.0), "j3": (174.4, 69.3), "j0": (149.7, 120.0), "j3-lp2": (174.4, 0.0)}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()


def test_masks():
    m = dpe.engine.leave_one_out_masks(8)
    assert m.dtype == np.uint64 and [int(x) for x in m] == [0xFF & ~(1 << j) for j in range(8)]
    assert [int(x) for x in dpe.engine.leave_one_out_masks(2)] == [2, 1]
    with pytest.raises(dpe.DpeError):
        dpe.engine.leave_one_out_masks(1)


def test_only_the_samples_differ(built):
    base = ew.build(N=1, K=fw.K, seed=fw.SEED)
    clean = fw.build("clean")
    assert np.array_equal(clean["wins"][0]["iq"], base["wins"][0]["iq"])
    for name in ("j3", "j0", "j3-lp2"):
        world = fw.build(name)
        assert world["pos"] is base["pos"] and world["vel"] is base["vel"] and (world["L"], world["B"]) == (base["L"], base["B"])
        a, b = world["wins"][0], base["wins"][0]
        assert not np.array_equal(a["iq"], b["iq"])
        for k in b:
            if k == "iq":
                continue
            if isinstance(b[k], dict):
                assert all(np.array_equal(a[k][n], b[k][n]) for n in b[k]), k
            else:
                assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("name", sorted(fw.WORLDS))
def test_fault_world(built, oracle, name):
    world = fw.build(name)
    j = world["fault"]
    truth = world["pos_at"]
    full_mask = (1 << fw.K) - 1
    masks = fw.masks_loo()
    full = fw.oracle_subset(world, full_mask)
    rows = [fw.oracle_subset(world, m) for m in masks]
    for r in [full] + rows:
        assert r["oob_pos_x"] == 0 and r["oob_vel"] == 0                     # no out-of-window pair
    at_full = oracle.argmax_first(full["pos_x"])
    off = float(np.linalg.norm(world["pos"][at_full] - world["pos"][truth]))
    margins = [fw.margin(r["pos_x"]) for r in rows]
    print("%s: full set's arg-max %.1f m off the truth (margin %.3g); leave-one-out margins %s"
          % (name, off, fw.margin(full["pos_x"]), ["%.3g" % m for m in margins]))
    assert abs(off - EXPECT[name][0]) < 0.05
    assert fw.margin(full["pos_x"]) >= NEED
    for k, r in enumerate(rows):
        at = oracle.argmax_first(r["pos_x"])
        assert margins[k] >= NEED, k
        if j is None or k == j:
            assert at == truth, k
        else:
            assert at != truth, k
    # the velocity manifold is untouched by a code-phase fault: every subset peaks on the expected point
    for r in [full] + rows:
        assert oracle.argmax_first(r["vel"]) == world["vel_at"] and fw.margin(r["vel"]) >= NEED
    f, subs = fw.oracle_fixes(world)
    suspect, sep = dpe.pipeline.solution_separation(f, subs, masks, fw.THRESHOLD_M)
    print("%s: separations (m) %s -> suspect %d" % (name, np.round(sep, 1).tolist(), suspect))
    assert suspect == (-1 if j is None else j)
    if j is None:
        assert np.all(sep == 0.0)
    else:
        others = np.delete(sep, j)
        assert abs(sep[j] - EXPECT[name][0]) < 0.05 and sep[j] > fw.THRESHOLD_M
        assert others.max() <= EXPECT[name][1] + 0.05 and others.max() < sep[j]


def test_solution_separation_rules():
    """The suspect is a SINGLE-SV exclusion; other masks are measured but never named; the threshold is required."""
    pos = [dict(offset=np.array([x, 0.0, 0.0, 0.0, 0, 0, 0, 0], dtype=np.float64)) for x in (0.0, 30.0, 80.0, 500.0)]
    masks = np.array([0b110, 0b101, 0b001], dtype=np.uint64)           # without 0, without 1, SV 0 alone (K = 3)
    s, sep = dpe.pipeline.solution_separation(pos[0], [pos[1], pos[2], pos[3]], masks, 40.0)
    assert s == 1 and sep.tolist() == [30.0, 80.0, 500.0]
    s, _ = dpe.pipeline.solution_separation(pos[0], [pos[1], pos[2], pos[3]], masks, 80.0)      # "exceeds": strictly
    assert s == -1
    with pytest.raises(TypeError):
        dpe.pipeline.solution_separation(pos[0], [pos[1]], masks[:1])
    with pytest.raises(ValueError):
        dpe.pipeline.solution_separation(pos[0], [pos[1]], masks, 40.0)


def test_closed_loop_world(built, oracle):
    """The six-window world of the closed-loop test (fde_world.build_loop: SV 3 late by 250 m and 6 x stronger in windows 2 .. 4
    only; found with this oracle, see fde_world.LOOP_*), through fde_world.oracle_fde_loop -- run_fde_closed_loop by the oracle
    alone.  As found: with exclusion the suspects are -1, -1, 3, 3, 3, -1 and every fix stays within 0.15 m of the moving truth
    (smallest margin over all rows relied on 3.3e-3 of the row maximum); without exclusion the same loop is 169.1, 277.0 and
    215.8 m off in windows 2 .. 4 (smallest margin 4.1e-4); no pair leaves the banks in either loop."""
    world = fw.build_loop()
    assert world["iq"].shape == (fw.LOOP_N, 2 * world["S"]) and world["fault_windows"] == (2, 3, 4) and world["fault"] == 3
    step = ew.POS_STEP
    want = [3 if w in world["fault_windows"] else -1 for w in range(fw.LOOP_N)]
    with_x, without = fw.oracle_fde_loop(world, True), fw.oracle_fde_loop(world, False)
    for name, r in (("with exclusion", with_x), ("without", without)):
        err = np.abs(r["fixes"][:, :4] - world["truth"][:, :4]).max(axis=1)
        print("%s: suspects %s, fix off the truth (m) %s, smallest margin %.3g" % (name, r["suspects"].tolist(), np.round(err, 3).tolist(),
                                                                                    r["margin"].min()))
        assert r["margin"].min() >= NEED and not r["oob"].any()
    err = np.abs(with_x["fixes"][:, :4] - world["truth"][:, :4]).max(axis=1)
    assert with_x["suspects"].tolist() == want and err.max() < step / 2          # on the truth's grid point in all six windows
    for w in range(fw.LOOP_N):
        am = with_x["argmax"][w]
        assert (am[0] == (world["centre_at"], world["centre_at"])) == (w not in world["fault_windows"]), w
        if w in world["fault_windows"]:
            assert am[1 + 3] == (world["centre_at"], world["centre_at"]) and with_x["seps"][w, 3] > step, w
            assert np.delete(with_x["seps"][w], 3).max() < with_x["seps"][w, 3], w
        else:
            assert not with_x["seps"][w].any(), w
    err0 = np.abs(without["fixes"][:, :4] - world["truth"][:, :4]).max(axis=1)
    assert err0[:2].max() < step / 2 and err0[2:5].min() > step and without["suspects"][:3].tolist() == [-1, -1, 3]
