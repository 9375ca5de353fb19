"""CPU, oracle only: the batch of tests/refine_world.py is a fair input for the coarse-to-fine scan, and the span rule of
DESIGN.md 2.4g is a fact of these data.

(a) the four windows' coarse arg-maxes are not all the same point (a batch needs a centre per window);
(b) two levels, the fine one over +-2 coarse steps, end on the first maximum of the dense 31^4 grid of the fine step, on every
    window and both manifolds -- through the numpy restatement of the level chain (tests/refine_ref.py: fp32 centres);
(c) every arg-max used (coarse, fine, dense rows) leads its runner-up by at least ten oracle tolerances (ORACLE_TOL = 2e-6 of
    the maximum), and the oracle counts no pair outside the banks on the dense grids;
(d) with the fine level over +-1 coarse step the chain misses the dense maximum on at least one window: the coarse arg-max
    slides along the up / clock ridge by more than one coarse step.  That is the span rule, pinned."""
import numpy as np
import pytest

from tests import refine_ref as rr
from tests import refine_world as rw

TEN_TOL = 10 * rw.ORACLE_TOL


@pytest.fixture(scope="module")
def world():
    return rw.build()


@pytest.fixture(scope="module")
def chains(world):
    """[half][window][manifold] -> (per-level dicts, final point) of the level chain on the oracle's rows."""
    out = {}
    for half in (2, 1):
        lv = rw.levels(half)
        out[half] = [[rr.chain(rw.axes_of(lv, m), rw.scorer(world, w, m)) for m in (0, 1)] for w in range(world["N"])]
    return out


def test_decode_encode_and_key_zero():
    dims = (3, 5, 7, 25)
    for i in (0, 1, 24, 25, 3 * 5 * 7 * 25 - 1, 1234):
        assert rr.encode(rr.decode(i, dims), dims) == i
    assert rr.decode(((1 * 5 + 2) * 7 + 3) * 25 + 4, dims) == (1, 2, 3, 4)
    assert rr.first_max(np.array([np.nan, np.nan])) == -1 and rr.make_key(0.0, -1) == 0
    assert rr.first_max(np.array([1.0, np.nan, 2.0, 2.0])) == 2
    # a chain whose first level has no score stops: index -1 at every level, NaN point
    ax = [[np.array([0.0, 1.0])] * 4] * 3
    lv, pt = rr.chain(ax, lambda p: np.full(p.shape[0], np.nan))
    assert [x["index"] for x in lv] == [-1, -1, -1] and np.isnan(pt).all()
    # the centre is a sum of fp32 roundings, not of fp64 axes
    a = [[np.array([0.1])] * 4, [np.array([0.2])] * 4, [np.array([0.3])] * 4]
    c = rr.point_of(a, [0, 0, 0])
    want = np.float32(np.float32(np.float32(0.1) + np.float32(0.2)) + np.float32(0.3))
    assert c.dtype == np.float32 and c[0] == want


def test_dense_grids_stay_inside_the_banks(world):
    for w, (_p, _v, oob) in enumerate(rw.dense_rows(world)):
        assert oob == 0, (w, oob, world["L"], world["B"])


def test_coarse_maxima_differ_between_windows(chains):
    for m in (0, 1):
        assert len({chains[2][w][m][0][0]["index"] for w in range(4)}) > 1, m


def test_two_levels_reach_the_dense_maximum_with_margins(world, chains):
    dense = rw.dense_rows(world)
    for w in range(world["N"]):
        for m in (0, 1):
            lv, _pt = chains[2][w][m]
            i_dense, mg = rw.margin(dense[w][m])
            print("window %d manifold %d: dense margin %.3g, coarse %.3g, fine %.3g" % (w, m, mg, rw.margin(lv[0]["row"])[1], rw.margin(lv[1]["row"])[1]))
            assert mg >= TEN_TOL, (w, m, mg)
            for x in lv:
                i, g = rw.margin(x["row"])
                assert i == x["index"] and g >= TEN_TOL, (w, m, g)
            assert rw.dense_index(lv[0]["index"], lv[1]["index"], 2) == i_dense, (w, m)


def test_one_coarse_step_of_span_misses(world, chains):
    dp, dv = rw.dense(2)
    missed = []
    for w in range(world["N"]):
        for m in (0, 1):
            _lv, pt = chains[1][w][m]
            best = (dp, dv)[m].global_point(rr.first_max(rw.dense_rows(world)[w][m]))
            d = np.abs(pt - best)
            if d.max() > 0.5 * (rw.ew.POS_STEP, rw.ew.VEL_STEP)[m] / rw.RATIO:
                missed.append((w, m, d))
    print("misses at +-1 coarse step:", [(w, m, np.round(d, 1).tolist()) for w, m, d in missed])
    assert missed
