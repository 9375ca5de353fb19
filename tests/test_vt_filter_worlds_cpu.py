"""CPU: proof of the inputs of tests/test_gpu_vt_filter.py (tests/vt_cases.py).  Every case's closed loop in tests/vt_ref.py shows the
included masks and status words the case is built for; no lock metric lies near the gate, so a deviation at the 1e-6 level cannot
flip a channel; a maths library that is 2 ulps off (vt_ref.Nudge) gives the same masks; and the HOST form of vt_filter_epoch passes
the exact class and the bounds of vt_cases.check_epoch on those inputs -- the bounds are attainable before a GPU is involved."""
import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import vt_cases, vt_ref
from tests.test_vt_host_cpu import host_state

VT = dpe.engine.VectorTracker


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return dpe.engine.lib()


@pytest.fixture(scope="module")
def loops(oracle):
    return {name: (vt_cases.case(oracle, name),) + (vt_cases.closed_loop(vt_cases.case(oracle, name), oracle),) for name in vt_cases.NAMES}


@pytest.mark.parametrize("name", vt_cases.NAMES)
def test_case_shows_its_masks_and_status(loops, capsys, name):
    c, steps = loops[name]
    recs = [r for _, _, r in steps]
    lock = np.array([r["lock"] for r in recs])
    incl = np.array([[(r["mask"] >> k) & 1 for k in range(c["cfg"].K)] for r in recs], dtype=bool)
    with capsys.disabled():
        print("\n%s: masks %s status %s; lock metric of included channels >= %.1f, of excluded <= %.1f"
              % (name, [bin(r["mask"]) for r in recs], [r["status"] for r in recs], lock[incl].min(), lock[~incl].max() if (~incl).any() else 0.0))
    assert [r["mask"] for r in recs] == c["masks"] and [r["status"] for r in recs] == c["status"]
    assert [r["n_incl"] for r in recs] == [bin(m).count("1") for m in c["masks"]]
    assert np.all(np.abs(lock - c["cfg"].lock_thr) > vt_cases.LOCK_MARGIN), lock
    final = 0
    for s in c["status"]:
        final |= s
    assert steps[-1][0]["status"] | recs[-1]["status"] == final


def test_what_the_cases_are_built_to_reach(loops):
    """The branches themselves, on vt_ref's states: the first epoch without cached satellite states, measured W and a wrapped history
    ring, rows off the identity chanOf, a sum case of -1 with zero sums, rxTime0 off the millisecond grid."""
    c, steps = loops["nominal"]
    assert steps[0][0]["sat"] is None and steps[1][0]["sat"] is not None
    for e, (_, _, r) in enumerate(steps):
        assert np.all((r["wR"] != c["cfg"].init_var[0]) == (e >= vt_cases.NUM_PREV)), (e, r["wR"])
    assert np.all(steps[5][0]["histPos"] == 5 % vt_cases.NUM_PREV) and np.all(steps[5][0]["histN"] == vt_cases.NUM_PREV)
    c, steps = loops["k16_partial"]
    assert [2 * r["n_incl"] for _, _, r in steps] == [32, 30, 26, 28, 32]
    c, steps = loops["bad_window"]
    for _, sums, r in steps:
        assert np.all(sums[:, 1, 6] == -1.0) and np.all(sums[:, 1, :6] == 0.0)
        others = [k for k in range(6) if k != 1]
        assert all(np.all(np.isfinite(r[n][others])) for n in vt_ref.CHAN_NAMES) and np.all(np.isfinite(r["X"])) and np.all(np.isfinite(r["diag"]))
    c, steps = loops["off_grid"]
    assert not c["cfg"].round_ms
    assert any(abs(r["rxTime0"] * 1000.0 - round(r["rxTime0"] * 1000.0)) > 1e-4 for _, _, r in steps)
    c, steps = loops["too_few"]
    before, _, r = steps[2]
    F = np.eye(8)
    F[:4, 4:] = c["cfg"].NT * np.eye(4)
    assert np.array_equal(r["X"], F @ before["X"]) and np.array_equal(r["X"][4:], before["X"][4:])          # predict only
    assert np.allclose(r["diag"], np.diag(F @ before["Sigma"] @ F.T + np.diag(c["cfg"].q)), rtol=1e-14, atol=0)


@pytest.mark.parametrize("name", vt_cases.NAMES)
def test_a_nudged_maths_library_gives_the_same_masks(oracle, loops, name):
    c, steps = loops[name]
    alt = vt_cases.closed_loop(c, oracle, nudge=vt_ref.Nudge(5))
    assert [r["mask"] for _, _, r in alt] == [r["mask"] for _, _, r in steps]
    assert [r["status"] for _, _, r in alt] == [r["status"] for _, _, r in steps]


@pytest.mark.parametrize("name", vt_cases.NAMES)
def test_host_form_passes_the_exact_class_and_the_bounds(built, oracle, loops, capsys, name):
    c, steps = loops[name]
    cfg, s = c["cfg"], c["w"]["start"]
    ccfg = VT.config(cfg.fs, cfg.prns, T=cfg.T, N=cfg.N, num_prev=cfg.num_prev)
    lines = []
    for e, (before, sums, _) in enumerate(steps):
        h = host_state(cfg, before)
        h.status = before["status"]
        got = VT.filter_step_host(ccfg, s["eph"], s["tow"], s["cps"], h, sums)
        assert h.satValid == 1
        vt_cases.check_epoch(c, oracle, e, before, sums, got, vt_ref.state_from_rec(cfg, h), lines=lines)
    with capsys.disabled():
        print("\nhost form against vt_ref, %s" % name)
        print("\n".join(lines))


def test_state_from_rec_inverts_host_state(oracle, loops):
    c, steps = loops["nominal"]
    for before, _, _ in (steps[0], steps[4]):
        h = host_state(c["cfg"], before)
        h.status = before["status"]
        back = vt_ref.state_from_rec(c["cfg"], h)
        assert set(back) == set(before)
        for n, v in before.items():
            assert (back[n] is None and v is None) or np.array_equal(back[n], v), n
