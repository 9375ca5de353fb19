"""GPU: dpe_nav_solve_log -- every logged epoch of a scalar tracker solved in one launch -- against the reference twin's
calculate_nav_soln (fixture O15), held to the host form's bound; and its invariances: epoch ranges and strides, channel subsets,
one launch against two."""
import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests.test_nav_cpu import OUT_NAMES, fix_row, o15_navigator, sol_bound

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(golden):
    import __graft_entry__ as ge
    ge.build()
    g = golden("o15_scalar_nav")
    M = g["sol_cp"].shape[0]
    trk = dpe.ScalarTracker(2.5e6, g["sol_prn"], log_capacity_windows=64)
    trk.load_log(dict(cp=g["sol_cp"], rc=g["sol_rc"], fi=g["sol_fi"]))      # O15's epochs as the tracker's log rows
    nav = o15_navigator(g)
    yield g, M, trk, nav
    trk.close()
    nav.close()


def rows(out):
    return np.concatenate([out["rxTime_a"][:, None], out["rxTime"][:, None], out["X_ECEF"]], axis=1)


def test_solve_log_matches_twin(world, capsys):
    g, M, trk, nav = world
    out = nav.solve_log(trk)
    assert out.shape == (M,) and np.all(out["status"] == 0) and np.all(out["iterations"] <= 10)
    got = rows(out)
    err = np.abs(got - g["sol_twin"]).max(axis=0)              # every epoch, against the twin
    bound = sol_bound(g)
    host = np.array([fix_row(nav.solve(g["sol_cp"][m], g["sol_rc"][m], g["sol_fi"][m])) for m in range(M)])
    dev_host = np.abs(got - host).max(axis=0)
    with capsys.disabled():
        print("\nO15 device solve_log: max |ours - twin| over %d epochs / bound, and device - host" % M)
        for n, e, b, d in zip(OUT_NAMES, err, bound, dev_host):
            print("  %-9s err %.3e  bound %.3e  device - host %.3e" % (n, e, b, d))
    assert np.all(err <= bound), (err, bound)
    t0, dt = float(g["sol_sched_rxTime0"]), float(g["sol_sched_step"])
    out = nav.solve_log(trk, rx_time0=t0, rx_time_step=dt)
    assert np.all(np.abs(rows(out) - g["sol_sched"]).max(axis=0) <= bound)
    assert nav.status() == 0


def test_ranges_strides_and_split_launches(world):
    g, M, trk, nav = world
    full = nav.solve_log(trk)
    for first, stride in [(0, 2), (1, 3), (5, 1), (M - 1, 1), (2, 7)]:
        n = (M - first + stride - 1) // stride
        part = nav.solve_log(trk, first=first, n_epochs=n, stride=stride)
        assert part.tobytes() == full[first::stride].tobytes(), (first, stride)
    a, b = nav.solve_log(trk, first=0, n_epochs=M // 2), nav.solve_log(trk, first=M // 2, n_epochs=M - M // 2)
    assert np.concatenate([a, b]).tobytes() == full.tobytes()
    for n in (1, 3, 4, 5):                                       # partial blocks of the launch
        assert nav.solve_log(trk, first=2, n_epochs=n).tobytes() == full[2:2 + n].tobytes()


def test_channel_subsets(world):
    g, M, trk, nav = world
    sel = [0, 2, 3, 5, 7]
    masked = nav.solve_log(trk, chans=sel)
    sub_trk = dpe.ScalarTracker(2.5e6, g["sol_prn"][sel], log_capacity_windows=M)
    sub_trk.load_log(dict(cp=g["sol_cp"][:, sel], rc=g["sol_rc"][:, sel], fi=g["sol_fi"][:, sel]))
    sub = dpe.ScalarNavigator(g["sol_prn"][sel])
    sub.set_ephemerides(g["sol_eph"][sel], g["sol_tow"][sel], g["sol_cp_timestamp"][sel])
    alone = sub.solve_log(sub_trk)
    assert masked.tobytes() == alone.tobytes() and np.all(masked["status"] == 0)     # a subset by mask and as a handle of its own
    host = np.array([fix_row(nav.solve(g["sol_cp"][m], g["sol_rc"][m], g["sol_fi"][m], chans=sel)) for m in range(M)])
    assert np.abs(rows(masked) - host)[:, 2:6].max() < 1e-6 and np.abs(rows(masked) - host)[:, 6:].max() < 1e-10
    few = nav.solve_log(trk, chans=[1, 4, 6])                    # three satellites: a status bit and finite numbers
    assert np.all(few["status"] & dpe.ScalarNavigator.SOL_RANK_POS) and np.isfinite(rows(few)).all()
    with pytest.raises(dpe.DpeError):
        nav.solve_log(trk, first=M - 2, n_epochs=5)              # beyond the tracked windows
    sub_trk.close()
    sub.close()
