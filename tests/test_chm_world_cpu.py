"""The channel-manager worlds of tests/chm_world.py proven without a GPU: on every world the host ChanMgr agrees with the oracle's
independent C restatement at the bounds of test_abi_cpu.py::test_chanmgr_matches_oracle, and every world reaches the branch it is
built for -- computed from the world alone.  The filter matrices of tests/test_gpu_chm_filter.py: each has the pivot pattern or
the singular column it claims, by a numpy copy of the host form's pivot rule, and the host filter accepts or refuses it as stated."""
import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import chm_world as cw


def _oracle_mgr(oracle, ho, T):
    return oracle.ChanMgr(ho["prn_list"], ho["rc"], ho["ri"], ho["fc"], ho["fi"], ho["cp"], ho["cp_timestamp"], ho["TOW"], ho["eph"],
                          ho["rxTime"], T)


def _host_vs_oracle(oracle, ho, T, tg, fixes):
    """Start + len(fixes) - 1 Updates; the bounds of test_chanmgr_matches_oracle, none wider."""
    cm = dpe.ChanMgr.from_handoff(ho, T)
    om = _oracle_mgr(oracle, ho, T)
    for it, (x1, xk) in enumerate(fixes):
        if it == 0:
            cm.Start(x1, xk, tg)
            ob, oR = om.start(x1, xk, tg)
        else:
            cm.Update(x1, xk, tg)
            ob, oR = om.update(x1, xk, tg)
        s, e, w, batch = cm.outputs(with_batch=True)
        assert np.array_equal(s["codePhaseStart"], om.rcStart) and np.array_equal(s["cpElapsedStart"], om.cpElaStart), it
        assert np.abs(e["codePhaseEnd"] - om.rcEnd).max() < 1e-9 and np.array_equal(e["cpElapsedEnd"], om.cpElaEnd), it
        assert np.abs(s["carrierPhaseStart"] - om.riStart).max() < 1e-12, it
        assert np.abs(s["codeFrequency"] - om.fc).max() < 1e-6 and np.abs(s["carrierFrequency"] - om.fi).max() < 1e-6, it
        assert w["rxTime"][0] == om.rxTime, it
        assert np.abs(batch - ob).max() < 1e-6 and np.abs(w["enu2ecef"][0] - oR).max() < 1e-14, it
        assert np.abs(e["satState"] - ob[:, len(tg) // 2]).max() < 1e-6, it
    cm.Stop()


@pytest.mark.parametrize("name", cw.WORLDS)
def test_host_form_matches_the_oracle_on_every_world(oracle, name):
    """Start + 4 Updates with the moving fix of the device test (tens of metres per window)."""
    wd = cw.world(name)
    ho = wd["good"] if name == "kepler_fail" else wd["ho"]
    X = ho["X_ECEF"]
    _host_vs_oracle(oracle, ho, wd["T"], wd["tg"], [(X, X)] + cw.moving_fixes(X, 4))
    if "elev" in ho and name != "kepler_fail":
        assert np.nanmin(ho["elev"]) >= 5.0          # visibility, where the builder placed the SVs


@pytest.mark.parametrize("name,sign", [("week_lo", -1), ("week_hi", +1)])
def test_week_worlds_cross_the_half_week(name, sign):
    """|tx - t_oe| > 302 400 with the sign the world claims (t_oc = t_oe: both tc and tk wrap); the wrapped tk is hours, not a week."""
    ho = cw.world(name)["ho"]
    d = ho["tx"] - ho["eph"][:, cw.I_TOE]
    assert np.array_equal(ho["eph"][:, cw.I_TOC], ho["eph"][:, cw.I_TOE])
    assert (sign * d > 302400.0).all(), d
    assert (np.abs([cw.half_week(v) for v in d]) < 4 * 3600.0).all()
    assert len(ho["prn_list"]) == 8


def test_ecc_world_has_its_eccentricities():
    wd = cw.world("ecc")
    assert np.array_equal(wd["ho"]["eph"][:, cw.I_E], np.array(cw.ECC_LIST))
    assert {0.0, 0.02, 0.3} == set(cw.ECC_LIST) and wd["ho"]["eph"][0, cw.I_E] == 0.0


def test_sites_land_in_four_different_quadrants(oracle):
    """(hemisphere, longitude quadrant) of the four sites from oracle.ecef2ll: pairwise different, none the handoff's (+40, -88);
    the pole has p = 0 exactly, the equator site z = 0 exactly and a longitude one step short of +180."""
    def quadrant(X):
        lat, lon = np.degrees(oracle.ecef2ll(X))
        hemi = "pole" if abs(lat) > 89.999 else ("equator" if lat == 0.0 else ("N" if lat > 0 else "S"))
        return hemi, int(np.floor(lon / 90.0))
    q = {n: quadrant(cw.world("site_" + n)["ho"]["X_ECEF"]) for n in cw.SITES}
    q0 = quadrant(cw.base_handoff()["X_ECEF"])
    assert q0 == ("N", -1)
    assert len(set(q.values())) == 4 and q0 not in q.values(), q
    assert q["sydney"] == ("S", 1) and q["arctic"] == ("N", -2) and q["equator180"] == ("equator", 1) and q["pole"][0] == "pole"
    Xp, Xe = cw.world("site_pole")["ho"]["X_ECEF"], cw.world("site_equator180")["ho"]["X_ECEF"]
    assert Xp[0] == 0.0 and Xp[1] == 0.0 and Xe[2] == 0.0 and Xe[0] < 0.0 and 0.0 < Xe[1] < 1.0


def test_wide_time_grid_takes_both_batch_branches():
    """omega_e x (tg[t] - tg[mid]) / c >= 1e-8 for the outer entries (direct evaluation), < 1e-8 for the inner ones (first order);
    dimT even, the mid entry dimT / 2 and not 0."""
    tg = cw.world("wide_tg")["tg"]
    mid = len(tg) // 2
    assert len(tg) % 2 == 0 and mid != (len(tg) - 1) // 2 and tg[mid] != 0.0
    d = np.abs(cw.OMEGA_E * (tg - tg[mid]) / cw.C_LIGHT)
    outer, inner = [0, 1, 6, 7], [2, 3, 5]
    assert (d[outer] >= 1e-8).all() and (d[inner] < 1e-8).all() and d[mid] == 0.0, d
    assert tg[mid - 1] != tg[mid]       # the row a wrong mid index would take is a different state


def test_full_world_walks_the_batch_loop_twice():
    wd = cw.world("full")
    K, dimT = len(wd["ho"]["prn_list"]), len(wd["tg"])
    assert K == cw.MAX_CHAN == 37 and dimT == 9 and K * dimT > 256


def test_kepler_fail_world_fails_where_it_says(oracle):
    wd = cw.world("kepler_fail")
    ho, k = wd["ho"], wd["bad_chan"]
    assert len(ho["prn_list"]) == 5 and ho["eph"][k, cw.I_E] == 0.99
    assert oracle.sat_pos(ho["eph"][k], wd["bad_tx"])[1] != 0
    n = np.sqrt(cw.MU / ho["eph"][k, 0] ** 6) + ho["eph"][k, cw.I_DELN]
    # the margin: the tenth Newton step is >= 1e-5 where the cap asks for 1e-12, everywhere the mean anomaly goes in the test's windows
    assert wd["bad_margin"] >= 1e-5
    for d in np.arange(-2e-6, 3e-5, 1e-7):
        assert cw.kepler_last_step(wd["bad_M"] + d, 0.99) >= 1e-5, d
    for dm in (-0.04, 0.04, -1e-9, 1e-9, -1e-12, 1e-12):                         # the neighbours at +-0.04 rad fail too
        eph = ho["eph"][k].copy()
        eph[cw.I_M0] += dm
        assert oracle.sat_pos(eph, wd["bad_tx"])[1] != 0, dm
    for w in range(8):                                                            # ... and so does every window's transmit time
        for dt in (0.0, 1e-7, -1e-7, 2.0 ** -10):
            assert oracle.sat_pos(ho["eph"][k], wd["bad_tx"] + w * wd["T"] + dt)[1] != 0, (w, dt)
    assert n * 6 * wd["T"] < 1e-4
    for j in range(5):
        if j != k:
            assert oracle.sat_pos(ho["eph"][j], wd["bad_tx"])[1] == 0
    X = ho["X_ECEF"]
    cm = dpe.ChanMgr.from_handoff(ho, wd["T"])
    with pytest.raises(dpe.DpeError, match=r"Kepler iteration failed \(PRN %d\)" % ho["prn_list"][k]):
        cm.Start(X, X, wd["tg"])
    cm.Stop()
    good = dpe.ChanMgr.from_handoff(wd["good"], wd["T"])
    good.Start(X, X, wd["tg"])
    assert np.array_equal(good.outputs()[0]["prn"], np.delete(ho["prn_list"], k))
    good.Stop()


def test_no_eccentricity_up_to_0_97_fails(oracle):
    """Why `ecc` stays at e <= 0.3 and `kepler_fail` needs 0.99: at e <= 0.97 no mean anomaly misses the 10-iteration cap."""
    ho = cw.base_handoff()
    eph = ho["eph"][0].copy()
    tx = float(ho["rxTime"]) - 0.07
    for e in (0.3, 0.9, 0.97):
        eph[cw.I_E] = e
        for m in np.arange(-3.14, 3.14, 0.02):
            eph[cw.I_M0] = m
            assert oracle.sat_pos(eph, tx)[1] == 0, (e, m)


@pytest.mark.parametrize("name", ["long_1ms", "long_5ms"])
def test_long_runs_stay_clear_of_the_code_period_edges(oracle, name):
    """A condition on the seeds (tests/chm_world.py), not a measurement: in no step is the host's rcEnd within 1e-3 chips of 0 or
    1023 -- which lets the GPU test demand exact integers of a device form that agrees to 1e-4 chips -- and the counters do roll over.
    The host form against the oracle over the whole run, at the bounds of test_chanmgr_long_runs_random_subsets."""
    wd = cw.world(name)
    ho, T, tg = wd["ho"], wd["T"], wd["tg"]
    cm = dpe.ChanMgr.from_handoff(ho, T)
    om = _oracle_mgr(oracle, ho, T)
    cp0 = None
    for it, (xk, centre) in enumerate(cw.long_run_fixes(ho["X_ECEF"], T, wd["n"], wd["seed"])):
        if it == 0:
            cm.Start(xk, centre, tg)
            ob, oR = om.start(xk, centre, tg)
        else:
            cm.Update(xk, centre, tg)
            ob, oR = om.update(xk, centre, tg)
        s, e, w, batch = cm.outputs(with_batch=True)
        rc = e["codePhaseEnd"]
        assert (rc > 1e-3).all() and (rc < 1023.0 - 1e-3).all(), (it, rc)
        assert np.array_equal(s["cpElapsedStart"], om.cpElaStart) and np.array_equal(e["cpElapsedEnd"], om.cpElaEnd), it
        assert np.array_equal(e["cpRef"], om.cpRef) and np.array_equal(e["cpRefTOW"], om.cpRefTOW), it
        assert np.abs(s["codePhaseStart"] - om.rcStart).max() < 1e-8 and np.abs(rc - om.rcEnd).max() < 1e-8, it
        d = np.abs(s["carrierPhaseStart"] - om.riStart)
        assert np.minimum(d, 1.0 - d).max() < 1e-7, it
        assert np.abs(batch - ob).max() < 1e-5 and np.abs(w["enu2ecef"][0] - oR).max() < 1e-13, it
        if cp0 is None:
            cp0 = e["cpElapsedEnd"].copy()
    assert (e["cpElapsedEnd"] - cp0 >= round((wd["n"] - 1) * T * 1000) - 2).all()     # one code period per millisecond went by
    cm.Stop()


# ---------------------------------------------------------------------------------------------------------------------------------
# the filter's P_k|k-1 loads (tests/test_gpu_chm_filter.py): pivot patterns by the numpy copy of the rule, and what the host filter does

def _host_filter(P, couple=True):
    x0 = np.arange(8.0) * 3.0 + 1.0
    f = dpe.engine.cuEKF(x0, SampleLength=0.02, EnableEKF=True, couple_velocity=couple)
    f.load(None, P)
    return f, x0


def test_swaps_case_leaves_the_diagonal_in_the_claimed_columns():
    P = cw.filter_case("swaps")
    assert np.array_equal(P, P.T) and np.linalg.eigvalsh(P).min() > 0.0                  # a covariance: symmetric, positive definite
    rows, vals, sing, _ = cw.lu_pivots(P + np.eye(8))
    sw = [c for c, p in enumerate(rows) if p != c]
    assert sing is None and len(sw) >= 4 and 0 in sw and 6 in sw, rows
    assert any(rows[c] == 7 for c in sw if c < 6) and any(rows[c] == c + 1 for c in sw if c < 6), rows
    assert P[0, 0] < 0.1 * np.abs(P[1:, 0]).max()                                         # small leading diagonal, large coupling


def test_tie_case_keeps_the_first_of_two_equal_magnitudes():
    P = cw.filter_case("tie")
    Smat = P + np.eye(8)
    col = Smat[:, 0]
    order = np.argsort(-np.abs(col), kind="stable")
    assert list(order[:2]) == [2, 5] and abs(col[2]) == abs(col[5]) and col[2] == -col[5] and abs(col[order[2]]) < abs(col[2])
    rows, vals, sing, _ = cw.lu_pivots(Smat)
    assert sing is None and rows[0] == 2 and vals[0] == col[2]


def test_negative_case_has_negative_pivots_chosen_by_magnitude():
    P = cw.filter_case("negative")
    assert np.array_equal(P, P.T)
    ev = np.linalg.eigvalsh(P + np.eye(8))
    assert ev.min() < 0.0 < ev.max() and np.abs(ev).min() > 1e-2                          # indefinite, non-singular
    rows, vals, sing, cands = cw.lu_pivots(P + np.eye(8))
    assert sing is None and sum(v < 0.0 for v in vals) >= 3
    # a column whose pivot row is not the diagonal, whose pivot is NEGATIVE, and that had a positive candidate of smaller magnitude:
    # a search that compared the values instead of the magnitudes would have taken that one
    hit = [c for c in range(7) if rows[c] != c and vals[c] < 0.0 and (cands[c] > 0.0).any()]
    assert hit and all(cands[c].max() < -vals[c] for c in hit), (rows, vals)


@pytest.mark.parametrize("name,col", [("singular0", 0), ("singular5", 5)])
def test_singular_cases_stop_at_the_claimed_column(name, col):
    P = cw.filter_case(name)
    rows, vals, sing, cands = cw.lu_pivots(P + np.eye(8))
    assert sing == col and rows == list(range(col)) and (cands[col] == 0.0).all()          # clean eliminations, then a zero column
    for couple in (True, False):
        f, x0 = _host_filter(P, couple)
        before = f.state()
        with pytest.raises(dpe.DpeError, match="S inversion failed"):
            f.step_update(x0 + 0.5, np.eye(8))
        after = f.state()
        assert all(before[k].tobytes() == after[k].tobytes() for k in cw.EKF_KEYS)
        f.load(None, cw.filter_case("fresh"))                                              # ... and a fresh load is accepted
        f.Update(x0 + 0.5)
        assert all(np.isfinite(v).all() for v in f.state().values())
        f.Stop()


@pytest.mark.parametrize("name", ["swaps", "tie", "negative", "fresh"])
def test_host_filter_accepts_the_regular_cases(name):
    P = cw.filter_case(name)
    for couple in (True, False):
        f, x0 = _host_filter(P, couple)
        assert f.state()["Pkk1"].tobytes() == P.tobytes()
        f.Update(x0 + np.linspace(-1.0, 1.0, 8))
        st = f.state()
        assert all(np.isfinite(v).all() for v in st.values())
        # the inverse the filter took is the inverse: K = P S^-1 (H = I), so K S = P to rounding
        assert np.abs(st["K"] @ (P + np.eye(8)) - P).max() < 1e-9 * max(1.0, np.abs(st["K"]).max()) * np.abs(P).max()
        f.Stop()


def test_filter_accessors_are_declared_exported_and_wrapped():
    """dpe_chm_dev_ekf_state / dpe_chm_dev_ekf_load / dpe_ekf_load: additive, the ABI version stays 4."""
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dpe_hip.h")).read()
    for n in ("dpe_chm_dev_ekf_state", "dpe_chm_dev_ekf_load", "dpe_ekf_load"):
        assert re.search(r"\bint %s\(" % n, hdr) and n in dpe.engine.EXPORTS
    assert callable(dpe.engine.ChanMgrDev.ekf_state) and callable(dpe.engine.ChanMgrDev.ekf_load) and callable(dpe.engine.cuEKF.load)
    lib = dpe.engine.lib()
    assert lib.dpe_abi_version() == 4
    with pytest.raises(dpe.DpeError, match="ekf_load: no filter"):
        dpe.engine._check(lib.dpe_chm_dev_ekf_load(None, None, None, None))
    with pytest.raises(dpe.DpeError, match="ekf_state: no filter"):
        dpe.engine._check(lib.dpe_chm_dev_ekf_state(None, None, None, None, None, None, None, None))
    with pytest.raises(dpe.DpeError, match="load: null handle"):
        dpe.engine._check(lib.dpe_ekf_load(None, None, None))
