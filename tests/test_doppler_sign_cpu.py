"""CPU: DopplerSign = -1 -- the inputs the GPU tests of tests/test_gpu_doppler_sign.py run on, proven with the oracle, tests/vt_ref.py
and the library's host code alone.

A sign error cannot hide inside a tolerance: the facts below say that the -1 inputs are self-consistent (every fi the +1 run's negated,
every fc the +1 run's), that the oracle peaks where the world puts the peak, and that the SAME -1 record scanned or tracked with the
sign left at +1 ends somewhere else by far more than any bound of the suite.  (The channel manager at -1 against the oracle:
tests/test_abi_cpu.py, parametrised over the sign.)"""
import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import helpers, mirror, vt_ref, vt_world
from tests.test_nav_cpu import fix_row, o15_navigator

SEED, S, K, W, G = 3, 5000, 8, 3, 1025      # 1025 points: two tiles of the scan, the second ragged; windows 2 and 3 come out of propagate
WIDE = (8, 24)                              # every (point, SV) pair inside the banks
NARROW = (1, 1)                             # both manifolds reach beyond the banks: the clamped scan variants
VT_SHAPE = dict(K=6, T=1e-3, N=20, n_epochs=8)


def sign_case(ds):
    """The scan case of both files: the handoff geometry at 2.5 Msps, 2 ms windows, random grids whose point 0 is the centre."""
    case = helpers.make_case(seed=SEED, ds=ds, S=S, K=K, W=W, G=G, vel_G=G, grid="rand")
    case["pos"][0] = 0.0
    case["vel"][0] = 0.0
    return case


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return dpe.engine.lib()


@pytest.fixture(scope="module")
def minus(oracle):
    case = sign_case(-1)
    return case, helpers.run_oracle(case, *WIDE), helpers.run_oracle(case, *NARROW)


def test_fi_is_negated_and_fc_is_equal_exactly(oracle, minus):
    """propagate divides the Doppler by the sign and multiplies the code aiding by it: fi flips, fc does not -- to the last bit, in
    the handoff's window and in the two that come out of propagate."""
    plus = sign_case(1)
    for wm, wp in zip(minus[0]["wins"], plus["wins"]):
        assert np.array_equal(wm["fi"], -wp["fi"]) and np.array_equal(wm["start"]["fi"], -wp["start"]["fi"])
        assert np.array_equal(wm["fc"], wp["fc"]) and np.array_equal(wm["start"]["fc"], wp["start"]["fc"])
        assert np.array_equal(wm["rcEnd"], wp["rcEnd"]) and np.array_equal(wm["cpElaEnd"], wp["cpElaEnd"])
        assert np.sum(np.abs(wm["fi"]) > 500.0) >= 6        # Dopplers whose sign matters: 13 bins of the velocity bank and more
    assert minus[0]["ds"] == -1 and plus["ds"] == 1
    bw = helpers.pack_gpu_inputs(minus[0])[3]
    assert np.all(bw["dopplerSign"] == -1) and np.all(helpers.pack_gpu_inputs(plus)[3]["dopplerSign"] == 1)


def test_oracle_peaks_on_the_centre_with_every_pair_inside(minus):
    _, wide, _ = minus
    for r in wide["res"]:
        assert r["posIndex"] == 0 and r["velIndex"] == 0
        assert r["posOutOfWindow"] == 0 and r["posOutOfWindowX"] == 0 and r["velOutOfWindow"] == 0


def test_narrow_banks_run_the_clamped_variants_within_the_parity_caps(minus):
    """L = B = 1: some pairs of both manifolds fall outside the banks, not all.  What helpers.assert_parity sets aside at truncated
    banks is capped there; the caps hold on the oracle's own two evaluations of this case."""
    case, _, narrow = minus
    for w, r in enumerate(narrow["res"]):
        assert 0 < r["velOutOfWindow"] < K * G and 0 < r["posOutOfWindowX"] < K * G
        assert r["posIndex"] == 0 and r["velIndex"] == 0
        p, px = narrow["pos"][w], narrow["pos_x"][w]
        keep = np.ones(p.size, dtype=bool)
        keep[narrow["pos_quirk"][w]] = False
        flips = np.abs(p - px) > 10 * helpers.POS_REF_NOISE * p.max()
        assert (flips & keep).sum() <= 16 + p.size * K // 2000
        assert abs(r["posOutOfWindow"] - r["posOutOfWindowX"]) <= 8 + p.size * K // 2000


def test_the_wrong_sign_shows_in_the_scan(minus):
    """The -1 banks scanned with doppler_sign = +1: the velocity manifold's index runs the other way about a centre 2 fi off."""
    case, wide, _ = minus
    wrong = helpers.run_oracle(dict(case, ds=1), *WIDE)
    for w in range(W):
        assert np.array_equal(wrong["pos"][w], wide["pos"][w])                    # (the position manifold does not take the sign)
        assert wrong["res"][w]["velOutOfWindow"] > 0 and wrong["res"][w]["velIndex"] != 0
        d = np.abs(wrong["vel"][w] - wide["vel"][w]).max() / wide["vel"][w].max()
        assert d > 0.5, d                                                        # against bounds of 2e-5 and below


def vt_minus(oracle, ds_loop, round_epl=None):
    """The vector tracker's short world at ds = -1 (tests/test_gpu_doppler_sign.py runs the same), tracked by vt_ref at ds_loop."""
    s = VT_SHAPE
    n = s["n_epochs"] * s["N"] * int(round(s["T"] * vt_world.FS))
    w = vt_world.build(oracle, n, chans=vt_world.CHANS[:s["K"]], ds=-1.0)
    iq = vt_world.record(w)
    cfg = vt_ref.Config(vt_world.FS, w["start"]["prns"], T=s["T"], N=s["N"], ds=ds_loop, num_prev=4)
    X0 = vt_world.perturbed(w)
    out = vt_ref.run(iq, cfg, oracle, w["start"], X0, vt_world.sigma0(), s["n_epochs"], round_epl=round_epl)
    return w, iq, cfg, X0, out


def test_vt_world_at_minus_one_is_the_plus_world_with_fi_negated(oracle):
    n = 2 * 20 * 2500
    a, b = vt_world.build(oracle, n, ds=-1.0), vt_world.build(oracle, n)
    assert np.array_equal(a["ch"]["fi"], -np.asarray(b["ch"]["fi"])) and np.array_equal(a["start"]["chan"][:, 3], -b["start"]["chan"][:, 3])
    assert np.array_equal(a["start"]["chan"][:, [0, 1, 2, 4]], b["start"]["chan"][:, [0, 1, 2, 4]])
    assert np.array_equal(a["ch"]["fc"], b["ch"]["fc"])
    qa, qb = vt_world.record(a), vt_world.record(b)                               # record() rotates by ch["fi"]: another record
    assert qa.shape == qb.shape and np.abs(qa.astype(np.int64) - qb).max() > 100


def test_vt_ref_converges_at_the_right_sign_and_loses_channels_at_the_wrong_one(oracle, capsys):
    w, _, cfg, _, out = vt_minus(oracle, -1.0)
    t = vt_ref.table(out["recs"])
    err = np.linalg.norm(t["X"][:, :3] - w["start"]["X"][:3], axis=1)
    _, _, _, _, bad = vt_minus(oracle, 1.0)
    tb = vt_ref.table(bad["recs"])
    errb = np.linalg.norm(tb["X"][:, :3] - w["start"]["X"][:3], axis=1)
    with capsys.disabled():
        print("\nvt_ref on the ds = -1 world: position error by epoch (m) %s, masks %s" % (np.round(err, 1), list(t["mask"])))
        print("  the same record with the loop at ds = +1:          %s, masks %s" % (np.round(errb, 1), list(tb["mask"])))
    assert np.all(t["mask"] == (1 << cfg.K) - 1) and np.all(t["status"] == 0)
    assert err[-1] < err[0]
    assert np.any(tb["mask"] != (1 << cfg.K) - 1)


def test_mirror_helpers():
    iq = np.array([[1, 2, -3, 4], [5, -6, 7, 32767]], dtype=np.int16)
    m = mirror.mirror_iq(iq)
    assert m.dtype == np.int16 and np.array_equal(m, [[1, -2, -3, -4], [5, 6, 7, -32767]]) and np.array_equal(mirror.mirror_iq(m), iq)
    assert np.array_equal(iq, [[1, 2, -3, 4], [5, -6, 7, 32767]])                 # the input is left alone
    with pytest.raises(AssertionError):
        mirror.mirror_iq(np.array([0, -32768], dtype=np.int16))
    ho = dpe.handoff.read_handoff(helpers.HANDOFF)
    mh = mirror.mirror_handoff(ho)
    assert np.array_equal(mh["fi"], -ho["fi"]) and np.all((mh["ri"] >= 0) & (mh["ri"] < 1))
    d = np.abs(mh["ri"] + ho["ri"] - np.round(mh["ri"] + ho["ri"]))
    assert d.max() < 1e-15 and set(mh) == set(ho)
    assert all(mh[k] is ho[k] for k in ho if k not in ("fi", "ri"))
    back = mirror.mirror_handoff(mh)
    assert np.array_equal(back["fi"], ho["fi"]) and np.abs(back["ri"] - ho["ri"]).max() < 1e-15
    log = dict(cp=np.arange(6).reshape(3, 2), rc=np.ones((3, 2)), fi=np.array([[1.0, -2.0]] * 3))
    ml = mirror.mirror_log(log)
    assert np.array_equal(ml["fi"], -log["fi"]) and ml["cp"] is log["cp"] and ml["rc"] is log["rc"]


def test_a_mirrored_window_is_the_window_of_the_mirrored_parameters():
    """synth.gen_iq without noise and DC on channel parameters and on their mirror image: Q negated (to the rounding of the last
    int16 step, where the two phases round differently)."""
    ch = dpe.synth.random_channels(11, 4)
    ch["cp_ref"] = ch["cp"].copy()
    mh = mirror.mirror_handoff(dict(fi=ch["fi"], ri=ch["ri"]))
    chm = dict(ch, fi=mh["fi"], ri=mh["ri"])
    kw = dict(amp=2000.0, sigma=0.0, dc=(0.0, 0.0), flip=np.zeros(4, dtype=bool))
    a, b = dpe.synth.gen_iq(1, 2.5e6, 5000, ch, **kw), dpe.synth.gen_iq(1, 2.5e6, 5000, chm, **kw)
    assert np.abs(a.astype(np.int64) - mirror.mirror_iq(b)).max() <= 1
    assert np.abs(a[1::2].astype(np.int64) - b[1::2]).max() > 1000              # ... and the mirror image is another record


def test_host_navigator_takes_the_sign_as_fi_times_ds_alone(built, golden):
    """ScalarNavigator(ds = -1).solve on O15's rows with fi negated: the bytes of the ds = +1 result on the rows as they are (the sign
    enters as fi * ds, and a product with +/-1 is exact)."""
    g = golden("o15_scalar_nav")
    plus = o15_navigator(g)
    neg = dpe.ScalarNavigator(g["sol_prn"], ds=-1.0)
    neg.set_ephemerides(g["sol_eph"], g["sol_tow"], g["sol_cp_timestamp"])
    M = g["sol_cp"].shape[0]
    for m in range(M):
        a = fix_row(plus.solve(g["sol_cp"][m], g["sol_rc"][m], g["sol_fi"][m]))
        b = fix_row(neg.solve(g["sol_cp"][m], g["sol_rc"][m], -g["sol_fi"][m]))
        assert a.tobytes() == b.tobytes(), m
    wrong = fix_row(neg.solve(g["sol_cp"][0], g["sol_rc"][0], g["sol_fi"][0]))    # ... and the sign is not ignored
    right = fix_row(plus.solve(g["sol_cp"][0], g["sol_rc"][0], g["sol_fi"][0]))
    assert np.abs(wrong[6:9] - right[6:9]).max() > 1.0
    assert neg.status() == 0
    plus.close(); neg.close()
