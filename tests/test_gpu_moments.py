"""Manifold moments on the device (dpe_bcm_moments, csrc/dpe_bcm_moments.h) against the numpy restatement (tests/moments_ref.py)
on the rows and keys read back from the device -- those come from the unchanged scan, not from the new code -- and the fp32
grid the device holds (the float32 rounding of the host grid, which is what create uploads).

Tolerance of the sums: |S_gpu - S_ref| <= 1e-9 * sum_i |term_i| per sum, i.e. N * 2^-53 for N <= 2^22 points rounded up, the
bound of ANY fp64 summation order (the reference is the correctly rounded sum).  nAbove and the threshold are exact; zValMom and
RValMom equal dpe_bcm_moments_from_sums of the device's own sums to 1e-12 relative.
Against the handle's weightedSums (pair-packed fp32 partial sums) the bound is 1e-5 of sum_i |term_i|: the scale a sum's
rounding error has, whatever cancels in the sum itself."""
import ctypes as C

import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import helpers
from tests import moments_ref as mr

pytestmark = pytest.mark.gpu

FS, S, K, AMP = 2.5e6, 5000, 4, 200.0


def _half_widths(case):
    return dpe.pipeline.bank_half_widths(case["pos"], case["vel"], case["fs"], case["C"])


def _banks(case, L, B):
    import torch
    iq, cs, ce, bw = helpers.pack_gpu_inputs(case)
    W, Kc = cs.shape
    bcs = dpe.BatchCorrScores(case["fs"], samples_per_window=case["S"], lag_half_width=L, bin_half_width=B, max_windows=W, max_channels=Kc)
    bcs.Start()
    bcs.Update(torch.from_numpy(iq).to("cuda:0"), cs)
    return bcs, bw, ce


def _manifold(case, bcs, pos, vel, L, B, max_windows, cls=dpe.BatchCorrManifold, **kw):
    m = cls(case["fs"], case["S"], bcs.NumFFTPoints, pos, vel, lag_half_width=L, bin_half_width=B, max_windows=max_windows,
            max_channels=case["K"], **kw)
    m.Start()
    return m


def _keys(m, W):
    return np.array(dpe.engine.d2h(m.Keys, 16 * W, np.uint64)).reshape(W, 2)


def _grid32(g):
    return (g.points() if hasattr(g, "points") else np.asarray(g)).astype(np.float32)


_REFS = {}


def _ref(row, grid, smax, rho):
    """moments_ref.moments, computed once per (row, grid, maximum, rho) and shared by the tests that ask again (the injected
    rows serve both manifolds of two handles).  The arrays are kept with the result, so a key names one live array."""
    key = (row.ctypes.data, row.size, grid.ctypes.data, np.float32(smax).tobytes(), float(rho))
    if key not in _REFS:
        _REFS[key] = (mr.moments(row, grid, smax, rho), row, grid)
    return _REFS[key][0]


def check_against_ref(got, rows, keys, grids, rho, frames):
    """got: BatchCorrManifold.moments' list; rows = (pos [W, G], vel [W, G]); keys [W, 2]; grids = (pos, vel) float32 [G, 4];
    frames: BCM_WINDOW_DTYPE [W].  Returns the references, [W][2]."""
    refs = []
    for w, g in enumerate(got):
        refs.append([_ref(rows[m][w], grids[m], mr.smax_of_key(keys[w, m]), rho[m]) for m in range(2)])
        for m, r in enumerate(refs[w]):
            err, bound = np.abs(g["sums"][m] - r["sums"]), 1e-9 * r["abs_sums"]
            assert (err <= bound).all(), (w, m, list(zip(mr.NAMES, err, bound)))
            assert g["nAbove"][m] == r["nAbove"], (w, m, g["nAbove"][m], r["nAbove"])
            assert g["threshold"][m] == r["tau"] or (np.isnan(g["threshold"][m]) and np.isnan(r["tau"])), (w, m)
        if w >= len(frames):      # overridden rows beyond the last Update's windows: sums, but no frame
            assert np.isnan(g["zValMom"]).all() and np.isnan(g["RValMom"]).all()
            continue
        z, R = dpe.engine.moments_from_sums(g["sums"], frames["xCurrkk1"][w], frames["enu2ecef"][w])
        assert np.allclose(g["zValMom"], z, rtol=1e-12, atol=0, equal_nan=True) and np.allclose(g["RValMom"], R, rtol=1e-12, atol=0, equal_nan=True)
        assert np.array_equal(g["RValMom"], g["RValMom"].T, equal_nan=True)
    return refs


# ---- case 1: random point lists, ragged last tile, pitch pad, unequal manifolds, three maxima --------------------------------
@pytest.fixture(scope="module")
def list_case():
    case = helpers.make_case(seed=5, fs=FS, S=S, K=K, G=4096 + 37, vel_G=1000, amp=AMP, W=3)
    L, B = _half_widths(case)
    bcs, bw, ce = _banks(case, L, B)
    m = _manifold(case, bcs, case["pos"], case["vel"], L, B, 3, weighted_mean=True)
    m.Update(bcs.CodeScores, bcs.CarrScores, bw, ce)
    res = m.results()
    out = dict(case=case, m=m, bw=bw, res=res, rows=m.read_scores(), keys=_keys(m, 3), grids=(_grid32(case["pos"]), _grid32(case["vel"])))
    yield out
    m.Stop(); bcs.Stop()


@pytest.mark.parametrize("rho", [(0.0, 0.0), (0.5, 0.9), (0.999, 0.999)])
def test_random_point_lists(list_case, rho):
    c = list_case
    assert c["m"].PosScoresPitch > 4133 and c["m"].VelScoresPitch > 1000     # a pad behind every row
    assert len({int(k) >> 32 for k in c["keys"][:, 0]}) == 3                # three different maxima
    got = c["m"].moments(rho)
    refs = check_against_ref(got, c["rows"], c["keys"], c["grids"], rho, c["bw"])
    for w in range(3):
        assert got[w]["nAbove"].min() >= 1 and np.isfinite(got[w]["RValMom"]).all()
        if rho == (0.0, 0.0):      # raw-score weights: the first five sums are the weighted-mean estimator's
            ws = c["res"][w]["weightedSums"]
            for m in range(2):
                assert (np.abs(got[w]["sums"][m][:5] - ws[m]) <= 1e-5 * refs[w][m]["abs_sums"][:5]).all(), (w, m)
    # the device copies are the mirror's numbers
    sp, ap = c["m"].moments_dev()
    sums = dpe.engine.d2h(sp, 3 * 2 * 15 * 8, np.float64).reshape(3, 2, 15)
    above = dpe.engine.d2h(ap, 3 * 2 * 8, np.int64).reshape(3, 2)
    assert all(np.array_equal(sums[w], got[w]["sums"]) and np.array_equal(above[w], got[w]["nAbove"]) for w in range(3))


# ---- case 2: a single point; under one wave and a bit ------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 33])
def test_tiny_grids(G):
    case = helpers.make_case(seed=6, fs=FS, S=S, K=K, G=G, amp=AMP, W=1)
    L, B = _half_widths(case)
    bcs, bw, ce = _banks(case, L, B)
    m = _manifold(case, bcs, case["pos"], case["vel"], L, B, 1)
    m.Update(bcs.CodeScores, bcs.CarrScores, bw, ce)
    rows, keys, grids = m.read_scores(), _keys(m, 1), (_grid32(case["pos"]), _grid32(case["vel"]))
    for rho in ((0.0, 0.0), (0.5, 0.5)):
        got = m.moments(rho)
        check_against_ref(got, rows, keys, grids, rho, bw)
        if G == 1 and rho == (0.0, 0.0):
            assert list(got[0]["nAbove"]) == [1, 1]
            assert not got[0]["RValMom"].any()                   # one point: the covariance is exactly 0
            z = dpe.engine.moments_from_sums(got[0]["sums"], bw["xCurrkk1"][0], bw["enu2ecef"][0])[0]
            # the mean is the point itself: zVal but for the fp32 rounding of the offsets (3 x 2^-24 x at most 50 m)
            assert np.abs(got[0]["zValMom"] - m.results()[0]["zVal"]).max() < 1e-5 and np.array_equal(z, got[0]["zValMom"])
    m.Stop(); bcs.Stop()


# ---- case 3: every score 0 ------------------------------------------------------------------------------------------------
def test_all_scores_zero():
    case = helpers.make_case(seed=7, fs=FS, S=S, K=K, G=300, vel_G=200, amp=AMP, W=2, center_offset=(2000.0, 0.0, 0.0, 0.0))
    for w in case["wins"]:       # the velocity manifold too: a clock drift far outside a bank of half width 1
        w["centre"] = w["centre"].copy()
        w["centre"][7] += 5000.0
    bcs, bw, ce = _banks(case, 1, 1)
    m = _manifold(case, bcs, case["pos"], case["vel"], 1, 1, 2)
    m.Update(bcs.CodeScores, bcs.CarrScores, bw, ce)
    rows, keys = m.read_scores(), _keys(m, 2)
    assert not rows[0].any() and not rows[1].any() and not (keys >> np.uint64(32)).any()      # smax = 0
    for rho in ((0.0, 0.0), (0.5, 0.9)):
        for g in m.moments(rho):                                                               # no error
            assert not g["sums"].any() and not g["nAbove"].any() and not g["threshold"].any()
            assert np.isnan(g["zValMom"]).all() and np.isnan(g["RValMom"][:4, :4]).all() and np.isnan(g["RValMom"][4:, 4:]).all()
    m.Stop(); bcs.Stop()


# ---- case 4: axes handle, slices that cut rows, the full handle's keys ---------------------------------------------------------
def test_axes_handle_and_slices():
    import torch
    pos_ax = dpe.GridAxes.uniform((5, 4, 3, 7), (3.0, 3.0, 3.0, 2.0))
    vel_ax = dpe.GridAxes.uniform((5, 4, 3, 7), 0.5)
    case = helpers.make_case(seed=8, fs=FS, S=S, K=K, G=64, amp=AMP, W=2)
    case["pos"], case["vel"] = pos_ax.points(), vel_ax.points()
    L, B = _half_widths(case)
    bcs, bw, ce = _banks(case, L, B)
    rho = (0.3, 0.6)
    full = _manifold(case, bcs, pos_ax, vel_ax, L, B, 2)
    full.Update(bcs.CodeScores, bcs.CarrScores, bw, ce)
    keys = _keys(full, 2)
    whole = full.moments(rho)
    check_against_ref(whole, full.read_scores(), keys, (_grid32(pos_ax), _grid32(vel_ax)), rho, bw)
    keys_d = torch.from_numpy(keys.view(np.int64)).to("cuda:0")
    total, bound = np.zeros((2, 2, 15)), np.zeros((2, 2, 15))
    above = np.zeros((2, 2), dtype=np.int64)
    for b, e in ((0, 11), (11, 11 + 300), (311, 420)):      # 11 is no multiple of dimT = 7: the slices begin and end inside rows
        pa, va = pos_ax.shard(b, e), vel_ax.shard(b, e)
        part = _manifold(case, bcs, pa, va, L, B, 2)
        part.Update(bcs.CodeScores, bcs.CarrScores, bw, ce)
        got = part.moments(rho, keys=keys_d)          # the shard's own maxima are not the rows' maxima: one threshold for all
        refs = check_against_ref(got, part.read_scores(), keys, (_grid32(pa), _grid32(va)), rho, bw)
        for w in range(2):
            total[w] += got[w]["sums"]
            above[w] += got[w]["nAbove"]
            bound[w] += [1e-9 * r["abs_sums"] for r in refs[w]]
            assert np.array_equal(got[w]["threshold"], whole[w]["threshold"])
        part.Stop()
    for w in range(2):
        assert (np.abs(total[w] - whole[w]["sums"]) <= 2 * bound[w]).all() and np.array_equal(above[w], whole[w]["nAbove"])
    full.Stop(); bcs.Stop()


# ---- case 5: the call between Updates changes nothing; it reads the latest key set; repeated calls carry the same bits --------
def test_between_updates_and_repeatability(list_case):
    case = list_case["case"]
    L, B = _half_widths(case)
    bcs, bw, ce = _banks(case, L, B)
    rho = (0.5, 0.9)
    snap = []
    for with_moments in (False, True):
        m = _manifold(case, bcs, case["pos"], case["vel"], L, B, 1)
        code, carr = dpe.engine.bank_rows(bcs, 0)
        m.Update(code, carr, bw[0:1], ce[0:1])
        if with_moments:
            first = m.moments(rho)
        code, carr = dpe.engine.bank_rows(bcs, 1)
        m.Update(code, carr, bw[1:2], ce[1:2])
        if with_moments:
            a, b = m.moments(rho), m.moments(rho)
            for k in a[0]:
                assert np.array_equal(a[0][k], b[0][k], equal_nan=True), k                    # identical bits
            assert not np.array_equal(a[0]["sums"], first[0]["sums"])
        res, keys, rows = m.results()[0], _keys(m, 1), m.read_scores()
        if with_moments:      # the latest key set and rows: window 1's
            check_against_ref(a, rows, keys, list_case["grids"], rho, bw[1:2])
            assert np.array_equal(keys[0], list_case["keys"][1])
        snap.append((res, keys, rows))
        m.Stop()
    (r0, k0, s0), (r1, k1, s1) = snap
    assert np.array_equal(k0, k1) and np.array_equal(s0[0], s1[0]) and np.array_equal(s0[1], s1[1])
    assert r0.keys() == r1.keys() and all(np.array_equal(r0[k], r1[k]) for k in r0)
    bcs.Stop()


# ---- case 6: injected Gaussian rows, axes and point-list handles of one grid -------------------------------------------------
@pytest.fixture(scope="module")
def gaussian_rows():
    grid, iso, ax = mr.gaussian_case()
    _, cor, _ = mr.gaussian_case(mr.SIGMA_XY)
    hit = np.arange(100) * 1931 + 7
    bad, zeroed = cor.copy(), cor.copy()
    bad[hit], zeroed[hit] = np.nan, 0.0
    rows = np.stack([iso, cor, bad, zeroed])
    keys = np.zeros((4, 2), dtype=np.uint64)
    for w, r in enumerate(rows):       # a hand-made key per row: (bits of the maximum, ~index of its first occurrence)
        i = int(np.nanargmax(r))
        keys[w, :] = (int(np.array([r[i]], dtype=np.float32).view(np.uint32)[0]) << 32) | (0xFFFFFFFF - i)
    return grid, ax, rows, keys


@pytest.mark.parametrize("kind", ["axes", "points"])
def test_injected_gaussian_rows(gaussian_rows, kind):
    import torch
    grid, ax, rows, keys = gaussian_rows
    G = rows.shape[1]
    assert G == 21 ** 4 and G % 32 != 0
    pitch = (G + 31) // 32 * 32
    padded = np.full((4, pitch), np.inf, dtype=np.float32)      # a pad float that is read shows in every sum
    padded[:, :G] = rows
    rows_d, keys_d = torch.from_numpy(padded).to("cuda:0"), torch.from_numpy(keys.view(np.int64)).to("cuda:0")
    case = helpers.make_case(seed=9, fs=FS, S=S, K=K, G=64, amp=AMP, W=2)
    axes4 = dpe.GridAxes(ax, ax, ax, ax)
    case["pos"], case["vel"] = axes4.points(), axes4.points()
    assert np.array_equal(case["pos"].astype(np.float32), grid)
    L, B = _half_widths(case)
    bcs, bw, ce = _banks(case, L, B)
    g = axes4 if kind == "axes" else case["pos"]
    m = _manifold(case, bcs, g, g, L, B, 4)
    m.Update(bcs.CodeScores, bcs.CarrScores, bw, ce)         # two windows' frames; their rows and keys are not used below
    frames = bw
    for rho in ((0.0, 0.0), (0.5, 0.25)):
        got = m.moments(rho, keys=keys_d, pos_scores=rows_d, vel_scores=rows_d, n_windows=4)      # 24 blocks per row: waves walk units
        check_against_ref(got, (rows, rows), keys, (grid, grid), rho, frames)
        for k in got[2]:               # NaN over 100 points = those points set to 0
            assert np.array_equal(got[2][k], got[3][k], equal_nan=True), k      # (windows 2 and 3 have no frame: NaN fixes)
        if rho == (0.0, 0.0):
            for w, sigma in ((0, np.eye(4)), (1, mr.SIGMA_XY)):
                J = np.eye(4)
                J[:3, :3] = bw["enu2ecef"][w].reshape(3, 3)
                C0 = J.T @ got[w]["RValMom"][:4, :4] @ J          # back to the grid's frame
                assert np.abs(C0 - sigma).max() < 1e-4, (w, np.abs(C0 - sigma).max())
        one = m.moments(rho, keys=keys_d, pos_scores=rows_d, vel_scores=rows_d, n_windows=1)      # 128 blocks per row
        check_against_ref(one, (rows, rows), keys, (grid, grid), rho, frames)
    # rows that start on no 16-byte boundary (pitch = G, odd): the scalar loads give the same bits
    tight = torch.from_numpy(np.ascontiguousarray(rows)).to("cuda:0")
    a = m.moments((0.5, 0.25), keys=keys_d, pos_scores=tight, vel_scores=(tight.data_ptr(), G), n_windows=4)
    assert all(np.array_equal(a[w]["sums"], got[w]["sums"]) and np.array_equal(a[w]["nAbove"], got[w]["nAbove"]) for w in range(4))
    m.Stop(); bcs.Stop()


# ---- case 7: refusals with a device ----------------------------------------------------------------------------------------
def test_refusals(list_case):
    import torch
    case, m = list_case["case"], list_case["m"]
    L, B = _half_widths(case)
    bcs, bw, ce = _banks(case, L, B)
    fresh = _manifold(case, bcs, case["pos"], case["vel"], L, B, 3)
    with pytest.raises(dpe.DpeError, match="moments: no update yet"):
        fresh.moments(0.5)
    fresh.Stop()
    blind = _manifold(case, bcs, case["pos"], case["vel"], L, B, 3, write_scores=False)
    blind.Update(bcs.CodeScores, bcs.CarrScores, bw, ce)
    with pytest.raises(dpe.DpeError, match="moments: created with writeScores=0"):
        blind.moments(0.5)
    rows = torch.zeros((3, 4160), dtype=torch.float32, device="cuda:0")
    with pytest.raises(dpe.DpeError, match="moments: created with writeScores=0"):
        blind.moments(0.5, pos_scores=rows)               # one manifold's rows are not enough
    blind.Stop()
    with pytest.raises(dpe.DpeError, match="moments: nWindows 4 out of range"):
        m.moments(0.5, n_windows=4)
    with pytest.raises(dpe.DpeError, match="moments: nWindows 4 out of range"):
        m.moments(0.5, keys=m.Keys, pos_scores=rows, vel_scores=rows, n_windows=4)      # beyond maxWindows with everything overridden
    with pytest.raises(dpe.DpeError, match="moments: posPitch 4132 is below the position grid size 4133"):
        m.moments(0.5, pos_scores=(rows.data_ptr(), 4132))
    with pytest.raises(dpe.DpeError, match="moments: velPitch 999 is below the velocity grid size 1000"):
        m.moments(0.5, vel_scores=(rows.data_ptr(), 999))
    with pytest.raises(dpe.DpeError, match=r"moments: rho\[1\] = 1 outside \[0, 1\)"):
        m.moments((0.5, 1.0))
    assert len(m.moments(0.5, n_windows=2)) == 2            # fewer windows than the last Update's are fine
    kinds = [(dpe.JointManifold, (2, 8), "joint"), (dpe.EpochManifold, (2,), "epochs"), (dpe.SubsetManifold, (4,), "subsets")]
    for cls, extra, word in kinds:
        h = cls(case["fs"], case["S"], bcs.NumFFTPoints, case["pos"], case["vel"], *extra, lag_half_width=L, bin_half_width=B, max_channels=case["K"])
        h.Start()
        with pytest.raises(dpe.DpeError, match="moments: an? %s handle" % word):
            h.moments(0.5)
        h.Stop()
    ax = dpe.GridAxes.uniform(3, 1.0)
    h = dpe.RefineManifold(case["fs"], case["S"], bcs.NumFFTPoints, [(ax, ax)], lag_half_width=L, bin_half_width=B, max_channels=case["K"])
    h.Start()
    cfg = dpe.engine.BcmMomentsConfig((C.c_double * 2)(0.5, 0.5), None, None, None, 0, 0, 0, 0)
    assert dpe.engine.lib().dpe_bcm_moments(h._h, C.byref(cfg), None) != 0
    assert "moments: a refine handle" in dpe.engine.lib().dpe_last_error().decode()
    h.Stop(); bcs.Stop()


# ---- case 8: the closed loop with the moments as the filter's measurement covariance -----------------------------------------
def test_closed_loop_measurement_cov():
    W = 4
    iq, _, _, _ = dpe.workload.build_windows(W, FS, S, K, seed=12, amp=AMP)
    ho = dpe.handoff.read_handoff(dpe.workload.HANDOFF_CSV)
    pos, vel = dpe.synth.uniform_grid(7, 20.0), dpe.synth.uniform_grid(7, 2.0)
    tg = np.unique(pos[:, 3])
    fixes, res = dpe.pipeline.run_closed_loop(iq, ho, FS, pos, vel, time_grid=tg, K=K, enable_ekf=True, measurement_cov=(0.99, 0.99))
    floor = min(20.0 ** 2 / 12, 2.0 ** 2 / 12)
    assert np.array_equal(dpe.pipeline.quantisation_floor(pos), np.full(4, 20.0 ** 2 / 12))
    x0 = np.array(ho["X_ECEF"], dtype=np.float64)
    ekf = dpe.engine.cuEKF(x0, SampleLength=S / FS, EnableEKF=True)
    for w, r in enumerate(res):
        R = r["RVal"]
        assert R.shape == (8, 8) and np.array_equal(R, R.T) and np.isfinite(R).all()
        assert np.linalg.eigvalsh(R).min() >= floor - 1e-9 * np.trace(R), (w, np.linalg.eigvalsh(R).min())
        assert r["moments"]["nAbove"].min() >= 1 and set(r["moments"]) == {"sums", "nAbove", "threshold", "zValMom", "RValMom"}
        ekf.Update(r["zVal"], R)               # the measurement stays the arg-max zVal
        assert np.abs(ekf.xCurrk1k1 - fixes[w]).max() < 1e-9, w
    ekf.Stop()
    plain, res0 = dpe.pipeline.run_closed_loop(iq, ho, FS, pos, vel, time_grid=tg, K=K, enable_ekf=True)
    none, res1 = dpe.pipeline.run_closed_loop(iq, ho, FS, pos, vel, time_grid=tg, K=K, enable_ekf=True, measurement_cov=None)
    assert np.array_equal(plain, none) and all("moments" not in r and np.array_equal(r["RVal"], np.eye(8)) for r in res1)
