"""GPU: the coarse-to-fine scan (dpe_bcm_create_refine / engine.RefineManifold) against dpe_bcm_create_axes handles, against
one axes handle on the dense grid of equal resolution and reach, and in the closed loop against the numpy restatement of the
level chain (tests/refine_ref.py) driven by the GPU's own banks.  Inputs: tests/refine_world.py, proven on the CPU by
tests/test_refine_world_cpu.py.

Bounds.  Between GPU paths everything is bit equality: for every window, level and manifold the score row, the key and the
out-of-window count -- and at the last level offset and zVal -- are those of an axes handle (weightedMean 0) given that one
window and fp64 axes equal to the fp32 values np.float32(c) + a.astype(np.float32).  Against the dense grid the refined point
maps to the dense first maximum by integer arithmetic on (coarse index, fine index), and the score is within 2e-6 of the dense
score (the project's oracle tolerance: the centred point is rounded once more than the dense axis entry)."""
import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import epoch_world as ew
from tests import refine_ref as rr
from tests import refine_world as rw
from tests.test_gpu_epochs import TOL, key_index, same_bits
from tests.test_gpu_epochs_walk import Banks

pytestmark = pytest.mark.gpu


def run_refine(world, banks, lv, lpower=1, n_windows=None, n_chan=None, code=None, carr=None, handle=None, max_windows=None):
    """One Update of all windows of `banks` (or the first n_windows, the first n_chan channels); everything read back."""
    W = banks.W if n_windows is None else n_windows
    K = world["K"] if n_chan is None else n_chan
    h = handle or dpe.RefineManifold(world["fs"], world["S"], world["C"], lv, LPower=lpower, lag_half_width=world["L"], bin_half_width=world["B"],
                                     max_windows=banks.W if max_windows is None else max_windows, max_channels=banks.maxK)
    h.Start()
    try:
        h.Update(banks.bcs.CodeScores if code is None else code, banks.bcs.CarrScores if carr is None else carr, banks.bw[:W],
                 np.ascontiguousarray(banks.ce[:W, :K]))
        res = h.results()
        out = dict(res=res, split=h.last_split(), rows=[h.read_scores(l) for l in range(len(lv))],
                   keys=[h.read_keys(l) for l in range(len(lv))], all_keys=[h.read_keys(l, all_windows=True) for l in range(len(lv))])
    finally:
        if handle is None:
            h.Stop()
    return out


class AxesRef:
    """dpe_bcm_create_axes handles (the comparator) for single windows of a batch: the window's bank rows and records as they
    are, fp64 axes equal to the fp32 values the level scores."""

    def __init__(self, world, banks, lpower=1, code=None, carr=None, n_chan=None):
        self.world, self.banks, self.lpower = world, banks, lpower
        self.code = banks.bcs.CodeScores if code is None else code
        self.carr = banks.bcs.CarrScores if carr is None else carr
        self.K = world["K"] if n_chan is None else n_chan

    def run(self, w, pos_axes, vel_axes):
        world, b = self.world, self.banks
        pa, va = dpe.GridAxes(*[a.astype(np.float64) for a in pos_axes]), dpe.GridAxes(*[a.astype(np.float64) for a in vel_axes])
        h = dpe.BatchCorrManifold(world["fs"], world["S"], world["C"], pa, va, LPower=self.lpower, lag_half_width=world["L"],
                                  bin_half_width=world["B"], max_windows=1, max_channels=b.maxK)
        h.Start()
        try:
            code = self.code + w * b.maxK * (2 * world["L"] + 1) * 8
            carr = self.carr + w * b.maxK * (2 * world["B"] + 1) * 8
            h.Update(code, carr, b.bw[w:w + 1], np.ascontiguousarray(b.ce[w:w + 1, :self.K]))
            r = h.results()[0]
            ps, vs = h.read_scores()
            r["pos"], r["vel"] = ps[0], vs[0]
            r["keys"] = dpe.engine.d2h(h.Keys, 16, np.uint64).copy()
        finally:
            h.Stop()
        return r


def _ptr(x):
    return x.data_ptr() if hasattr(x, "data_ptr") else int(x)


def assert_chain_is_axes(world, banks, out, lv, lpower=1, windows=None, code=None, carr=None, n_chan=None, skip=()):
    """Every level of every window against its own axes handle: rows, keys, counts; at the last level offset and zVal.
    skip: (window, manifold) pairs without a score (their own checks are the caller's)."""
    ref = AxesRef(world, banks, lpower, None if code is None else _ptr(code), None if carr is None else _ptr(carr), n_chan)
    nL = len(lv)
    for w in (range(len(out["res"])) if windows is None else windows):
        r = out["res"][w]
        c = [np.zeros(4, dtype=np.float32), np.zeros(4, dtype=np.float32)]
        for l in range(nL):
            ax = [rr.scored_axes(c[m], lv[l][m].axes) for m in (0, 1)]
            want = ref.run(w, ax[0], ax[1])
            for m, name in ((0, "pos"), (1, "vel")):
                if (w, m) in skip:
                    continue
                where = (w, l, name, lpower)
                assert same_bits(out["rows"][l][m][w], want[name]), where
                assert int(out["keys"][l][w, m]) == int(want["keys"][m]), where
                assert r[name + "Index"][l] == want[name + "Index"] and r[name + "OutOfWindow"][l] == want[name + "OutOfWindow"], where
                assert np.float32(r[name + "Score"][l]).tobytes() == np.float32(want[name + "Score"]).tobytes(), where
                dims = [a.size for a in ax[m]]
                c[m] = np.array([a[j] for a, j in zip(ax[m], rr.decode(r[name + "Index"][l], dims))], dtype=np.float32)
                if l == nL - 1:
                    sl = slice(4 * m, 4 * m + 4)
                    assert r["offset"][sl].tobytes() == c[m].astype(np.float64).tobytes(), where
                    assert r["zVal"][sl].tobytes() == want["zVal"][sl].tobytes(), where


@pytest.fixture(scope="module")
def four():
    world = rw.build()
    banks = Banks(world)
    yield world, banks
    banks.close()


@pytest.fixture(scope="module")
def plain(four):
    """The 4-window batch through the levels 7^4 -> 13^4, LPower 1 (shared by several tests; never modified)."""
    world, banks = four
    return run_refine(world, banks, rw.levels(2))


@pytest.mark.parametrize("lpower", [1, 2, 3])
def test_levels_are_axes_handles_bit_for_bit(four, plain, lpower):
    """1.  4 distinct windows, 7^4 -> 13^4 (2 197 rows: 9 row groups, the last ragged; one 13-entry chunk)."""
    world, banks = four
    lv = rw.levels(2)
    out = plain if lpower == 1 else run_refine(world, banks, lv, lpower)
    assert out["rows"][1][0].shape == (4, 13 ** 4) and out["rows"][0][1].shape == (4, 7 ** 4)
    assert len({int(r["posIndex"][0]) for r in out["res"]}) > 1      # the windows peak on different coarse points
    assert_chain_is_axes(world, banks, out, lv, lpower)


def test_refined_point_is_the_dense_first_maximum(four, plain):
    """2.  The same batch against ONE axes handle on the dense 31^4 grid."""
    world, banks = four
    dp, dv = rw.dense(2)
    h = dpe.BatchCorrManifold(world["fs"], world["S"], world["C"], dp, dv, lag_half_width=world["L"], bin_half_width=world["B"],
                              max_windows=banks.W, max_channels=banks.maxK, write_scores=False)
    h.Start()
    try:
        h.Update(banks.bcs.CodeScores, banks.bcs.CarrScores, banks.bw, banks.ce)
        dense = h.results()
    finally:
        h.Stop()
    for w in range(banks.W):
        r = plain["res"][w]
        for name in ("pos", "vel"):
            assert dense[w][name + "OutOfWindow"] == 0 and r[name + "OutOfWindow"].sum() == 0
            assert rw.dense_index(r[name + "Index"][0], r[name + "Index"][1], 2) == dense[w][name + "Index"], (w, name)
            err = abs(float(r[name + "Score"][1]) - float(dense[w][name + "Score"])) / float(dense[w][name + "Score"])
            print("window %d %s: refined score vs dense score %.3g (bound %.3g)" % (w, name, err, TOL))
            assert err <= TOL, (w, name, err)


def three_levels():
    """5^4 -> 7.7.7.25 -> 3.3.3.17: the t chunks are 13 + 12 and 9 + 8; steps that are not fp32 numbers."""
    def ax(n, nt, step, tstep, shift):
        a = [step * (np.arange(n) - (n - 1) // 2) + s for s in shift[:3]]
        return dpe.GridAxes(*a, tstep * (np.arange(nt) - (nt - 1) // 2) + shift[3])
    return [(ax(5, 5, 60.1, 60.1, rw.SHIFT_POS), ax(5, 5, 18.1, 18.1, rw.SHIFT_VEL)),
            (ax(7, 25, 20.3, 5.1, (0.1, 0.2, 0.3, 0.7)), ax(7, 25, 6.1, 1.5, (0.01, 0.02, 0.03, 0.07))),
            (ax(3, 17, 6.7, 0.7, (0, 0, 0, 0)), ax(3, 17, 2.1, 0.2, (0, 0, 0, 0)))]


def test_three_levels_chain_through_fp32_centres(four):
    """3.  Bit equality along a three-level chain; level 2's centre is level 1's scored fp32 point."""
    world, banks = four
    lv = three_levels()
    out = run_refine(world, banks, lv)
    assert_chain_is_axes(world, banks, out, lv)      # (its comparators are built from the fp32 chain)
    differs = 0
    for w, r in enumerate(out["res"]):
        for m, name in ((0, "pos"), (1, "vel")):
            idx = r[name + "Index"]
            assert (idx >= 0).all()
            c32 = rr.point_of(rw.axes_of(lv, m), idx)
            assert r["offset"][4 * m:4 * m + 4].tobytes() == c32.astype(np.float64).tobytes(), (w, name)
            c64 = sum(np.array([a[j] for a, j in zip(l[m].axes, rr.decode(i, l[m].dim))]) for l, i in zip(lv, idx))
            differs += int((np.float32(c64) != c32).any())
    print("chains whose fp32 point is not the rounded fp64 sum of the axes: %d of 8" % differs)


def walk_levels():
    """7^4 -> 15.15.15.25: 3 375 rows are 14 row groups (the last ragged) x 2 t chunks (13 + 12) = 28 tiles; with 32 windows
    scan_split gives 24 blocks, so blocks 0 .. 3 walk two tiles, the second in the ragged group.  (15^4 would be 14 tiles, one
    per block: no walk.)"""
    step = ew.POS_STEP / rw.RATIO, ew.VEL_STEP / rw.RATIO
    fine = [dpe.GridAxes(*[s * (np.arange(n) - (n - 1) // 2) for n in (15, 15, 15, 25)]) for s in step]
    return [rw.coarse(), tuple(fine)]


def test_blocks_walk_several_tiles(four):
    """4.  32 windows (the 4 dealt round-robin); then the used handle again with 5 windows and 6 channels."""
    world, _ = four
    banks = Banks(world, windows=32)
    lv = walk_levels()
    h = dpe.RefineManifold(world["fs"], world["S"], world["C"], lv, lag_half_width=world["L"], bin_half_width=world["B"], max_windows=32,
                           max_channels=banks.maxK)
    try:
        out = run_refine(world, banks, lv, handle=h)
        tiles = -(-15 ** 3 // 256) * 2
        assert out["split"] == (24, 24) and tiles == 28 and out["split"][0] < tiles
        for w in range(4, 32):
            for l in (0, 1):
                assert same_bits(out["rows"][l][0][w], out["rows"][l][0][w % 4]) and same_bits(out["rows"][l][1][w], out["rows"][l][1][w % 4])
                assert np.array_equal(out["keys"][l][w], out["keys"][l][w % 4])
            assert out["res"][w]["offset"].tobytes() == out["res"][w % 4]["offset"].tobytes()
        assert_chain_is_axes(world, banks, out, lv, windows=range(4))
        # the used handle: fewer windows, fewer channels; twice, so that both alternating key sets are used after the large batch
        fresh = run_refine(world, banks, lv, n_windows=5, n_chan=6, max_windows=32)
        for _ in range(2):
            again = run_refine(world, banks, lv, n_windows=5, n_chan=6, handle=h)
            for l in (0, 1):
                assert np.array_equal(again["all_keys"][l], fresh["all_keys"][l])
                assert not again["all_keys"][l][5:].any()
                assert same_bits(again["rows"][l][0], fresh["rows"][l][0]) and same_bits(again["rows"][l][1], fresh["rows"][l][1])
            for a, b in zip(again["res"], fresh["res"]):
                assert a["zVal"].tobytes() == b["zVal"].tobytes() and np.array_equal(a["posOutOfWindow"], b["posOutOfWindow"])
    finally:
        h.Stop()
        banks.close()


@pytest.mark.parametrize("widen", [False, "L"])
def test_clamp_variants(widen):
    """5.  Narrow banks (L = 1, B = 2): counts and rows equal the comparator's; "L": only the lag banks narrow, velocity clean."""
    world = rw.build(widen)
    banks = Banks(world)
    try:
        lv = rw.levels(2)
        out = run_refine(world, banks, lv)
        assert all(r["posOutOfWindow"].min() > 0 for r in out["res"])
        assert all((r["velOutOfWindow"].min() > 0) == (widen is False) and (r["velOutOfWindow"].max() > 0) == (widen is False) for r in out["res"])
        assert_chain_is_axes(world, banks, out, lv)
    finally:
        banks.close()


def test_ties_keep_the_first_index(four, plain):
    """6.  Axes may repeat a value: the first index wins at every level and across chunks, row groups and blocks."""
    world, banks = four
    (cp, cv), (fp, fv) = rw.levels(2)
    # a. the maximal coarse x entry of window 0 duplicated right behind itself: index of the first copy, the same centre
    ix = rr.decode(plain["res"][0]["posIndex"][0], cp.dim)[0]
    x2 = np.insert(cp.axes[0], ix + 1, cp.axes[0][ix])
    out = run_refine(world, banks, [(dpe.GridAxes(x2, *cp.axes[1:]), cv), (fp, fv)], n_windows=1, max_windows=1)
    got = rr.decode(out["res"][0]["posIndex"][0], (8, 7, 7, 7))
    assert got == rr.decode(plain["res"][0]["posIndex"][0], cp.dim) and got[0] == ix
    assert same_bits(out["rows"][1][0][0], plain["rows"][1][0][0]) and out["res"][0]["offset"].tobytes() == plain["res"][0]["offset"].tobytes()
    # b. / c. the fine position grid 13.13.13.25 whose t entries 12 and 13 (the chunk boundary) both hold the peak's t, and whose
    # x entries j and j + 2 (338 rows apart: different row groups, different blocks) both hold the peak's x
    jx, _jy, _jz, jt = rr.decode(plain["res"][0]["posIndex"][1], fp.dim)
    t = fp.axes[3][jt] + ew.POS_STEP * (np.arange(25) - 12.5)       # far from the peak, except:
    t[12] = t[13] = fp.axes[3][jt]
    j0 = min(jx, 10)
    x = fp.axes[0].copy()
    x[j0] = x[j0 + 2] = fp.axes[0][jx]
    x[j0 + 1] = fp.axes[0][jx] + ew.POS_STEP
    tie = dpe.GridAxes(x, fp.axes[1], fp.axes[2], t)
    out = run_refine(world, banks, [(cp, cv), (tie, fv)], n_windows=1, max_windows=1)
    row = out["rows"][1][0][0].reshape(13, 13, 13, 25)
    assert same_bits(row[..., 12], row[..., 13]) and same_bits(row[j0], row[j0 + 2])
    first = int(np.argmax(row))                                     # numpy: the first maximum
    assert out["res"][0]["posIndex"][1] == first == key_index(out["keys"][1][0, 0])
    assert rr.decode(first, tie.dim)[0] == j0 and rr.decode(first, tie.dim)[3] == 12      # the tie was at the maximum, both ways
    assert (row.reshape(-1) == row.reshape(-1)[first]).sum() >= 4


def test_window_without_a_score_is_not_refined(four, plain):
    """7.  Window 1's code banks of channel 2 are NaN: its position manifold has no score at level 0 and is not scanned at
    level 1; its velocity manifold and the other windows keep their bits."""
    import torch
    world, banks = four
    code, _carr = banks.bcs.read_banks()
    full = np.zeros((banks.W, banks.maxK, 2 * world["L"] + 1), dtype=np.complex64)
    full[:, :world["K"]] = code
    full[1, 2] = np.nan
    code_d = torch.from_numpy(full.view(np.float32)).to("cuda:0")
    lv = rw.levels(2)
    out = run_refine(world, banks, lv, code=code_d.data_ptr())
    r = out["res"][1]
    assert (r["posIndex"] == -1).all() and (r["posScore"] == 0).all() and (r["posOutOfWindow"] == 0).all()
    assert np.isnan(r["offset"][:4]).all() and np.isnan(r["zVal"][:4]).all()
    assert not out["keys"][0][1, 0] and not out["keys"][1][1, 0]
    assert (r["velIndex"] == plain["res"][1]["velIndex"]).all() and r["zVal"][4:].tobytes() == plain["res"][1]["zVal"][4:].tobytes()
    for w in range(banks.W):
        for l in (0, 1):
            assert same_bits(out["rows"][l][1][w], plain["rows"][l][1][w])
            assert out["keys"][l][w, 1] == plain["keys"][l][w, 1]
            if w != 1:
                assert same_bits(out["rows"][l][0][w], plain["rows"][l][0][w]) and out["keys"][l][w, 0] == plain["keys"][l][w, 0]
        if w != 1:
            assert out["res"][w]["zVal"].tobytes() == plain["res"][w]["zVal"].tobytes()


def test_refusals_and_one_level(four, plain):
    """8.  Every refusal with its message; a 1-level handle is the plain axes handle."""
    world, banks = four
    lv = rw.levels(2)
    kw = dict(lag_half_width=world["L"], bin_half_width=world["B"], max_windows=banks.W, max_channels=banks.maxK)

    def make(levels, **over):
        h = dpe.RefineManifold(world["fs"], world["S"], world["C"], levels, **dict(kw, **over))
        h.Start()
        return h

    ax3 = dpe.GridAxes.uniform(3, 10.0)
    for levels, msg in (([], "nLevels 0 out of range"), ([lv[0]] * 5, "nLevels 5 out of range"),
                        ([(dpe.GridAxes([0.0, np.inf], [0.0], [0.0], [0.0]), ax3)], "level 0 position axis 0 entry 1 is not finite"),
                        ([lv[0], (ax3, dpe.GridAxes([0.0], [np.nan], [0.0], [0.0]))], "level 1 velocity axis 1 entry 0 is not finite"),
                        ([(dpe.GridAxes.uniform((70000, 70000, 1, 1), 1e-3), ax3)], "does not fit 32 bits"),
                        ([(dpe.GridAxes.uniform(3, 900.0), ax3), (dpe.GridAxes.uniform(3, 900.0), ax3)], "together extend beyond 3 km")):
        with pytest.raises(dpe.DpeError, match=msg):
            make(levels)
    with pytest.raises(dpe.DpeError, match="exceed the LDS"):
        make(lv, lag_half_width=300, max_channels=37)
    lib, C = dpe.engine.lib(), dpe.engine.C
    h_out = C.c_void_p()
    pa, va = lv[0][0].c_struct(), lv[0][1].c_struct()
    for field, msg in (("weightedMean", "weightedMean must be 0"), ("referencePair", "referencePair must be 0"),
                       ("posGridIndexOffset", "index offsets must be 0"), ("velGridIndexOffset", "index offsets must be 0")):
        cfg = dpe.engine.BcmConfig(world["S"], world["L"], world["B"], 1, 1, 8, world["C"], world["fs"], None, None, 0, 0, 0, 0, 1, 0, 0, 0)
        setattr(cfg, field, 1)
        assert lib.dpe_bcm_create_refine(C.byref(cfg), 1, C.byref(pa), C.byref(va), C.byref(h_out)) != 0
        assert msg in lib.dpe_last_error().decode()
    grid = np.zeros((1, 4))
    cfg = dpe.engine.BcmConfig(world["S"], world["L"], world["B"], 1, 1, 8, world["C"], world["fs"], grid.ctypes.data_as(C.POINTER(C.c_double)),
                               None, 0, 0, 0, 0, 1, 0, 0, 0)
    assert lib.dpe_bcm_create_refine(C.byref(cfg), 1, C.byref(pa), C.byref(va), C.byref(h_out)) != 0
    assert "posGrid / velGrid must be NULL" in lib.dpe_last_error().decode()
    # the other kinds' calls on a refine handle, the refine calls on another kind of handle
    h = make(lv)
    plainh = dpe.BatchCorrManifold(world["fs"], world["S"], world["C"], lv[0][0], lv[0][1], **kw)
    plainh.Start()
    try:
        args = (banks.bcs.CodeScores, banks.bcs.CarrScores, banks.bw, banks.ce)
        h.Update(*args)
        h.results()
        with pytest.raises(dpe.DpeError, match="use dpe_bcm_update_refine"):
            dpe.BatchCorrManifold.Update(h, *args)
        with pytest.raises(dpe.DpeError, match="use dpe_bcm_update_refine"):
            dpe.BatchCorrManifold.UpdatePrepared(h, args[0], args[1], 8)
        ports = dpe.engine.BcmPortsDev(dimT=1, reserved=0)
        assert lib.dpe_bcm_update_dev(h._h, C.c_void_p(args[0]), C.c_void_p(args[1]), 8, C.byref(ports), C.c_double(0.0), None) != 0
        assert "use dpe_bcm_update_refine" in lib.dpe_last_error().decode()
        res = (dpe.engine.BcmResult * 4)()
        keys = np.ones((4, 2), dtype=np.uint64)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        for call, msg in ((lambda: lib.dpe_bcm_results(h._h, res, None), "use dpe_bcm_results_refine"),
                          (lambda: lib.dpe_bcm_results_from_keys(h._h, keys.ctypes.data_as(C.POINTER(C.c_uint64)), 4, vp(grid), C.c_int64(1), vp(grid),
                                                                 C.c_int64(1), res), "use dpe_bcm_results_refine"),
                          (lambda: lib.dpe_bcm_set_graph(h._h, 1), "refine Updates"),
                          (lambda: lib.dpe_bcm_update_joint(h._h, 1, 1, None, None), "update_joint"),
                          (lambda: lib.dpe_bcm_update_epochs(h._h, C.c_void_p(args[0]), C.c_void_p(args[1]), 1, 1, 8, vp(banks.bw), vp(banks.ce), None),
                           "not made by dpe_bcm_create_epochs"),
                          (lambda: lib.dpe_bcm_update_subsets(h._h, C.c_void_p(args[0]), C.c_void_p(args[1]), 1, 8, vp(banks.bw), vp(banks.ce), 0, None,
                                                              None), "not made by dpe_bcm_create_subsets")):
            assert call() != 0 and msg in lib.dpe_last_error().decode(), msg
        assert lib.dpe_bcm_exchange_keys(h._h, C.c_void_p(1), None, None) != 0      # (refused before the communicator is touched)
        assert "a refine handle" in lib.dpe_last_error().decode()
        for call in (lambda: lib.dpe_bcm_scores(h._h, None, None), lambda: lib.dpe_bcm_keys(h._h, C.byref(C.c_void_p()))):
            assert call() != 0 and "a refine handle" in lib.dpe_last_error().decode()
        cm =dpe.engine.ChanMgrDev.from_handoff(ew.build(N=1, K=8, seed=0)["ho"], world["S"] / world["fs"], 8)
        try:
            with pytest.raises(dpe.DpeError, match="a refine handle"):
                cm.attach(None, h)
        finally:
            cm.Stop()
        rres = (dpe.engine.BcmRefineResult * 4)()
        p = C.c_void_p()
        for call in (lambda: lib.dpe_bcm_update_refine(plainh._h, C.c_void_p(args[0]), C.c_void_p(args[1]), 4, 8, vp(banks.bw), vp(banks.ce), None),
                     lambda: lib.dpe_bcm_results_refine(plainh._h, rres, None),
                     lambda: lib.dpe_bcm_refine_scores(plainh._h, 0, C.byref(p), None, None, None),
                     lambda: lib.dpe_bcm_refine_keys(plainh._h, 0, C.byref(p))):
            assert call() != 0 and "not made by dpe_bcm_create_refine" in lib.dpe_last_error().decode()
        with pytest.raises(dpe.DpeError, match="level 2 out of range"):
            h.read_keys(2)
        # one level: the plain axes handle on the level's own axes (batch of 4)
        one = run_refine(world, banks, lv[:1])
        plainh.Update(*args)
        want, (ps, vs) = plainh.results(), plainh.read_scores()
        wk = dpe.engine.d2h(plainh.Keys, 4 * 16, np.uint64).reshape(4, 2)
        assert same_bits(one["rows"][0][0], ps) and same_bits(one["rows"][0][1], vs) and np.array_equal(one["keys"][0], wk)
        assert same_bits(one["rows"][0][0], plain["rows"][0][0])
        for a, b in zip(one["res"], want):
            assert a["zVal"].tobytes() == b["zVal"].tobytes() and a["posIndex"][0] == b["posIndex"] and a["velIndex"][0] == b["velIndex"]
    finally:
        h.Stop()
        plainh.Stop()


def test_closed_loop_follows_the_level_chain():
    """9.  run_refine_closed_loop over the 6-window epoch world: every window's per-level indices are those of the numpy level
    chain with the oracle's rows on the GPU's own banks and the channel manager's own records."""
    base = rw.build()
    world = ew.build(N=6, K=8)
    iq = np.stack([w["iq"] for w in world["wins"]])
    lv = rw.levels(2)
    fixes, results = dpe.pipeline.run_refine_closed_loop(iq, world["ho"], world["fs"], lv, lag_half_width=base["L"], bin_half_width=base["B"],
                                                         keep_banks=True)
    assert fixes.shape == (6, 8) and np.isfinite(fixes).all()
    for w, r in enumerate(results):
        _cs, ce, bw = r["inputs"]
        win = dict(sat=ce["satState"], centre=bw["xCurrkk1"][0], R=bw["enu2ecef"][0], fc=ce["codeFrequency"], fi=ce["carrierFrequency"],
                   cpRefTOW=ce["cpRefTOW"], cpElaEnd=ce["cpElapsedEnd"], cpRef=ce["cpRef"], rcEnd=ce["codePhaseEnd"],
                   rxTime=float(bw["rxTime"][0]))      # (the channel manager's records: [K] per channel, [1] per window)
        one = dict(fs=world["fs"], S=world["S"], C=world["C"], K=world["K"], L=base["L"], B=base["B"], N=1, wins=[win])
        for m, name in ((0, "pos"), (1, "vel")):
            chain, pt = rr.chain(rw.axes_of(lv, m), rw.scorer(one, 0, m, code=r["codeBank"], carr=r["carrBank"]))
            print("window %d %s: GPU %s, level chain %s, margins %s" % (w, name, r[name + "Index"].tolist(), [x["index"] for x in chain],
                                                                       ["%.2g" % rw.margin(x["row"])[1] for x in chain]))
            assert r[name + "Index"].tolist() == [x["index"] for x in chain], (w, name)
            assert r["offset"][4 * m:4 * m + 4].tobytes() == pt.tobytes(), (w, name)
