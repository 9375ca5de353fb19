"""GPU: the subsets scan (dpe_bcm_create_subsets / engine.SubsetManifold) -- the arg-max of every SV subset of a window from
one launch -- against dpe_bcm_update handed only a subset's channels, against the oracle, and in the closed loop with fault
exclusion.  Inputs: tests/epoch_world.py and tests/fde_world.py, proven on the CPU by tests/test_epoch_world_cpu.py and
tests/test_fde_world_cpu.py.

Bounds.  Against dpe_bcm_update everything is bit equality: a subset's key, index, score, zVal and out-of-window counts are
those of an Update on the subset's channels alone (their bank rows gathered into one contiguous buffer, bit for bit copies),
and the full set's row, key and counts are those of an Update on all channels.  Against the oracle: tests/test_gpu_parity.py's
scores tolerance (2e-6 of the row maximum against the extended-precision position rows and the velocity rows); the arg-max of
every subset is the one tests/test_fde_world_cpu.py proves with margins of at least ten tolerances."""
import ctypes as C

import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import epoch_world as ew, fde_world as fw
from tests.test_gpu_epochs import TOL, key_index, same_bits
from tests.test_gpu_epochs_walk import Banks, tiles

pytestmark = pytest.mark.gpu


def sel_of(mask, K):
    return np.array([k for k in range(K) if (int(mask) >> k) & 1])


def make_key(score, index):
    return (int(np.float32(score).view(np.uint32)) << 32) | (0xFFFFFFFF - int(index))


def run_subsets(world, banks, masks, pos=None, vel=None, lpower=1, max_subsets=None, max_windows=None, split=None, code=None, carr=None,
                twice=False):
    """One launch over all windows of `banks` with masks [W, M] (or [M]); rows, keys and results read back."""
    masks = np.asarray(masks, dtype=np.uint64)
    M = masks.shape[-1]
    h = dpe.SubsetManifold(world["fs"], world["S"], world["C"], world["pos"] if pos is None else pos, world["vel"] if vel is None else vel,
                           max(M, 1) if max_subsets is None else max_subsets, LPower=lpower, lag_half_width=world["L"],
                           bin_half_width=world["B"], max_windows=banks.W if max_windows is None else max_windows, max_channels=banks.maxK)
    h.Start()
    try:
        for _ in range(2 if twice else 1):
            h.Update(banks.bcs.CodeScores if code is None else code, banks.bcs.CarrScores if carr is None else carr, banks.bw, banks.ce, masks)
        got = h.last_split()
        assert split is None or got == split, "scan_split gave %s, the test needs %s" % (got, split)
        res = h.results()
        ps, vs = h.read_scores()
        keys = h.read_keys()
    finally:
        h.Stop()
    return dict(res=res, pos=ps, vel=vs, keys=keys)


def run_full(world, banks, pos=None, vel=None, lpower=1, code=None, carr=None):
    """Every window through dpe_bcm_update on all channels (one batch)."""
    h = dpe.BatchCorrManifold(world["fs"], world["S"], world["C"], world["pos"] if pos is None else pos, world["vel"] if vel is None else vel,
                              LPower=lpower, lag_half_width=world["L"], bin_half_width=world["B"], max_windows=banks.W, max_channels=banks.maxK)
    h.Start()
    try:
        h.Update(banks.bcs.CodeScores if code is None else code, banks.bcs.CarrScores if carr is None else carr, banks.bw, banks.ce)
        res = h.results()
        ps, vs = h.read_scores()
        keys = dpe.engine.d2h(h.Keys, banks.W * 16, np.uint64).reshape(-1, 2)
    finally:
        h.Stop()
    return dict(res=res, pos=ps, vel=vs, keys=keys)


class SubsetRef:
    """dpe_bcm_update on a subset's channels alone: the channels' bank rows of the window are gathered (bit-for-bit copies) into
    one contiguous device buffer with the handle's channel stride, their dpe_chan_end records into one list."""

    def __init__(self, world, banks, pos=None, vel=None, lpower=1, code=None, carr=None):
        import torch
        self.torch, self.world, self.banks = torch, world, banks
        if code is None:
            code, carr = banks.bcs.read_banks()
        self.code, self.carr = np.ascontiguousarray(code), np.ascontiguousarray(carr)
        self.h = dpe.BatchCorrManifold(world["fs"], world["S"], world["C"], world["pos"] if pos is None else pos,
                                       world["vel"] if vel is None else vel, LPower=lpower, lag_half_width=world["L"],
                                       bin_half_width=world["B"], max_windows=1, max_channels=banks.maxK)
        self.h.Start()
        self.cache = {}

    def run(self, w, mask):
        key = (w, int(mask))
        if key not in self.cache:
            sel = sel_of(mask, self.world["K"])
            bufs = []
            for src in (self.code, self.carr):
                b = np.zeros((self.banks.maxK, src.shape[2]), dtype=np.complex64)
                b[:len(sel)] = src[w, sel]
                bufs.append(self.torch.from_numpy(b.view(np.float32)).to("cuda:0"))
            self.h.Update(bufs[0], bufs[1], self.banks.bw[w:w + 1], np.ascontiguousarray(self.banks.ce[w:w + 1, sel]))
            r = self.h.results()[0]
            r["keys"] = dpe.engine.d2h(self.h.Keys, 16, np.uint64).copy()
            self.cache[key] = r
        return self.cache[key]

    def close(self):
        self.h.Stop()


def assert_same_fix(got, want, where):
    """A subset's result against dpe_bcm_update's on its channels: keys, indices, scores, zVal, counts -- bit for bit."""
    for k in ("posIndex", "velIndex", "posOutOfWindow", "velOutOfWindow"):
        assert got[k] == want[k], (where, k, got[k], want[k])
    for k in ("posScore", "velScore"):
        assert np.float32(got[k]).tobytes() == np.float32(want[k]).tobytes(), (where, k)
    assert got["zVal"].tobytes() == want["zVal"].tobytes(), where
    if "keys" in want:
        assert make_key(got["posScore"], got["posIndex"]) == int(want["keys"][0]), where
        assert make_key(got["velScore"], got["velIndex"]) == int(want["keys"][1]), where


def assert_full_is_update(out, full, W):
    assert same_bits(out["pos"], full["pos"]) and same_bits(out["vel"], full["vel"])
    assert np.array_equal(out["keys"], full["keys"])
    for w in range(W):
        assert_same_fix(out["res"][w], dict(full["res"][w], keys=full["keys"][w]), ("full", w))


def assert_subsets_are_updates(world, out, ref, masks, W):
    masks = np.broadcast_to(np.asarray(masks, dtype=np.uint64), (W, np.asarray(masks).shape[-1]))
    for w in range(W):
        assert len(out["res"][w]["subs"]) == masks.shape[1]
        for m, mask in enumerate(masks[w]):
            assert_same_fix(out["res"][w]["subs"][m], ref.run(w, mask), (w, m, hex(int(mask))))


@pytest.fixture(scope="module")
def eight():
    """8 windows x K = 8 on the 7^4 grids."""
    world = ew.build(N=8, K=8, seed=0)
    banks = Banks(world)
    yield world, banks
    banks.close()


def test_leave_one_out_bit_for_bit(eight):
    """1.  8 windows x 8 SVs with the 8 leave-one-out masks in one launch."""
    world, banks = eight
    masks = dpe.engine.leave_one_out_masks(8)
    out, full = run_subsets(world, banks, masks), run_full(world, banks)
    assert out["pos"].shape == (8, 2401)
    assert_full_is_update(out, full, 8)
    ref = SubsetRef(world, banks)
    try:
        assert_subsets_are_updates(world, out, ref, masks, 8)
    finally:
        ref.close()
    for w in range(8):
        assert out["res"][w]["posIndex"] == world["pos_at"] and out["res"][w]["velIndex"] == world["vel_at"]
        assert np.array_equal(out["res"][w]["offset"], world["offset"])
        assert not out["res"][w]["oobPerSv"].any()
        for s in out["res"][w]["subs"]:          # the strong clean world: every exclusion still peaks on the point
            assert s["posIndex"] == world["pos_at"] and s["velIndex"] == world["vel_at"]
            assert np.array_equal(s["offset"], world["offset"]) and np.abs(s["zVal"] - world["truth"][w]).max() < 1e-6


def arbitrary_masks(K, M, W, seed):
    """[W, M]: a single SV, the first half, alternating SVs, all but two, then random non-empty masks; rotated per window."""
    rng = np.random.Generator(np.random.PCG64(seed))
    allsv = (1 << K) - 1
    out = np.zeros((W, M), dtype=np.uint64)
    for w in range(W):
        named = [1 << ((w + 1) % K), (1 << (K // 2)) - 1, (0x5555555555 if w % 2 == 0 else 0xAAAAAAAAAA) & allsv,
                 allsv & ~(1 << (w % K)) & ~(1 << ((w + 2) % K))]
        named = named[w % 4:] + named[:w % 4]
        while len(named) < M:
            named.append(int(rng.integers(1, allsv + 1)))
        out[w] = named[:M]
    return out


@pytest.mark.parametrize("K,M", [(4, 1), (4, 16), (12, 1), (12, 16)])
def test_arbitrary_masks(K, M):
    """2.  Masks that differ per window, 1 and 16 subsets, 4 and 12 channels, on a handle made for 16 channels, 16 subsets and 5
    windows that is given 3 windows."""
    world = ew.build(N=3, K=K, seed=2)
    banks = Banks(world, max_channels=16)
    masks = arbitrary_masks(K, M, 3, 100 + K + M)
    assert len({int(x) for x in masks[:, 0]}) == 3 and (masks != 0).all() and (masks >> np.uint64(K) == 0).all()
    ref = SubsetRef(world, banks)
    try:
        out, full = run_subsets(world, banks, masks, max_subsets=16, max_windows=5), run_full(world, banks)
        assert_full_is_update(out, full, 3)
        assert_subsets_are_updates(world, out, ref, masks, 3)
    finally:
        ref.close()
        banks.close()


@pytest.mark.parametrize("lpower,widen", [(2, True), (3, True), (2, False), (3, "L"), (1, "B"), (1, False)])
def test_lpower_and_clamped_variants(lpower, widen):
    """3.  LPower 2 and 3 (the generic powf variant) and the clamp variants: narrow banks on both sides, on the lag side only, on
    the bin side only.  Per-SV out-of-window counts are those of an Update on that SV alone; a subset's count is its own run's."""
    world = ew.build(N=2, K=4, seed=1, widen=widen)
    banks = Banks(world)
    masks = np.array([[0b0111, 0b1010, 0b0100, 0b1101], [0b1110, 0b0101, 0b1000, 0b1011]], dtype=np.uint64)
    ref = SubsetRef(world, banks, lpower=lpower)
    try:
        out, full = run_subsets(world, banks, masks, lpower=lpower), run_full(world, banks, lpower=lpower)
        assert_full_is_update(out, full, 2)
        assert_subsets_are_updates(world, out, ref, masks, 2)
        per = np.zeros((2, 2, 4), dtype=np.int64)
        for w in range(2):
            for k in range(4):
                r = ref.run(w, 1 << k)
                per[w, 0, k], per[w, 1, k] = r["posOutOfWindow"], r["velOutOfWindow"]
            assert np.array_equal(out["res"][w]["oobPerSv"], per[w]), w
            assert out["res"][w]["posOutOfWindow"] == per[w, 0].sum() and out["res"][w]["velOutOfWindow"] == per[w, 1].sum()
        print("LPower %d, widen %s: per-SV out-of-window pairs (window, manifold, SV) %s" % (lpower, widen, per.tolist()))
        assert (per[:, 0].sum() > 0) == (widen in (False, "L")) and (per[:, 1].sum() > 0) == (widen in (False, "B"))
        assert np.isfinite(out["pos"]).all() and np.isfinite(out["vel"]).all()
    finally:
        ref.close()
        banks.close()


def test_an_excluded_nan_stays_out_of_the_sum(eight):
    """SV 5's bank rows are NaN in window 0: the full row is NaN there, the subset without SV 5 carries the bits of an Update on the
    other seven channels -- the excluded term is skipped, not multiplied by 0."""
    import torch
    world, banks = eight
    code, carr = banks.bcs.read_banks()
    code, carr = code.copy(), carr.copy()
    code[0, 5] = np.nan
    carr[0, 5] = np.nan
    cd = torch.from_numpy(np.ascontiguousarray(code).view(np.float32)).to("cuda:0")
    fd = torch.from_numpy(np.ascontiguousarray(carr).view(np.float32)).to("cuda:0")
    masks = np.array([0xFF & ~(1 << 5), 1 << 5, 0x0F], dtype=np.uint64)
    out = run_subsets(world, banks, masks, code=cd, carr=fd)
    assert np.isnan(out["pos"][0]).all() and np.isnan(out["vel"][0]).all() and np.isfinite(out["pos"][1:]).all()
    r0 = out["res"][0]
    assert r0["posIndex"] == -1 and r0["velIndex"] == -1 and np.isnan(r0["zVal"]).all() and r0["subs"][1]["posIndex"] == -1
    ref = SubsetRef(world, banks, code=code, carr=carr)
    try:
        for w in range(2):
            for m in (0, 2):
                assert_same_fix(out["res"][w]["subs"][m], ref.run(w, masks[m]), (w, m))
        assert np.isfinite(out["res"][0]["subs"][0]["posScore"]) and out["res"][0]["subs"][0]["posIndex"] == world["pos_at"]
    finally:
        ref.close()


WALK_MASKS = np.array([0b1111, 0b0101, 0b1000], dtype=np.uint64)


def with_ties(world):
    """The world's grids with the expected arg-max point copied onto an EARLIER point of an earlier tile and onto a later one:
    three points of every score row tie exactly, and the first must win."""
    pos, vel = world["pos"].copy(), world["vel"].copy()
    first = {}
    for name, g, at in (("pos", pos, world["pos_at"]), ("vel", vel, world["vel_at"])):
        early, late = at - 1024 - 77, min(at + 1024 + 5, g.shape[0] - 1)
        assert 0 <= early < at < late and early // 1024 != at // 1024
        g[early] = g[at]
        g[late] = g[at]
        first[name] = early
    return pos, vel, first


def test_batch_walk_with_ties(oracle):
    """4a.  32 windows on 15^4 / 14^4 grids: 24 blocks per window walk 50 and 38 tiles through the double buffer (the ragged
    tile by the even path and through the bufB -> bufA copy).  The arg-max point is duplicated in an earlier and a later tile."""
    world = ew.build(N=8, K=4, seed=5, pos_dim=15, vel_dim=14)
    assert (tiles(world["pos"].shape[0]), tiles(world["vel"].shape[0])) == (50, 38)
    banks = Banks(world, 32)
    pos, vel, first = with_ties(world)
    masks = np.stack([np.roll(WALK_MASKS, w % 3) for w in range(32)])
    ref = SubsetRef(world, banks, pos=pos, vel=vel)
    try:
        out = run_subsets(world, banks, masks, pos=pos, vel=vel, split=(24, 24))
        full = run_full(world, banks, pos=pos, vel=vel)
        assert_full_is_update(out, full, 32)
        assert_subsets_are_updates(world, out, ref, masks, 32)
        for w in range(32):
            r = out["res"][w]
            assert r["posIndex"] == first["pos"] and r["velIndex"] == first["vel"], w
            assert out["pos"][w][first["pos"]].tobytes() == out["pos"][w][world["pos_at"]].tobytes()
            assert key_index(out["keys"][w, 0]) == int(np.argmax(out["pos"][w])) == first["pos"]
            assert key_index(out["keys"][w, 1]) == int(np.argmax(out["vel"][w])) == first["vel"]
            m = int(np.where(masks[w] == 0b1111)[0][0])          # the subset of all four SVs: its row is the full row, tie included
            assert r["subs"][m]["posIndex"] == first["pos"] and r["subs"][m]["velIndex"] == first["vel"], w
    finally:
        ref.close()
        banks.close()


@pytest.mark.parametrize("lpower,widen", [(1, False), (2, True), (2, False), (3, True), (3, False)])
def test_batch_walk_lpower_and_clamped_variants(lpower, widen):
    """4a for the other (LPower, clamp) variants (LPower 1 on clean banks is 4a itself): 32 windows, 24 blocks per window walk
    50 and 38 tiles.  The full rows, keys and fixes are dpe_bcm_update's at the same power on every window; on three windows
    every subset is an Update on its channels and the per-SV out-of-window counts are those of an Update on that SV alone:
    non-zero on both manifolds with narrow banks, zero with clean ones."""
    world = ew.build(N=8, K=4, seed=5, widen=widen, pos_dim=15, vel_dim=14)
    assert (tiles(world["pos"].shape[0]), tiles(world["vel"].shape[0])) == (50, 38)
    banks = Banks(world, 32)
    masks = np.stack([np.roll(WALK_MASKS, w % 3) for w in range(32)])
    ref = SubsetRef(world, banks, lpower=lpower)
    try:
        out = run_subsets(world, banks, masks, lpower=lpower, split=(24, 24))
        full = run_full(world, banks, lpower=lpower)
        assert_full_is_update(out, full, 32)
        assert np.isfinite(out["pos"]).all() and np.isfinite(out["vel"]).all()
        for w in range(32):
            assert key_index(out["keys"][w, 0]) == int(np.argmax(out["pos"][w])) == out["res"][w]["posIndex"], w
            assert key_index(out["keys"][w, 1]) == int(np.argmax(out["vel"][w])) == out["res"][w]["velIndex"], w
        for w in (0, 13, 31):
            for m, mask in enumerate(masks[w]):
                assert_same_fix(out["res"][w]["subs"][m], ref.run(w, mask), (w, m, hex(int(mask))))
            per = np.zeros((2, 4), dtype=np.int64)
            for k in range(4):
                r = ref.run(w, 1 << k)
                per[0, k], per[1, k] = r["posOutOfWindow"], r["velOutOfWindow"]
            assert np.array_equal(out["res"][w]["oobPerSv"], per), w
            assert out["res"][w]["posOutOfWindow"] == per[0].sum() and out["res"][w]["velOutOfWindow"] == per[1].sum()
            assert (per[0].sum() > 0) == (not widen) and (per[1].sum() > 0) == (not widen), (w, per.tolist())
    finally:
        ref.close()
        banks.close()


@pytest.mark.parametrize("side", [True, "L"])
def test_one_window_walk_with_unequal_splits(oracle, side):
    """4b.  One window on a 20^4 position grid (157 tiles for 128 blocks) and a 7^4 velocity grid (3 tiles: 125 velocity blocks
    only take the publish ticket); widened banks, and only the lag banks narrow (the position manifold clamps, the velocity
    manifold does not)."""
    world = ew.build(N=4, K=4, seed=7, widen=side, pos_dim=20, vel_dim=7)
    assert (tiles(world["pos"].shape[0]), tiles(world["vel"].shape[0])) == (157, 3)
    banks = Banks(world, 1)
    pos, vel = world["pos"].copy(), world["vel"]
    early = world["pos_at"] - 3 * 1024 - 11
    pos[early] = pos[world["pos_at"]]
    masks = np.array([0b1111, 0b0110, 0b0001, 0b1110], dtype=np.uint64)
    ref = SubsetRef(world, banks, pos=pos)
    try:
        out = run_subsets(world, banks, masks, pos=pos, split=(128, 3))
        full = run_full(world, banks, pos=pos)
        assert_full_is_update(out, full, 1)
        assert_subsets_are_updates(world, out, ref, masks, 1)
        r = out["res"][0]
        if side is True:
            assert r["posIndex"] == early and r["velIndex"] == world["vel_at"] and r["subs"][0]["posIndex"] == early
            assert r["posOutOfWindow"] == 0 and not r["oobPerSv"].any()
        else:
            assert r["posOutOfWindow"] > 0 and r["velOutOfWindow"] == 0 and r["oobPerSv"][0].sum() == r["posOutOfWindow"]
            assert r["velIndex"] == world["vel_at"]
    finally:
        ref.close()
        banks.close()


@pytest.mark.parametrize("name", sorted(fw.WORLDS))
def test_fault_worlds_against_the_oracle(oracle, name):
    """5.  The full row is within the score tolerance of the oracle's on every point; the full set's and every leave-one-out
    subset's arg-max is the oracle's, which tests/test_fde_world_cpu.py proves: pulled off the truth by SV j, back on it without j."""
    world = fw.build(name)
    j, lpower = world["fault"], world["lpower"]
    banks = Banks(world)
    masks = fw.masks_loo()
    try:
        out = run_subsets(world, banks, masks, lpower=lpower)
    finally:
        banks.close()
    allsv = (1 << fw.K) - 1
    want = fw.oracle_subset(world, allsv)
    for gname, rname in (("pos", "pos_x"), ("vel", "vel")):
        err = np.abs(out[gname][0].astype(np.float64) - want[rname])
        print("%s: full %s row vs the oracle's %s row: %.3g of the row maximum (bound %.3g)" % (name, gname, rname, err.max() / want[rname].max(), TOL))
        assert err.max() <= TOL * want[rname].max()
    r = out["res"][0]
    assert r["posIndex"] == oracle.argmax_first(want["pos_x"]) and r["velIndex"] == oracle.argmax_first(want["vel"]) == world["vel_at"]
    assert (r["posIndex"] == world["pos_at"]) == (j is None)
    for k, mask in enumerate(masks):
        o = fw.oracle_subset(world, mask)
        s = r["subs"][k]
        assert s["posIndex"] == oracle.argmax_first(o["pos_x"]) and s["velIndex"] == oracle.argmax_first(o["vel"]), k
        assert (s["posIndex"] == world["pos_at"]) == (j is None or k == j), k
        assert s["posOutOfWindow"] == 0 and s["velOutOfWindow"] == 0
    suspect, sep = dpe.pipeline.solution_separation(r, r["subs"], masks, fw.THRESHOLD_M)
    print("%s: separations (m) %s -> suspect %d" % (name, np.round(sep, 1).tolist(), suspect))
    assert suspect == (-1 if j is None else j)
    if j is not None:
        assert np.abs(r["subs"][j]["zVal"] - world["truth"][0]).max() < 1e-6 and np.abs(r["zVal"][:4] - world["truth"][0][:4]).max() > 40.0


def test_closed_loop_without_a_suspect_is_run_closed_loop_bit_for_bit(golden):
    """6a.  Six windows of the O13 closed-loop input with a threshold nothing exceeds: the full set's fix is dpe_bcm_update's, so
    the loop is run_closed_loop's, bit for bit, and no window names a suspect."""
    from tests.test_gpu_loop_o13 import _setup
    g = golden("o13_dp_track")
    ho, delta, pos, vel, iq = _setup(g)
    iq = iq[:6]
    tg = np.unique(pos[:, 3])
    want, _ = dpe.pipeline.run_closed_loop(iq, ho, float(g["fs"]), pos, vel, time_grid=tg, init_delta=delta)
    got, suspects, seps, res = dpe.pipeline.run_fde_closed_loop(iq, ho, float(g["fs"]), pos, vel, np.inf, time_grid=tg, init_delta=delta)
    K = len(ho["prn_list"])
    assert got.shape == want.shape == (6, 8) and got.tobytes() == want.tobytes()
    assert suspects.tolist() == [-1] * 6 and seps.shape == (6, K) and all(len(r["subs"]) == K for r in res)


def test_closed_loop_detects_excludes_and_recovers(oracle):
    """6.  run_fde_closed_loop over the six consecutive windows of fde_world.build_loop, SV 3 faulty in windows 2 .. 4 only, at a
    threshold of one position step: the suspect is 3 exactly there and -1 elsewhere, the chosen fix is on the truth's grid point
    in all six windows, and every window's arg-max pairs (full set and all eight exclusions) are those of the oracle's loop,
    which tests/test_fde_world_cpu.py proves with margins of at least ten score tolerances.  Without exclusion the same loop
    is off the truth by more than a step in windows 2 .. 4."""
    world = fw.build_loop()
    step = ew.POS_STEP
    kw = dict(lpower=world["lpower"], lag_half_width=world["L"], bin_half_width=world["B"])
    args = (world["iq"], world["ho"], world["fs"], world["pos"], world["vel"], fw.THRESHOLD_M)
    fixes, suspects, seps, res = dpe.pipeline.run_fde_closed_loop(*args, **kw)
    plain, s0, _, res0 = dpe.pipeline.run_fde_closed_loop(*args, exclude=False, **kw)
    err = np.abs(fixes[:, :4] - world["truth"][:, :4]).max(axis=1)
    err0 = np.abs(plain[:, :4] - world["truth"][:, :4]).max(axis=1)
    print("suspects %s (without exclusion %s); fix off the truth (m): with exclusion %s, without %s"
          % (suspects.tolist(), s0.tolist(), np.round(err, 3).tolist(), np.round(err0, 1).tolist()))
    assert suspects.tolist() == [3 if w in world["fault_windows"] else -1 for w in range(fw.LOOP_N)] == [-1, -1, 3, 3, 3, -1]
    assert err.max() < step / 2
    assert err0[:2].max() < step / 2 and err0[2:5].min() > step
    for got, r, want in ((fixes, res, fw.oracle_fde_loop(world, True)), (plain, res0, fw.oracle_fde_loop(world, False))):
        for w in range(fw.LOOP_N):
            am = [(r[w]["posIndex"], r[w]["velIndex"])] + [(s["posIndex"], s["velIndex"]) for s in r[w]["subs"]]
            assert am == want["argmax"][w], w
            assert r[w]["suspect"] == want["suspects"][w], w
            if r is res:
                assert np.array_equal(seps[w], want["seps"][w]), w
            assert r[w]["posOutOfWindow"] == 0 and r[w]["velOutOfWindow"] == 0
        assert np.abs(got - want["fixes"]).max() < 1e-6
    for w in world["fault_windows"]:
        assert res[w]["posIndex"] != world["centre_at"] and res[w]["subs"][3]["posIndex"] == world["centre_at"], w


def test_refusals_carry_a_message_and_launch_nothing(eight):
    """7.  Every refusal of dpe_hip.h's subsets block; a second Update on a used handle; nSubsets = 0 is the plain scan."""
    world, banks = eight
    e, lib = dpe.engine, dpe.engine.lib()
    args = (world["fs"], world["S"], world["C"], world["pos"], world["vel"])
    kw = dict(lag_half_width=world["L"], bin_half_width=world["B"], max_windows=8, max_channels=world["K"])
    loo = e.leave_one_out_masks(8)
    # nSubsets = 0: the plain scan's bits; then the same handle again with masks, twice
    full = run_full(world, banks)
    plain_bits = run_subsets(world, banks, np.zeros((8, 0), dtype=np.uint64), max_subsets=4)
    assert_full_is_update(plain_bits, full, 8)
    assert all(r["subs"] == [] for r in plain_bits["res"])
    once, twice = run_subsets(world, banks, loo), run_subsets(world, banks, loo, twice=True)
    assert np.array_equal(once["keys"], twice["keys"]) and same_bits(once["pos"], twice["pos"])
    for w in range(8):
        assert_same_fix(twice["res"][w], once["res"][w], ("twice", w))
        assert np.array_equal(twice["res"][w]["oobPerSv"], once["res"][w]["oobPerSv"])
        for m in range(8):
            assert_same_fix(twice["res"][w]["subs"][m], once["res"][w]["subs"][m], ("twice", w, m))
    h = dpe.SubsetManifold(*args, 8, **kw)
    h.Start()
    plain = dpe.BatchCorrManifold(*args, **kw)
    plain.Start()
    joint = dpe.JointManifold(*args, 2, 16, **kw)
    joint.Start()
    epochs = dpe.EpochManifold(*args, 4, 0, **kw)
    epochs.Start()
    code, carr = banks.bcs.CodeScores, banks.bcs.CarrScores
    bwp, cep = banks.bw.ctypes.data_as(C.POINTER(e.BcmWindow)), banks.ce.ctypes.data_as(C.POINTER(e.ChanEnd))
    try:
        h.Update(code, carr, banks.bw, banks.ce, loo)
        before = h.read_keys().copy()
        assert before.all()
        with pytest.raises(dpe.DpeError, match="empty mask"):
            h.Update(code, carr, banks.bw, banks.ce, np.array([0xFE, 0], dtype=np.uint64))
        with pytest.raises(dpe.DpeError, match="bit at or above nChan 8"):
            h.Update(code, carr, banks.bw, banks.ce, np.array([0x1FE], dtype=np.uint64))
        with pytest.raises(dpe.DpeError, match="nSubsets 9 out of range"):
            h.Update(code, carr, banks.bw, banks.ce, np.arange(1, 10, dtype=np.uint64))
        with pytest.raises(dpe.DpeError, match="use dpe_bcm_update_subsets"):
            e._check(lib.dpe_bcm_update(h._h, e._ptr(code), e._ptr(carr), C.c_int32(1), C.c_int32(8), bwp, cep, e._stream(None)))
        ports = e.BcmPortsDev(dimT=1, reserved=0)      # (null ports: the refusal comes first and nothing is launched)
        with pytest.raises(dpe.DpeError, match="use dpe_bcm_update_subsets"):
            e._check(lib.dpe_bcm_update_dev(h._h, e._ptr(code), e._ptr(carr), C.c_int32(8), C.byref(ports), C.c_double(0.0), e._stream(None)))
        with pytest.raises(dpe.DpeError, match="use dpe_bcm_update_subsets"):
            e._check(lib.dpe_bcm_update_prepared(h._h, e._ptr(code), e._ptr(carr), C.c_int32(8), e._stream(None)))
        with pytest.raises(dpe.DpeError, match="use dpe_bcm_results_subsets"):
            dpe.BatchCorrManifold.results(h)
        with pytest.raises(dpe.DpeError, match="use dpe_bcm_results_subsets"):
            dpe.BatchCorrManifold.results_from_keys(h, before, world["pos"], world["vel"])
        with pytest.raises(dpe.DpeError, match="always launch eagerly"):
            h.set_graph(True)
        comm = e.Comm(0, 1)
        try:
            with pytest.raises(dpe.DpeError, match="sharding is not supported"):
                dpe.BatchCorrManifold.exchange_keys(h, comm)
        finally:
            comm.close()
        cm = e.ChanMgrDev.from_handoff(world["ho"], world["S"] / world["fs"], world["K"])
        try:
            with pytest.raises(dpe.DpeError, match="subsets handle"):
                cm.attach(None, h)
        finally:
            cm.Stop()
        # the joint and epochs calls on a subsets handle
        with pytest.raises(dpe.DpeError, match="not made by dpe_bcm_create_joint"):
            e._check(lib.dpe_bcm_update_joint(h._h, C.c_int32(1), C.c_int32(1), (e.BcmJointRx * 1)(), e._stream(None)))
        with pytest.raises(dpe.DpeError, match="no joint update yet"):
            e._check(lib.dpe_bcm_results_joint(h._h, (e.BcmJointResult * 1)(), (e.BcmJointRxResult * 1)(), e._stream(None)))
        with pytest.raises(dpe.DpeError, match="not a handle of dpe_bcm_create_joint"):
            e._check(lib.dpe_bcm_joint_set_own_keys(h._h, C.c_int32(1)))
        with pytest.raises(dpe.DpeError, match="not made by dpe_bcm_create_epochs"):
            e._check(lib.dpe_bcm_update_epochs(h._h, e._ptr(code), e._ptr(carr), C.c_int32(1), C.c_int32(1), C.c_int32(8), bwp, cep, e._stream(None)))
        with pytest.raises(dpe.DpeError, match="not made by dpe_bcm_create_epochs"):
            e._check(lib.dpe_bcm_results_epochs(h._h, (e.BcmEpochsResult * 1)(), e._stream(None)))
        # nothing was launched by the refused calls: the key set of the last good Update is still the current one, unchanged
        keys = C.c_void_p()
        e._check(lib.dpe_bcm_keys(h._h, C.byref(keys)))
        assert keys.value == h.Keys and np.array_equal(h.read_keys(), before)
        # the calls that work unchanged on the full row and key
        assert h.last_split() == (3, 3) and h.PosScores and h.PosScoresPitch >= 2401
        assert "bcm_scan" in h.profile(False)
        # the subset calls on every other kind of handle
        mp = loo.ctypes.data_as(C.POINTER(C.c_uint64))
        for other in (plain, joint, epochs):
            with pytest.raises(dpe.DpeError, match="not made by dpe_bcm_create_subsets"):
                e._check(lib.dpe_bcm_update_subsets(other._h, e._ptr(code), e._ptr(carr), C.c_int32(1), C.c_int32(8), bwp, cep, C.c_int32(8), mp,
                                                    e._stream(None)))
            with pytest.raises(dpe.DpeError, match="not made by dpe_bcm_create_subsets"):
                e._check(lib.dpe_bcm_results_subsets(other._h, (e.BcmSubsetResult * 1)(), (e.BcmSubsetResult * 8)(), None, e._stream(None)))
    finally:
        for x in (h, plain, joint, epochs):
            x.Stop()
    for bad in (0, 17):
        with pytest.raises(dpe.DpeError, match="maxSubsets %d out of range" % bad):
            dpe.SubsetManifold(*args, bad, **kw).Start()
    with pytest.raises(dpe.DpeError, match="no 12-byte bank entries"):        # 37 channels x 345 entries do not fit the LDS as 16-byte entries
        dpe.SubsetManifold(*args, 8, lag_half_width=8, bin_half_width=172, max_windows=1, max_channels=37).Start()
    with pytest.raises(dpe.DpeError, match="point-list grids only"):
        ax = dpe.GridAxes.uniform(3, 10.0)
        dpe.SubsetManifold(world["fs"], world["S"], world["C"], ax, ax, 8)
    cfg = e._bcm_config(world["S"], world["L"], world["B"], 1, 1, 8, world["C"], world["fs"], world["pos"], world["vel"], 0, 0, False, True, False, False)
    for field, match in (("weightedMean", "weightedMean must be 0"), ("referencePair", "referencePair must be 0"),
                         ("posGridIndexOffset", "index offsets must be 0"), ("velGridIndexOffset", "index offsets must be 0")):
        setattr(cfg, field, 1)
        out = C.c_void_p(None)
        with pytest.raises(dpe.DpeError, match=match):
            e._check(lib.dpe_bcm_create_subsets(C.byref(cfg), C.c_int32(8), C.byref(out)))
        assert not out.value
        setattr(cfg, field, 0)
