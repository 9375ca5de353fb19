"""GPU: bcm_scan_joint_kernel (csrc/dpe_bcm_joint.h) where a block walks several tiles -- the shape it is measured at
(scripts/joint_scan_time.py) -- and on the inputs tests/test_gpu_joint.py holds constant.

tests/test_gpu_joint.py runs on 7^4 grids: three 1024-point tiles, never fewer tiles than blocks, so a block scores one tile.
Here the grids have 38 to 157 tiles against the 24 blocks of a 32-window batch or the 128 blocks of a single window
(scan_split), so the double-buffered prefetch, the bufB -> bufA copy before the ragged tile, the ragged tile as a block's
second or third tile, the running maxima (joint and per receiver, with their tile * 8 + it encoding) and the per-receiver
out-of-window counts all carry state across tiles.  Every test asserts through last_split() that the walk really happens.
Further: unequal splits, handles larger than their use (capacity strides against the caller's strides), channel sets that
change from window to window, 8 receivers / 64 pairs, the generic LPower variant, the mixed clamp variants, exact ties between
tiles of one block and lane, and a second Update on a handle with a stale state.

Inputs: tests/joint_world.py on larger grids, proven by the oracle alone in tests/test_joint_world_cpu.py.  A batch is a few
distinct windows dealt round-robin into 32 before stage 1; the oracle is evaluated on the distinct ones only.

Tolerances are tests/test_gpu_joint.py's, unchanged: TOL = 2e-6 against the extended-precision position rows and the velocity
rows, helpers.POS_REF_NOISE against the faithful rows, 1e-5 for LPower = 3 (tests/test_gpu_parity.py::test_lpower), all
relative to the window's joint maximum with no point set aside on clean worlds; the narrow-bank caps are those of
test_narrow_banks_clamp_path_counts_per_receiver.  Everything else is bit equality."""
import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import helpers, joint_world as jw
from tests.test_gpu_joint import TOL, check_against_oracle, moved

pytestmark = pytest.mark.gpu
W32 = 32
TILE = 1024


def tiles(G):
    return -(-G // TILE)


class Banks:
    """One BatchCorrScores per receiver over the world's distinct windows dealt round-robin into W windows (window w is the
    world's window w % n) BEFORE stage 1, so a single-receiver handle can take the W windows as one batch; the handles stay
    alive (their banks are the scans' inputs)."""

    def __init__(self, world, W):
        import torch
        self.world, self.W, self.n = world, W, world["W"]
        idx = np.arange(W) % self.n
        self.bcs, self.ce, self.bw = [], [], []
        for rx in world["rx"]:
            wins = rx["wins"]
            cs = np.stack([dpe.engine.chan_start_array(w["start"]["prn"], w["start"]["rc"], w["start"]["ri"], w["start"]["fc"],
                                                       w["start"]["fi"], w["start"]["cp"], w["start"]["cp_ref"]) for w in wins])
            ce = np.stack([dpe.engine.chan_end_array(w["sat"], w["rcEnd"], w["fc"], w["fi"], w["cpRefTOW"], w["cpElaEnd"], w["cpRef"])
                           for w in wins])
            bw = np.concatenate([dpe.engine.bcm_window_array(w["centre"][None, :], w["R"][None, :], [w["rxTime"]]) for w in wins])
            iq = np.stack([w["iq"] for w in wins])
            self.ce.append(np.ascontiguousarray(ce[idx]))
            self.bw.append(np.ascontiguousarray(bw[idx]))
            b = dpe.BatchCorrScores(world["fs"], samples_per_window=world["S"], lag_half_width=world["L"], bin_half_width=world["B"],
                                    max_windows=W, max_channels=rx["K"])
            b.Start()
            b.Update(torch.from_numpy(np.ascontiguousarray(iq[idx])).to("cuda:0"), np.ascontiguousarray(cs[idx]))
            self.bcs.append(b)

    def one(self, w, r, n_chan=None):
        """Receiver r of window w as JointManifold.Update takes it; n_chan: only its first n_chan channels."""
        code, carr = dpe.engine.bank_rows(self.bcs[r], w)
        return dict(code=code, carr=carr, win=self.bw[r][w], chan=self.ce[r][w][:n_chan])

    def rx(self, windows=None, plan=None):
        """[window][receiver] dicts; plan(w) -> [(receiver, n_chan or None)] in the order they are passed (default: all, in order)."""
        windows = range(self.W) if windows is None else windows
        plan = plan or (lambda w: [(r, None) for r in range(len(self.bcs))])
        return [[self.one(w, r, n) for r, n in plan(w)] for w in windows]

    def close(self):
        for b in self.bcs:
            b.Stop()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run_joint(world, rx, lpower=1, own=True, caps=None, grids=None, split=None, keep=None):
    """One Update of a joint handle sized exactly for `rx` (or by caps: max_rx, max_total, max_windows, max_channels).
    split: asserted against last_split().  keep: a list that receives the started handle instead of stopping it."""
    W, nRx = len(rx), len(rx[0])
    ks = [[len(d["chan"]) for d in row] for row in rx]
    caps = caps or dict(max_rx=nRx, max_total=max(sum(k) for k in ks), max_windows=W, max_channels=max(max(k) for k in ks))
    pos, vel = grids or (world["pos"], world["vel"])
    h = dpe.JointManifold(world["fs"], world["S"], world["C"], pos, vel, caps["max_rx"], caps["max_total"], LPower=lpower,
                          lag_half_width=world["L"], bin_half_width=world["B"], max_windows=caps["max_windows"],
                          max_channels=caps["max_channels"], own_keys=own)
    h.Start()
    try:
        out = update_joint(h, rx, split)
    except BaseException:
        h.Stop()
        raise
    if keep is None:
        h.Stop()
    else:
        keep.append(h)
    return out


def update_joint(h, rx, split=None):
    h.Update(rx)
    got = h.last_split()
    if split is not None:
        assert got == split, "scan_split gave %s, the test needs %s" % (got, split)
    ps, vs = h.read_scores()
    return dict(res=h.results(), pos=ps, vel=vs, keys=h.read_keys(), split=got)


def run_single(world, banks, r, n_chan=None, windows=None, lpower=1, grids=None):
    """Receiver r alone through dpe_bcm_update: all W windows as one batch, or one window (windows=(w,)); n_chan: its first
    n_chan channels only (the bank rows keep the handle's channel stride)."""
    K = world["rx"][r]["K"]
    pos, vel = grids or (world["pos"], world["vel"])
    w0, W = (0, banks.W) if windows is None else (windows[0], len(windows))
    h = dpe.BatchCorrManifold(world["fs"], world["S"], world["C"], pos, vel, LPower=lpower, lag_half_width=world["L"],
                              bin_half_width=world["B"], max_windows=W, max_channels=K)
    h.Start()
    try:
        code, carr = dpe.engine.bank_rows(banks.bcs[r], w0)
        h.Update(code, carr, banks.bw[r][w0:w0 + W], np.ascontiguousarray(banks.ce[r][w0:w0 + W, :n_chan]))
        out = dict(res=h.results(), split=h.last_split())
    finally:
        h.Stop()
    return out


def assert_own_is_single(own, s, where):
    """A receiver's own arg-max, score bits and counts in the joint launch are dpe_bcm_update's on that receiver alone."""
    for k in ("posIndex", "velIndex", "posOutOfWindow", "velOutOfWindow"):
        assert own[k] == s[k], (where, k, own[k], s[k])
    assert np.float32(own["posScore"]).tobytes() == np.float32(s["posScore"]).tobytes(), where
    assert np.float32(own["velScore"]).tobytes() == np.float32(s["velScore"]).tobytes(), where


def assert_key_is_first_maximum(out, w):
    for m, name, key in ((0, "pos", "posIndex"), (1, "vel", "velIndex")):
        row = out[name][w]
        at = int(np.argmax(row))
        k = int(out["keys"][w, m])
        assert 0xFFFFFFFF - (k & 0xFFFFFFFF) == at == out["res"][w][key], (w, name)
        assert k >> 32 == int(row[at].view(np.uint32)), (w, name)


def assert_twins(out, n):
    """Windows w and w % n had identical inputs: identical rows, keys, counts and per-receiver results."""
    for w in range(n, len(out["res"])):
        a, b = out["res"][w], out["res"][w % n]
        assert np.array_equal(bits(out["pos"][w]), bits(out["pos"][w % n])), w
        assert np.array_equal(bits(out["vel"][w]), bits(out["vel"][w % n])), w
        assert np.array_equal(out["keys"][w], out["keys"][w % n]), w
        assert (a["posOutOfWindow"], a["velOutOfWindow"]) == (b["posOutOfWindow"], b["velOutOfWindow"]), w
        for x, y in zip(a["rx"], b["rx"]):
            for k in ("posIndex", "velIndex", "posOutOfWindow", "velOutOfWindow", "posScore", "velScore"):
                assert x[k] == y[k], (w, k)


def probe(out, windows):
    """The windows of `out` as an output of their own (window i of the result is windows[i])."""
    return dict(res=[out["res"][w] for w in windows], pos=[out["pos"][w] for w in windows], vel=[out["vel"][w] for w in windows],
                keys=out["keys"][list(windows)])


def last_twins(world, W=W32):
    """The LAST window of the batch that carries each distinct window's inputs (the oracle is held against these, so a slip in
    a late window's row offset shows)."""
    n = world["W"]
    return [max(w for w in range(W) if w % n == d) for d in range(n)]


WALK = {"15x14": dict(pos_dim=15, vel_dim=14), "14x15": dict(pos_dim=14, vel_dim=15)}


@pytest.fixture(scope="module", params=sorted(WALK))
def walk(request):
    """Receivers (5, 8, 4), 32 windows from 2 distinct ones; grids 15^4 (49 full tiles + 449 points: blocks 0 and 1 walk three
    tiles, block 1 reaches the ragged tile by the even path) and 14^4 (37 full tiles + 528 points: block 13 reaches the ragged
    tile as its second tile, through the bufB -> bufA copy), and swapped."""
    world = jw.build((5, 8, 4), seed=3, W=2, **WALK[request.param])
    assert sorted((tiles(world["pos"].shape[0]), tiles(world["vel"].shape[0]))) == [38, 50]
    banks = Banks(world, W32)
    yield world, banks
    banks.close()


def test_batch_walk(walk, oracle):
    """J1."""
    world, banks = walk
    out = run_joint(world, banks.rx(), split=(24, 24))
    assert_twins(out, 2)
    singles = [run_single(world, banks, r) for r in range(3)]
    assert all(s["split"] == (24, 24) for s in singles)
    for w in range(W32):
        assert_key_is_first_maximum(out, w)
        assert out["res"][w]["posIndex"] == world["pos_at"] and out["res"][w]["velIndex"] == world["vel_at"], w
        for r in range(3):
            assert_own_is_single(out["res"][w]["rx"][r], singles[r]["res"][w], (w, r))
            assert out["res"][w]["rx"][r]["posIndex"] == world["pos_at"] and out["res"][w]["rx"][r]["velIndex"] == world["vel_at"]
    ref = jw.oracle_rows(world)
    pr = probe(out, last_twins(world))
    for d in range(2):
        check_against_oracle(world, pr, ref, d)


@pytest.mark.parametrize("widen", [True, False])
def test_capacity_strides_and_per_window_channel_sets(oracle, widen):
    """J2.  A handle of 8 receivers, 64 pairs, 40 windows and 10 channels per receiver, used with 3 receivers, 17 or 16 pairs
    and 32 windows (4 distinct): the device indexes with the capacities, the host indexes the caller's arrays with the use.  In
    odd windows the receivers are passed in rotated order and receiver 1 brings only its first 7 channels, so kOff differs
    between even and odd windows.  Each window against a tight handle given that window alone (bits), and every receiver's
    own arg-max and counts against dpe_bcm_update on the same channel subset.  Clean banks, and the narrow ones (non-zero
    counts per receiver).  The 7^4 grid is enough: the walk is test_batch_walk's."""
    world = jw.build((5, 8, 4), seed=7, W=4, widen=widen)
    banks = Banks(world, W32)
    try:
        def plan(w):
            return [(1, 7), (2, None), (0, None)] if w % 2 else [(0, None), (1, None), (2, None)]
        rx = banks.rx(plan=plan)
        out = run_joint(world, rx, caps=dict(max_rx=8, max_total=64, max_windows=40, max_channels=10), split=(3, 3))
        tight = [run_joint(world, banks.rx(windows=(w,), plan=plan)) for w in range(4)]
        singles = {(r, n): run_single(world, banks, r, n) for r, n in ((0, None), (1, None), (1, 7), (2, None))}
    finally:
        banks.close()
    assert_twins(out, 4)
    for w in range(W32):
        t = tight[w % 4]
        assert np.array_equal(bits(out["pos"][w]), bits(t["pos"][0])) and np.array_equal(bits(out["vel"][w]), bits(t["vel"][0])), w
        assert np.array_equal(out["keys"][w], t["keys"][0]), w
        assert_key_is_first_maximum(out, w)
        j = out["res"][w]
        assert (j["posOutOfWindow"], j["velOutOfWindow"]) == (t["res"][0]["posOutOfWindow"], t["res"][0]["velOutOfWindow"])
        assert j["posOutOfWindow"] == sum(x["posOutOfWindow"] for x in j["rx"]) and j["velOutOfWindow"] == sum(x["velOutOfWindow"] for x in j["rx"])
        for i, (r, n) in enumerate(plan(w)):
            assert_own_is_single(j["rx"][i], singles[(r, n)]["res"][w], (w, r))
            assert np.abs(j["rx"][i]["zVal"] - jw_moved(world, r, w % 4, j)).max() < 1e-6, (w, r)
        if widen:
            assert j["posIndex"] == world["pos_at"] and j["velIndex"] == world["vel_at"] and j["posOutOfWindow"] == 0
        else:
            assert all(x["posOutOfWindow"] > 0 and x["velOutOfWindow"] > 0 for x in j["rx"]), w


def jw_moved(world, r, d, j):
    """Receiver r's centre of distinct window d moved by the joint arg-max of result j."""
    from oracle import oracle as o
    win = world["rx"][r]["wins"][d]
    return o.make_meas(j["posIndex"], j["velIndex"], win["centre"], world["pos"], world["vel"], win["R"])[0]


def test_eight_receivers_sixty_four_pairs(oracle):
    """J3.  The handle's limits (the receiver loop is unrolled to 8; thread r < nRx reduces receiver r's keys) on the walk
    shape: oracle parity on the last window, all eight own keys against dpe_bcm_update, eight fixes per window."""
    world = jw.build((8,) * 8, seed=6, W=1, pos_dim=15, vel_dim=14)
    banks = Banks(world, W32)
    try:
        out = run_joint(world, banks.rx(), split=(24, 24))
        singles = [run_single(world, banks, r) for r in range(8)]
    finally:
        banks.close()
    assert_twins(out, 1)
    for w in range(W32):
        j = out["res"][w]
        assert len(j["rx"]) == 8 and j["posIndex"] == world["pos_at"] and j["velIndex"] == world["vel_at"]
        assert_key_is_first_maximum(out, w)
        for r in range(8):
            assert_own_is_single(j["rx"][r], singles[r]["res"][w], (w, r))
            assert j["rx"][r]["posIndex"] == world["pos_at"] and j["rx"][r]["velIndex"] == world["vel_at"]
            assert np.abs(j["rx"][r]["zVal"] - moved(world, r)).max() < 1e-6
    check_against_oracle(world, probe(out, [W32 - 1]), jw.oracle_rows(world))


def test_lpower_3_and_own_keys_off(walk, oracle):
    """J4.  The generic powf variant (LP == 0) on the walk shape against the oracle at test_lpower's 1e-5, and the same joint
    bits with and without the per-receiver keys."""
    world, banks = walk
    rx = banks.rx()
    on, off = run_joint(world, rx, lpower=3, split=(24, 24)), run_joint(world, rx, lpower=3, own=False, split=(24, 24))
    assert np.array_equal(bits(on["pos"]), bits(off["pos"])) and np.array_equal(bits(on["vel"]), bits(off["vel"]))
    assert np.array_equal(on["keys"], off["keys"]) and on["keys"].all()
    assert_twins(on, 2)
    for w in range(W32):
        assert_key_is_first_maximum(on, w)
        for r in range(3):
            assert off["res"][w]["rx"][r]["posIndex"] == -1 and on["res"][w]["rx"][r]["posIndex"] == world["pos_at"]
            assert np.array_equal(off["res"][w]["rx"][r]["zVal"], on["res"][w]["rx"][r]["zVal"])
    ref = jw.oracle_rows(world, lpower=3)
    pr = probe(on, last_twins(world))
    for d in range(2):
        check_against_oracle(world, pr, ref, d, tol=1e-5)


@pytest.fixture(scope="module", params=[True, False], ids=["clean", "narrow"])
def walk_banks(request):
    """J1's 15^4 / 14^4 shape with widened banks and with deliberately narrow ones (both manifolds clamp and recount)."""
    world = jw.build((5, 8, 4), seed=3, W=2, widen=request.param, **WALK["15x14"])
    assert (tiles(world["pos"].shape[0]), tiles(world["vel"].shape[0])) == (50, 38)
    banks = Banks(world, W32)
    yield world, banks, request.param
    banks.close()


@pytest.mark.parametrize("lpower", [1, 2, 3])
def test_walk_every_lpower_clean_and_clamped(walk_banks, oracle, lpower):
    """J4b.  Every (LPower, clamp) variant on the walk: 24 blocks walk 50 and 38 tiles (block 1 of the position manifold the
    tiles 1, 25 and the ragged 49; block 13 of the velocity manifold tile 13 and the ragged 37 through the copy).  Per receiver
    the own arg-max, score bits and out-of-window counts are dpe_bcm_update's on that receiver alone at the same power, the
    joint count is their sum, the joint key is the first maximum of the joint row; narrow banks count on both manifolds, clean
    ones on neither.  LPower 2 on clean banks is also held to the oracle at TOL (LPower 1: J1, LPower 3: J4)."""
    world, banks, widen = walk_banks
    out = run_joint(world, banks.rx(), lpower=lpower, split=(24, 24))
    assert_twins(out, 2)
    singles = [run_single(world, banks, r, lpower=lpower) for r in range(3)]
    assert all(s["split"] == (24, 24) for s in singles)
    assert np.isfinite(out["pos"]).all() and np.isfinite(out["vel"]).all()
    for w in range(W32):
        j = out["res"][w]
        assert_key_is_first_maximum(out, w)
        for r in range(3):
            assert_own_is_single(j["rx"][r], singles[r]["res"][w], (w, r))
        for k in ("posOutOfWindow", "velOutOfWindow"):
            assert j[k] == sum(x[k] for x in j["rx"]), (w, k)
            assert (j[k] > 0) == (not widen), (w, k, j[k])
        if widen:
            assert j["posIndex"] == world["pos_at"] and j["velIndex"] == world["vel_at"], w
    if widen and lpower == 2:
        ref = jw.oracle_rows(world, lpower=2)
        pr = probe(out, last_twins(world))
        for d in range(2):
            check_against_oracle(world, pr, ref, d)


def check_clamped_side(world, out, ref, d, name, rname_x, rows):
    """The narrow manifold of distinct window d (out: its probe) by test_narrow_banks_clamp_path_counts_per_receiver's rule."""
    G = ref[rname_x][d].size
    cmp_ = [(rname_x, TOL, 2 * len(rows))]
    flips = np.zeros(G, dtype=bool)
    if name == "pos":
        for r, x in enumerate(rows):
            f = np.abs(x["pos"] - x["pos_x"]) > 10 * helpers.POS_REF_NOISE * x["pos"].max()
            f[x["quirks"]] = False
            assert f.sum() <= 16 + G * world["rx"][r]["K"] // 2000
            flips |= f
        cmp_.append(("pos", helpers.POS_REF_NOISE, 0))
    for rname, lim, aside in cmp_:
        r_, g_ = ref[rname][d], out[name][d]
        dd = np.abs(g_ - r_) / r_.max()
        if rname == "pos":
            dd = dd[~flips]
        edge = np.argsort(-dd)[:aside]
        edge = edge[dd[edge] > 100 * lim]
        keep = np.ones(dd.size, dtype=bool)
        keep[edge] = False
        print("narrow %s banks, window %d, %s vs %s: rel err %.3g (bound %.3g), %d points set aside"
              % (name, d, name, rname, dd[keep].max(), lim, edge.size))
        assert dd[keep].max() < lim


@pytest.mark.parametrize("side", ["L", "B"])
def test_mixed_clamp_counts_across_tiles(walk, oracle, side):
    """J5.  Only the lag banks narrow (the position manifold clamps, <CLAMP_P, !CLAMP_V>), then only the bin banks: the
    per-receiver counts are summed over a block's tiles and equal the oracle's, the clean manifold counts nothing and meets the
    clean bounds on every point, the narrow one follows the existing narrow-bank caps."""
    base, _ = walk
    world = jw.build((5, 8, 4), seed=3, W=2, widen=side, pos_dim=base["dims"][0], vel_dim=base["dims"][1])
    assert world["pos"] is base["pos"] and (world["L"], world["B"]) == ((1, base["B"]) if side == "L" else (base["L"], 2))
    banks = Banks(world, W32)
    try:
        out = run_joint(world, banks.rx(), split=(24, 24))
    finally:
        banks.close()
    assert_twins(out, 2)
    ref = jw.oracle_rows(world)
    picks = last_twins(world)
    pr = probe(out, picks)
    narrow, clean = ("pos", "vel") if side == "L" else ("vel", "pos")
    for d in range(2):
        rows, j = ref["rx"][d], pr["res"][d]
        for r, x in enumerate(rows):
            own = j["rx"][r]
            print("window %d receiver %d: out of window pos %d (oracle %d, faithful %d), vel %d (oracle %d)"
                  % (d, r, own["posOutOfWindow"], x["oob_pos_x"], x["oob_pos"], own["velOutOfWindow"], x["oob_vel"]))
        for r, x in enumerate(rows):
            own = j["rx"][r]
            assert own["posOutOfWindow"] == x["oob_pos_x"] and own["velOutOfWindow"] == x["oob_vel"], (d, r)
            assert (x["oob_pos_x"] > 0) == (side == "L") and (x["oob_vel"] > 0) == (side == "B")
        assert j["posOutOfWindow"] == sum(x["oob_pos_x"] for x in rows) and j["velOutOfWindow"] == sum(x["oob_vel"] for x in rows)
        assert_key_is_first_maximum(pr, d)
        assert j["posIndex"] == int(np.argmax(ref["pos_x"][d])) and j["velIndex"] == int(np.argmax(ref["vel"][d]))
        # the clean manifold: every point, nothing set aside
        for rname, lim in ((("vel", TOL),) if clean == "vel" else (("pos_x", TOL), ("pos", helpers.POS_REF_NOISE))):
            r_, g_ = ref[rname][d], pr[clean][d]
            e = np.abs(g_ - r_).max() / r_.max()
            print("clean %s manifold, window %d, vs %s: rel err %.3g (bound %.3g)" % (clean, d, rname, e, lim))
            assert e < lim
        assert j["velIndex" if clean == "vel" else "posIndex"] == world["vel_at" if clean == "vel" else "pos_at"]
        check_clamped_side(world, pr, ref, d, narrow, "pos_x" if narrow == "pos" else "vel", rows)


@pytest.mark.parametrize("widen", [True, False])
def test_exact_ties_across_tiles(oracle, widen):
    """J6.  P = the first 24 * 1024 points of a 13^4 grid (the expected point is among them); the grids are P + P + P[:333]:
    49 tiles for 24 blocks, so the copy of a point sits 24 tiles on, in the same lane of the same block, and a third copy of
    the first 333 points in block 0's ragged third tile.  Copies score equal bits; the joint arg-max and every receiver's own
    name the FIRST copy; with narrow banks the counts are twice those of P plus those of P[:333], per receiver and jointly."""
    world = jw.build((5, 8, 4), seed=5, W=1, widen=widen, pos_dim=13, vel_dim=13)
    n, tail = 24 * TILE, 333
    assert world["pos_at"] < n and world["vel_at"] < n and world["pos_at"] >= TILE and world["vel_at"] >= TILE
    P, V = world["pos"][:n], world["vel"][:n]
    three = (np.concatenate([P, P, P[:tail]]), np.concatenate([V, V, V[:tail]]))
    banks = Banks(world, W32)
    try:
        rx = banks.rx()
        out = run_joint(world, rx, grids=three, split=(24, 24))
        one = run_joint(world, rx, grids=(P, V), split=(24, 24))
        end = run_joint(world, rx, grids=(P[:tail], V[:tail]), split=(1, 1))
        singles = [run_single(world, banks, r, grids=three) for r in range(3)]
    finally:
        banks.close()
    assert_twins(out, 1)
    for w in (0, 13, W32 - 1):
        for name in ("pos", "vel"):
            row = bits(out[name][w])
            assert np.array_equal(row[:n], row[n:2 * n]) and np.array_equal(row[2 * n:], row[:tail]), (w, name)
            assert np.array_equal(row[:n], bits(one[name][w])), (w, name)
    for w in range(W32):
        j = out["res"][w]
        assert_key_is_first_maximum(out, w)
        assert (j["posIndex"], j["velIndex"]) == (one["res"][w]["posIndex"], one["res"][w]["velIndex"])
        if widen:
            assert j["posIndex"] == world["pos_at"] and j["velIndex"] == world["vel_at"]
        assert out["pos"][w][j["posIndex"]] == out["pos"][w][j["posIndex"] + n]      # (the tie is there)
        for r in range(3):
            own = j["rx"][r]
            assert_own_is_single(own, singles[r]["res"][w], (w, r))
            assert (own["posIndex"], own["velIndex"]) == (one["res"][w]["rx"][r]["posIndex"], one["res"][w]["rx"][r]["velIndex"])
            assert own["posIndex"] < n and own["velIndex"] < n
            if widen:
                assert own["posIndex"] == world["pos_at"] and own["velIndex"] == world["vel_at"]
            for k in ("posOutOfWindow", "velOutOfWindow"):
                assert own[k] == 2 * one["res"][w]["rx"][r][k] + end["res"][w]["rx"][r][k], (w, r, k)
                assert (own[k] > 0) == (not widen)
        for k in ("posOutOfWindow", "velOutOfWindow"):
            assert j[k] == 2 * one["res"][w][k] + end["res"][w][k] == sum(x[k] for x in j["rx"]), (w, k)


def test_closed_loop_shape_unequal_splits_and_a_second_update(oracle):
    """J7.  One window, position grid 20^4 (157 tiles for the 128 blocks of a single window), velocity grid 7^4 (3 tiles):
    grid.x is 128 and 125 blocks of the velocity manifold only take the publish ticket.  Oracle parity on every point, own
    keys against the single scan; then a second Update on the same handle with another window gives what a fresh handle gives
    (the key sets alternate, the per-receiver keys are cleared under a stale larger state)."""
    world = jw.build((5, 8, 4), seed=4, W=2, pos_dim=20, vel_dim=7)
    assert (tiles(world["pos"].shape[0]), tiles(world["vel"].shape[0])) == (157, 3)
    banks = Banks(world, 2)
    kept = []
    try:
        first = run_joint(world, banks.rx(windows=(0,)), split=(128, 3), keep=kept)
        h = kept[0]
        second = update_joint(h, banks.rx(windows=(1,)), (128, 3))
        again = update_joint(h, banks.rx(windows=(0,)), (128, 3))
        fresh = run_joint(world, banks.rx(windows=(1,)), split=(128, 3))
        singles = [[run_single(world, banks, r, windows=(w,)) for r in range(3)] for w in range(2)]
    finally:
        for h in kept:
            h.Stop()
        banks.close()
    ref = jw.oracle_rows(world)
    for d, out in ((0, first), (1, second)):
        pr = dict(res=[None] * d + out["res"], pos=[None] * d + list(out["pos"]), vel=[None] * d + list(out["vel"]))
        check_against_oracle(world, pr, ref, d)
        assert_key_is_first_maximum(out, 0)
        for r in range(3):
            assert singles[d][r]["split"] == (128, 3)
            assert_own_is_single(out["res"][0]["rx"][r], singles[d][r]["res"][0], (d, r))
    for a, b in ((second, fresh), (again, first)):
        assert np.array_equal(bits(a["pos"]), bits(b["pos"])) and np.array_equal(bits(a["vel"]), bits(b["vel"]))
        assert np.array_equal(a["keys"], b["keys"])
        ja, jb = a["res"][0], b["res"][0]
        for k in ("posIndex", "velIndex", "posScore", "velScore", "posOutOfWindow", "velOutOfWindow"):
            assert ja[k] == jb[k], k
        for x, y in zip(ja["rx"], jb["rx"]):
            for k in ("posIndex", "velIndex", "posScore", "velScore", "posOutOfWindow", "velOutOfWindow"):
                assert x[k] == y[k], k
            assert x["zVal"].tobytes() == y["zVal"].tobytes()


def test_last_split_is_refused_before_the_first_update():
    world = jw.build((6,))
    h = dpe.JointManifold(world["fs"], world["S"], world["C"], world["pos"], world["vel"], 1, 6, lag_half_width=world["L"],
                          bin_half_width=world["B"], max_windows=1, max_channels=6)
    h.Start()
    try:
        with pytest.raises(dpe.DpeError, match="last_split: no Update yet"):
            h.last_split()
    finally:
        h.Stop()
