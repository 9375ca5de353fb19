"""bcm_scan_axes_kernel (csrc/dpe_bcm_axes.h) held to the point-list scan's standard.

The axes scan has its own tile walk (256 rows x one t-chunk of <= 16 entries, tiles row group major, a block walking every
split-th tile), its own index formula (B + g t), its own shard test, LDS score stage and fp32 weighted-sum accumulation.  Here:
- config R's batch shape (256 windows: 16 blocks per manifold, each walking ~8 tiles) against a point-list handle on every
  window, against the oracle on probe windows, and the exact invariants (own arg-max, key score bits, identical windows);
- exact first-maximum ties: copies of the maximal point across a chunk boundary, across row groups and inside one wave;
- grids shifted by whole rows and cut into shards anywhere: bit-identical score rows, keys, counts; weighted sums that add up;
- the weighted sums against fp64 sums of the written scores;
- a seeded random sweep of axes handles against the oracle (DPE_FUZZ_AXES_CASES, DPE_FUZZ_SEED);
- the widest banks create_axes admits at K = 37;
- the sharded device-resident loop on axes (dpe_flow --device-loop --grid-axes --ranks 2)."""
import os
import subprocess

import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import helpers

pytestmark = pytest.mark.gpu

TOL = 2e-6          # against the oracle's extended-precision index and the velocity scores (test_gpu_parity.py)


def _repeat(arrs, W):
    """Inputs of the case's windows dealt round-robin into W windows (window w is case window w % n)."""
    n = arrs[0].shape[0]
    return tuple(np.ascontiguousarray(np.concatenate([a] * ((W + n - 1) // n))[:W]) for a in arrs)


def _run(case, grids, L, B, W=None, lpower=1, write_scores=True, weighted_mean=True, point_list=False):
    """One BatchCorrScores + BatchCorrManifold pass over the case's windows (repeated to W) with the given grids
    (GridAxes, or point lists when point_list).  -> dict(res, pos, vel, keys, code, carr, idx_next, no_flip, mean)."""
    import torch
    iq, cs, ce, bw = helpers.pack_gpu_inputs(case)
    if W is not None:
        iq, cs, ce, bw = _repeat((iq, cs, ce, bw), W)
    W, K = cs.shape
    bcs = dpe.BatchCorrScores(case["fs"], samples_per_window=case["S"], lag_half_width=L, bin_half_width=B, max_windows=W,
                              max_channels=K)
    bcs.Start()
    bcs.Update(torch.from_numpy(iq).to("cuda:0"), cs)
    pos, vel = grids if not point_list else (grids[0].points(), grids[1].points())
    m = dpe.BatchCorrManifold(case["fs"], case["S"], bcs.NumFFTPoints, pos, vel, LPower=lpower, lag_half_width=L,
                              bin_half_width=B, max_windows=W, max_channels=K, write_scores=write_scores,
                              weighted_mean=weighted_mean)
    m.Start()
    m.Update(bcs.CodeScores, bcs.CarrScores, bw, ce)
    out = dict(res=m.results(), keys=dpe.engine.d2h(m.Keys, 16 * W, np.uint64).reshape(W, 2))
    if write_scores:
        out["pos"], out["vel"] = m.read_scores()
    code, carr = bcs.read_banks()
    out["idx_next"], out["no_flip"], out["mean"] = bcs.read_info()
    out["code"], out["carr"] = code, carr
    m.Stop(); bcs.Stop()
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_own_argmax(out, pos_off=0, vel_off=0):
    """Exact: the reported index is the FIRST maximum of the scores the kernel wrote, the reported score is that score's bits,
    and the key packs both (score bits, ~index)."""
    for w, r in enumerate(out["res"]):
        for name, key, sk, off, slot in (("pos", "posIndex", "posScore", pos_off, 0), ("vel", "velIndex", "velScore", vel_off, 1)):
            s = out[name][w]
            i = int(np.argmax(s))
            assert r[key] - off == i, "%s window %d: index %d, first maximum %d" % (name, w, r[key] - off, i)
            assert _bits(r[sk]) == _bits(s[i]), "%s window %d: reported score is not the written one" % (name, w)
            k = int(out["keys"][w, slot])
            assert k >> 32 == int(_bits(s[i])) and 0xFFFFFFFF - (k & 0xFFFFFFFF) == r[key], "%s window %d key" % (name, w)


def assert_matches_point_list(ax, pl):
    """Scores within 2e-6 of the maximum, an arg-max difference only as an fp32 tie (test_gpu_grid_axes.py's comparison)."""
    for w, (ra, rp) in enumerate(zip(ax["res"], pl["res"])):
        for name, key in (("pos", "posIndex"), ("vel", "velIndex")):
            a, p = ax[name][w], pl[name][w]
            assert np.abs(a - p).max() <= 2e-6 * p.max(), "%s scores window %d" % (name, w)
            if ra[key] != rp[key]:
                assert abs(p[ra[key]] - p[rp[key]]) <= 2e-6 * p.max(), "%s arg-max window %d" % (name, w)
        if ra["posIndex"] == rp["posIndex"] and ra["velIndex"] == rp["velIndex"]:
            assert np.array_equal(ra["zVal"], rp["zVal"])


def assert_identical_windows(out, n):
    """Windows w and w % n had identical inputs: identical scores, keys, out-of-window counts and weighted sums."""
    W = len(out["res"])
    for w in range(n, W):
        a, b = out["res"][w], out["res"][w % n]
        assert np.array_equal(out["keys"][w], out["keys"][w % n]), "keys window %d" % w
        assert (a["posOutOfWindow"], a["velOutOfWindow"]) == (b["posOutOfWindow"], b["velOutOfWindow"]), "counts window %d" % w
        assert np.array_equal(a["weightedSums"], b["weightedSums"]), "weighted sums window %d" % w
        if "pos" in out:
            assert np.array_equal(_bits(out["pos"][w]), _bits(out["pos"][w % n])), "pos scores window %d" % w
            assert np.array_equal(_bits(out["vel"][w]), _bits(out["vel"][w % n])), "vel scores window %d" % w


def _subset(out, windows):
    """The output dict of helpers.run_gpu for the given windows only (to pair with run_oracle(..., windows=...))."""
    sub = dict(res=[out["res"][w] for w in windows], idx_next=out["idx_next"][windows], no_flip=out["no_flip"][windows],
               mean=out["mean"][windows])
    for k in ("code", "carr", "pos", "vel"):
        if k in out:
            sub[k] = [out[k][w] for w in windows]
    return sub


def wsum_errors(out, grids):
    """Relative error of every window's weightedSums against fp64 sums over the scores the kernel wrote, with the axes as the
    device holds them (fp32): |ws_0 - sum s| / sum s and |ws_j - sum s c_j| / sum s |c_j| (the coordinate sums may cancel).
    -> [W, 2 manifolds, 5]."""
    err = np.zeros((len(out["res"]), 2, 5))
    for m, (name, ga) in enumerate(zip(("pos", "vel"), grids)):
        P = ga.points().astype(np.float32).astype(np.float64)
        A = np.abs(P)
        for w, r in enumerate(out["res"]):
            s = out[name][w].astype(np.float64)
            ref = np.concatenate([[s.sum()], s @ P])
            scale = np.concatenate([[s.sum()], s @ A])
            err[w, m] = np.abs(r["weightedSums"][m] - ref) / np.where(scale > 0, scale, 1.0)
    return err


# The per-lane fp32 accumulation of the weighted sums, measured on one MI355X as wsum_errors (worst over every window, manifold
# and component): 2.6e-9 at config R's shape (25^4 and spread grids, 256 windows, 16 blocks of ~8 tiles per window), 1.7e-9 on
# the 57^4 grid at W = 1 (128 blocks of ~23 tiles).  The bound keeps a margin of ~8; a block that dropped the sums of all but
# its last tile is off by ~0.9.
WSUM_TOL = 2e-8


# ---- 1. config R's batch shape on axes -------------------------------------------------------------------------------------
def _grids(name):
    if name == "uniform25":
        return dpe.GridAxes.uniform(25, 1.0), dpe.GridAxes.uniform(25, 1.0)
    return dpe.GridAxes.pygnss_spread()


@pytest.mark.parametrize("grid,L,B", [
    ("uniform25", 4, 20),
    ("spread", 4, 20),
    ("spread", 2, 6),          # banks narrower than the grids reach: both clamp variants, out-of-window pairs
])
def test_batch_shape_config_r(grid, L, B):
    """2.5 Msps, S = 50000, 8 SVs, 256 windows (16 distinct ones repeated): scan_split gives 16 blocks per manifold, each
    walking ~8 of the 124 tiles of a 25^4 grid, carrying its running maximum, weighted sums and counts across them.  Every
    window: the exact invariants, the point-list handle on the same banks, weightedSums against fp64 sums of the written
    scores (measured worst 2.6e-9 of sum s |c|, bound WSUM_TOL = 2e-8).  Probe windows 0, 100, 255: the oracle on the whole
    grid (every point, so every tile and chunk edge and the last row group) at test_gpu_parity.py's tolerances."""
    W, distinct = 256, 16
    grids = _grids(grid)
    case = helpers.make_case(seed=31, fs=2.5e6, S=50000, K=8, G=64, amp=48.0, W=distinct)
    case["pos"], case["vel"] = grids[0].points(), grids[1].points()
    ax = _run(case, grids, L, B, W=W)
    assert_own_argmax(ax)
    assert_identical_windows(ax, distinct)
    err = wsum_errors(ax, grids)
    print("weighted sums vs fp64, %s L=%d B=%d: worst %.3g (pos) %.3g (vel)" % (grid, L, B, err[:, 0].max(), err[:, 1].max()))
    assert err.max() < WSUM_TOL
    if L > 2:
        pl = _run(case, grids, L, B, W=W, point_list=True)
        assert_matches_point_list(ax, pl)
        del pl
    else:
        assert sum(r["posOutOfWindow"] + r["velOutOfWindow"] for r in ax["res"]) > 0
    # the oracle on the whole grid for probe windows (0, 100, 255 are case windows 0, 4, 15): scores, arg-max, counts,
    # weighted mean, at test_gpu_parity.py's tolerances
    probe = [0, 100, 255]
    assert [w % distinct for w in probe] == sorted({w % distinct for w in probe})   # run_oracle keeps the case's order
    ref = helpers.run_oracle(case, L, B, windows={w % distinct for w in probe})
    helpers.assert_parity(_subset(ax, probe), ref, tol=TOL)


# ---- 2. exact first-maximum ties -------------------------------------------------------------------------------------------
def _tie_grids():
    """17 x 16 x 16 x 33 grids (143616 points): a row group (256 rows) is one x entry, a row's 33 t entries are 3 chunks of 11.
    The centre (0, 0, 0, 0) is repeated on three axes: x at entries 4 and 12 (row groups 4 and 12: 8 groups = 24 tiles apart,
    the same lane of the same block when 24 blocks walk the 51 tiles), z at entries 3 and 9 (lanes 6 apart in one wave), t at
    entries 10 and 11 (the last slot of chunk 0 and the first of chunk 1).  With this case's banks the maximum of both
    manifolds sits on the 8 copies of the centre (checked below, so the test cannot silently stop testing ties)."""
    pos = dpe.GridAxes(np.array([-40, -30, -20, -10, 0, 10, 20, 30, -35, -25, -15, -5, 0, 5, 15, 25, 35], float) * 0.5,
                       (np.arange(16) - 7) * 2.5,
                       np.array([-20, -15, -10, 0, 5, 10, 15, 20, -17.5, 0, -12.5, -7.5, -2.5, 2.5, 7.5, 12.5]) * 0.5,
                       np.concatenate([np.arange(-10, 0) * 2.0, [0, 0], np.arange(1, 22) * 2.0]))
    vel = dpe.GridAxes(np.array([-8, -6, -4, -2, 0, 2, 4, 6, -7, -5, -3, -1, 0, 1, 3, 5, 7], float) * 0.25,
                       (np.arange(16) - 7) * 0.25,
                       np.array([-8, -6, -4, 0, 2, 4, 6, 8, -7, 0, -5, -3, -1, 1, 3, 5]) * 0.25,
                       np.concatenate([np.arange(-10, 0) * 0.25, [0, 0], np.arange(1, 22) * 0.25]))
    return pos, vel


def _canonical(ga):
    """For every point of the grid, the index of its first copy (each axis entry replaced by the first entry of equal value)."""
    first = []
    for a in ga.axes:
        _, inv = np.unique(a, return_inverse=True)
        f = np.full(inv.max() + 1, a.size)
        np.minimum.at(f, inv, np.arange(a.size))
        first.append(f[inv])
    idx = np.arange(ga.size)
    sub = np.unravel_index(idx, ga.dim)
    return np.ravel_multi_index(tuple(first[c][sub[c]] for c in range(4)), ga.dim)


@pytest.mark.parametrize("W", [1, 48])   # 1: inline parameters, 51 blocks of one tile; 48: 24 blocks walking 2 or 3 tiles each
def test_exact_ties_keep_the_first_maximum(W):
    grids = _tie_grids()
    case = helpers.make_case(seed=5, fs=2.5e6, S=50000, K=8, G=64, amp=200.0, W=min(W, 2))
    out = _run(case, grids, 4, 20, W=W)
    assert_own_argmax(out)
    for name, ga in zip(("pos", "vel"), grids):
        canon = _canonical(ga)
        for w in range(W):
            s = _bits(out[name][w])
            assert np.array_equal(s, s[canon]), "%s window %d: copies of a point score different bits" % (name, w)
            top = np.flatnonzero(out[name][w] == out[name][w].max())
            assert top.size == 8 and np.all(canon[top] == top[0]), "%s window %d: the maximum is not the repeated centre" % (name, w)
            key = "posIndex" if name == "pos" else "velIndex"
            assert out["res"][w][key] == top[0], "%s window %d: index %d, first maximal copy %d" % (name, w, out["res"][w][key], top[0])


# ---- 3. shifted and cut slices ---------------------------------------------------------------------------------------------
def _slice_grids(extra=0):
    """40 x 16 x 16 x 33 grids (337920 points, 10240 rows: 40 row groups x 3 chunks = 120 tiles), the x axis with `extra`
    entries prepended (the original grid is then the slice from extra * 16 * 16 * 33 on)."""
    rng = np.random.default_rng(3)
    pre = rng.uniform(-30, 30, extra)
    pos = dpe.GridAxes(np.concatenate([pre, np.linspace(-39, 39, 40)]), (np.arange(16) - 8) * 7.0, (np.arange(16) - 7.5) * 6.0,
                       (np.arange(33) - 16) * 9.0)
    vel = dpe.GridAxes(np.concatenate([pre / 10, (np.arange(40) - 20) * 0.3]), (np.arange(16) - 8) * 0.6, (np.arange(16) - 8) * 0.5,
                       (np.arange(33) - 16) * 0.2)
    return pos, vel


def _slice_case(W):
    case = helpers.make_case(seed=17, fs=2.5e6, S=50000, K=8, G=64, amp=200.0, W=min(W, 3))
    return case


L_CUT, B_CUT = 2, 6        # narrow banks: the 9 m / 7 m / 6 m steps reach past them, so the counts are not all zero


@pytest.mark.parametrize("W", [2, 48])
def test_shifted_grid_changes_only_the_index(W):
    """Prepending 3 x entries (3 x 16 x 16 = 768 rows) and scanning the slice that covers the original points: the same
    tiles relative to the slice, so scores, weighted sums and counts are bit-identical and the indices move by exactly the
    offset."""
    case = _slice_case(W)
    base = _slice_grids(0)
    shifted = _slice_grids(3)
    off = 3 * 16 * 16 * 33
    g = base[0].size
    a = _run(case, base, L_CUT, B_CUT, W=W)
    b = _run(case, (shifted[0].shard(off, off + g), shifted[1].shard(off, off + g)), L_CUT, B_CUT, W=W)
    assert_own_argmax(a)
    assert_own_argmax(b, off, off)
    for name in ("pos", "vel"):
        assert np.array_equal(_bits(a[name]), _bits(b[name]))
    for ra, rb in zip(a["res"], b["res"]):
        assert rb["posIndex"] == ra["posIndex"] + off and rb["velIndex"] == ra["velIndex"] + off
        assert (rb["posScore"], rb["velScore"]) == (ra["posScore"], ra["velScore"])
        assert (rb["posOutOfWindow"], rb["velOutOfWindow"]) == (ra["posOutOfWindow"], ra["velOutOfWindow"])
        assert np.array_equal(rb["weightedSums"], ra["weightedSums"])
    assert sum(r["posOutOfWindow"] + r["velOutOfWindow"] for r in a["res"]) > 0


# Shards' weighted sums added up against the whole grid's, relative to sum s |c| as wsum_errors: measured on one MI355X 1.7e-11
# at W = 2 and 1.0e-9 at W = 48 (the fp32 lane sums regroup where a shard edge cuts a tile); bound with a margin of 10.
SHARD_WSUM_TOL = 1e-8


def _cuts(G, seed):
    """Shard boundaries of a 10240-row x 33 grid: a start mid-chunk, a single point, a slice shorter than a row, boundaries on
    a chunk edge and a row edge, a single point and a short slice in the last row group (rows 9984 ...), and random cuts."""
    T = 33
    mine = [100 * T + 5, 100 * T + 6, 100 * T + 26, 300 * T + 11, 700 * T, 4000 * T + 17, 9990 * T + 3, 9990 * T + 4,
            10100 * T + 30, G - 7]
    rng = np.random.default_rng(seed)
    return sorted(set([0, G] + mine + [int(c) for c in rng.integers(1, G, 5)]))


@pytest.mark.parametrize("W", [2, 48])
def test_shards_add_up_to_the_whole_grid(W):
    """The grid cut into ~16 shards at the boundaries of _cuts: concatenated score rows bit-equal to the whole grid's, the max
    of the shards' keys equal to the whole grid's keys, counts that sum exactly, weighted sums that sum to the whole grid's
    within SHARD_WSUM_TOL (relative to sum s |c|, as wsum_errors)."""
    case = _slice_case(W)
    grids = _slice_grids(0)
    G = grids[0].size
    whole = _run(case, grids, L_CUT, B_CUT, W=W)
    cuts = _cuts(G, W)
    parts = []
    for b, e in zip(cuts[:-1], cuts[1:]):
        p = _run(case, (grids[0].shard(b, e), grids[1].shard(b, e)), L_CUT, B_CUT, W=W)
        for w, r in enumerate(p["res"]):   # a shard's own arg-max: first maximum of its rows, global index
            assert r["posIndex"] - b == int(np.argmax(p["pos"][w])) and r["velIndex"] - b == int(np.argmax(p["vel"][w]))
        parts.append(p)
    for name in ("pos", "vel"):
        assert np.array_equal(_bits(np.concatenate([p[name] for p in parts], axis=1)), _bits(whole[name]))
    assert np.array_equal(np.max(np.stack([p["keys"] for p in parts]), axis=0), whole["keys"])
    worst = 0.0
    for w, r in enumerate(whole["res"]):
        assert sum(p["res"][w]["posOutOfWindow"] for p in parts) == r["posOutOfWindow"]
        assert sum(p["res"][w]["velOutOfWindow"] for p in parts) == r["velOutOfWindow"]
        ws = np.sum([p["res"][w]["weightedSums"] for p in parts], axis=0)
        for m, name in enumerate(("pos", "vel")):
            s = whole[name][w].astype(np.float64)
            P = np.abs(grids[m].points())
            scale = np.concatenate([[s.sum()], s @ P])
            worst = max(worst, float((np.abs(ws[m] - r["weightedSums"][m]) / scale).max()))
    print("shards' weighted sums vs the whole grid's, W=%d: worst %.3g" % (W, worst))
    assert worst < SHARD_WSUM_TOL
    assert sum(r["posOutOfWindow"] + r["velOutOfWindow"] for r in whole["res"]) > 0


# ---- 4. weighted sums against fp64 -----------------------------------------------------------------------------------------
def test_weighted_sums_large_grid():
    """57^4 = 1.06e7 points at W = 1 (128 blocks, ~23 tiles of 256 rows x 15 t entries per block): each lane adds ~23 row sums
    of 15 scores in fp32.  weightedSums against fp64 sums of the written scores (wsum_errors): measured worst 1.7e-9 of
    sum s |c|, bound WSUM_TOL = 2e-8."""
    grids = (dpe.GridAxes.uniform(57, 1.0), dpe.GridAxes.uniform(57, 0.2))
    case = helpers.make_case(seed=9, fs=2.5e6, S=50000, K=8, G=64, amp=200.0, W=1)
    out = _run(case, grids, 4, 20)
    assert_own_argmax(out)
    err = wsum_errors(out, grids)
    print("weighted sums vs fp64, 57^4: %s (pos) %s (vel)" % (err[0, 0], err[0, 1]))
    assert err.max() < WSUM_TOL


# ---- 5. random sweep of axes handles ---------------------------------------------------------------------------------------
N_AXES = int(os.environ.get("DPE_FUZZ_AXES_CASES", "120"))
SEED = int(os.environ.get("DPE_FUZZ_SEED", "1234"))
ORACLE_BUDGET = 1.5e6       # grid points x SVs x oracle windows per manifold and case: the oracle stays ~1 s per case
LDS_BYTES = 150 * 1024 - 256 * 17 * 4   # create_axes: K (nEnt 16 + 32) bytes of banks beside the score stage


def _axis(rng, d, half):
    """d entries: uniform, or random (sorted or not), some of them duplicated."""
    u = rng.random()
    if u < 0.25 or d == 1:
        a = (np.arange(d) - (d - 1) / 2) * (2 * half / max(d - 1, 1))
    else:
        a = rng.uniform(-half, half, d)
        if u < 0.5:
            a.sort()
    if d > 1 and rng.random() < 0.4:
        n = int(rng.integers(1, max(2, d // 3)))
        a[rng.integers(0, d, n)] = a[rng.integers(0, d, n)]
    return a


def _dims(rng):
    d = [int(rng.integers(1, 41)) for _ in range(3)]
    t = int(rng.choice([1, 2, 15, 16, 17, 31, 32, 33, 34, int(rng.integers(1, 301))]))
    return d + [t]


def _fit(dims, budget):
    """Shrink the largest axis until the grid fits the oracle budget."""
    dims = list(dims)
    while int(np.prod(dims)) > budget:
        c = int(np.argmax(dims))
        dims[c] = max(1, dims[c] * 2 // 3)
    return dims


def draw_axes(i):
    rng = np.random.Generator(np.random.PCG64((SEED + 31) * 100003 + i))
    fs = float(rng.choice([2.046e6, 2.5e6, 4.0e6, 5.0e6]))
    S = 2 * int(rng.integers(1024, 15001))
    if rng.random() < 0.25:
        S = int(rng.choice([8192, 16384, 12500, 25000, 50000]))
    K = int(rng.choice([1, 2, 3, 5, 8, 12, 20, 37, int(rng.integers(1, 38))]))
    W = int(rng.choice([1, 2, 3, 5, 8, 48]))
    Wd = min(W, 3)            # distinct windows (the oracle scores these); a batch repeats them
    budget = ORACLE_BUDGET / (K * Wd)
    pdim, vdim = _fit(_dims(rng), budget), _fit(_dims(rng), budget)
    need_L = int(np.ceil(140.0 / 299792458.0 * fs)) + 2
    L = max(need_L, int(rng.choice([need_L, need_L + 1, 8, 16, 17, 32, 33, 40])))
    C = 8 * (1 << int(np.ceil(np.log2(S))))
    b_max = int(np.floor((720 * 2e-7) ** (1.0 / 6.0) * C / (2 * np.pi * 127.5) * 0.999))
    B = min(int(rng.choice([12, 20, 32, 33, 64, b_max])), b_max)
    lpower = int(rng.choice([1, 1, 2, 3]))
    u = rng.random()
    if u < 0.2:                # banks narrower than the grids reach: the clamped variants
        L, B = int(rng.integers(1, 3)), min(B, int(rng.integers(1, 3)))
    offset = None
    if rng.random() < 0.3:     # grid centre away from the truth (ENU metres, clock metres)
        offset = [float(v) for v in rng.uniform(-40.0, 40.0, 4)]
        L = L if u < 0.2 else max(L, need_L + int(np.ceil(70.0 / 299792458.0 * fs)))
    h = ((LDS_BYTES // K - 32) // 16 - 1) // 2          # widest max(L, B) the axes scan's LDS takes at this K
    L, B = min(L, h), min(B, h)
    pos_axes = [_axis(rng, d, 45.0) for d in pdim[:3]] + [_axis(rng, pdim[3], 40.0)]
    vel_axes = [_axis(rng, d, 6.0) for d in vdim[:3]] + [_axis(rng, vdim[3], 3.0)]
    shard = []
    for dims in (pdim, vdim):
        G = int(np.prod(dims))
        if G > 1 and rng.random() < 0.35:
            b = int(rng.integers(0, G - 1))
            shard.append((b, int(rng.integers(b + 1, G + 1))))
        else:
            shard.append(None)
    ws, wm = bool(rng.random() < 0.8), bool(rng.random() < 0.5)
    return dict(seed=7000 + i, fs=fs, S=S, K=K, W=W, Wd=Wd, L=L, B=B, lpower=lpower, offset=offset, pos_axes=pos_axes,
                vel_axes=vel_axes, shard=shard, write_scores=ws, weighted_mean=wm, amp=float(rng.choice([48.0, 200.0])))


@pytest.mark.parametrize("i", range(N_AXES))
def test_random_axes_case(i):
    p = draw_axes(i)
    try:
        grids = []
        for axes, sh in zip((p["pos_axes"], p["vel_axes"]), p["shard"]):
            ga = dpe.GridAxes(*axes)
            grids.append(ga.shard(*sh) if sh else ga)
        case = helpers.make_case(seed=p["seed"], fs=p["fs"], S=p["S"], K=p["K"], G=4, amp=p["amp"], W=p["Wd"],
                                 center_offset=p["offset"])
        case["pos"], case["vel"] = grids[0].points(), grids[1].points()
        out = _run(case, grids, p["L"], p["B"], W=p["W"], lpower=p["lpower"], write_scores=p["write_scores"],
                   weighted_mean=p["weighted_mean"])
        po, vo = grids[0].begin, grids[1].begin
        if p["write_scores"]:
            assert_own_argmax(out, po, vo)
        assert_identical_windows(out, p["Wd"])
        sub = _subset(out, list(range(p["Wd"])))
        sub["res"] = [dict(r, posIndex=r["posIndex"] - po, velIndex=r["velIndex"] - vo) for r in sub["res"]]
        ref = helpers.run_oracle(case, p["L"], p["B"], lpower=p["lpower"])
        helpers.assert_parity(sub, ref, tol=float(os.environ.get("DPE_FUZZ_TOL", "2e-5")), pos_ref_noise=3e-4,
                              check_scores=p["write_scores"])
    except Exception:
        q = dict(p, pos_axes=[a.size for a in p["pos_axes"]], vel_axes=[a.size for a in p["vel_axes"]])
        print("axes fuzz case %d: %r" % (i, q))
        raise


# ---- 6. the widest banks create_axes admits ----------------------------------------------------------------------------------
@pytest.mark.parametrize("S,L,B,tol", [
    (20000, 113, 20, 2e-5),    # lag windows beyond +-32: the boundary-difference bank kernel, test_gpu_fuzz.py's tolerance
    (50000, 4, 113, TOL),
])
def test_widest_banks_at_37_svs(S, L, B, tol):
    """K = 37 and max(L, B) = 113: 37 (227 x 16 + 32) + 17408 = 152976 bytes of the 153600 create_axes admits (114 is
    refused: test_grid_axes_cpu.py).  Oracle parity on a 5 x 6 x 7 x 17 grid, one window and a batch of 3."""
    grids = (dpe.GridAxes.uniform((5, 6, 7, 17), (9.0, 8.0, 7.0, 5.0)), dpe.GridAxes.uniform((7, 6, 5, 17), (0.7, 0.6, 0.5, 0.3)))
    for W in (1, 3):
        case = helpers.make_case(seed=50 + W, fs=2.5e6, S=S, K=37, G=4, amp=200.0, W=W)
        case["pos"], case["vel"] = grids[0].points(), grids[1].points()
        out = _run(case, grids, L, B)
        assert_own_argmax(out)
        helpers.assert_parity(out, helpers.run_oracle(case, L, B), tol=tol)


# ---- 7. the sharded device-resident loop on axes ---------------------------------------------------------------------------
def test_sharded_device_loop_on_axes_equals_the_unsharded_point_list_loop(tmp_path):
    """dpe_flow --device-loop --grid-axes --ranks 2 --comm files (two ranks on one GPU, each scanning its slice of the axes,
    keys all-reduced (MAX) through the host-file transport, the measurement kernel decoding the arg-max from the axes) against
    the unsharded --device-loop run with point lists: the same X rows (test_flow_grid_axes' comparison)."""
    from tests.test_gpu_comm import _inputs
    W = 12
    dat, ho = _inputs(tmp_path, W)
    exe = os.path.join(os.path.dirname(dpe.engine.LIB_PATH), "dpe_flow")
    base = [exe, "--samples", dat, "--handoff", ho, "--iters", str(W), "--grid-dim", "9", "--spacing", "1.0", "--init-delta", "2", "-1", "1", "3",
            "--device-loop", "--fix-lag", "3"]
    full = str(tmp_path / "X_dev.csv")
    subprocess.check_call(base + ["--out", full], timeout=200)
    ref = np.loadtxt(full, delimiter=",")
    assert ref.shape == (W, 8)
    rdv = str(tmp_path / "rdv")
    os.makedirs(rdv)
    outs = [str(tmp_path / ("X_axes_rank%d.csv" % r)) for r in range(2)]
    procs = [subprocess.Popen(base + ["--grid-axes", "--out", outs[r], "--ranks", "2", "--rank", str(r), "--rendezvous", rdv,
                                      "--comm", "files"], stderr=subprocess.PIPE, text=True) for r in range(2)]
    for p in procs:
        _, err = p.communicate(timeout=300)
        assert p.returncode == 0, err[-2000:]
    for o in outs:
        rows = np.loadtxt(o, delimiter=",")
        assert rows.shape == ref.shape and np.abs(rows - ref).max() < 1e-6
