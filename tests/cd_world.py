"""The worlds of the collective-detection tests (tests/test_cd_world_cpu.py, tests/test_gpu_cd.py).

Geometry: the handoff fixture's eight PRNs and ephemerides, its X_ECEF as the truth, its rxTime as the (exact) receive time of the
window's first sample.  One 10 ms window at 2.5 Msps (S = 25 000, M = 2 500) from synth.gen_iq without nav-bit flips: every SV's code
phase and carrier frequency are what cd_ref.predict gives AT THE TRUTH, plus one common delay M_TRUE (the sub-millisecond part of the
receive time, whole samples) and one common Doppler offset J_TRUE bins (the receiver clock's drift).  The a-priori position p0 lies
P0_OFFSET_ENU (about 2.6 km) from the truth; the grid is a horizontal lattice of 150 m about p0, shifted so that the truth is one of
its points (TRUE_POINT).

Two noise levels: noiseless (sigma = 0), and the weak level WEAK_CN0 -- chosen once, on the CPU, by stepping down from 40 dB-Hz in
1 dB steps (choose_weak_level below) to the first level at which the oracle's per-PRN acquisition (coherent, the reference's mode 0)
reports `found` for at most half of the SVs while the reference's collective arg-max is still the truth point with a top-two margin
between distinct points of at least ten times the GPU tolerance.  Level and seed are recorded here; tests/test_cd_world_cpu.py
asserts the three conditions."""
import functools

import numpy as np

import navlab_dpe_sdr_amd as dpe
from tests import cd_ref, helpers

FS, S, M = 2.5e6, 25000, 2500
SIGMA = 300.0
M_TRUE, J_TRUE = 777, 1
P0_OFFSET_ENU = (-2100.0, 1500.0, -40.0)     # p0 - truth, in the ENU frame at p0
RADIUS, STEP, J = 3000.0, 150.0, 2
NOISELESS_AMP = 200.0
WEAK_CN0, WEAK_SEED = 34.0, 20261020        # dB-Hz; see choose_weak_level


def bins():
    from oracle import oracle as o
    return o.acq_bins(coherent=True)         # 125 bins of 100 Hz


@functools.lru_cache(maxsize=None)
def geometry():
    """-> dict: ho, prns, eph, rx_time, truth, p0, R [3, 3], grid [P, 3], true_point, sv_true (predictions at the truth),
    sv (predictions at p0, rows 0..7)."""
    from oracle import oracle as o
    ho = dpe.handoff.read_handoff(helpers.HANDOFF)
    truth = ho["X_ECEF"][:3].copy()
    # p0: the point whose own ENU frame sees the truth at -P0_OFFSET_ENU (two rounds: the frame turns by 4e-4 rad over 2.6 km)
    p0 = truth.copy()
    for _ in range(3):
        p0 = truth + dpe.synth.enu2ecef_matrix(p0) @ np.asarray(P0_OFFSET_ENU)
    R = dpe.synth.enu2ecef_matrix(p0)
    d_true = R.T @ (truth - p0)
    lattice = dpe.synth.enu_disc_grid(RADIUS, STEP)
    near = int(np.argmin(((lattice[:, :2] - d_true[None, :2]) ** 2).sum(1)))
    grid = lattice + (d_true - lattice[near])[None, :]
    grid[near] = d_true
    prns = [int(p) for p in ho["prn_list"]]
    b = bins()
    kw = dict(fs=FS, M=M, bin_start=float(b[0]), bin_step=float(b[1] - b[0]))
    rows = list(range(len(prns)))
    sv_true = cd_ref.predict(o, ho["eph"], prns, rows, truth, ho["rxTime"], **kw)
    sv = cd_ref.predict(o, ho["eph"], prns, rows, p0, ho["rxTime"], **kw)
    return dict(ho=ho, prns=prns, eph=ho["eph"], rx_time=float(ho["rxTime"]), truth=truth, p0=p0, R=R, grid=grid, true_point=near,
                sv_true=sv_true, sv=sv)


def channels():
    """synth.gen_iq's channel dict for the window, and each SV's true delay in samples (fractional, [0, M))."""
    g = geometry()
    delay = np.array([np.mod(s["delay0"] + M_TRUE, M) for s in g["sv_true"]])
    fi = np.array([s["doppler_hz"] for s in g["sv_true"]]) + J_TRUE * 100.0
    rng = np.random.Generator(np.random.PCG64(5))
    K = len(g["prns"])
    ch = dict(prn=np.array(g["prns"], dtype=np.int32), rc=np.mod(cd_ref.L_CA - delay / FS * cd_ref.F_CA, cd_ref.L_CA), ri=rng.uniform(0, 1, K),
              fc=cd_ref.F_CA + (cd_ref.F_CA / cd_ref.F_L1) * fi, fi=fi, cp=np.full(K, 1000, dtype=np.int32),
              cp_ref=np.full(K, 1000, dtype=np.int32))
    return ch, delay


@functools.lru_cache(maxsize=None)
def window(cn0=None, seed=WEAK_SEED):
    """int16 I/Q [2 S].  cn0 None: noiseless at NOISELESS_AMP; else every SV at that C/N0 against SIGMA."""
    ch, _ = channels()
    if cn0 is None:
        return dpe.synth.gen_iq(seed, FS, S, ch, amp=NOISELESS_AMP, sigma=0.0, dc=(0.0, 0.0), flip=np.zeros(len(ch["prn"]), dtype=bool))
    amp = float(dpe.synth.cn0_to_amp(cn0, SIGMA, FS))
    return dpe.synth.gen_iq(seed, FS, S, ch, amp=amp, sigma=SIGMA, dc=(0.0, 0.0), flip=np.zeros(len(ch["prn"]), dtype=bool))


@functools.lru_cache(maxsize=None)
def oracle_acq(cn0=None, seed=WEAK_SEED):
    """The oracle's coarse acquisition of every PRN on the window: (surface float32 [K, 125, M], list of its result dicts)."""
    from oracle import oracle as o
    iq = window(cn0, seed)
    res = [o.coarse_acquisition(iq, FS, p, bins(), coherent=True, wrap_mask=True) for p in geometry()["prns"]]
    surf = np.stack([r["surface"] for r in res]).astype(np.float32)
    return surf, res


@functools.lru_cache(maxsize=None)
def reference(cn0=None, seed=WEAK_SEED):
    """cd_ref.scan of the oracle's surfaces over the world's grid."""
    g = geometry()
    surf, _ = oracle_acq(cn0, seed)
    return cd_ref.scan(surf, g["sv"], g["p0"], g["R"], g["grid"], FS, J)


SUBSET_ROWS = (7, 5, 4, 3, 1, 0)             # six of the eight PRNs, reversed: rows that differ from 0..K-1


def subset():
    """(prns, eph, sv) of the permuted-subset tests: the PRNs of SUBSET_ROWS in that order, their ephemerides, and the predictions
    at p0 with `row` each one's place among the world's eight."""
    g = geometry()
    rows = list(SUBSET_ROWS)
    return [g["prns"][r] for r in rows], np.asarray(g["eph"])[rows], [g["sv"][r] for r in rows]


def weak_conditions(cn0=WEAK_CN0, seed=WEAK_SEED):
    """(SVs the oracle's per-PRN acquisition reports found, collective arg-max point, top-two margin between distinct points,
    ten times the GPU tolerance at that score)."""
    _, res = oracle_acq(cn0, seed)
    ref = reference(cn0, seed)
    return sum(int(r["found"]) for r in res), ref["point"], ref["point_margin"], 10.0 * cd_ref.TOL * max(ref["score"], ref["row_max"])


def choose_weak_level(seed=WEAK_SEED):
    """How WEAK_CN0 was chosen: the first level, stepping down from 40 dB-Hz by 1 dB, that meets the three conditions."""
    g = geometry()
    for cn0 in np.arange(40.0, 19.0, -1.0):
        found, point, margin, need = weak_conditions(float(cn0), seed)
        if found <= len(g["prns"]) // 2 and point == g["true_point"] and margin >= need:
            return float(cn0)
    return None


# ---- injected random surfaces (uniform [0, 1) fp32, seeded): the parity cases of tests/test_gpu_cd.py, each the smallest shape that
# takes one of the scan's paths.  name: (M, K, P, J, seed)
RANDOM_CASES = {
    "lds-2500-k8": (2500, 8, 49, 2, 1),              # the flagship row length, rows staged in LDS
    "lds-2046-k4-j32-walk": (2046, 4, 131, 32, 2),   # M no multiple of 64 or of the run; 15 blocks per j walk 9 points: two key flushes
    "lds-2046-k1-wide": (2046, 1, 1031, 0, 3),       # more points than blocks at J = 0 (1024): a block walks two
    "lds-2500-k1": (2500, 1, 5, 0, 4),
    "l2-5000-k8": (5000, 8, 5, 2, 5),                # 8 rows of 5 005 floats exceed a block's LDS: rows read from L2
    "l2-5000-k16": (5000, 16, 49, 0, 6),
    "l2-2500-k16": (2500, 16, 1, 2, 7),              # 16 rows of 2 505 floats: 160 320 B, just above
}
RANDOM_BIN_STEP = 500.0


def _generate(M, K, P, J, seed, bins="edge", plant=0, surface="uniform", grid="random", delays="edge"):
    """The generator behind random_case and new_case.  The defaults are RANDOM_CASES' form and draw in its order.  The options:
    bins "interior": every SV's bin is drawn so that b_k +- J stays inside the raster (k = 0, 1, 2 included);
    plant -1 / +1: the surface is multiplied by 4 along [row_k, b_k + plant J, :] for every SV whose bin is inside the raster there;
    surface "uniform" [0, 1), "zeros", "ones", "ternary" (values of {0, 0.5, 1}), "exp2" (squared exponential times 1e9);
    grid "random" (with the three fixed points), "origin" (every point (0, 0, 0)), "repeat3" (the first P / 3 points three times over);
    delays "edge" (within a sample of 0 and of M, the rest uniform), "whole" (whole numbers, 0 and M - 1 among them)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n_bins = 2 * J + 9
    p0 = dpe.handoff.read_handoff(helpers.HANDOFF)["X_ECEF"][:3].copy()
    R = dpe.synth.enu2ecef_matrix(p0)
    rows = rng.permutation(K + 1)[:K]
    sv = []
    for k in range(K):
        az, el, rg = rng.uniform(0, 2 * np.pi), np.radians(rng.uniform(10.0, 90.0)), rng.uniform(2.0e7, 2.5e7)
        d = rg * np.array([np.cos(el) * np.sin(az), np.cos(el) * np.cos(az), np.sin(el)])
        if delays == "whole":
            delay0 = float((0, M - 1)[k]) if k < 2 else float(rng.integers(0, M))
        else:
            delay0 = (0.3, M - 0.4)[k] if k < 2 else float(rng.uniform(0, M))
        if bins == "interior":
            bin0 = float(rng.uniform(J, n_bins - 1 - J))
        else:
            bin0 = (0.4, n_bins - 1 - 0.3, 2.5)[k] if k < 3 else float(rng.uniform(J, n_bins - 1 - J))
        sv.append(dict(prn=k + 1, row=int(rows[k]), sat=p0 + R @ d, delay0=delay0, bin0=bin0))
    if grid == "origin":
        pts = np.zeros((P, 3))
    else:
        n = P // 3 if grid == "repeat3" else P
        pts = np.concatenate([rng.uniform(-3000.0, 3000.0, (n, 2)), rng.uniform(-50.0, 50.0, (n, 1))], axis=1)
        far = 0.999 * 0.5 * RANDOM_BIN_STEP / cd_ref.DOPPLER_HZ_PER_KM * 1000.0
        for i, d in enumerate(([0.0, 0.0, 0.0], [3000.0, 0.0, 0.0], [far * 0.6, -far * 0.8, 0.0])[:n]):
            pts[i] = d
        if grid == "repeat3":
            pts = np.concatenate([pts, pts, pts])
    shape = (K + 1, n_bins, M)
    if surface == "uniform":
        surf = rng.random(shape, dtype=np.float32)
    elif surface == "exp2":
        surf = (rng.standard_exponential(shape) ** 2 * 1.0e9).astype(np.float32)
    elif surface == "ternary":
        surf = (rng.integers(0, 3, shape) * 0.5).astype(np.float32)
    else:
        surf = np.full(shape, {"zeros": 0.0, "ones": 1.0}[surface], dtype=np.float32)
    if plant:
        for s, b in zip(sv, cd_ref.bins_of(sv) + plant * J):
            if 0 <= b < n_bins:
                surf[s["row"], b, :] *= np.float32(4.0)
    bin_hz = -1000.0 + RANDOM_BIN_STEP * np.arange(n_bins)
    ref = cd_ref.scan(surf, sv, p0, R, pts, FS, J)
    return dict(surface=surf, sv=sv, p0=p0, R=R, grid=pts, fs=FS, J=J, M=M, K=K, P=P, bins=bin_hz, ref=ref)


@functools.lru_cache(maxsize=None)
def random_case(name):
    """-> dict(surface fp32 [K + 1, nBins, M], sv, p0, R, grid, fs, J, bins, ref = cd_ref.scan of it).  SV 0 has delay0 within a
    sample of 0 and its bin at the raster's low edge, SV 1 delay0 within a sample of M and its bin at the high edge (so some (k, j)
    leave the raster whenever J > 0), SV 2 a bin0 of exactly 2.5 (half to even: 2).  Point 0 is p0 itself, point 1 lies 3 km east,
    point 2 at 0.999 of the largest distance create accepts for the bin step."""
    return _generate(*RANDOM_CASES[name])


# ---- the second table: what RANDOM_CASES' seven shapes leave undecided (tests/test_cd_world_cpu.py asserts of each case what it is
# here for).  name: ((M, K, P, J, seed), generator options)
DRIFT_CASES = {                                       # the drift axis decides: a wrong bin row, a wrong jj or a wrong SV dropped shows
    "interior-2500-k8": ((2500, 8, 49, 2, 31), dict(bins="interior")),
    "interior-2046-k4-j32": ((2046, 4, 131, 32, 32), dict(bins="interior")),
    "interior-l2-5000-k8": ((5000, 8, 5, 2, 33), dict(bins="interior")),
    "plant-minus-2500-k8": ((2500, 8, 9, 2, 25), dict(plant=-1)),
    "plant-plus-2500-k8": ((2500, 8, 9, 2, 25), dict(plant=+1)),
    "plant-minus-l2-2500-k16": ((2500, 16, 3, 2, 26), dict(plant=-1)),
}
TIE_CASES = {                                         # every point (0, 0, 0), whole delays, values of {0, 0.5, 1}: exact ties
    "tie-250-zeros": ((250, 2, 40, 2, 41), dict(surface="zeros", grid="origin", delays="whole")),
    "tie-250-ones": ((250, 2, 40, 2, 42), dict(surface="ones", grid="origin", delays="whole")),
    "tie-250-ternary": ((250, 2, 40, 2, 43), dict(surface="ternary", grid="origin", delays="whole")),
    "tie-2561-zeros": ((2561, 3, 40, 32, 44), dict(surface="zeros", grid="origin", delays="whole")),
    "tie-2561-ones": ((2561, 3, 40, 32, 45), dict(surface="ones", grid="origin", delays="whole")),
    "tie-2561-ternary": ((2561, 3, 40, 32, 46), dict(surface="ternary", grid="origin", delays="whole")),
}
SHAPE_CASES = {
    "repeat-2046-k4-j32": ((2046, 4, 60, 32, 10), dict(grid="repeat3")),    # 20 offsets three times over: blocks and flush slots differ
    "k3": ((250, 3, 9, 1, 11), {}),                   # the remainder of the SV loop unrolled by four: K mod 4 = 3 (3, 7), 1 (5, 13);
                                                      # K mod 4 = 2 in the K = 2 cases below
    "k5": ((250, 5, 9, 1, 12), {}),
    "k7": ((250, 7, 9, 1, 13), {}),
    "k13": ((250, 13, 9, 1, 14), {}),
    "lds-4092-k2": ((4092, 2, 5, 1, 15), {}),         # 819 runs: a lane of the LDS form takes a second one
    "lds-32768-k1": ((32768, 1, 3, 0, 16), {}),       # the M maximum: 6 554 runs, 13 passes, 131 092 B
    "lds-2475-k16": ((2475, 16, 3, 0, 17), {}),       # 16 x 2 480 x 4 = 158 720 B: the LDS limit itself
    "l2-2476-k16": ((2476, 16, 3, 0, 18), {}),        # 158 784 B: its other side
    "lds-4955-k8": ((4955, 8, 3, 0, 19), {}),         # 8 x 4 960 x 4 = 158 720 B
    "runs-512": ((2560, 2, 5, 1, 20), {}),            # exactly one run per lane
    "runs-513": ((2561, 2, 5, 1, 21), {}),            # a second pass of one lane
    "m-16": ((16, 2, 9, 2, 22), {}),                  # the M minimum: 4 runs, seven of eight waves without one
    "walk-20": ((64, 2, 289, 32, 23), {}),            # 15 blocks per j walk 19 or 20 points: a flush slot is used three times
    "walk-64": ((16, 1, 65536, 0, 24), {}),           # the P maximum: 1 024 blocks walk 64 points
    "dynamic-range": ((2500, 8, 9, 2, 27), dict(surface="exp2")),
}
NEW_CASES = {**DRIFT_CASES, **TIE_CASES, **SHAPE_CASES}
PARITY_CASES = {**DRIFT_CASES, **SHAPE_CASES}         # judged by tests/cd_checks.py check_parity; the tie cases by exact equality


@functools.lru_cache(maxsize=None)
def new_case(name):
    """random_case's dict for a case of NEW_CASES."""
    shape, opts = NEW_CASES[name]
    return _generate(*shape, **opts)


def any_case(name):
    return random_case(name) if name in RANDOM_CASES else new_case(name)


def tolerance(ref):
    """Per point: TOL max(score, row maximum)."""
    return cd_ref.TOL * np.maximum(ref["map_score"], ref["row_max"])
