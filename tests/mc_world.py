"""The Monte-Carlo world of tests/test_monte_carlo_cpu.py and tests/test_gpu_monte_carlo.py: one shape, one seed, two C/N0 levels far
apart, and the oracle's answer for every realisation (computed once per process and shared).

S = 12 500, K = 4, two 8^4-point grids, 16 realisations per level.  The manifold interpolates the sample-rate correlation linearly,
so a score's maxima sit on its nodes (scripts/monte_carlo.py): a +-12 m grid about the centre sees one node only and its ML fix never
moves.  Here the position grid spans -90 .. +120 m in steps of 30 m, and the grid's centre is put 30 .. 60 m from the truth so that the
truth is the grid point (2, 5, 3, 4) and not the centre: the replica is aligned with the truth, that point is the node, and every
other point loses correlation in proportion to its line-of-sight offset (120 m per sample at 2.5 Msps).  The velocity grid (2 m/s
steps) keeps its centre on the truth."""
import functools

import numpy as np

import navlab_dpe_sdr_amd as dpe
from tests import helpers, syn_ref

FS, S, K, N_REAL, SEED, SIGMA = 2.5e6, 12500, 4, 16, 20261020, 300.0
LEVELS = (55.0, 25.0)          # dB-Hz: amplitude 151 and 4.8 against sigma = 300
POS = dpe.synth.uniform_grid(8, 30.0)
VEL = dpe.synth.uniform_grid(8, 2.0)
TRUE_POINT = (2, 5, 3, 4)      # axis entries 30 (i - 3): the truth lies at (-30, 60, 0, 30) m from the centre
CENTRE_OFFSET = (30.0, -60.0, 0.0, -30.0)      # centre - truth in the local ENU frame and the clock, m
L, B = 8, 32


def true_index():
    i = TRUE_POINT
    return ((i[0] * 8 + i[1]) * 8 + i[2]) * 8 + i[3]


def init_delta():
    """CENTRE_OFFSET as pipeline.run_monte_carlo takes it: added to X_ECEF (ECEF metres, then the clock)."""
    from oracle import oracle as o
    ho = dpe.handoff.read_handoff(helpers.HANDOFF)
    R0 = o.enu2ecef(o.ecef2ll(ho["X_ECEF"])).reshape(3, 3)
    return np.concatenate([R0 @ np.asarray(CENTRE_OFFSET[:3]), [CENTRE_OFFSET[3]]])


@functools.lru_cache(maxsize=None)
def oracle_run():
    """Per level: the oracle's arg-max indices, fixes and out-of-window counts for every realisation, from syn_ref's samples."""
    case = helpers.make_case(seed=1, fs=FS, S=S, K=K, G=4096, amp=1.0, grid="uniform", center_offset=CENTRE_OFFSET,
                             flips=np.zeros(K, dtype=bool))
    case["pos"], case["vel"] = POS, VEL
    w0 = case["wins"][0]
    truth = dpe.handoff.read_handoff(helpers.HANDOFF)["X_ECEF"]
    out = []
    for lev, cn0 in enumerate(LEVELS):
        amp = float(dpe.synth.cn0_to_amp(cn0, SIGMA, FS))
        case["wins"] = [dict(w0, iq=syn_ref.quantise(syn_ref.window(FS, S, w0["start"], amp, SIGMA, (0.0, 0.0), None, SEED, lev * N_REAL + r)))
                        for r in range(N_REAL)]
        ref = helpers.run_oracle(case, L=L, B=B)
        res = ref["res"]
        fixes = np.stack([r["zVal"] for r in res])
        Rm = w0["R"].reshape(3, 3)
        enu = (fixes[:, :3] - truth[None, :3]) @ Rm
        out.append(dict(cn0=cn0, pos_index=np.array([r["posIndex"] for r in res]), vel_index=np.array([r["velIndex"] for r in res]),
                        fixes=fixes, rmse_3d=float(np.sqrt(np.mean(np.sum(enu ** 2, axis=1)))),
                        oob=np.array([[r["posOutOfWindowX"], r["velOutOfWindow"]] for r in res]),
                        margin=np.array([np.sort(s)[-1] - np.sort(s)[-2] for s in ref["pos"]]) / np.array([s.max() for s in ref["pos"]])))
    return out
