"""Inputs of tests/test_gpu_trk_shapes.py and tests/test_trk_shapes_cpu.py (test infrastructure, no GPU): the synthetic two-channel
record of test_closed_loop_at_25_msps_vs_trk_ref at window shapes the tracker's other tests never use, the fp64 reference runs on
it (tests/trk_ref.py), and the hand-made parameter rows of the teacher-forced correlator test.  Everything is computed once per
process and shared; callers must not modify what they get."""
import functools

import numpy as np

import navlab_dpe_sdr_amd as dpe
from tests import trk_ref

PRNS = (8, 27)
FI = np.array([2210.4, -1475.8])                     # Dopplers of both signs
RC0, RI0 = np.array([402.6, 771.3]), np.array([0.3, 0.8])
D_START = np.array([[0.06, 0.05, 12.0], [-0.04, -0.07, -18.0]])   # start parameters off the truth: rc (chip), ri (cycle), fi (Hz)
AMP, SIGMA, SEED = np.array([90.0, 110.0]), 300.0, 25

# (fs, T, M, ds): the closed-loop shapes.  The first three have S % 4 == 2: every odd window starts 8 bytes off a 16-byte
# boundary and every window ends in a half-filled quad of samples.
SHAPES = ((2.5e6, 0.5e-3, 160, 1.0), (2.5e6, 1.5e-3, 80, 1.0), (2.046e6, 1e-3, 100, 1.0), (2.5e6, 1e-3, 100, -1.0))
RING_SHAPE = (2.5e6, 1e-3, 100, 1.0)                 # the ring tests' record (M windows, and RING_EXTRA more)
RING_EXTRA = 7
SHAPE_IDS = ["%.4gMsps-%.4gms-ds%+d" % (s[0] / 1e6, s[1] * 1e3, int(s[3])) for s in SHAPES]


def fc_of(fi, ds=1.0):
    return trk_ref.F_CA * (1.0 + ds * np.asarray(fi) / trk_ref.F_L1)


@functools.lru_cache(maxsize=None)
def record(fs, T, M, ds, extra=1):
    """The record of M + extra windows at (fs, T) and its start parameters [K, 4]."""
    S = int(round(T * fs))
    ch = dict(prn=np.array(PRNS), rc=RC0, ri=RI0, fc=fc_of(FI, ds), fi=FI, cp_ref=np.array([5, 14]))
    iq, _ = dpe.synth.gen_iq_record(SEED, fs, (M + extra) * S, ch, amp=AMP, sigma=SIGMA)
    fi0 = FI + D_START[:, 2]
    start = np.stack([RC0 + D_START[:, 0], RI0 + D_START[:, 1], trk_ref.F_CA + ds * trk_ref.F_CA / trk_ref.F_L1 * fi0, fi0], axis=1)
    iq.setflags(write=False)
    start.setflags(write=False)
    return dict(fs=fs, T=T, M=M, ds=ds, S=S, iq=iq, start=start, truth=ch)


@functools.lru_cache(maxsize=None)
def reference(fs, T, M, ds, extra=1, chans=None):
    """trk_ref on record(...): dict(ref, case, signs, ps: the fp64 run; rounded: the logs of the run with fp32 E / P / L; g: what
    trk_ref.scale measures correlations against).  chans: a tuple of channel indices (None: both)."""
    r = record(fs, T, M, ds, extra)
    sel = list(range(len(PRNS))) if chans is None else list(chans)
    prns, start = [PRNS[k] for k in sel], r["start"][sel]
    n = M + extra - 1
    ref, case, signs, _, ps = trk_ref.track(r["iq"], fs, T, prns, start, n, ds=ds)
    rounded = trk_ref.track(r["iq"], fs, T, prns, start, n, ds=ds, round_epl=np.float32)[0]
    return dict(ref=ref, case=case, signs=signs, ps=ps, rounded=rounded, g=dict(M=n, log_iP=ref["iP"], log_qP=ref["qP"]))


def sign_margin(x):
    """Per channel: the smallest |Re p_s| a sign of the reference run x was decided on, over the median prompt magnitude."""
    M = int(x["g"]["M"])
    return [float(np.abs(p).min() / np.median(np.hypot(x["ref"]["iP"][:M, k], x["ref"]["qP"][:M, k]))) for k, p in enumerate(x["ps"])]


# ------------------------------------------------------------------------------------------------ teacher-forced correlator rows
def _idxs1(rc, fc, fs):
    return int(np.floor((trk_ref.L_CA - rc) * (fs / fc))) + 1


def boundary_rc_pair(fs, fc, S):
    """(rc_a, rc_b), neighbouring doubles: the first boundary floor((1023 - rc) fs / fc) + 1 is S at rc_a (the window's last
    segment is empty: case 1) and S + 1 at rc_b (no boundary inside: case 0).  Needs S fc / fs < 1023: at S fc / fs = 1023 chips
    per window, the nominal 1 ms, that takes fc below nominal."""
    mid = trk_ref.L_CA - S * fc / fs                   # where the boundary crosses S
    lo, hi = max(mid - 0.5, 0.0), mid + 0.5            # idxs1(lo) > S >= idxs1(hi)
    assert _idxs1(lo, fc, fs) > S >= _idxs1(hi, fc, fs)
    while np.nextafter(lo, hi) < hi:
        mid = 0.5 * (lo + hi)
        if _idxs1(mid, fc, fs) > S:
            lo = mid
        else:
            hi = mid
    assert _idxs1(hi, fc, fs) == S and _idxs1(lo, fc, fs) == S + 1
    return hi, lo


FC_BELOW = trk_ref.F_CA - 30.0                         # S fc / fs = 1022.97 chips per nominal 1 ms window: rc_b > 0 exists
BAD_FC = -trk_ref.F_CA
EDGE_ROWS = ("truth", "rc=0", "rc=1023", "rc=1023-1e-9", "idxs1=S", "idxs1=S+1", "ri=-0.37", "ri=3.25", "fi=+10k", "fi=-10k",
             "fc=+30", "fc=-30", "truth again", "fc<0", "fc=nan")
N_EDGE = len(EDGE_ROWS)


@functools.lru_cache(maxsize=None)
def edge_params(fs, T):
    """(params [M, K, 4], clean [M, K, 4]) for the windows 0 .. M - 1 of record(fs, T, N_EDGE, 1.0): row m of both channels starts
    from the truth at window m (rc, ri, fc, fi) and has the one entry its name says replaced.  The last two rows are the fourth
    branch: channel 1 of "fc<0" has fc = -1.023e6 and channel 0 of "fc=nan" a NaN; `clean` has the truth in those two places."""
    S = int(round(T * fs))
    fc = fc_of(FI)
    p = np.empty((N_EDGE, len(PRNS), 4))
    for m in range(N_EDGE):
        t = m * S / fs
        p[m, :, 0] = np.mod(RC0 + fc * t, trk_ref.L_CA)
        p[m, :, 1] = np.mod(RI0 + FI * t, 1.0)
        p[m, :, 2], p[m, :, 3] = fc, FI
    row = EDGE_ROWS.index
    p[row("rc=0"), :, 0] = 0.0
    p[row("rc=1023"), :, 0] = 1023.0
    p[row("rc=1023-1e-9"), :, 0] = 1023.0 - 1e-9
    a, b = boundary_rc_pair(fs, FC_BELOW, S)
    p[row("idxs1=S"), :, 0], p[row("idxs1=S"), :, 2] = a, FC_BELOW
    p[row("idxs1=S+1"), :, 0], p[row("idxs1=S+1"), :, 2] = b, FC_BELOW
    p[row("ri=-0.37"), :, 1] = -0.37
    p[row("ri=3.25"), :, 1] = 3.25
    p[row("fi=+10k"), :, 3] = 10000.0
    p[row("fi=-10k"), :, 3] = -10000.0
    p[row("fc=+30"), :, 2] = trk_ref.F_CA + 30.0
    p[row("fc=-30"), :, 2] = trk_ref.F_CA - 30.0
    clean = p.copy()
    p[row("fc<0"), 1, 2] = BAD_FC
    p[row("fc=nan"), 0, 2] = np.nan
    p.setflags(write=False)
    clean.setflags(write=False)
    return p, clean


def correlate_ref(iq, fs, S, params):
    """trk_ref.correlate (carried p_a = 0) for every row and channel of params, in the layout ScalarTracker.correlate returns.
    A row whose parameters are not finite has no reference (numpy cannot cast its boundaries): it is reported as case -1 with
    zero outputs, like the rows trk_ref.correlate itself returns case -1 for."""
    M, K = params.shape[:2]
    out = dict(seg=np.zeros((M, K, 3, 3), dtype=np.complex128), epl=np.zeros((M, K, 3), dtype=np.complex128),
               case=np.full((M, K), -1, dtype=np.int64), cp_compl=np.zeros((M, K), dtype=np.int64), idxs1=np.full((M, K), np.nan),
               idxs2=np.full((M, K), np.nan), signs=np.zeros((M, K, 2), dtype=np.int8), ps=np.zeros((M, K, 2)))
    chips = [dpe.synth.ca_code(p).astype(np.float64) for p in PRNS]
    for m in range(M):
        w = iq[2 * S * m: 2 * S * (m + 1)]
        x = w[0::2] + 1j * w[1::2]
        for k in range(K):
            rc, ri, fc, fi = params[m, k]
            if not np.isfinite(params[m, k]).all():
                continue
            e, p_, l, compl_, sg, _, case, seg = trk_ref.correlate(x, chips[k], fs, rc, ri, fc, fi, 0j)
            out["case"][m, k] = case
            out["idxs1"][m, k] = np.floor((trk_ref.L_CA - rc) * (fs / fc)) + 1
            out["idxs2"][m, k] = np.floor((2.0 * trk_ref.L_CA - rc) * (fs / fc)) + 1
            if case < 0:
                continue
            out["seg"][m, k], out["epl"][m, k], out["cp_compl"][m, k] = seg, (e, p_, l), compl_
            out["signs"][m, k, :compl_] = sg
            out["ps"][m, k, :compl_] = [seg[0, 1].real, seg[1, 1].real][:compl_]
    return out


def tie_margin(fs, S, rc, fc):
    """Smallest distance (chips) of a sample's early / prompt / late code phase t fc + rc (+ 0.5, 0, - 0.5) from an integer, over
    the samples 1 .. S - 1 of a window: how far the row is from asking which chip a sample exactly on a chip edge belongs to.
    (Sample 0 is left out: rc = 0 and rc = 1023 put it on an edge on purpose, and there both sides hold rc itself, exactly.)"""
    f = 2.0 * (np.arange(1, S) / fs * fc + rc)
    return float(np.abs(f - np.rint(f)).min() / 2.0)
