"""Fault worlds for the subsets scan (dpe_bcm_create_subsets): tests/epoch_world.py's world with ONE satellite whose signal
arrives late and strong -- a reflection that outweighs the direct path, or a spoofed PRN.

Built on epoch_world.build: the windows, the channel records handed to stage 1 and to the scan, and the grids are unchanged.
Only the generated samples differ: in the gen_iq call SV j's code phase is reduced by bias_m / CHIP_M chips (the code arrives
bias_m metres late) and its amplitude is multiplied by gain.

The constants in WORLDS were found with the oracle's extended-precision position rows on channel subsets, on
epoch_world.build(N=1, K=8, seed=0); tests/test_fde_world_cpu.py proves them again: the full set's arg-max is pulled off the
truth, the set without j peaks on the truth, no other single exclusion does, and every margin is at least ten oracle
tolerances.  build_loop is the six-window world of the closed loop (see the comment above it), proven there as well."""
import functools

import numpy as np

import navlab_dpe_sdr_amd as dpe
from tests import epoch_world as ew

CHIP_M = 293.0523          # one C/A chip in metres (c / 1.023e6)
THRESHOLD_M = ew.POS_STEP  # solution separation threshold of the tests: one position step (40 m)
K, SEED = 8, 0

# name -> (j, bias_m, gain, LPower)
WORLDS = {
    "clean": (None, 0.0, 1.0, 1),
    "j3": (3, 200.0, 4.0, 1),
    "j0": (0, 200.0, 4.0, 1),
    "j3-lp2": (3, 120.0, 3.0, 2),
}
# the closed-loop world (build_loop): 6 consecutive windows, SV 3 faulty in windows 2 .. 4 only
# (bias and gain searched with oracle_fde_loop over 150 .. 300 m x 3 .. 12: the one-window constants 200 m x 4 name SV 2 in window 4)
LOOP_N, LOOP_FAULT, LOOP_J, LOOP_BIAS_M, LOOP_GAIN, LOOP_LPOWER = 6, (2, 3, 4), 3, 250.0, 6.0, 1


def build(name):
    j, bias_m, gain, lpower = WORLDS[name]
    return _build(j, bias_m, gain, lpower)


def faulty_iq(base, e, j, bias_m, gain):
    """Window e of the epoch world `base` generated again with SV j late by bias_m and stronger by gain (same noise seed)."""
    win = base["wins"][e]
    start = dict(win["start"])
    start["rc"] = start["rc"].copy()
    start["rc"][j] -= bias_m / CHIP_M
    amp = np.full(base["K"], ew.AMP, dtype=np.float64)
    amp[j] *= gain
    return dpe.synth.gen_iq((9000 + SEED) * 1000 + e, ew.FS, ew.S, start, amp=amp, flip=np.zeros(base["K"], dtype=bool))


@functools.lru_cache(maxsize=None)
def _build(j, bias_m, gain, lpower):
    """-> epoch_world's one-window world dict (a copy) with the faulty samples, plus fault = j (or None) and lpower."""
    base = ew.build(N=1, K=K, seed=SEED)
    world = dict(base)
    wins = [dict(w) for w in base["wins"]]
    if j is not None:
        wins[0]["iq"] = faulty_iq(base, 0, j, bias_m, gain)
    world.update(wins=wins, fault=j, lpower=lpower)
    return world


def masks_loo():
    return dpe.engine.leave_one_out_masks(K)


_BANKS, _ROWS = {}, {}


def oracle_banks(world, e=0):
    """The oracle's stage 1 on window e: (code [K, 2L+1], carr [K, 2B+1]), once per (world, window)."""
    key = (id(world), e)
    if key not in _BANKS:
        o = ew._o()
        win, s = world["wins"][e], world["wins"][e]["start"]
        L, B = world["L"], world["B"]
        code, carr = [], []
        for k in range(world["K"]):
            c, f, _inf = o.bcs_sv(win["iq"], world["fs"], int(s["prn"][k]), s["rc"][k], s["ri"][k], s["fc"][k], s["fi"][k], int(s["cp"][k]),
                                  int(s["cp_ref"][k]), -L, L, -B, B, world["C"])
            code.append(c)
            carr.append(f)
        _BANKS[key] = (np.stack(code), np.stack(carr))
    return _BANKS[key]


def oracle_subset(world, mask, e=0):
    """The oracle's rows of window e for the channels in `mask` alone: dict(pos_x, vel, oob_pos_x, oob_vel).  The oracle is handed
    only those channels, as dpe_bcm_update would be."""
    key = (id(world), e, int(mask))
    if key not in _ROWS:
        o = ew._o()
        win = world["wins"][e]
        code, carr = oracle_banks(world, e)
        sel = np.array([k for k in range(world["K"]) if (int(mask) >> k) & 1])
        L, B, S_, C, fs = world["L"], world["B"], world["S"], world["C"], world["fs"]
        spx, oobx = o.bcm_pos(win["sat"][sel], code[sel], S_ // 2 - L, win["centre"], world["pos"], win["R"], win["fc"][sel], win["cpRefTOW"][sel],
                              win["cpElaEnd"][sel], win["cpRef"][sel], win["rcEnd"][sel], win["rxTime"], fs, S_, world["lpower"], extended=True)
        sv, oobv = o.bcm_vel(win["sat"][sel], carr[sel], C // 2 - B, win["centre"], world["vel"], win["R"], win["fi"][sel], win["rxTime"], fs, C, 1,
                             world["lpower"])
        _ROWS[key] = dict(pos_x=spx, vel=sv, oob_pos_x=oobx, oob_vel=oobv)
    return _ROWS[key]


def margin(row):
    """(best - second best) / best of a score row."""
    top = np.sort(row)[-2:]
    return (top[1] - top[0]) / row.max()


def oracle_fixes(world, e=0):
    """(full, subs): result dicts (offset[8], posIndex, velIndex) of the oracle's arg-max for the full set and the K leave-one-out
    subsets of window e, in the form pipeline.solution_separation takes."""
    o = ew._o()

    def fix(mask):
        r = oracle_subset(world, mask, e)
        ip, iv = o.argmax_first(r["pos_x"]), o.argmax_first(r["vel"])
        return dict(posIndex=ip, velIndex=iv, offset=np.concatenate([world["pos"][ip], world["vel"][iv]]))
    return fix((1 << world["K"]) - 1), [fix(m) for m in masks_loo()]


# ---- the closed-loop world -----------------------------------------------------------------
# pipeline.run_fde_closed_loop steps its channel manager with the previous fix as BOTH states: the replicas of a window are
# aligned to the loop's own centre, not to a centre moved off the truth as in the one-window worlds.  The loop world is
# therefore generated the same way: the truth moves with constant velocity, every window's channel records come from a
# channel manager stepped with (truth, truth), the loop starts on the truth, and the expected arg-max of a healthy window
# is the grids' centre point (the fix stays on the truth's grid point: the truth moves 3 cm per window, a step is 40 m).
# In the windows LOOP_FAULT SV LOOP_J is generated late by LOOP_BIAS_M and stronger by LOOP_GAIN.


def build_loop():
    return _build_loop(LOOP_BIAS_M, LOOP_GAIN)


@functools.lru_cache(maxsize=None)
def _build_loop(bias_m, gain):
    """-> dict: fs, S, C, K, pos, vel, L, B, ho (the handoff on the truth at window 0), truth [N, 8], iq [N, 2S], centre_at (the
    index of the grids' centre point), lpower, fault, fault_windows."""
    from tests import joint_world as jw
    o = ew._o()
    base = ew.build(N=1, K=K, seed=SEED)
    hr = base["ho"]
    T = ew.S / ew.FS
    truth0 = np.array(hr["X_ECEF"], dtype=np.float64)
    cm = o.ChanMgr(hr["prn_list"], hr["rc"], hr["ri"], hr["fc"], hr["fi"], hr["cp"], hr["cp_timestamp"], hr["TOW"], hr["eph"],
                   hr["rxTime"], T)
    iqs, truths = [], []
    for e in range(LOOP_N):
        truth = truth0.copy()
        truth[:3] += truth0[4:7] * (T * e)
        truth[3] += truth0[7] * (T * e)
        (cm.start if e == 0 else cm.update)(truth, truth, np.zeros(1))
        start = dict(prn=cm.prns, rc=cm.rcStart.copy(), ri=cm.riStart.copy(), fc=cm.fc.copy(), fi=cm.fi.copy(),
                     cp=cm.cpElaStart.copy(), cp_ref=cm.cpRef.copy())
        amp = np.full(K, ew.AMP, dtype=np.float64)
        if e in LOOP_FAULT:
            start["rc"][LOOP_J] -= bias_m / CHIP_M
            amp[LOOP_J] *= gain
        iqs.append(dpe.synth.gen_iq((9500 + SEED) * 1000 + e, ew.FS, ew.S, start, amp=amp, flip=np.zeros(K, dtype=bool)))
        truths.append(truth)
    return dict(fs=ew.FS, S=ew.S, C=base["C"], K=K, pos=base["pos"], vel=base["vel"], L=base["L"], B=base["B"], ho=hr,
                truth=np.stack(truths), iq=np.stack(iqs), centre_at=jw.grid_index((3, 3, 3, 3)), lpower=LOOP_LPOWER, fault=LOOP_J,
                fault_windows=LOOP_FAULT)


_LOOPS = {}


def oracle_fde_loop(world, exclude=True, threshold_m=THRESHOLD_M):
    """pipeline.run_fde_closed_loop driven by the oracle alone: the oracle's channel manager stepped with the previous fix as both
    states, oracle banks, the extended-precision position rows and the velocity rows of the full set and of every leave-one-out
    subset (the oracle handed only that subset's channels), pipeline.solution_separation, the chosen subset's measurement.
    -> dict(fixes [W, 8], suspects [W], seps [W, K], argmax [W][1 + K] (pos, vel) of the full set then the subsets,
    margin [W]: the smallest (best - second best) / best over the window's position and velocity rows, oob [W])."""
    key = (id(world), exclude, threshold_m)
    if key in _LOOPS:
        return _LOOPS[key]
    o = ew._o()
    fs, S_, C, L, B, Kw, lp = world["fs"], world["S"], world["C"], world["L"], world["B"], world["K"], world["lpower"]
    h = world["ho"]
    cm = o.ChanMgr(h["prn_list"], h["rc"], h["ri"], h["fc"], h["fi"], h["cp"], h["cp_timestamp"], h["TOW"], h["eph"], h["rxTime"], S_ / fs)
    x = np.array(h["X_ECEF"], dtype=np.float64)
    masks = masks_loo()
    W = world["iq"].shape[0]
    out = dict(fixes=np.zeros((W, 8)), suspects=np.full(W, -1, dtype=np.int64), seps=np.zeros((W, Kw)), argmax=[], margin=np.zeros(W),
               oob=np.zeros(W, dtype=np.int64))
    for w in range(W):
        batch, R = cm.start(x, x, np.zeros(1)) if w == 0 else cm.update(x, x, np.zeros(1))
        sat = batch[:, 0]
        code, carr = [], []
        for k in range(Kw):
            c, f, _ = o.bcs_sv(world["iq"][w], fs, int(cm.prns[k]), cm.rcStart[k], cm.riStart[k], cm.fc[k], cm.fi[k], int(cm.cpElaStart[k]),
                               int(cm.cpRef[k]), -L, L, -B, B, C)
            code.append(c)
            carr.append(f)
        code, carr = np.stack(code), np.stack(carr)
        fixes, am, worst = [], [], np.inf
        for mask in [(1 << Kw) - 1] + [int(m) for m in masks]:
            sel = np.array([k for k in range(Kw) if (mask >> k) & 1])
            sp, oobp = o.bcm_pos(sat[sel], code[sel], S_ // 2 - L, x, world["pos"], R, cm.fc[sel], cm.cpRefTOW[sel], cm.cpElaEnd[sel],
                                 cm.cpRef[sel], cm.rcEnd[sel], cm.rxTime, fs, S_, lp, extended=True)
            sv, oobv = o.bcm_vel(sat[sel], carr[sel], C // 2 - B, x, world["vel"], R, cm.fi[sel], cm.rxTime, fs, C, 1, lp)
            ip, iv = o.argmax_first(sp), o.argmax_first(sv)
            fixes.append(dict(posIndex=ip, velIndex=iv, offset=np.concatenate([world["pos"][ip], world["vel"][iv]])))
            am.append((ip, iv))
            worst = min(worst, margin(sp), margin(sv))
            out["oob"][w] += oobp + oobv
        s, sep = dpe.pipeline.solution_separation(fixes[0], fixes[1:], masks, threshold_m, Kw)
        chosen = fixes[1 + s] if (exclude and s >= 0) else fixes[0]
        x = o.make_meas(chosen["posIndex"], chosen["velIndex"], x, world["pos"], world["vel"], R)[0]
        out["fixes"][w], out["suspects"][w], out["seps"][w], out["margin"][w] = x, s, sep, worst
        out["argmax"].append(am)
    _LOOPS[key] = out
    return out
