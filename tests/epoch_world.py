"""A synthetic world for the multi-epoch manifold scan (dpe_bcm_create_epochs): ONE receiver on the handoff geometry at
2.5 Msps, N consecutive short windows (S = 5000, 2 ms), 7^4-point grids with the joint world's 40 m and 12 m/s steps (or
larger grids of the same extent, pos_dim / vel_dim: the worlds of tests/test_gpu_epochs_walk.py).

The truth moves with constant velocity (and constant clock drift).  Every window's centre is the truth AT THAT EPOCH moved
back by ONE common grid offset that is not the grids' centre point, so each window alone, and the sum over windows, peak on
the same known grid point.  The banks of every window come from stage 1 on generated samples (own noise per window).

AMP is the joint world's strong signal (every single window peaks on the point).  WEAK_AMP with WEAK_SEED is the
capability's case: with the oracle alone fewer than half of the 16 single windows put their arg-max on the true point while
the 16-window sum does, with a margin of at least ten oracle tolerances (tests/test_epoch_world_cpu.py proves all three)."""
import functools

import numpy as np

import navlab_dpe_sdr_amd as dpe
from tests import joint_world as jw

FS, S, AMP = jw.FS, jw.S, jw.AMP
POS_STEP, VEL_STEP = jw.POS_STEP, jw.VEL_STEP
POS_AT, VEL_AT = (4, 2, 5, 1), (2, 4, 1, 5)       # the common offset as grid coordinates (centre: 3, 3, 3, 3)
VEL_ENU = np.array([14.0, -9.0, 2.0, 0.5])        # the truth's velocity (ENU, m/s) and clock drift (m/s)
WEAK_AMP, WEAK_SEED, WEAK_N = 7.0, 5, 16           # found with the oracle on the CPU (a scan over amplitudes 30 .. 3); fixed here
ORACLE_TOL = 2e-6                                 # tests/test_gpu_parity.py: scores against the extended-precision oracle


def _o():
    from oracle import oracle as o
    return o


def build(N=5, K=8, seed=0, amp=AMP, widen=True, bin_half_width=None, shift=0.0, pos_dim=7, vel_dim=7, pos_step=None,
          vel_step=None):
    """One world per set of arguments, however they are passed (see _build)."""
    return _build(N, K, seed, amp, widen, bin_half_width, shift, pos_dim, vel_dim, pos_step, vel_step)


@functools.lru_cache(maxsize=None)
def _build(N, K, seed, amp, widen, bin_half_width, shift, pos_dim, vel_dim, pos_step, vel_step):
    """-> world dict: fs, S, C, N, K, pos, vel, L, B, pos_at / vel_at (the expected arg-max indices), offset[8] (ENU-dt),
    truth[N, 8], wins[N] (the window records of joint_world.build, each with its own centre).
    widen: bank half-widths from pipeline.bank_half_widths, enlarged until the oracle reports no pair outside the banks;
    False: deliberately narrow banks (the clamp path).  bin_half_width: B forced (with L as widened).
    shift: windows 1 and 3 have their centres moved by `shift` metres in the clock term (pairs leave the banks there).
    widen "L" / "B": only the lag (bin) banks narrow, the other side as widened -- one manifold clamps, the other is clean.
    pos_dim / vel_dim, pos_step / vel_step: as joint_world.build (the walk worlds of tests/test_gpu_epochs_walk.py)."""
    if widen in ("L", "B"):
        world = dict(build(N, K, seed, amp, True, bin_half_width, shift, pos_dim, vel_dim, pos_step, vel_step))
        world["L" if widen == "L" else "B"] = 1 if widen == "L" else 2
        return world
    o = _o()
    ho = jw._extended()
    X = np.array(ho["X_ECEF"], dtype=np.float64)
    R = o.enu2ecef(o.ecef2ll(X))
    R3 = R.reshape(3, 3)
    pos, vel = jw.grids(pos_step, pos_dim, vel_dim, vel_step)
    ip, iv = jw.grid_index(jw.scaled_at(POS_AT, pos_dim), pos_dim), jw.grid_index(jw.scaled_at(VEL_AT, vel_dim), vel_dim)
    dp, dv = pos[ip], vel[iv]
    C = dpe.engine.carr_fft_len(S)
    T = S / FS
    rng = np.random.Generator(np.random.PCG64(7000 + seed))
    sel = np.sort(rng.choice(jw.K_EXT, size=K, replace=False))
    truth0 = X.copy()
    truth0[4:7] = R3 @ VEL_ENU[:3]
    truth0[7] = VEL_ENU[3]
    hr = jw.handoff_at(sel, truth0)
    cm = o.ChanMgr(hr["prn_list"], hr["rc"], hr["ri"], hr["fc"], hr["fi"], hr["cp"], hr["cp_timestamp"], hr["TOW"], hr["eph"],
                   hr["rxTime"], T)
    wins, truths = [], []
    for e in range(N):
        truth = truth0.copy()
        truth[:3] += truth0[4:7] * (T * e)                  # constant velocity
        truth[3] += truth0[7] * (T * e)
        centre = truth.copy()
        centre[:3] -= R3 @ dp[:3]
        centre[3] -= dp[3]
        centre[4:7] -= R3 @ dv[:3]
        centre[7] -= dv[3]
        if shift and e in (1, 3):
            centre[3] += shift
        batch, own_R = (cm.start(truth, centre, np.zeros(1)) if e == 0 else cm.update(truth, centre, np.zeros(1)))
        start = dict(prn=cm.prns, rc=cm.rcStart.copy(), ri=cm.riStart.copy(), fc=cm.fc.copy(), fi=cm.fi.copy(),
                     cp=cm.cpElaStart.copy(), cp_ref=cm.cpRef.copy())
        iq = dpe.synth.gen_iq((9000 + seed) * 1000 + e, FS, S, start, amp=amp, flip=np.zeros(K, dtype=bool))
        wins.append(dict(iq=iq, start=start, sat=batch[:, 0].copy(), R=R.copy(), rxTime=cm.rxTime, rcEnd=cm.rcEnd.copy(),
                         cpElaEnd=cm.cpElaEnd.copy(), cpRef=cm.cpRef.copy(), cpRefTOW=cm.cpRefTOW.copy(), fc=cm.fc.copy(),
                         fi=cm.fi.copy(), centre=centre.copy()))
        truths.append(truth)
    L, B = dpe.pipeline.bank_half_widths(pos, vel, FS, C)
    world = dict(fs=FS, S=S, C=C, N=N, K=K, pos=pos, vel=vel, R=R, wins=wins, truth=np.stack(truths), ho=hr, pos_at=ip, vel_at=iv,
                 offset=np.concatenate([dp, dv]), prn=np.asarray(cm.prns), dims=(pos_dim, vel_dim))
    if widen:
        while True:
            world["L"], world["B"] = L, B
            if shift:
                break
            ref = oracle_rows(world, cache=False)
            if all(x["oob_pos"] == 0 and x["oob_pos_x"] == 0 and x["oob_vel"] == 0 for x in ref["win"]):
                break
            L, B = L + 1, B + 2
    else:
        world["L"], world["B"] = 1, 2
    if bin_half_width is not None:
        world["B"] = int(bin_half_width)
    return world


_ROWS = {}


def oracle_rows(world, lpower=1, cache=True):
    """The oracle's rows per window (faithful and extended-precision position, velocity, out-of-window counts) and their fp64
    sums over the windows -- computed once per (world, lpower) and shared."""
    key = (id(world), lpower, world.get("L"), world.get("B"))
    if cache and key in _ROWS:
        return _ROWS[key]
    o = _o()
    fs, S_, C, L, B, K = world["fs"], world["S"], world["C"], world["L"], world["B"], world["K"]
    out = dict(win=[])
    for win in world["wins"]:
        s = win["start"]
        code, carr = [], []
        for k in range(K):
            c, f, _inf = o.bcs_sv(win["iq"], fs, int(s["prn"][k]), s["rc"][k], s["ri"][k], s["fc"][k], s["fi"][k], int(s["cp"][k]),
                                  int(s["cp_ref"][k]), -L, L, -B, B, C)
            code.append(c)
            carr.append(f)
        code, carr = np.stack(code), np.stack(carr)
        args = (win["sat"], code, S_ // 2 - L, win["centre"], world["pos"], win["R"], win["fc"], win["cpRefTOW"], win["cpElaEnd"],
                win["cpRef"], win["rcEnd"], win["rxTime"], fs, S_, lpower)
        sp, oobp = o.bcm_pos(*args)
        spx, oobx = o.bcm_pos(*args, extended=True)
        sv, oobv = o.bcm_vel(win["sat"], carr, C // 2 - B, win["centre"], world["vel"], win["R"], win["fi"], win["rxTime"], fs, C, 1,
                             lpower)
        out["win"].append(dict(pos=sp, pos_x=spx, vel=sv, oob_pos=oobp, oob_pos_x=oobx, oob_vel=oobv))
    for name in ("pos", "pos_x", "vel"):
        out[name] = np.sum([x[name] for x in out["win"]], axis=0)          # fp64 sum of the oracle's per-window rows
    if cache:
        _ROWS[key] = out
    return out


def weak():
    """The weak-signal variant: WEAK_N windows at WEAK_AMP."""
    return build(N=WEAK_N, K=8, seed=WEAK_SEED, amp=WEAK_AMP)


def gpu_inputs(world):
    """(chan_start [N, K], chan_end [N, K], bcm_window [N], iq [N, 2S]) as the engine takes them."""
    wins = world["wins"]
    cs = np.stack([dpe.engine.chan_start_array(w["start"]["prn"], w["start"]["rc"], w["start"]["ri"], w["start"]["fc"],
                                               w["start"]["fi"], w["start"]["cp"], w["start"]["cp_ref"]) for w in wins])
    ce = np.stack([dpe.engine.chan_end_array(w["sat"], w["rcEnd"], w["fc"], w["fi"], w["cpRefTOW"], w["cpElaEnd"], w["cpRef"])
                   for w in wins])
    bw = np.concatenate([dpe.engine.bcm_window_array(w["centre"][None, :], w["R"][None, :], [w["rxTime"]]) for w in wins])
    return cs, ce, bw, np.stack([w["iq"] for w in wins])
