"""A synthetic multi-receiver world for the joint manifold scan (dpe_bcm_create_joint): N receivers of a rigid set on the
handoff geometry, each with its own SV subset, noise, true position X + R b_r (baselines of 0.5 .. 3 m) and clock offset.

Code phases, code rates and Dopplers of every (receiver, SV) pair are re-derived for that receiver's position by the fixed
point workload.extend_handoff uses for its synthetic SVs.  Every centre is the truth moved back by ONE common grid offset
(position and velocity), so that each receiver alone, and the sum over receivers, peak on the same known grid point, which
is not the grids' centre point.  All receivers carry the same ENU->ECEF matrix (the set's reference point's): one grid
offset is one ECEF displacement for all of them.

Spacings: at 2.5 Msps a sample is 120 m and a 2 ms window resolves Doppler to ~95 m/s per main lobe; with amp 200 against
sigma 300 over 5000 samples a single SV's peak is known to ~1/33 of that.  The grids step by 40 m / 12 m/s so that the
expected point wins for every receiver alone (tests/test_joint_world_cpu.py proves it with the oracle).  Larger grids
(pos_dim / vel_dim of build) keep that extent with finer steps (17.1 m and 5.1 m/s at 15^4), on which the point still wins for
every receiver alone, by the same proof."""
import functools

import numpy as np

import navlab_dpe_sdr_amd as dpe
from tests import helpers

FS, S, AMP = 2.5e6, 5000, 200.0
POS_STEP, VEL_STEP = 40.0, 12.0
K_EXT = 12
_C, _FCA = 299792458.0, 1.023e6
BASELINES = np.array([[0.0, 0.0, 0.0], [1.2, -0.5, 0.0], [-0.4, 2.9, 0.3], [2.1, 1.9, -0.6], [0.5, 0.0, 0.0], [-3.0, 0.1, 0.2],
                      [0.3, -2.2, 1.0], [1.0, 1.0, 1.0]])
CLOCKS = np.array([0.0, 7.5, -3.25, 12.0, 1.0, -8.0, 4.0, 2.0])     # calibrated clock offsets (m)
POS_AT, VEL_AT = (4, 2, 5, 1), (2, 4, 1, 5)                         # the common offset as grid coordinates (centre: 3, 3, 3, 3)


def scaled_at(at, dim):
    """POS_AT / VEL_AT of the 7^4 grid as coordinates of a dim^4 grid: the same direction from the centre point, scaled with
    the grid's half width ((dim - 1) // 2 entries, synth.uniform_grid's centre).  dim = 7 gives `at` itself.  For the walk
    worlds (dim 13, 14, 15, 20) the point lies far beyond the first 1024-point tile: its x coordinate alone puts it past
    4 * 13^3 points."""
    half = (dim - 1) // 2
    return tuple(half + int(np.rint((a - 3) * half / 3.0)) for a in at)


def scaled_step(step, dim):
    """The spacing that keeps a dim^4 grid at the 7^4 grid's extent (3 steps to its far edge): step for dim = 7."""
    return step * 3 / (dim // 2)


def _o():
    from oracle import oracle as o
    return o


def grid_index(at, dim=7):
    return ((at[0] * dim + at[1]) * dim + at[2]) * dim + at[3]


@functools.lru_cache(maxsize=None)
def _extended():
    return dpe.workload.extend_handoff(dpe.handoff.read_handoff(helpers.HANDOFF), K_EXT)


def handoff_at(sel, Xr):
    """The extended handoff's SVs `sel` as a receiver at state Xr sees them at rxTime: the fixed point of
    workload.extend_handoff (transmit time <-> satellite position <-> pseudorange), for real and synthetic SVs alike."""
    ho = _extended()
    out = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in ho.items()}
    rcs, fcs, fis, cprs, cps = [], [], [], [], []
    for k in sel:
        eph, tow = ho["eph"][k], int(ho["TOW"][k])
        cp, rc, cpr, fc, fi = 1000, 0.0, 1000, _FCA, 0.0
        for _ in range(4):
            cm = dpe.engine.ChanMgr([1], [rc], [0.0], [fc], [fi], [cp], [cpr], [tow], eph[None, :], ho["rxTime"], 0.02)
            cm.Start(Xr, Xr, (0.0,))
            cm.Update(Xr, Xr, (0.0,))
            s, e, w, _b = cm.outputs(with_batch=True)
            cm.Stop()
            sat = e["satState"][0]
            rng = np.linalg.norm(sat[:3] - Xr[:3])
            tx = ho["rxTime"] - (rng - _C * sat[3] + Xr[3]) / _C
            whole = np.floor((tx - tow) * 1000.0)
            cpr = int(cp - whole)
            rc = float((tx - tow - whole * 1e-3) * _FCA)
            fc, fi = float(s["codeFrequency"][0]), float(s["carrierFrequency"][0])
        assert 0.0 <= rc < 1023.0
        rcs.append(rc); fcs.append(fc); fis.append(fi); cprs.append(cpr); cps.append(cp)
    sel = np.asarray(sel)
    out["prn_list"], out["eph"], out["TOW"], out["ri"] = ho["prn_list"][sel], ho["eph"][sel], ho["TOW"][sel], ho["ri"][sel]
    out["rc"], out["fc"], out["fi"] = np.array(rcs), np.array(fcs), np.array(fis)
    out["cp"], out["cp_timestamp"] = np.array(cps, dtype=np.int32), np.array(cprs, dtype=np.int32)
    out["X_ECEF"] = np.array(Xr, dtype=np.float64)
    return out


SAMPLE = _C / FS     # one sample of code delay, in metres


def grids(pos_step=None, pos_dim=7, vel_dim=7, vel_step=None):
    """Position and velocity grids of pos_dim^4 / vel_dim^4 points; a step left out keeps the 7^4 grid's extent."""
    pos_step = scaled_step(POS_STEP, pos_dim) if pos_step is None else pos_step
    vel_step = scaled_step(VEL_STEP, vel_dim) if vel_step is None else vel_step
    return dpe.synth.uniform_grid(pos_dim, pos_step), dpe.synth.uniform_grid(vel_dim, vel_step)


def build(n_sv=(5, 8, 4), seed=0, W=1, widen=True, pos_step=None, pos_dim=7, vel_dim=7, vel_step=None):
    """One world per set of arguments, however they are passed (see _build)."""
    return _build(tuple(n_sv), seed, W, widen, pos_step, pos_dim, vel_dim, vel_step)


@functools.lru_cache(maxsize=None)
def _build(n_sv, seed, W, widen, pos_step, pos_dim, vel_dim, vel_step):
    """-> world dict: fs, S, C, pos, vel, R, L, B, pos_at / vel_at (expected arg-max indices), offset[8] (ENU-dt), and per
    receiver rx[r] = dict(K, ho, truth, centre, wins[W]) with the window records of helpers.make_case.
    widen: bank half-widths from pipeline.bank_half_widths, enlarged until the oracle reports no pair outside the banks;
    False: deliberately narrow banks (the clamp path); "L": only the lag banks narrow, B as widened (the position manifold
    clamps, the velocity manifold is clean); "B": its mirror.  pos_step: spacing of the position grid (the closed-loop world
    uses SAMPLE, see oracle_loop).  pos_dim / vel_dim: points per axis of each grid (7: three tiles; 15, 14, 20, 13: the
    walk worlds of tests/test_gpu_joint_walk.py), with POS_AT / VEL_AT and, unless given, the steps scaled to the 7^4 grid's
    extent (scaled_at, scaled_step)."""
    if widen in ("L", "B"):
        base = build(n_sv, seed, W, True, pos_step, pos_dim, vel_dim, vel_step)
        world = dict(base)
        world["L" if widen == "L" else "B"] = 1 if widen == "L" else 2
        return world
    o = _o()
    ho = _extended()
    X = np.array(ho["X_ECEF"], dtype=np.float64)
    R = o.enu2ecef(o.ecef2ll(X))
    R3 = R.reshape(3, 3)
    pos, vel = grids(pos_step, pos_dim, vel_dim, vel_step)
    ip, iv = grid_index(scaled_at(POS_AT, pos_dim), pos_dim), grid_index(scaled_at(VEL_AT, vel_dim), vel_dim)
    dp, dv = pos[ip], vel[iv]
    C = dpe.engine.carr_fft_len(S)
    T = S / FS
    rxs = []
    for r, K in enumerate(n_sv):
        rng = np.random.Generator(np.random.PCG64(1000 * seed + r))
        sel = np.sort(rng.choice(K_EXT, size=K, replace=False))
        truth = X.copy()
        truth[:3] += R3 @ BASELINES[r]
        truth[3] += CLOCKS[r]
        hr = handoff_at(sel, truth)
        centre = truth.copy()
        centre[:3] -= R3 @ dp[:3]
        centre[3] -= dp[3]
        centre[4:7] -= R3 @ dv[:3]
        centre[7] -= dv[3]
        cm = o.ChanMgr(hr["prn_list"], hr["rc"], hr["ri"], hr["fc"], hr["fi"], hr["cp"], hr["cp_timestamp"], hr["TOW"], hr["eph"],
                       hr["rxTime"], T)
        wins = []
        for w in range(W):
            batch, _own_R = (cm.start(truth, centre, np.zeros(1)) if w == 0 else cm.update(truth, centre, np.zeros(1)))
            start = dict(prn=cm.prns, rc=cm.rcStart.copy(), ri=cm.riStart.copy(), fc=cm.fc.copy(), fi=cm.fi.copy(),
                         cp=cm.cpElaStart.copy(), cp_ref=cm.cpRef.copy())
            iq = dpe.synth.gen_iq((1000 * seed + r) * 1000 + w, FS, S, start, amp=AMP, flip=np.zeros(K, dtype=bool))
            wins.append(dict(iq=iq, start=start, sat=batch[:, 0].copy(), R=R.copy(), rxTime=cm.rxTime, rcEnd=cm.rcEnd.copy(),
                             cpElaEnd=cm.cpElaEnd.copy(), cpRef=cm.cpRef.copy(), cpRefTOW=cm.cpRefTOW.copy(), fc=cm.fc.copy(),
                             fi=cm.fi.copy(), centre=centre.copy()))
        rxs.append(dict(K=K, ho=hr, truth=truth, centre=centre, wins=wins, prn=np.asarray(cm.prns)))
    L, B = dpe.pipeline.bank_half_widths(pos, vel, FS, C)
    world = dict(fs=FS, S=S, C=C, W=W, pos=pos, vel=vel, R=R, rx=rxs, pos_at=ip, vel_at=iv, offset=np.concatenate([dp, dv]),
                 dims=(pos_dim, vel_dim))
    if widen:
        while True:
            world["L"], world["B"] = L, B
            ref = oracle_rows(world, cache=False)
            if all(x["oob_pos"] == 0 and x["oob_pos_x"] == 0 and x["oob_vel"] == 0 for row in ref["rx"] for x in row):
                break
            L, B = L + 1, B + 2
    else:
        world["L"], world["B"] = 1, 2
    return world


_ROWS = {}


def oracle_rows(world, lpower=1, cache=True):
    """The oracle's rows per window and receiver (faithful and extended-precision position, velocity, out-of-window counts,
    banks) and their fp64 sums over receivers -- computed once per (world, lpower) and shared."""
    key = (id(world), lpower, world.get("L"), world.get("B"))
    if cache and key in _ROWS:
        return _ROWS[key]
    o = _o()
    fs, S_, C, L, B = world["fs"], world["S"], world["C"], world["L"], world["B"]
    out = dict(rx=[], pos=[], pos_x=[], vel=[])
    for w in range(world["W"]):
        row = []
        for rx in world["rx"]:
            win, s = rx["wins"][w], rx["wins"][w]["start"]
            code, carr = [], []
            for k in range(rx["K"]):
                c, f, _inf = o.bcs_sv(win["iq"], fs, int(s["prn"][k]), s["rc"][k], s["ri"][k], s["fc"][k], s["fi"][k], int(s["cp"][k]),
                                      int(s["cp_ref"][k]), -L, L, -B, B, C)
                code.append(c)
                carr.append(f)
            code, carr = np.stack(code), np.stack(carr)
            args = (win["sat"], code, S_ // 2 - L, win["centre"], world["pos"], win["R"], win["fc"], win["cpRefTOW"], win["cpElaEnd"],
                    win["cpRef"], win["rcEnd"], win["rxTime"], fs, S_, lpower)
            sp, oobp = o.bcm_pos(*args)
            quirks = o.bcm_pos_quirks()
            spx, oobx = o.bcm_pos(*args, extended=True)
            sv, oobv = o.bcm_vel(win["sat"], carr, C // 2 - B, win["centre"], world["vel"], win["R"], win["fi"], win["rxTime"], fs, C, 1,
                                 lpower)
            row.append(dict(code=code, carr=carr, pos=sp, pos_x=spx, vel=sv, oob_pos=oobp, oob_pos_x=oobx, oob_vel=oobv,
                            quirks=quirks))
        out["rx"].append(row)
        for name in ("pos", "pos_x", "vel"):
            out[name].append(np.sum([x[name] for x in row], axis=0))
    if cache:
        _ROWS[key] = out
    return out


# closed-loop starts as ENU-dt grid steps of the SAMPLE-spaced grid: (start, the arg-max coordinates of window 1, bound on the
# final error in metres)
LOOP_STARTS = {"clock": ((0, 0, 0, -1), (3, 3, 3, 4), 1e-6), "enu_clock": ((-1, -1, -1, -1), (4, 4, 4, 4), 1e-2)}


def loop_step(world, name):
    """The common ECEF / clock offset [4] of start `name`."""
    e = np.array(LOOP_STARTS[name][0], dtype=np.float64) * SAMPLE
    return np.concatenate([world["R"].reshape(3, 3) @ e[:3], [e[3]]])


def oracle_loop(world, step):
    """The closed loop of pipeline.run_joint_closed_loop driven by the oracle alone: one oracle channel manager per receiver,
    oracle banks, the summed extended-precision position rows and velocity rows, one arg-max, every receiver moved by it; all
    receivers use receiver 0's ENU->ECEF matrix.  step: the common ECEF / clock offset [4] of the initial states.
    -> dict(argmax=[(pos, vel)] per window, fixes [W, N, 8]).
    The scan interpolates the banks linearly, so a per-SV score is piecewise linear in the offset with its maxima ON bank
    samples: an initial error of a fraction of a sample (120 m at 2.5 Msps) along one axis leaves every SV preferring the lag it
    is closest to, and the loop does not move.  The closed-loop world therefore spaces its position grid by exactly one sample
    and starts one grid step off in the clock term: every SV's peak then sits one whole lag from its bank centre and exactly one
    grid point (x, y, z at the centre, dt one step back) lines all of them up.  A second start is one grid step off in all four
    of east, north, up and clock (LOOP_STARTS): there the per-SV shifts are fractions of a sample that differ from SV to SV, and
    only the geometry of the whole set picks the point; the loop then ends within |step|^2 / Earth radius = 7 mm of the truth,
    because the set's ENU frame is taken at receiver 0's current state, 208 m from where the truth's is.  On the 40 m grid of the
    other worlds the oracle's loop does not move from any one-step start (measured): every SV prefers the lag it is closest to."""
    o = _o()
    fs, S_, Cf, L, B = world["fs"], world["S"], world["C"], world["L"], world["B"]
    hos = [rx["ho"] for rx in world["rx"]]
    cms = [o.ChanMgr(h["prn_list"], h["rc"], h["ri"], h["fc"], h["fi"], h["cp"], h["cp_timestamp"], h["TOW"], h["eph"], h["rxTime"],
                     S_ / fs) for h in hos]
    xs = [np.array(h["X_ECEF"], dtype=np.float64) + np.concatenate([step, np.zeros(4)]) for h in hos]
    tg = np.zeros(1)
    out = dict(argmax=[], fixes=np.zeros((world["W"], len(hos), 8)))
    for w in range(world["W"]):
        sp, sv, R0 = 0.0, 0.0, None
        for r, cm in enumerate(cms):
            batch, R = cm.start(xs[r], xs[r], tg) if w == 0 else cm.update(xs[r], xs[r], tg)
            R0 = R.copy() if r == 0 else R0
            iq = world["rx"][r]["wins"][w]["iq"]
            code, carr = [], []
            for k in range(cm.K):
                c, f, _ = o.bcs_sv(iq, fs, int(cm.prns[k]), cm.rcStart[k], cm.riStart[k], cm.fc[k], cm.fi[k], int(cm.cpElaStart[k]),
                                   int(cm.cpRef[k]), -L, L, -B, B, Cf)
                code.append(c)
                carr.append(f)
            sp = sp + o.bcm_pos(batch[:, 0], np.stack(code), S_ // 2 - L, xs[r], world["pos"], R0, cm.fc, cm.cpRefTOW, cm.cpElaEnd,
                                cm.cpRef, cm.rcEnd, cm.rxTime, fs, S_, 1, extended=True)[0]
            sv = sv + o.bcm_vel(batch[:, 0], np.stack(carr), Cf // 2 - B, xs[r], world["vel"], R0, cm.fi, cm.rxTime, fs, Cf, 1, 1)[0]
        ip, iv = o.argmax_first(sp), o.argmax_first(sv)
        out["argmax"].append((ip, iv))
        xs = [o.make_meas(ip, iv, xs[r], world["pos"], world["vel"], R0)[0] for r in range(len(hos))]
        out["fixes"][w] = np.stack(xs)
    return out
