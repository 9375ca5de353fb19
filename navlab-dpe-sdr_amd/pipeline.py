"""Closed-loop DPE iteration on top of the C-ABI -- the Python twin of host/dpe_flow_main.cpp and of
Flow::FlowThread's module order (cudarecv/dsp/src/flow.cu:122-137; dpeflow.cpp:55-62):
SampleBlock -> BatchCorrScores -> BatchCorrManifold -> cuEKF(pass-through) -> cuChanMgr."""
import contextlib
import types
from functools import partial

import numpy as np

from . import engine


def bank_half_widths(pos_grid, vel_grid, fs, nfft):
    """INTEGRATION.md section 3 (same rule as host/grids.hpp::bank_half_widths)."""
    ep = (np.linalg.norm(pos_grid[:, :3], axis=1) + np.abs(pos_grid[:, 3])).max()
    ev = (np.linalg.norm(vel_grid[:, :3], axis=1) + np.abs(vel_grid[:, 3])).max()
    L = int(np.ceil(ep * fs / 299792458.0)) + 2
    B = int(np.ceil(ev * (nfft / fs) * 1.57542e9 / 299792458.0)) + 3
    return L, B


def bank_half_widths_refine(levels, fs, nfft):
    """Bank half-widths for a chain of refine levels (engine.RefineManifold): levels = [(GridAxes pos, GridAxes vel), ...].  A
    scored point is a sum of one axis entry per level, so the extent is the sum over levels of each level's corner distance
    and largest |delta_t| -- the rule of bank_half_widths on the summed extents."""
    ep = sum(np.sqrt(sum(np.abs(a).max() ** 2 for a in p.axes[:3])) + np.abs(p.axes[3]).max() for p, _ in levels)
    ev = sum(np.sqrt(sum(np.abs(a).max() ** 2 for a in v.axes[:3])) + np.abs(v.axes[3]).max() for _, v in levels)
    L = int(np.ceil(ep * fs / 299792458.0)) + 2
    B = int(np.ceil(ev * (nfft / fs) * 1.57542e9 / 299792458.0)) + 3
    return L, B


def quantisation_floor(grid):
    """h^2 / 12 per grid axis [4], h = the smallest non-zero spacing of that axis's values: the variance of the grid's own
    quantisation (a fix is a grid point).  An axis with a single value has no spacing and gets 0.  grid: a [G, 4] point list or
    a GridAxes."""
    cols = grid.axes if hasattr(grid, "axes") else [np.asarray(grid, dtype=np.float64)[:, c] for c in range(4)]
    out = np.zeros(4)
    for c, v in enumerate(cols):
        d = np.diff(np.unique(v))      # (unique sorts; its differences are > 0)
        out[c] = d.min() ** 2 / 12.0 if d.size else 0.0
    return out


def measurement_cov_floor(pos_floor, vel_floor, enu2ecef):
    """The quantisation floors of both manifolds (quantisation_floor of each grid) as an 8x8 matrix in the frame of zVal:
    blockdiag(J D_pos J^T, J D_vel J^T), D = diag(floor), J = blockdiag(enu2ecef, 1) -- diag(h^2 / 12) itself where the three
    ENU spacings are equal."""
    J = np.eye(4)
    J[:3, :3] = np.asarray(enu2ecef, dtype=np.float64).reshape(3, 3)
    F = np.zeros((8, 8))
    F[:4, :4] = J @ np.diag(pos_floor) @ J.T
    F[4:, 4:] = J @ np.diag(vel_floor) @ J.T
    return 0.5 * (F + F.T)


@contextlib.contextmanager
def _single_rx_loop(iq_windows, ho, fs, K, init_delta, half_widths, make_bcm, make_cm=None, lag_half_width=None, bin_half_width=None,
                    max_windows=1):
    """What the single-receiver closed loops open and close with.  half_widths(fs, nfft) -> (L, B) is the caller's rule (the
    overrides win); make_bcm(S, nfft, L, B, K) constructs the manifold; make_cm(bcs, bcm, T, K) the channel manager once both
    modules have started (default: the host ChanMgr from the handoff).  Yields a namespace: W, S, K, bcs, bcm, cm, iq_d (the
    samples on the device) and x (X_ECEF + init_delta, 4 entries or all 8).  nfft is engine.carr_fft_len(S), the value a started
    BatchCorrScores reports as NumFFTPoints.  Everything is stopped on the way out -- channel
    manager, manifold, correlator -- whether or not the body raised."""
    import torch
    iq_windows = np.ascontiguousarray(iq_windows)
    W, S2 = iq_windows.shape
    S = S2 // 2
    K = len(ho["prn_list"]) if K is None else K
    nfft = engine.carr_fft_len(S)
    L, B = half_widths(fs, nfft)
    L = L if lag_half_width is None else int(lag_half_width)
    B = B if bin_half_width is None else int(bin_half_width)
    bcs = engine.BatchCorrScores(fs, samples_per_window=S, lag_half_width=L, bin_half_width=B, max_windows=max_windows, max_channels=K)
    bcm = make_bcm(S, nfft, L, B, K)
    cm = None
    try:
        bcs.Start()
        bcm.Start()
        cm = engine.ChanMgr.from_handoff(ho, S / fs, K) if make_cm is None else make_cm(bcs, bcm, S / fs, K)
        x = np.array(ho["X_ECEF"], dtype=np.float64).copy()
        d0 = np.asarray(init_delta, dtype=np.float64)
        x[:d0.shape[0]] += d0
        iq_d = torch.from_numpy(iq_windows).to("cuda:0")
        yield types.SimpleNamespace(W=W, S=S, K=K, bcs=bcs, bcm=bcm, cm=cm, iq_d=iq_d, x=x)
    finally:      # an error in the middle of the loop must not leave device handles behind
        if cm is not None:
            cm.Stop()
        bcm.Stop()
        bcs.Stop()


def run_closed_loop(iq_windows, ho, fs, pos_grid, vel_grid, time_grid=(0.0,), init_delta=(0, 0, 0, 0), K=None,
                    lpower=1, enable_ekf=False, reference_pair=False, keep_scores=False, couple_velocity=True, doppler_sign=1,
                    measurement_cov=None):
    """iq_windows: int16 [W, 2S] (host).  Returns fixes [W, 8] (= xCurrk1k1 per window) and the raw
    per-window result dicts.  One window per Update, fix fed back to the channel manager.
    enable_ekf: route the fix through cuEKF's real filter (EnableEKF=true) instead of the shipped pass-through.
    reference_pair: dpe_bcm_config.referencePair; keep_scores: every result dict also carries the window's position and velocity scores;
    couple_velocity: the filter's F couples position and velocity over one window (cuekf.cu:111-143) or is the identity (ekf.py:47).
    doppler_sign: the channel manager's DopplerSign (+1 / -1); the handoff's fi is the front end's own, the handoff names no sign.
    measurement_cov: None (the reference's identity RVal), or (rho_pos, rho_vel): after each Update the thresholded moments of the
    score rows are taken (BatchCorrManifold.moments) and the filter is fed R = RValMom + the grid's quantisation floor
    (measurement_cov_floor; it keeps R positive definite when one point is above the threshold).  The measurement stays the
    arg-max zVal.  The result dicts then carry `moments` and, as RVal, the R handed to the filter; a manifold with no point above
    its threshold (every score 0) has no moments and keeps the identity block."""
    def make_bcm(S, nfft, L, B, K):
        return engine.BatchCorrManifold(fs, S, nfft, pos_grid, vel_grid, LPower=lpower, lag_half_width=L, bin_half_width=B,
                                        max_channels=K, reference_pair=reference_pair)

    def make_cm(bcs, bcm, T, K):
        return engine.ChanMgr.from_handoff(ho, T, K, DopplerSign=doppler_sign)

    with _single_rx_loop(iq_windows, ho, fs, K, init_delta, partial(bank_half_widths, pos_grid, vel_grid), make_bcm, make_cm) as lp:
        bcs, bcm, cm = lp.bcs, lp.bcm, lp.cm
        fixes, results = np.zeros((lp.W, 8)), []
        ekf = engine.cuEKF(lp.x, SampleLength=lp.S / fs, EnableEKF=enable_ekf, couple_velocity=couple_velocity)
        floors = None if measurement_cov is None else (quantisation_floor(pos_grid), quantisation_floor(vel_grid))
        try:
            xk1k1, xkk1 = lp.x, lp.x
            for w in range(lp.W):
                (cm.Start if w == 0 else cm.Update)(xk1k1, xkk1, time_grid)
                cs, ce, bw = cm.outputs()
                bcs.Update(lp.iq_d[w], cs)
                bcm.Update(bcs.CodeScores, bcs.CarrScores, bw, ce)
                r = bcm.results()[0]
                if keep_scores:
                    ps, vs = bcm.read_scores()
                    r["posScores"], r["velScores"] = ps[0].copy(), vs[0].copy()
                if measurement_cov is not None:
                    mom = bcm.moments(measurement_cov)[0]
                    R = mom["RValMom"] + measurement_cov_floor(floors[0], floors[1], bw["enu2ecef"][0])
                    for m in (slice(0, 4), slice(4, 8)):
                        if not np.isfinite(R[m, m]).all():
                            R[m, m] = np.eye(4)
                    r["moments"], r["RVal"] = mom, R
                ekf.Update(r["zVal"], r["RVal"])    # EKF_PassMeas (the ML point is the new state) or the filter
                xk1k1, xkk1 = ekf.xCurrk1k1.copy(), ekf.xCurrkk1.copy()
                fixes[w] = xk1k1
                results.append(r)
        finally:
            ekf.Stop()
    return fixes, results


def run_device_loop(iq_windows, ho, fs, pos_grid, vel_grid, time_grid=(0.0,), init_delta=(0, 0, 0, 0), K=None, lpower=1,
                    ring_depth=64, stream=None, reference_pair=False, keep_scores=False, enable_ekf=False, couple_velocity=True,
                    doppler_sign=1, measurement_cov=None):
    """The same loop with nothing read back per window: the channel manager lives on the device (engine.ChanMgrDev), forms
    the measurement from the scan's keys, passes it through and writes the next window's parameter blocks; the host enqueues
        BatchCorrScores.UpdatePrepared -> BatchCorrManifold.UpdatePrepared -> ChanMgrDev.step
    for every window and collects the fixes from the pinned ring afterwards (at most ring_depth - 1 windows ahead).
    reference_pair: dpe_bcm_config.referencePair (the prepared form re-evaluates from the attached manager's port arrays);
    keep_scores (tests): waits for every window and keeps its position and velocity scores, its code banks and the channel manager's outputs the
    window was scored with (`inputs` = ChanMgrDev.outputs() before the window) -- the loop then does read back.
    enable_ekf: cuEKF's filter inside the measurement kernel (dpe_chm_dev_set_ekf) instead of the pass-through; the fixes are then x_k|k.
    doppler_sign: the channel manager's DopplerSign, as in run_closed_loop.
    measurement_cov: None (R = I), or (rho_pos, rho_vel) with enable_ekf: the device filter takes R from each window's manifold
    moments plus the grids' quantisation floors (ChanMgrDev.set_measurement_cov; still nothing read back per window).  The result
    dicts then carry RVal (the R the filter took), sums, nAbove, threshold and fallback (ChanMgrDev.rval)."""
    def make_bcm(S, nfft, L, B, K):
        return engine.BatchCorrManifold(fs, S, nfft, pos_grid, vel_grid, LPower=lpower, lag_half_width=L, bin_half_width=B,
                                        max_channels=K, reference_pair=reference_pair)

    def make_cm(bcs, bcm, T, K):
        cm = engine.ChanMgrDev.from_handoff(ho, T, K, time_grid, DopplerSign=doppler_sign)
        try:
            cm.attach(bcs, bcm, ring_depth)
        except Exception:      # (the helper only stops a manager that make_cm returned)
            cm.Stop()
            raise
        return cm

    with _single_rx_loop(iq_windows, ho, fs, K, init_delta, partial(bank_half_widths, pos_grid, vel_grid), make_bcm, make_cm) as lp:
        bcs, bcm, cm, W, K = lp.bcs, lp.bcm, lp.cm, lp.W, lp.K
        if enable_ekf:
            cm.set_ekf(lp.S / fs, lp.x, couple_velocity=couple_velocity)
        if measurement_cov is not None:
            cm.set_measurement_cov(measurement_cov, quantisation_floor(pos_grid), quantisation_floor(vel_grid))
        cm.Start(lp.x, stream)
        fixes, results, got = np.zeros((W, 8)), [], 0

        def collect(w):      # (the R record lives in a ring of the fix ring's depth: collected with the fix)
            r = cm.fix(w)
            if measurement_cov is not None:
                rv = cm.rval(w, stream)
                r.update(RVal=rv["R"], sums=rv["sums"], nAbove=rv["nAbove"], threshold=rv["threshold"], fallback=rv["fallback"])
            return r
        for w in range(W):
            while w - got >= ring_depth - 1:          # never more than the ring holds ahead of the fixes already collected
                results.append(collect(got))
                got += 1
            inputs = cm.outputs(stream=stream) if keep_scores else None     # (the previous window's time update has run: fix() flushed it)
            bcs.UpdatePrepared(lp.iq_d[w], K, stream)
            bcm.UpdatePrepared(bcs.CodeScores, bcs.CarrScores, K, stream)
            cm.step(stream)
            if keep_scores:
                while got <= w:
                    results.append(collect(got))
                    got += 1
                ps, vs = bcm.read_scores(stream)
                results[w]["posScores"], results[w]["velScores"] = ps[0].copy(), vs[0].copy()
                results[w]["codeBank"] = bcs.read_banks(stream)[0][0].copy()
                results[w]["inputs"] = inputs
        while got < W:
            results.append(collect(got))
            got += 1
        for w, r in enumerate(results):
            fixes[w] = r["zVal"]
        cm.outputs()
        status = cm.status
    return fixes, results, status


def run_joint_closed_loop(iq_windows_per_rx, handoffs, fs, pos_grid, vel_grid, time_grid=(0.0,), init_delta=(0, 0, 0, 0), lpower=1,
                          lag_half_width=None, bin_half_width=None, own_keys=True, keep_scores=False):
    """The closed loop for a rigid set of receivers (engine.JointManifold): iq_windows_per_rx[r] = int16 [W, 2S] of receiver r,
    handoffs[r] its handoff state (its own SVs and X_ECEF: baseline and clock offset live there).  One host ChanMgr and one
    BatchCorrScores per receiver, ONE joint scan per window over the shared grids; every receiver's state is then updated with
    its own zVal (its centre moved by the joint ML offset; pass-through filter).  All receivers of a window are given receiver
    0's ENU->ECEF matrix, so that one grid offset is one ECEF displacement for the whole set.  init_delta: a common ECEF / clock
    offset added to every receiver's initial state.  Returns fixes [W, N, 8] and the per-window joint result dicts."""
    import torch
    N = len(handoffs)
    iqs = [np.ascontiguousarray(q) for q in iq_windows_per_rx]
    W, S2 = iqs[0].shape
    S = S2 // 2
    Ks = [len(ho["prn_list"]) for ho in handoffs]
    nfft = engine.carr_fft_len(S)
    L, B = bank_half_widths(pos_grid, vel_grid, fs, nfft)
    L = L if lag_half_width is None else int(lag_half_width)
    B = B if bin_half_width is None else int(bin_half_width)
    bcss = [engine.BatchCorrScores(fs, samples_per_window=S, lag_half_width=L, bin_half_width=B, max_channels=K) for K in Ks]
    bcm = engine.JointManifold(fs, S, nfft, pos_grid, vel_grid, N, sum(Ks), LPower=lpower, lag_half_width=L,
                               bin_half_width=B, max_channels=max(Ks), own_keys=own_keys)
    cms = []
    try:
        for b in bcss:
            b.Start()
        bcm.Start()
        cms = [engine.ChanMgr.from_handoff(ho, S / fs, K) for ho, K in zip(handoffs, Ks)]
        xs = []
        for ho in handoffs:
            x = np.array(ho["X_ECEF"], dtype=np.float64).copy()
            x[:4] += np.asarray(init_delta, dtype=np.float64)
            xs.append(x)
        iq_d = [torch.from_numpy(q).to("cuda:0") for q in iqs]
        fixes, results = np.zeros((W, N, 8)), []
        for w in range(W):
            rx = []
            for r in range(N):
                (cms[r].Start if w == 0 else cms[r].Update)(xs[r], xs[r], time_grid)
                cs, ce, bw = cms[r].outputs()
                bw = bw.copy()
                if r:
                    bw["enu2ecef"] = rx[0]["win"]["enu2ecef"]
                bcss[r].Update(iq_d[r][w], cs)
                code, carr = engine.bank_rows(bcss[r])
                rx.append(dict(code=code, carr=carr, win=bw, chan=ce))
            bcm.Update(rx)
            res = bcm.results()[0]
            if keep_scores:
                ps, vs = bcm.read_scores()
                res["posScores"], res["velScores"] = ps[0].copy(), vs[0].copy()
            for r in range(N):
                xs[r] = res["rx"][r]["zVal"].copy()
                fixes[w, r] = xs[r]
            results.append(res)
    finally:      # an error in the middle of the loop must not leave N + 1 device handles behind
        for c in cms:
            c.Stop()
        bcm.Stop()
        for b in bcss:
            b.Stop()
    return fixes, results


def predict_state(x, T, couple_velocity=True):
    """The time update x_k+1|k = F x_k|k of the DPE random-walk model (EKF_MakeDPERandomWalkFMatrix, cuekf.cu:133-139), by the
    library's own cuEKF StepPredict."""
    ekf = engine.cuEKF(x, SampleLength=T, EnableEKF=True, couple_velocity=couple_velocity)
    try:
        ekf.step_predict()
        return ekf.state()["xkk1"].copy()
    finally:
        ekf.Stop()


def run_epoch_closed_loop(iq_windows, ho, fs, pos_grid, vel_grid, n_epochs, time_grid=(0.0,), init_delta=(0, 0, 0, 0), K=None, lpower=1,
                          lag_half_width=None, bin_half_width=None, pairs_per_pass=0, keep_scores=False):
    """The closed loop with ONE fix per group of n_epochs consecutive windows (engine.EpochManifold): inside a group the channel
    manager is stepped window by window with the PREDICTED state (predict_state: the filter's time update, no measurement),
    one BatchCorrScores call covers the group's windows, one EpochManifold.Update sums their manifold scores and takes one
    arg-max.  The group's zVal -- its last window's centre moved by the ML offset -- is the state the next group starts from
    (pass-through filter).  A trailing group may be shorter.  n_epochs = 1 is run_closed_loop, bit for bit.
    Returns fixes [ceil(W / n_epochs), 8] and the per-group result dicts."""
    n = int(n_epochs)

    def make_bcm(S, nfft, L, B, K):
        return engine.EpochManifold(fs, S, nfft, pos_grid, vel_grid, n, pairs_per_pass, LPower=lpower, lag_half_width=L, bin_half_width=B,
                                    max_channels=K)

    with _single_rx_loop(iq_windows, ho, fs, K, init_delta, partial(bank_half_widths, pos_grid, vel_grid), make_bcm,
                         lag_half_width=lag_half_width, bin_half_width=bin_half_width, max_windows=n) as lp:
        bcs, bcm, cm, x = lp.bcs, lp.bcm, lp.cm, lp.x
        fixes, results = [], []
        for g0 in range(0, lp.W, n):
            m = min(n, lp.W - g0)
            cs, ce, bw = [], [], []
            for e in range(m):
                if e:
                    x = predict_state(x, lp.S / fs)
                (cm.Start if g0 + e == 0 else cm.Update)(x, x, time_grid)
                s_, e_, w_ = cm.outputs()
                cs.append(s_); ce.append(e_); bw.append(w_)
            bcs.Update(lp.iq_d[g0:g0 + m], np.stack(cs))
            bcm.Update(bcs.CodeScores, bcs.CarrScores, np.concatenate(bw), np.stack(ce), m)
            r = bcm.results()[0]
            if keep_scores:
                ps, vs = bcm.read_scores()
                r["posScores"], r["velScores"] = ps[0].copy(), vs[0].copy()
            x = r["zVal"].copy()
            fixes.append(x)
            results.append(r)
    return np.stack(fixes), results


def run_refine_closed_loop(iq_windows, ho, fs, levels, time_grid=(0.0,), init_delta=(0, 0, 0, 0), K=None, lpower=1,
                           lag_half_width=None, bin_half_width=None, keep_scores=False, keep_banks=False):
    """run_closed_loop with the coarse-to-fine scan (engine.RefineManifold) in place of the one-grid scan: one Update of all
    levels per window, the last level's fix (the window centre moved by the refined offset) fed back to the channel manager
    through the pass-through filter.  levels = [(GridAxes pos, GridAxes vel), ...]; their spans are the caller's choice
    (DESIGN.md 2.4g).  keep_scores: every result dict carries posScores / velScores, lists of the levels' rows; keep_banks: also
    the window's codeBank / carrBank [K, 2L+1] / [K, 2B+1] complex64 and `inputs` = the channel manager's outputs it was scored with.
    Returns fixes [W, 8] and the per-window result dicts."""
    def make_bcm(S, nfft, L, B, K):
        return engine.RefineManifold(fs, S, nfft, levels, LPower=lpower, lag_half_width=L, bin_half_width=B, max_channels=K)

    with _single_rx_loop(iq_windows, ho, fs, K, init_delta, partial(bank_half_widths_refine, levels), make_bcm,
                         lag_half_width=lag_half_width, bin_half_width=bin_half_width) as lp:
        bcs, bcm, cm, x = lp.bcs, lp.bcm, lp.cm, lp.x
        fixes, results = np.zeros((lp.W, 8)), []
        for w in range(lp.W):
            (cm.Start if w == 0 else cm.Update)(x, x, time_grid)
            cs, ce, bw = cm.outputs()
            bcs.Update(lp.iq_d[w], cs)
            bcm.Update(bcs.CodeScores, bcs.CarrScores, bw, ce)
            r = bcm.results()[0]
            if keep_scores:
                rows = [bcm.read_scores(l) for l in range(len(levels))]
                r["posScores"], r["velScores"] = [p[0].copy() for p, _ in rows], [v[0].copy() for _, v in rows]
            if keep_banks:
                code, carr = bcs.read_banks()
                r["codeBank"], r["carrBank"], r["inputs"] = code[0].copy(), carr[0].copy(), (cs, ce, bw)
            x = r["zVal"].copy()
            fixes[w] = x
            results.append(r)
    return fixes, results


def solution_separation(full, subs, masks, threshold_m, n_chan=None):
    """Solution separation over the subsets of one window (host fp64).  full / subs[m]: result dicts with `offset` (the ENU-dt
    position offset in offset[:4], as engine.SubsetManifold.results gives them); masks: uint64 [M], subset m's channels;
    n_chan: the window's channels.  PASS IT whenever the masks are not the complete leave-one-out list: left out, it is taken
    as the highest bit any mask holds plus one, which is the channel count only if some mask holds the last channel -- a list
    without it makes every mask look like an exclusion of the wrong set.
    Per subset the separation is the Euclidean distance (m) between its position ENU-dt offset and the full set's.  The suspect
    is the SV whose single exclusion (the mask of every channel but that one) separates most, if that distance exceeds
    threshold_m; otherwise -1.  Returns (suspect, separations float64 [M])."""
    masks = [int(m) for m in np.asarray(masks, dtype=np.uint64).reshape(-1)]
    if len(masks) != len(subs):
        raise ValueError("solution_separation: %d masks for %d subsets" % (len(masks), len(subs)))
    threshold_m = float(threshold_m)
    K = max(m.bit_length() for m in masks) if n_chan is None else int(n_chan)
    all_sv = (1 << K) - 1
    p0 = np.asarray(full["offset"], dtype=np.float64)[:4]
    sep = np.array([np.linalg.norm(np.asarray(r["offset"], dtype=np.float64)[:4] - p0) for r in subs], dtype=np.float64)
    suspect, worst = -1, threshold_m
    for m, d in zip(masks, sep):
        out = all_sv & ~m
        if m & ~all_sv or out == 0 or out & (out - 1):
            continue                                  # not a single-SV exclusion
        if d > worst:                                 # (a tie keeps the lower SV: masks are visited in order)
            suspect, worst = out.bit_length() - 1, d
    return suspect, sep


def run_fde_closed_loop(iq_windows, ho, fs, pos_grid, vel_grid, threshold_m, time_grid=(0.0,), init_delta=(0, 0, 0, 0), K=None, lpower=1,
                        lag_half_width=None, bin_half_width=None, exclude=True, keep_scores=False):
    """The closed loop with fault detection and exclusion (engine.SubsetManifold): every window is scanned ONCE with the K
    leave-one-out masks; solution_separation names a suspect SV or none.  With a suspect the window's fix is the zVal of the
    subset without that SV, else the full set's.  The channel manager keeps all K channels and back-computes them from the
    chosen fix; nothing is remembered from one window to the next (exclude=False: suspects are logged, the fix stays the full
    set's).  init_delta: ECEF / clock offset of the initial state, 4 entries, or 8 with the velocity and drift.
    Returns fixes [W, 8], suspects int [W], separations [W, K] and the per-window result dicts."""
    def make_bcm(S, nfft, L, B, K):
        return engine.SubsetManifold(fs, S, nfft, pos_grid, vel_grid, K, LPower=lpower, lag_half_width=L, bin_half_width=B, max_channels=K)

    with _single_rx_loop(iq_windows, ho, fs, K, init_delta, partial(bank_half_widths, pos_grid, vel_grid), make_bcm,
                         lag_half_width=lag_half_width, bin_half_width=bin_half_width) as lp:
        bcs, bcm, cm, x, W, K = lp.bcs, lp.bcm, lp.cm, lp.x, lp.W, lp.K
        masks = engine.leave_one_out_masks(K)
        fixes, suspects, seps, results = np.zeros((W, 8)), np.full(W, -1, dtype=np.int64), np.zeros((W, K)), []
        for w in range(W):
            (cm.Start if w == 0 else cm.Update)(x, x, time_grid)
            cs, ce, bw = cm.outputs()
            bcs.Update(lp.iq_d[w], cs)
            bcm.Update(bcs.CodeScores, bcs.CarrScores, bw, ce, masks)
            r = bcm.results()[0]
            if keep_scores:
                ps, vs = bcm.read_scores()
                r["posScores"], r["velScores"] = ps[0].copy(), vs[0].copy()
            suspects[w], seps[w] = solution_separation(r, r["subs"], masks, threshold_m, K)
            r["suspect"] = int(suspects[w])
            chosen = r["subs"][suspects[w]] if (exclude and suspects[w] >= 0) else r
            x = chosen["zVal"].copy()
            fixes[w] = x
            results.append(r)
    return fixes, suspects, seps, results


def run_vector_tracking(samples, start, fs, n_epochs=None, T=1e-3, N=20, fix=None, Sigma=None, stream=None, **cfg):
    """The vector-tracking loop (engine.VectorTracker) over `samples` (int16 interleaved I/Q, numpy or a device tensor;
    n_epochs * N windows of round(T fs) samples from the sample `start` refers to).
    start: a handoff dict (handoff.read_handoff's / ScalarNavigator.handoff's form: the state and the channels' rc ri fc fi cp at
    the first sample), or a (ScalarTracker, ScalarNavigator) pair -- then the channels are taken from the tracker's device state and
    `fix` (default: the navigator's solve_log at the tracker's last window) gives X and rxTime.
    Returns (log = VectorTracker.read_log's per-epoch states, handoff = the end state as a handoff dict, which ChanMgr.from_handoff
    and run_closed_loop accept as they accept ScalarNavigator.handoff's, device status)."""
    import torch
    from . import engine
    S = int(round(T * fs))
    x = samples if hasattr(samples, "data_ptr") else torch.from_numpy(np.ascontiguousarray(samples, dtype=np.int16)).to("cuda:0")
    if n_epochs is None:
        n_epochs = int(x.numel() // (2 * S * N))
    assert x.numel() >= 2 * S * N * n_epochs, "the record is shorter than n_epochs epochs"
    if isinstance(start, dict):
        prns = [int(p) for p in start["prn_list"]]
        vt = engine.VectorTracker(fs, prns, T=T, N=N, log_capacity_epochs=max(int(n_epochs), 1), **cfg)
        vt.set_ephemerides(start["eph"], start["TOW"], start["cp_timestamp"])
        chan = np.stack([np.asarray(start[n], dtype=np.float64) for n in ("rc", "ri", "fc", "fi", "cp")], axis=1)
        Sg = np.diag([1.0e4, 1.0e4, 1.0e4, 1.0e4, 1.0, 1.0, 1.0, 1.0]) if Sigma is None else Sigma
        vt.init(start["X_ECEF"], Sg, start["rxTime"], chan, stream)
    else:
        trk, nav = start
        vt = engine.VectorTracker(fs, trk.prns, T=T, N=N, log_capacity_epochs=max(int(n_epochs), 1), **cfg)
        vt.set_ephemerides(nav.eph, nav.tow, nav.cp_timestamp)
        if fix is None:
            fix = nav.solve_log(trk, first=trk.n_windows - 1, n_epochs=1, stream=stream)[0]
        vt.init_from_tracker(trk, fix, stream)
    vt.track(x, n_epochs, stream)
    log = vt.read_log(stream=stream)
    ho = vt.handoff(bytes_read=4 * S * N * n_epochs, stream=stream)
    status = vt.dev_status(stream)
    vt.close()
    return log, ho, status


def run_monte_carlo(ho, fs, S, K, pos_grid, vel_grid, cn0_dbhz, n_real, seed, init_delta=(0, 0, 0, 0), lpower=1, weighted_mean=False,
                    sigma=300.0, lag_half_width=None, bin_half_width=None):
    """RMSE against C/N0 over noise realisations made on the device: the batch dimension is the realisation.

    One ChanMgr.Start at the true state X_ECEF of the handoff, with the grids centred on X_ECEF + init_delta (up to 8 entries, ECEF),
    gives the window's parameters.  Per level c of cn0_dbhz (dB-Hz; every SV at amplitude synth.cn0_to_amp(c, sigma, fs)),
    Synthesizer.windows makes n_real windows of S samples that differ only in the noise stream -- realisation r of level l draws
    stream l n_real + r under `seed`, no nav-bit flip, no DC offset -- and one stage-1 update and one manifold update run over the
    batch.  Nothing but the fixes leaves the device.  Returns one dict per level: cn0_dbhz, amp, fixes [n_real, 8] (the ML fix
    zVal of every realisation), pos_index / vel_index [n_real], pos_out_of_window / vel_out_of_window [n_real], and the root mean
    square errors against the truth rmse_enu [3], rmse_3d, rmse_clock (m), rmse_vel (3-D, m/s), rmse_drift (m/s); with
    weighted_mean also mean_fixes [n_real, 8] and the same errors of the score-weighted mean under mean_rmse_*."""
    from . import synth
    truth = np.array(ho["X_ECEF"], dtype=np.float64).copy()
    centre = truth.copy()
    d0 = np.asarray(init_delta, dtype=np.float64)
    centre[:d0.shape[0]] += d0
    nfft = engine.carr_fft_len(S)
    L, B = bank_half_widths(pos_grid, vel_grid, fs, nfft)
    # the replica follows the truth and the grid its own centre: the banks have to reach across the offset between the two as well
    L += int(np.ceil((np.linalg.norm(d0[:3]) + (abs(d0[3]) if d0.shape[0] > 3 else 0.0)) * fs / 299792458.0))
    if d0.shape[0] > 4:
        dv = np.zeros(4)
        dv[:d0.shape[0] - 4] = d0[4:]
        B += int(np.ceil((np.linalg.norm(dv[:3]) + abs(dv[3])) * (nfft / fs) * 1.57542e9 / 299792458.0))
    L = L if lag_half_width is None else int(lag_half_width)
    B = B if bin_half_width is None else int(bin_half_width)
    n_real = int(n_real)
    cm = engine.ChanMgr.from_handoff(ho, S / fs, K)
    bcs = engine.BatchCorrScores(fs, samples_per_window=S, lag_half_width=L, bin_half_width=B, max_windows=n_real, max_channels=K)
    bcm = engine.BatchCorrManifold(fs, S, nfft, pos_grid, vel_grid, LPower=lpower, lag_half_width=L, bin_half_width=B,
                                   max_windows=n_real, max_channels=K, write_scores=False, weighted_mean=weighted_mean)
    syn = None
    out = []
    try:
        cm.Start(truth, centre, (0.0,))
        cs, ce, bw = cm.outputs()
        cs_b, ce_b, bw_b = np.tile(cs, (n_real, 1)), np.tile(ce, (n_real, 1)), np.tile(bw, n_real)
        R = np.asarray(bw["enu2ecef"][0], dtype=np.float64).reshape(3, 3)
        bcs.Start()
        bcm.Start()
        syn = engine.Synthesizer(fs, max_segments=n_real, max_channels=K)
        iq_d = None

        def rmse(fixes):
            e = fixes - truth[None, :]
            enu = e[:, :3] @ R                      # R maps ENU to ECEF: its transpose takes the error back
            ms = lambda v: float(np.sqrt(np.mean(np.sum(np.square(v), axis=-1))))    # noqa: E731
            return dict(rmse_enu=np.sqrt(np.mean(np.square(enu), axis=0)), rmse_3d=ms(enu), rmse_clock=ms(e[:, 3:4]),
                        rmse_vel=ms(e[:, 4:7]), rmse_drift=ms(e[:, 7:8]))

        for lev, c in enumerate(np.atleast_1d(np.asarray(cn0_dbhz, dtype=np.float64))):
            amp = float(synth.cn0_to_amp(c, sigma, fs))
            iq_d = syn.windows(S, cs_b, amp=amp, sigma=sigma, dc=(0.0, 0.0), flip=None, seed=seed, first_stream=lev * n_real, out=iq_d)
            bcs.Update(iq_d, cs_b)
            bcm.Update(bcs.CodeScores, bcs.CarrScores, bw_b, ce_b)
            res = bcm.results()
            fixes = np.stack([r["zVal"] for r in res])
            row = dict(cn0_dbhz=float(c), amp=amp, fixes=fixes, pos_index=np.array([r["posIndex"] for r in res]),
                       vel_index=np.array([r["velIndex"] for r in res]),
                       pos_out_of_window=np.array([r["posOutOfWindow"] for r in res]),
                       vel_out_of_window=np.array([r["velOutOfWindow"] for r in res]), **rmse(fixes))
            if weighted_mean:
                row["mean_fixes"] = np.stack([r["zValMean"] for r in res])
                row.update({"mean_" + k: v for k, v in rmse(row["mean_fixes"]).items()})
            out.append(row)
    finally:
        if syn is not None:
            syn.close()
        cm.Stop()
        bcm.Stop()
        bcs.Stop()
    return out


def collective_detection(acq, samples, eph, prns, p0, rx_time, enu_grid, drift_half_width=0, detector=None, stream=None):
    """Weak-signal cold start: acq.search on `samples` (device int16, one window), one collective scan of its surfaces over
    enu_grid x clock bias x clock drift about the a-priori ECEF position p0 at the coarse GPS time rx_time, then acq.fine on the
    per-SV results.  prns: the SVs to combine, each one of acq.prns; eph [K, 21] in their order.  Returns a dict: `fix`
    (CollectiveDetector.results()' first part), `coarse` (per SV of acq.prns, Acquisition.results()' shape: the collective entry
    for the SVs combined, the ordinary one for the others), `tracker_init` (Acquisition.fine's output with `found`, for
    ScalarTracker.set_params), `ordinary` (acq.results()) and `sv` (the predictions).  detector: a CollectiveDetector to reuse."""
    from . import synth
    prns = [int(p) for p in prns]
    rows = [acq.prns.index(p) for p in prns]
    cd = detector or engine.CollectiveDetector(acq.fs, acq.M, acq.bins, enu_grid, drift_half_width=drift_half_width,
                                               max_sv=min(max(len(prns), 1), engine.CollectiveDetector.MAX_SV), ds=acq.ds)
    try:
        sv = cd.predict(eph, prns, rows, p0, rx_time)
        acq.search(samples, stream)
        ordinary = acq.results(stream)
        cd.update(acq, sv, p0, synth.enu2ecef_matrix(p0), stream=stream)
        fix, per_sv = cd.results()
    finally:
        if detector is None:
            cd.close()
    coarse = [dict(r) for r in ordinary]
    for row, r in zip(rows, per_sv):
        coarse[row] = dict(ordinary[row], **r)
    fine = acq.fine(samples, coarse, stream)
    init = [dict(f, found=c["found"]) for f, c in zip(fine, coarse)]
    return dict(fix=fix, coarse=coarse, tracker_init=init, ordinary=ordinary, sv=sv)
