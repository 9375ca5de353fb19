#!/usr/bin/env python3
"""Fixture O16: the reference twin's multi receiver mode for two receivers of a rigid set.

Run where the reference tree is available (as make_golden.py, whose harness this imports and which stays as it is):

    python tests/golden/make_golden_o16.py

  O16 Receiver.dp_measurement_estimation_unfolded(gXk_grid=...)   receiver.py:325-388 ("multi receiver mode", :340-345, :385-388)

Two Receiver objects, each assembled as O7 assembles its one (make_golden.py: handoff state, ephemerides, one geometry-consistent
synthetic 20 ms window, dp_time_update_state / dp_time_update_channels_unfolded).  Receiver 0 is the handoff's own: its state X
and its 8 SVs.  Receiver 1 sits at X + R b (b = 1.2 m east, 0.5 m south, 0.3 m up) with a clock offset of 7.5 m and tracks 6 of
the SVs; its code phases, code rates and Dopplers are re-derived for that position (tests/joint_world.handoff_at).  The caller's
part of the mode: the grid of full states of receiver r is gX_r = X_r + offsets, the offsets being receiver 0's spread grid
about its own state (NavigationGuesses.get_nav_guesses, ECEF_only) minus that state -- one ENU->ECEF rotation for the set.
Every receiver leaves pos_corr / vel_fft behind; the caller sums them and takes one arg-max.

Only DATA is written: synthesis inputs and a digest of the samples (the test rebuilds them), every 97th entry and the top 32
of pos_corr / vel_fft per receiver, and the arg-max of the summed rows."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (import_pygnss / open_rawfile / Eph; puts the repository root on sys.path)

dpe = mg.dpe

O16_FS, O16_T, O16_AMP = 2.5e6, 0.02, 200.0
O16_SEEDS = (161, 162)
O16_SEL1 = (0, 2, 3, 5, 6, 7)                 # receiver 1's SVs, as indices into the handoff's list
O16_BASELINE = (1.2, -0.5, 0.3)               # ENU, metres
O16_CLOCK = 7.5                               # metres


def receivers():
    """-> the two handoff states (receiver 0: the file's own; receiver 1: re-derived at its position)."""
    from oracle import oracle as o
    from tests import joint_world as jw
    ho = dpe.handoff.read_handoff(dpe.workload.HANDOFF_CSV)
    X = np.array(ho["X_ECEF"], dtype=np.float64)
    R3 = o.enu2ecef(o.ecef2ll(X)).reshape(3, 3)
    X1 = X.copy()
    X1[:3] += R3 @ np.array(O16_BASELINE)
    X1[3] += O16_CLOCK
    return [ho, jw.handoff_at(list(O16_SEL1), X1)]


def window(ho, seed):
    S = int(round(O16_FS * O16_T))
    ch = dict(prn=ho["prn_list"], rc=ho["rc"], ri=ho["ri"], fc=ho["fc"], fi=ho["fi"], cp=ho["cp"], cp_ref=ho["cp_timestamp"])
    return dpe.synth.gen_iq(seed, O16_FS, S, ch, amp=O16_AMP, flip=np.zeros(len(ho["prn_list"]), dtype=bool))


def main():
    pg = mg.import_pygnss()
    fs, T = O16_FS, O16_T
    S = int(round(fs * T))
    hos = receivers()
    rxs, out = [], {}
    for r, ho in enumerate(hos):
        prns = [int(p) for p in ho["prn_list"]]
        iq = window(ho, O16_SEEDS[r])
        out["iq_sha256_%d" % r] = hashlib.sha256(iq.tobytes()).hexdigest()
        path = os.path.join(mg.SCRATCH, "o16_%d.dat" % r)
        iq.tofile(path)
        rf = mg.open_rawfile(pg, path, fs, T)
        rx = pg.receiver.Receiver(rf, mcount_max=8)
        rx.add_channels(prns)
        for k, p in enumerate(prns):
            rx.channels[p].ephemerides = mg.Eph(ho, k)
        rx.ekf = pg.ekf.ExtendedKalmanFilter(np.asmatrix(ho["X_ECEF"]).T, T=T)
        rx.navguess = pg.receiver.NavigationGuesses()
        rx.rxTime = ho["rxTime"]
        rx.ekf.X_ECEF = np.matrix(ho["X_ECEF"]).T
        rx.rxTime_a = rx.rxTime - (rx.ekf.X_ECEF[3, 0] / 299792458.0)
        for k, p in enumerate(prns):
            c = rx.channels[p]
            c.rc[0], c.ri[0], c.fc[0], c.fi[0], c.cp[0] = ho["rc"][k], ho["ri"][k], ho["fc"][k], ho["fi"][k], float(ho["cp"][k])
        rf.seek_rawfile(rf.S_skip)
        rf.update_rawsnippet()
        rx.dp_time_update_state()
        rx.dp_time_update_channels_unfolded()
        rx._mcount += 1
        rxs.append((rx, rf, prns))
    # the caller's part: one grid of offsets (receiver 0's spread grid about its own state), gX_r = X_r + offsets
    rx0 = rxs[0][0]
    gfv0, gfp0 = rx0.navguess.get_nav_guesses(rx0.ekf.X_ECEF, rx0.rxTime_a, ECEF_only=True)
    off_v, off_p = np.asarray(gfv0) - np.asarray(rx0.ekf.X_ECEF), np.asarray(gfp0) - np.asarray(rx0.ekf.X_ECEF)
    sum_p, sum_v = 0.0, 0.0
    for r, (rx, rf, prns) in enumerate(rxs):
        Xr = np.asarray(rx.ekf.X_ECEF)
        rx.dp_measurement_estimation_unfolded(gXk_grid=(np.matrix(Xr + off_v), np.matrix(Xr + off_p)))
        pos_corr, vel_fft = np.asarray(rx.pos_corr).ravel(), np.asarray(rx.vel_fft).ravel()
        sum_p, sum_v = sum_p + pos_corr, sum_v + vel_fft
        mc = rx._mcount
        top_p = np.argsort(-pos_corr, kind="stable")[:32]
        top_v = np.argsort(-vel_fft, kind="stable")[:32]
        out.update({"X_ECEF_%d" % r: Xr.ravel().copy(), "prn_%d" % r: np.array(prns), "rxTime_%d" % r: rx.rxTime,
                    "end_rc_%d" % r: np.array([rx.channels[p].rc[mc] for p in prns]),
                    "end_fi_%d" % r: np.array([rx.channels[p].fi[mc] for p in prns]),
                    "pos_every97_%d" % r: pos_corr[::97], "vel_every97_%d" % r: vel_fft[::97],
                    "top_pos_idx_%d" % r: top_p, "top_pos_%d" % r: pos_corr[top_p],
                    "top_vel_idx_%d" % r: top_v, "top_vel_%d" % r: vel_fft[top_v],
                    "argmax_pos_%d" % r: int(np.argmax(pos_corr)), "argmax_vel_%d" % r: int(np.argmax(vel_fft))})
        rf.close_rawfile()
    path = os.path.join(HERE, "o16_multi_receiver.npz")
    np.savez_compressed(path, fs=fs, T=T, S=S, C=int(rxs[0][1].carr_fftpts), seeds=np.array(O16_SEEDS), sel1=np.array(O16_SEL1),
                        baseline=np.array(O16_BASELINE), clock=O16_CLOCK, argmax_pos=int(np.argmax(sum_p)),
                        argmax_vel=int(np.argmax(sum_v)), max_pos=float(sum_p.max()), max_vel=float(sum_v.max()), **out)
    print("%s %d bytes" % (os.path.basename(path), os.path.getsize(path)))


if __name__ == "__main__":
    main()
