"""CPU: the oracle's per-receiver rows in the joint-scan contract against the O16 fixture = the reference's Python twin in its
multi receiver mode (Receiver.dp_measurement_estimation_unfolded(gXk_grid=...), receiver.py:340-345, 385-388) for two receivers
assembled as O7 assembles one (tests/golden/make_golden_o16.py).

The contract pinned: grid point j of receiver r is X_r + offsets_j with ONE ENU->ECEF rotation for the set (receiver 0's), each
receiver's geometry about its OWN state, receive time and channel parameters; the caller sums the rows and takes one arg-max.
That is what tests/joint_world.oracle_rows sums and what dpe_bcm_update_joint is held to.  Bounds are O7's (tests/test_oracle_o7.py):
rows to 1e-9 of their maximum, identical arg-max."""
import hashlib
import os
import sys

import numpy as np

import navlab_dpe_sdr_amd as dpe

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))


def test_o16_two_receivers_in_the_twins_multi_receiver_mode(golden, oracle):
    import __graft_entry__ as ge
    ge.build()                              # (the receivers' channel parameters come through the product's host channel manager)
    import make_golden_o16 as m16          # synthesis inputs only: receivers() and window() do not touch the reference tree
    o = oracle
    g = golden("o16_multi_receiver")
    fs, S, C = float(g["fs"]), int(g["S"]), int(g["C"])
    assert tuple(g["seeds"]) == m16.O16_SEEDS and tuple(g["sel1"]) == m16.O16_SEL1
    hos = m16.receivers()
    pos, vel = dpe.synth.spread_grid()
    tg = np.unique(pos[:, 3])
    sum_p, sum_v, R0 = 0.0, 0.0, None
    for r, ho in enumerate(hos):
        X = np.array(ho["X_ECEF"], dtype=np.float64)
        assert np.array_equal(X, g["X_ECEF_%d" % r]) and np.array_equal(ho["prn_list"], g["prn_%d" % r])
        iq = m16.window(ho, m16.O16_SEEDS[r])
        assert hashlib.sha256(iq.tobytes()).hexdigest() == str(g["iq_sha256_%d" % r])
        K = len(ho["prn_list"])
        cm = o.ChanMgr(ho["prn_list"], ho["rc"], ho["ri"], ho["fc"], ho["fi"], ho["cp"], ho["cp_timestamp"], ho["TOW"], ho["eph"],
                       ho["rxTime"], 0.02)
        batch, R = cm.start(X, X, tg)
        R0 = R.copy() if r == 0 else R0          # one rotation for the set: receiver 0's
        assert np.abs(cm.rcEnd - g["end_rc_%d" % r]).max() < 1e-7 and cm.rxTime == float(g["rxTime_%d" % r])
        code, carr = [], []
        for k in range(K):
            c, f, _ = o.bcs_sv(iq, fs, int(ho["prn_list"][k]), cm.rcStart[k], cm.riStart[k], cm.fc[k], cm.fi[k], int(cm.cpElaStart[k]),
                               int(cm.cpRef[k]), -64, 64, -256, 256, C)
            code.append(c)
            carr.append(f)
        sat = batch[:, tg.size // 2]
        sp, oobp = o.bcm_pos(sat, np.stack(code), S // 2 - 64, X, pos, R0, cm.fc, cm.cpRefTOW, cm.cpElaEnd, cm.cpRef, cm.rcEnd, cm.rxTime,
                             fs, S, 1)
        sv, oobv = o.bcm_vel(sat, np.stack(carr), C // 2 - 256, X, vel, R0, cm.fi, cm.rxTime, fs, C, 1, 1)
        assert oobp == 0 and oobv == 0
        errs = dict(pos97=np.abs(sp[::97] - g["pos_every97_%d" % r]).max() / g["pos_every97_%d" % r].max(),
                    vel97=np.abs(sv[::97] - g["vel_every97_%d" % r]).max() / g["vel_every97_%d" % r].max(),
                    pos_top=np.abs(sp[g["top_pos_idx_%d" % r]] - g["top_pos_%d" % r]).max() / g["top_pos_%d" % r].max(),
                    vel_top=np.abs(sv[g["top_vel_idx_%d" % r]] - g["top_vel_%d" % r]).max() / g["top_vel_%d" % r].max())
        print("receiver %d against the twin:" % r, {k: float("%.3g" % v) for k, v in errs.items()})
        assert all(v < 1e-9 for v in errs.values()), errs
        assert o.argmax_first(sp) == int(g["argmax_pos_%d" % r]) and o.argmax_first(sv) == int(g["argmax_vel_%d" % r])
        sum_p, sum_v = sum_p + sp, sum_v + sv
    # the caller's part: one arg-max over the summed rows
    assert o.argmax_first(sum_p) == int(g["argmax_pos"]) and o.argmax_first(sum_v) == int(g["argmax_vel"])
    assert abs(sum_p.max() - float(g["max_pos"])) < 1e-9 * float(g["max_pos"])
    assert abs(sum_v.max() - float(g["max_vel"])) < 1e-9 * float(g["max_vel"])
