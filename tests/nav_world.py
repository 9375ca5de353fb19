"""Test-side synthetic world for the scalar navigation chain: a continuous record whose geometry is exact at one epoch.

The receiver state X_true and the ephemerides are the shipped handoff's.  At the epoch (receive time t_e, sample n_e) every
channel's transmit time solves  tx = t_e - (|R(tau) sat(tx) - x| - c clk(tx) + c dt) / c  -- the fixed point workload.extend_handoff
iterates, here with the oracle's satellite routine -- and its Doppler is the line-of-sight rate there.  Code and carrier then run
backwards (and on) at constant fc, fi; a code period lasts 1 ms of transmit time, so nav bits change where the transmit time
passes a multiple of 20 ms and subframes start at multiples of 6 s (tests/nav_synth.py encodes them)."""
import numpy as np

from tests import nav_synth as ns

C, FCA, FL1, OE = 299792458.0, 1.023e6, 1.57542e9, 7.2921151467e-5


def channel_at(oracle, eph, X, t_e, ds=1.0):
    """-> transmit time, carrier Doppler fi (Hz), code rate fc at receive time t_e for the receiver state X [8]."""
    tx = t_e - 0.07
    for _ in range(8):
        s, rc = oracle.sat_pos(eph, tx)
        assert rc == 0
        tau = t_e - (tx + X[3] / C) + s[3]
        a = -OE * tau
        ca, sa = np.cos(a), np.sin(a)
        p = np.array([ca * s[0] - sa * s[1], sa * s[0] + ca * s[1], s[2]])
        v = np.array([ca * s[4] - sa * s[5] - OE * sa * s[0] - OE * ca * s[1], sa * s[4] + ca * s[5] + OE * ca * s[0] - OE * sa * s[1], s[6]])
        los = p - X[:3]
        rng = np.linalg.norm(los)
        tx = t_e - (rng - C * s[3] + X[3]) / C
    e = np.array([X[4] - OE * X[1], X[5] + OE * X[0], X[6]])
    lrr = (los / rng) @ (e - v)
    fi = FL1 * ((lrr - X[7]) / C + s[7]) / ds
    return tx, fi, FCA + (ds * FCA / FL1) * fi


def build(oracle, ho, chans, fs, n_epoch, seed=0, t_epoch=None):
    """The world for the handoff's channels `chans` with the epoch at sample n_epoch.  Returns dict(ch = gen_iq_record's channel
    dict referred to sample 0, nav_bits, truth = the handoff dict of the TRUE state at the epoch (code periods counted from the one
    sample 0 lies in), txms0 = the transmit time in ms at the start of that code period, per channel)."""
    X = np.array(ho["X_ECEF"], dtype=np.float64)
    t_e = float(ho["rxTime"]) if t_epoch is None else float(t_epoch)    # (chosen so that the record starts shortly before a subframe edge)
    K = len(chans)
    T = n_epoch / fs
    rng = np.random.default_rng(seed)
    ch = dict(prn=ho["prn_list"][chans].astype(np.int32), rc=np.zeros(K), ri=rng.uniform(0, 1, K), fc=np.zeros(K), fi=np.zeros(K),
              cp_ref=np.zeros(K, dtype=np.int64))
    truth = dict(rxTime=t_e, rxTime_a=t_e - X[3] / C, X_ECEF=X.copy(), bytes_read=4 * n_epoch, prn_list=ch["prn"].copy(),
                 rc=np.zeros(K), ri=np.zeros(K), fc=np.zeros(K), fi=np.zeros(K), cp=np.zeros(K, dtype=np.int32),
                 cp_timestamp=np.zeros(K, dtype=np.int32), TOW=np.zeros(K, dtype=np.int32), eph=ho["eph"][chans].copy())
    nav_bits, txms0 = [], np.zeros(K, dtype=np.int64)
    for j, k in enumerate(chans):
        tx, fi, fc = channel_at(oracle, ho["eph"][k], X, t_e)
        ms_e = int(np.floor(tx * 1000.0))                       # transmit time of the epoch's code period start, ms
        rc_e = (tx - ms_e / 1000.0) * FCA
        chips0 = rc_e - fc * T                                  # code phase at sample 0, in chips from the epoch's period start
        p0 = int(np.floor(chips0 / 1023.0))                     # (negative) period sample 0 lies in
        ch["rc"][j], ch["fc"][j], ch["fi"][j] = chips0 - 1023.0 * p0, fc, fi
        txms0[j] = ms_e + p0                                    # transmit time at the start of sample 0's code period, ms
        edge = int((-txms0[j]) % 20)
        ch["cp_ref"][j] = edge
        # nav bits from an encoded stream that starts one subframe before the record
        t0 = 6000 * (txms0[j] // 6000) - 6000
        n_sub = int((T + 0.2) // 6) + 4
        ids = [((t0 // 6000 + i) % 5) + 1 for i in range(n_sub)]
        q = ns.quantise(ns.eph_row_to_dict(ho["eph"][k]))
        enc = 1 - 2 * ns.encode_bits(ids, int(t0 // 1000), q, week=2008, iode=40 + j, iodc=40 + j).astype(np.int8)
        nb = int((T + 0.2) * 50) + 3
        first = txms0[j] + (edge if edge else 20) - 20          # bit 0 covers the periods before the first edge
        g = (first - t0) // 20 + np.arange(nb)
        nav_bits.append(enc[g])
        truth["rc"][j], truth["fc"][j], truth["fi"][j] = rc_e, fc, fi
        truth["ri"][j] = (ch["ri"][j] + fi * T) % 1.0
        truth["cp"][j] = -p0
        sf = 6000 * (-(-txms0[j] // 6000))                      # first subframe start at or after sample 0's period
        truth["cp_timestamp"][j], truth["TOW"][j] = sf - txms0[j], sf // 1000
    return dict(ch=ch, nav_bits=nav_bits, truth=truth, txms0=txms0)


def expected_timestamp(world, j, first_sign_period=0):
    """(TOW, cp) the twin's convention gives channel j when its sign stream starts in code period first_sign_period (counted from
    the one sample 0 lies in): the start of the first of subframes 1-3 whose preamble lies inside the stream."""
    t0 = int(world["txms0"][j])
    sf = 6000 * (-(-(t0 + first_sign_period + 40) // 6000))     # 40 entries of history before it
    while ((sf // 6000) % 5) + 1 > 3:
        sf += 6000
    return sf // 1000, sf - t0 - first_sign_period
