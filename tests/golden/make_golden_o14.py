#!/usr/bin/env python3
"""Fixture O14: the reference twin's own scalar tracking loop on one continuous synthetic recording.

Run where the reference tree is available (as make_golden.py, whose harness this imports and which stays as it is):

    python tests/golden/make_golden_o14.py

  O14 Receiver.scalar_track after Channel.set_scalar_params      receiver.py:522-542; scalar/channel.py:82-122,173-191,247-273;
      scalar/correlator.py:135-283

Recording: dpe.synth.gen_iq_record at 2.5 Msps, four PRNs with Dopplers of both signs, a nav-bit sign every 20 code periods.
Start parameters are off the truth by what acquisition leaves: a fraction of a chip, some tens of Hz, some hundredths of a cycle.
Channel 2 starts with its code phase 0.002 chips above 0 and a code Doppler of 0.04 chips/s, which the code loop's own
corrections outweigh: its windows visit all three boundary cases of scalar_correlate.  M = 360 windows: every channel's lock
detector declares lock (which takes more than 240 consecutive windows) and 18 nav bits per channel lie inside.
Only DATA is written: synthesis inputs, a digest of the samples (the tests rebuild them) and the twin's logs."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (import_pygnss / open_rawfile; puts the repository root on sys.path)

dpe = mg.dpe

O14_FS, O14_T, O14_M, O14_SEED, O14_SIGMA = 2.5e6, 1e-3, 360, 15, 300.0
O14_PRN = (4, 9, 17, 23)
O14_FI = (-2350.3, 1120.7, 60.0, -640.9)
O14_RC = (311.37, 870.81, 1022.99, 95.13)
O14_RI = (0.13, 0.71, 0.42, 0.88)
O14_CP_REF = (3, 11, 7, 16)            # first nav-bit edge, in code periods after the one sample 0 lies in
O14_AMP = (70.0, 55.0, 80.0, 60.0)
O14_D_RC = (0.17, -0.12, 0.012, -0.2)  # start - truth
O14_D_FI = (14.0, -22.0, 9.0, 31.0)
O14_D_RI = (0.06, -0.09, 0.04, 0.1)
LOG_NAMES = ("cp", "rc", "ri", "fc", "fi", "iE", "qE", "iP", "qP", "iL", "qL", "dc", "di", "efc", "efi", "dpc", "dpi",
             "fc_bias", "fi_bias", "lock", "lockval", "snr")


def o14_inputs():
    fi = np.array(O14_FI)
    ch = dict(prn=np.array(O14_PRN, dtype=np.int32), rc=np.array(O14_RC), ri=np.array(O14_RI), fc=1.023e6 * (1.0 + fi / 1.57542e9),
              fi=fi, cp_ref=np.array(O14_CP_REF, dtype=np.int32))
    S = int(round(O14_FS * O14_T))
    n_samples = (O14_M + 2) * S
    iq, bits = dpe.synth.gen_iq_record(O14_SEED, O14_FS, n_samples, ch, amp=np.array(O14_AMP), sigma=O14_SIGMA)
    fi0 = fi + np.array(O14_D_FI)
    start = np.stack([np.mod(ch["rc"] + np.array(O14_D_RC), 1023.0), ch["ri"] + np.array(O14_D_RI),
                      1.023e6 + 1.023e6 / 1.57542e9 * fi0, fi0], axis=1)      # fc as acquisition sets it: F_CA + fcaid fi
    return ch, iq, bits, start, n_samples


def make_o14(pg):
    ch, iq, bits, start, n_samples = o14_inputs()
    path = os.path.join(mg.SCRATCH, "o14.dat")
    iq.tofile(path)
    rf = mg.open_rawfile(pg, path, O14_FS, O14_T)
    prns = [int(p) for p in O14_PRN]
    rx = pg.receiver.Receiver(rf, mcount_max=O14_M + 4)
    rx.add_channels(prns)
    for k, p in enumerate(prns):
        rx.channels[p].set_scalar_params(rc=start[k, 0], ri=start[k, 1], fc=start[k, 2], fi=start[k, 3])
    rx.scalar_track(mtrack=O14_M)
    M = O14_M
    out = {"log_" + n: np.stack([np.asarray(getattr(rx.channels[p], n), dtype=np.float64)[:M + 1] for p in prns], axis=1) for n in LOG_NAMES}
    ncp = np.array([int(rx.channels[p]._cpcount) for p in prns])
    cp_sign = np.full((len(prns), 2 * M), np.nan)
    for k, p in enumerate(prns):
        cp_sign[k, :ncp[k]] = rx.channels[p].cp_sign[:ncp[k]]
    p_a = np.array([complex(rx.channels[p].correlator.p_a) for p in prns])
    rf.close_rawfile()
    nb = max(b.size for b in bits)
    nav = np.zeros((len(prns), nb), dtype=np.int8)
    for k, b in enumerate(bits):
        nav[k, :b.size] = b
    np.savez_compressed(os.path.join(HERE, "o14_scalar_track.npz"), iq_sha256=hashlib.sha256(iq.tobytes()).hexdigest(), fs=O14_FS, T=O14_T,
                        S=int(round(O14_FS * O14_T)), M=M, seed=O14_SEED, sigma=O14_SIGMA, n_samples=n_samples, amp=np.array(O14_AMP),
                        prn=ch["prn"], syn_rc=ch["rc"], syn_ri=ch["ri"], syn_fc=ch["fc"], syn_fi=ch["fi"], syn_cp_ref=ch["cp_ref"],
                        nav_bits=nav, nav_bits_n=np.array([b.size for b in bits]), start=start, cp_sign=cp_sign, cp_sign_n=ncp,
                        p_a_end=p_a, **out)
    print("o14_scalar_track.npz %d bytes" % os.path.getsize(os.path.join(HERE, "o14_scalar_track.npz")))


if __name__ == "__main__":
    make_o14(mg.import_pygnss())
