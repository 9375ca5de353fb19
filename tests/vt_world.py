"""Test-side synthetic world for vector tracking: tests/nav_world.py's world (a static receiver at the shipped handoff's state,
geometry exact at one epoch) on a short record whose exact-geometry epoch lies in the MIDDLE of the span, plus a record generator
that gives every channel an amplitude profile over time (the per-channel signals are summed before quantisation, as
synth.gen_iq_record sums them).

The world holds every channel's fc and fi constant away from the epoch.  Over the <= 0.5 s between the epoch and
either end of the record a satellite's line-of-sight acceleration (< 0.2 m/s^2) moves the true range by a t^2 / 2 < 2.5 cm and the
receiver's 0.18 m/s by < 9 cm: the record's truth is the static X_true to centimetres, far below the metres the tests resolve."""
import numpy as np

import navlab_dpe_sdr_amd as dpe
from tests import helpers, nav_world

FS = 2.5e6
CHANS = [0, 1, 2, 3, 4, 6]                      # rows of the shipped handoff (tests/test_gpu_nav_chain.py uses the same)
AMP, SIGMA = 90.0, 300.0
L_CA = 1023


def synthetic_handoff(ho, K):
    """A handoff of K channels with PRNs 1 .. K: the shipped ephemerides reused in turn, each reuse with its mean anomaly and its
    ascending node shifted, so that the K satellites stand in K different directions."""
    n = len(ho["prn_list"])
    out = dict(ho)
    eph = np.zeros((K, ho["eph"].shape[1]))
    for k in range(K):
        eph[k] = ho["eph"][k % n]
        eph[k, 5] += 0.11 * (k // n) + 0.013 * k       # M_0
        eph[k, 3] += 0.17 * (k // n) - 0.009 * k       # OMEGA_0
    out["eph"] = eph
    out["prn_list"] = np.arange(1, K + 1, dtype=np.int32)
    return out


def build(oracle, n_samples, chans=CHANS, fs=FS, seed=4, ho=None, ds=1.0):
    """nav_world.build with the epoch at sample n_samples // 2.  Adds `start`: the true state at sample 0 in the form the vector
    tracker is initialised with (rxTime0, chan [K, 5] = rc ri fc fi cp, tow, cps, eph, prns, X).
    ds = -1: the same world seen by a front end whose spectrum runs the other way: every fi negated, fc as it is (record() rotates by
    ch["fi"], so the record is the mirrored one)."""
    ho = dpe.handoff.read_handoff(helpers.HANDOFF) if ho is None else ho
    n_e = n_samples // 2
    w = nav_world.build(oracle, ho, list(chans), fs, n_e, seed=seed, t_epoch=ho["rxTime"] + 2.0)
    ch, truth = w["ch"], w["truth"]
    assert ds in (1.0, -1.0)
    if ds == -1.0:
        ch["fi"] = -np.asarray(ch["fi"], dtype=np.float64)
    K = len(chans)
    # nav_world encodes the bits up to its epoch; the second half of the span takes bits drawn from the seed (their content is not used)
    rng = np.random.default_rng(seed + 1000)
    need = int(n_samples / fs * 50) + 4
    w["nav_bits"] = [np.concatenate([np.asarray(b, dtype=np.int8), (2 * rng.integers(0, 2, need) - 1).astype(np.int8)]) for b in w["nav_bits"]]
    chan = np.stack([ch["rc"], ch["ri"], ch["fc"], ch["fi"], np.zeros(K)], axis=1)
    w["start"] = dict(rxTime0=truth["rxTime"] - n_e / fs, chan=chan, tow=truth["TOW"].astype(np.int32), cps=truth["cp_timestamp"].astype(np.int64),
                      eph=truth["eph"].copy(), prns=[int(p) for p in ch["prn"]], X=truth["X_ECEF"].copy())
    w["n_samples"], w["fs"] = n_samples, fs
    return w


def record(world, seed=41, amp=AMP, sigma=SIGMA, profile=None, chunk=1 << 19):
    """The world's record as interleaved int16 I/Q.  profile: {channel: [(first sample, end sample, amplitude factor), ...]} -- the
    channel's amplitude is amp x factor inside those spans.  Signal model and nav-bit convention are synth.gen_iq_record's."""
    ch, bits, fs, n = world["ch"], world["nav_bits"], world["fs"], world["n_samples"]
    K = len(ch["prn"])
    chips = [dpe.synth.ca_code(int(p)).astype(np.float64) for p in ch["prn"]]
    iq = np.empty(2 * n, dtype=np.int16)
    for i, n0 in enumerate(range(0, n, chunk)):
        m = min(chunk, n - n0)
        rng = np.random.Generator(np.random.PCG64([seed, i]))
        idx = np.arange(n0, n0 + m)
        t = idx.astype(np.float64) / fs
        x = sigma * (rng.standard_normal(m) + 1j * rng.standard_normal(m))
        for k in range(K):
            a = np.full(m, float(amp))
            for (s0, s1, f) in (profile or {}).get(k, ()):
                a[(idx >= s0) & (idx < s1)] = amp * f
            ci = np.floor(t * ch["fc"][k] + ch["rc"][k]).astype(np.int64)
            bit_idx = (ci // L_CA - int(ch["cp_ref"][k]) % 20 + 20) // 20
            ph = ch["fi"][k] * t + ch["ri"][k]
            x += a * np.asarray(bits[k], dtype=np.float64)[bit_idx] * chips[k][np.mod(ci, L_CA)] * np.exp(2j * np.pi * (ph - np.floor(ph)))
        iq[2 * n0:2 * (n0 + m):2] = np.clip(np.rint(x.real), -32768, 32767).astype(np.int16)
        iq[2 * n0 + 1:2 * (n0 + m):2] = np.clip(np.rint(x.imag), -32768, 32767).astype(np.int16)
    return iq


def perturbed(world, dpos=30.0, dvel=0.5):
    """The start state of the closed-loop tests: dpos metres and dvel m/s off X_true, in a fixed direction."""
    X = world["start"]["X"].copy()
    u = np.array([1.0, -2.0, 2.0]) / 3.0
    X[:3] += dpos * u
    X[4:7] += dvel * u[[2, 0, 1]]
    return X


def sigma0():
    return np.diag([1.0e4, 1.0e4, 1.0e4, 1.0e4, 1.0, 1.0, 1.0, 1.0])
