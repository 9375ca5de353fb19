"""GPU: scalar tracking (dpe_trk_*, csrc/dpe_trk.hip) against the twin's own logs (fixture O14) and tests/trk_ref.py.

Bounds and where they come from:
  * teacher-forced correlator (dpe_trk_correlate on O14's logged parameters): 2e-6 of the channel's prompt peak -- the tolerance
    tests/test_gpu_parity.py holds the banks to against the PyGNSS fixtures O3 / O12 (its TOL), same arithmetic class;
  * closed loop (dpe_trk_track): per logged quantity, 4 x the largest deviation from O14 of trk_ref run with its six correlator
    outputs rounded to fp32 at every window -- what fp32 correlations cost the REFERENCE loop, computed here on the CPU before
    the device is asked (correlations and lockval relative to the channel's median prompt magnitude, everything else absolute);
    quantities that yardstick leaves untouched (cp, lock, the biases) must be equal;
  * cp per window, the boundary case per window, the cp_sign streams and the lock flags: equal to O14's.  A sign decided on
    |Re p_s| below 1 % of the channel's median prompt magnitude may be left out, at most 1 % of them (the twin leaves out none:
    tests/test_trk_cpu.py);
  * K channels in one launch == each alone, track(M) == track(M / 2) twice, run == run: bit for bit;
  * dev_status == 0 after every run.
Each figure is printed before it is asserted (run with -s to see them)."""
import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import trk_ref

pytestmark = pytest.mark.gpu
TOL = 2e-6          # tests/test_gpu_parity.py: banks against the PyGNSS fixtures, relative to the peak
EXACT = ("cp", "lock", "fc_bias", "fi_bias")


def _init(prns, start):
    return [dict(prn=int(p), rc=float(s[0]), ri=float(s[1]), fc=float(s[2]), fi=float(s[3])) for p, s in zip(prns, start)]


@pytest.fixture(scope="module")
def o14(golden):
    import torch
    g = golden("o14_scalar_track")
    iq = trk_ref.o14_iq(g)
    return g, iq, torch.from_numpy(iq).to("cuda:0")


def _run(g, iq_d, M, chans=None, split=None):
    prns = [int(p) for p in g["prn"]]
    sel = list(range(len(prns))) if chans is None else list(chans)
    trk = dpe.ScalarTracker(float(g["fs"]), [prns[k] for k in sel], T=float(g["T"]), log_capacity_windows=M)
    trk.set_params(_init([prns[k] for k in sel], g["start"][sel]))
    S = trk.S
    if split is None:
        trk.track(iq_d, M)
    else:
        trk.track(iq_d, split)
        trk.track(iq_d[2 * S * split:], M - split)
    log = trk.read_log()
    signs = [trk.read_cp_signs(k) for k in range(len(sel))]
    st = trk.state()
    assert trk.dev_status() == 0
    trk.close()
    return log, signs, st


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _yardstick(g, ref, rounded, M):
    """per quantity: largest deviation of the fp32-rounded reference loop from the reference, over windows and channels, scaled"""
    K = ref["cp"].shape[1]
    y = {}
    for n in trk_ref.LOG_NAMES:
        sc = np.array([trk_ref.scale(n, g, k) for k in range(K)])
        y[n] = float(np.nanmax(np.abs(rounded[n][:M] - ref[n][:M]) / sc)) if not np.isnan(ref[n][:M]).all() else 0.0
    return y


def _compare(g, dev, ref, yard, M, label):
    K = ref["cp"].shape[1]
    worst = {}
    for n in trk_ref.LOG_NAMES:
        a, b = dev[n][:M], ref[n][:M]
        assert np.array_equal(np.isnan(a), np.isnan(b)), n
        sc = np.array([trk_ref.scale(n, g, k) for k in range(K)])
        r = float(np.nanmax(np.abs(a - b) / sc))
        worst[n] = r
        print("%s %-8s device %.3e   yardstick %.3e   ratio %s" % (label, n, r, yard[n], "%.2f" % (r / yard[n]) if yard[n] else "-"))
    for n in trk_ref.LOG_NAMES:
        if n in EXACT or yard[n] == 0.0:
            assert worst[n] == 0.0, n
        else:
            assert worst[n] <= 4.0 * yard[n], (n, worst[n], yard[n])


def test_teacher_forced_correlator_vs_o14(o14):
    g, iq, iq_d = o14
    M, K = int(g["M"]), len(g["prn"])
    trk = dpe.ScalarTracker(float(g["fs"]), g["prn"], T=float(g["T"]), log_capacity_windows=8)
    params = np.stack([g["log_" + n][:M] for n in ("rc", "ri", "fc", "fi")], axis=2)
    out = trk.correlate(iq_d, params)
    assert trk.dev_status() == 0
    trk.close()
    _, case, _, seg, _ = trk_ref.track(iq, float(g["fs"]), float(g["T"]), g["prn"], g["start"], M)
    assert np.array_equal(out["case"], case)
    for k in range(K):
        peak = np.hypot(g["log_iP"][:M, k], g["log_qP"][:M, k]).max()
        for j, (i_, q_) in enumerate((("iE", "qE"), ("iP", "qP"), ("iL", "qL"))):
            r = np.abs(out["epl"][:, k, j] - (g["log_" + i_][:M, k] + 1j * g["log_" + q_][:M, k])).max() / peak
            print("teacher-forced ch %d %s: %.3e of the prompt peak" % (k, i_[1], r))
            assert r < TOL, (k, i_, r)
        r = np.abs(out["seg"][:, k] - seg[:, k]).max() / peak
        print("teacher-forced ch %d segment sums: %.3e" % (k, r))
        assert r < TOL, (k, r)


def test_closed_loop_vs_o14(o14):
    g, iq, iq_d = o14
    M, K = int(g["M"]), len(g["prn"])
    ref = {n: g["log_" + n] for n in trk_ref.LOG_NAMES}
    rounded, case, _, _, ps = trk_ref.track(iq, float(g["fs"]), float(g["T"]), g["prn"], g["start"], M, round_epl=np.float32)
    yard = _yardstick(g, ref, rounded, M)
    dev, signs, st = _run(g, iq_d, M)
    # exact: cp, case, lock, the cp_sign streams
    assert np.array_equal(dev["cp"][:M], ref["cp"][:M]) and np.array_equal(dev["lock"][:M], ref["lock"][:M])
    _, case64, _, _, ps64 = trk_ref.track(iq, float(g["fs"]), float(g["T"]), g["prn"], g["start"], M)
    assert np.array_equal(dev["case"].astype(np.int64), case64)
    for k in range(K):
        n = int(g["cp_sign_n"][k])
        assert st[k]["nSigns"] == n == signs[k].size and st[k]["cp"] == n and st[k]["lock"] == 1 and st[k]["frozen"] == 0
        med = np.median(np.hypot(ref["iP"][:M, k], ref["qP"][:M, k]))
        keep = np.abs(ps64[k]) >= 0.01 * med
        print("cp_sign ch %d: %d signs, %d left out, %d differ" % (k, n, n - keep.sum(), (signs[k] != g["cp_sign"][k, :n]).sum()))
        assert keep.mean() >= 0.99 and np.array_equal(signs[k][keep], g["cp_sign"][k, :n][keep].astype(np.int8))
        assert abs(st[k]["paRe"] - g["p_a_end"][k].real) <= 4 * max(yard["iP"], 6e-8) * med
    _compare(g, dev, ref, yard, M, "O14")


def test_invariances_bit_identical(o14):
    g, _, iq_d = o14
    M, K = int(g["M"]), len(g["prn"])
    a, sa, _ = _run(g, iq_d, M)
    b, sb, _ = _run(g, iq_d, M)
    c, sc, _ = _run(g, iq_d, M, split=M // 2)
    for n in dpe.ScalarTracker.LOG_NAMES:
        assert np.array_equal(_bits(a[n]), _bits(b[n])), n            # run == run
        assert np.array_equal(_bits(a[n]), _bits(c[n])), n            # track(M) == track(M / 2) twice
    assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(sa, sb, sc))
    for k in range(K):                                                # K channels in one launch == each alone
        d, sd, _ = _run(g, iq_d, M, chans=[k])
        for n in dpe.ScalarTracker.LOG_NAMES:
            assert np.array_equal(_bits(a[n][:, k]), _bits(d[n][:, 0])), (n, k)
        assert np.array_equal(sa[k], sd[0])


def test_chain_acquisition_to_tracking():
    """gen_iq_record -> Acquisition.scalar_acquisition -> ScalarTracker.set_params -> track: every channel ends locked and its
    cp_sign stream is the synthesised nav-bit stream up to one sign per channel."""
    import torch
    fs, S, M = 2.5e6, 2500, 420
    prns = [5, 13, 20, 29]
    fi = np.array([1830.0, -2715.0, 640.0, -3390.0])
    ch = dpe.synth.random_channels(21, 4, prns=prns)
    ch["fi"], ch["fc"] = fi, 1.023e6 * (1.0 + fi / 1.57542e9)
    ch["cp_ref"] = np.array([4, 17, 9, 12])
    iq, bits = dpe.synth.gen_iq_record(77, fs, M * S, ch, amp=np.array([90.0, 75.0, 110.0, 80.0]), sigma=300.0)
    iq_d = torch.from_numpy(iq).to("cuda:0")
    acq = dpe.Acquisition(fs, 10 * S, prns, np.arange(-62, 63) * 100.0, mode="coherent")
    init = acq.scalar_acquisition(iq_d, iq_d[2 * 10 * S:])
    acq.close()
    assert all(r["found"] for r in init)
    for k, r in enumerate(init):
        print("acquired PRN %d: rc %.3f (truth %.3f) fi %.1f (truth %.1f)" % (r["prn"], r["rc"], ch["rc"][k], r["fi"], fi[k]))
    trk = dpe.ScalarTracker(fs, prns, log_capacity_windows=M)
    trk.set_params(init)
    trk.track(iq_d, M)
    st = trk.state()
    for k in range(4):
        s = trk.read_cp_signs(k)
        agree = trk_ref.nav_bit_agreement(s, bits[k], int(ch["cp_ref"][k]), skip=150)
        print("PRN %d: lock %d, %d signs, agreement with the nav bits %.3f" % (prns[k], st[k]["lock"], s.size, agree))
        assert st[k]["lock"] == 1 and st[k]["frozen"] == 0 and agree in (0.0, 1.0)
    assert trk.dev_status() == 0
    trk.close()


def test_closed_loop_at_25_msps_vs_trk_ref():
    """S = 25 000: the sample loop runs 25 tiles per window.  Reference: trk_ref in fp64; yardstick: trk_ref with fp32 E/P/L."""
    import torch
    fs, T, M = 25e6, 1e-3, 60
    prns = [8, 27]
    fi = np.array([2210.4, -1475.8])
    ch = dict(prn=np.array(prns), rc=np.array([402.6, 1022.4]), ri=np.array([0.3, 0.8]), fc=1.023e6 * (1.0 + fi / 1.57542e9), fi=fi,
              cp_ref=np.array([5, 14]))
    iq, _ = dpe.synth.gen_iq_record(25, fs, (M + 1) * 25000, ch, amp=np.array([60.0, 70.0]), sigma=300.0)
    fi0 = fi + np.array([12.0, -18.0])
    start = np.stack([ch["rc"] + np.array([0.06, -0.04]), ch["ri"] + np.array([0.05, -0.07]), 1.023e6 + 1.023e6 / 1.57542e9 * fi0, fi0], axis=1)
    ref, case, signs, _, _ = trk_ref.track(iq, fs, T, prns, start, M)
    rounded = trk_ref.track(iq, fs, T, prns, start, M, round_epl=np.float32)[0]
    g = dict(M=M, log_iP=ref["iP"], log_qP=ref["qP"])
    yard = _yardstick(g, ref, rounded, M)
    trk = dpe.ScalarTracker(fs, prns, T=T, log_capacity_windows=M)
    trk.set_params(_init(prns, start))
    trk.track(torch.from_numpy(iq).to("cuda:0"), M)
    dev = trk.read_log()
    assert trk.dev_status() == 0
    assert np.array_equal(dev["case"].astype(np.int64), case)
    for k in range(2):
        assert np.array_equal(trk.read_cp_signs(k), signs[k].astype(np.int8))
    trk.close()
    _compare(g, dev, ref, yard, M, "25 Msps")
