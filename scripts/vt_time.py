"""Time of vector tracking against scalar tracking on one record (profiles/vt_track.txt).

K = 8 channels, 2.5 Msps, 1 s of signal: dpe_vt_track(50 epochs of N = 20 windows) and dpe_trk_track(1000 windows), each from its
start state, HIP events on the launch stream, 3 untimed warm-up runs, then the median (min .. max) of 10 -- as
profiles/trk_scalar.txt was made.  --trk-lib PATH: also time dpe_trk_track of another build of the library (the parent commit's)
in the same run.  Also prints the two kernels' shares of an epoch (events around a loop of one kind of launch cannot be had
from outside the library, so: track(50) with N = 20 against N = 2, the filter kernel being the same in both).

    python scripts/vt_time.py [--trk-lib /path/to/parent/libdpe_hip.so] [--out profiles/vt_track.txt]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS, T, K, SECONDS = 2.5e6, 1e-3, 8, 1.0
PRNS = [2, 3, 6, 12, 17, 19, 24, 28]


def stats(ms):
    return "%.3f  (%.3f .. %.3f)" % (np.median(ms), np.min(ms), np.max(ms))


def timed(fn, reset, stream, warm=3, runs=10):
    import navlab_dpe_sdr_amd as dpe
    tm = dpe.engine.HipEventTimer()
    out = []
    for i in range(warm + runs):
        reset()
        tm.start(stream)
        fn()
        tm.stop(stream)
        ms = tm.elapsed_ms()
        if i >= warm:
            out.append(ms)
    return np.array(out)


def trk_of(lib, iq_d, init, M):
    """dpe_trk_* of `lib` (a ctypes.CDLL of some build of the library) by hand: -> (reset, run, close)."""
    import torch
    import navlab_dpe_sdr_amd as dpe
    e = dpe.engine
    cfg = e.TrkConfig(FS, T, K, 2, 0.0, 0.0, 1.0, M, (C.c_int32 * 37)(*PRNS), 0)
    h = C.c_void_p(None)
    assert lib.dpe_trk_create(C.byref(cfg), C.byref(h)) == 0
    a = (e.AcqTrackInit * K)()
    for r, c, p in zip(a, init, PRNS):
        r.prn, r.found, r.rc, r.ri, r.fc, r.fi = p, 1, c[0], c[1], c[2], c[3]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = C.c_void_p(iq_d.data_ptr())

    def reset():
        assert lib.dpe_trk_set_params(h, a, st) == 0

    def run():
        assert lib.dpe_trk_track(h, ptr, C.c_int32(M), st) == 0

    def status():
        v = C.c_int32()
        assert lib.dpe_trk_dev_status(h, C.byref(v), st) == 0
        return v.value
    return reset, run, status, lambda: lib.dpe_trk_destroy(h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trk-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    import navlab_dpe_sdr_amd as dpe
    from oracle import oracle
    from tests import helpers, vt_world
    oracle.lib()
    S = int(round(T * FS))
    n = int(SECONDS * FS)
    ho = dpe.handoff.read_handoff(helpers.HANDOFF)
    w = vt_world.build(oracle, n, chans=list(range(K)), ho=ho)
    iq = vt_world.record(w)
    iq_d = torch.from_numpy(iq).to("cuda:0")
    s = w["start"]
    stream = None
    lines = ["Vector tracking (dpe_vt_track: vt_correlate_kernel + vt_filter_kernel per epoch) against scalar tracking (dpe_trk_track,",
             "trk_scalar_kernel), %s, HIP events on the launch stream." % dpe.engine.device_info()[0],
             "Shape: K = %d channels (the shipped handoff's first %d), fs = 2.5 Msps, T = 1 ms (S = %d), 1 s of signal = 50 epochs of N = 20 windows"
             % (K, K, S),
             "= 1 000 windows; tests/vt_world.py's record (amp 90, sigma 300), start = the true state.  Every run starts from init / set_params.",
             "3 untimed warm-up runs, then 10 timed runs; median (min .. max).", "",
             "form                                                   ms per 1 s of signal         x real time"]
    res = {}
    for N in (20, 2):
        vt = dpe.VectorTracker(FS, s["prns"], T=T, N=N, log_capacity_epochs=64)
        vt.set_ephemerides(s["eph"], s["tow"], s["cps"])
        ms = timed(lambda: vt.track(iq_d, 50), lambda: vt.init(s["X"], vt_world.sigma0(), s["rxTime0"], s["chan"]), stream)
        log = vt.read_log(first=0, n=50)
        assert vt.dev_status() == 0 and np.all(log["mask"] == (1 << K) - 1), "a run ended with a status bit or an excluded channel"
        vt.close()
        res[N] = ms
    lines.append("vector   track(50), N = 20: 100 launches               %-28s %.1f" % (stats(res[20]), 1000.0 * SECONDS / np.median(res[20])))
    libs = [("this build", dpe.engine.lib())] + ([("--trk-lib", C.CDLL(a.trk_lib))] if a.trk_lib else [])
    trk_ms = {}
    for name, lib in libs:
        reset, run, status, close = trk_of(lib, iq_d, s["chan"], 1000)
        ms = timed(run, reset, stream)
        assert status() == 0
        close()
        trk_ms[name] = ms
        lines.append("scalar   track(1000), one launch, %-20s %-28s %.1f" % (name + ":", stats(ms), 1000.0 * SECONDS / np.median(ms)))
    per20, per2 = np.median(res[20]) / 50.0 * 1e3, np.median(res[2]) / 50.0 * 1e3
    lines += ["", "vector / scalar (this build) = %.2f." % (np.median(res[20]) / np.median(trk_ms["this build"])),
              "Per epoch: %.1f us at N = 20 (160 correlate blocks, then the filter kernel), %.1f us at N = 2 (16 blocks, the same filter kernel)."
              % (per20, per2),
              "The %.1f us between them is what 18 more windows per channel add to the correlate launch; what remains at N = 2 is one"
              % (per20 - per2),
              "window's latency chain in the correlate kernel (6.8 us per window in trk_scalar_kernel), the filter kernel's one-wave chain and",
              "the two launches.  The epoch is bound by that serial remainder, not by the N x K blocks."]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
