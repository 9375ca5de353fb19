"""Cases for the front end's tests (tests/test_fe_ref_cpu.py proves them on the CPU, tests/test_gpu_fe.py runs them on the device):
the parity table, the saturation case and the end-to-end world -- a 10 Msps synthetic record taken to a real IF of 2.5 MHz,
quantised to 2 bits and brought back to 2.5 Msps complex baseband for acquisition.  Every reference is computed once per process.

The tile size of the launch geometry is restated here in Python (csrc/dpe_fe_plan.h: fe_geom); tests/test_fe_plan_cpu.py holds the
C++ to it and the GPU test holds the handle's own figure to it."""
import functools

import numpy as np

from navlab_dpe_sdr_amd import frontend, synth
from tests import fe_ref

FS = 10.0e6
H3 = np.array([0.27, 0.46, 0.27])            # T = 3: no dyadic taps, so that outputs do not sit on half-integers by construction
INCOMMENSURATE = 0.12345678                  # of fs


def tile_outputs(D, T, real_in):
    """fe_geom's tileOut: the LDS limit (32 KiB) over the element size and D gives the row pitch, less the longest phase's taps,
    at most 256 lanes x 5 outputs, a multiple of 5."""
    pitch_max = 32768 // (4 if real_in else 8) // D
    return min(pitch_max - -(-T // D), 1280) // 5 * 5


def lds_bytes(D, T, real_in):
    return (tile_outputs(D, T, real_in) + -(-T // D)) * D * (4 if real_in else 8)


def taps(D, T):
    if T == 1:
        return np.array([1.0])
    if T == 3:
        return H3
    if T == 8 * D + 1:
        return frontend.design_lowpass(D)
    return _long_taps(D, T)


def _long_taps(D, T):
    """An odd length that is not 8 D + 1 (T = 1023 at D = 64): the same window and cut-off over T taps."""
    n = np.arange(T, dtype=np.float64) - (T - 1) // 2
    h = np.sinc(0.9 / D * n) * np.kaiser(T, 8.0)
    return h / h.sum()


# (format, D, T, output count, IF, gain): count in outputs or in tiles of the plan ("t-1", "t", "t+1", "3t+7"); IF 0, "+q" = +fs/4,
# "-q" = -fs/4, "inc" = an incommensurate fraction of fs.  The gains keep tol <= 0.02 (test_fe_ref_cpu asserts it).
PARITY = (
    ("I16C", 1, 1, 1, 0, 1.0), ("I8C", 1, 1, 2, "+q", 1.0), ("I16R", 1, 3, 63, "inc", 0.5), ("I8R", 1, 3, 64, "-q", 1.0),
    ("ARGPI4", 1, 9, 65, 0, 100.0), ("P2R", 1, 9, "t-1", "+q", 20.0), ("P2C", 1, 9, "t", "inc", 20.0),
    ("I16C", 2, 17, "t+1", "inc", 0.5), ("I8C", 2, 17, "3t+7", "-q", 1.0), ("I16R", 2, 1, 1, "+q", 1.0), ("I8R", 2, 3, 2, 0, 1.0),
    ("ARGPI4", 2, 17, 63, "inc", 100.0), ("P2R", 2, 17, 64, "-q", 20.0), ("P2C", 2, 3, 65, "+q", 20.0),
    ("I16C", 3, 25, "t-1", "+q", 0.5), ("I8C", 3, 25, "t", 0, 1.0), ("I16R", 3, 25, "t+1", "-q", 0.5), ("I8R", 3, 1, "3t+7", "inc", 1.0),
    ("ARGPI4", 3, 3, 1, "-q", 100.0), ("P2R", 3, 25, 2, "inc", 20.0), ("P2C", 3, 25, 63, 0, 20.0),
    ("I16C", 4, 33, 64, "-q", 0.5), ("I8C", 4, 33, 65, "inc", 1.0), ("I16R", 4, 33, "t-1", 0, 0.5), ("I8R", 4, 33, "t", "+q", 1.0),
    ("ARGPI4", 4, 33, "t+1", "+q", 100.0), ("P2R", 4, 33, "3t+7", 0, 20.0), ("P2C", 4, 1, 1, "inc", 20.0),
    ("I16C", 10, 81, "3t+7", 0, 0.5), ("I8C", 10, 81, "t", "+q", 1.0), ("I16R", 10, 81, 65, "inc", 0.5), ("I8R", 10, 3, "t+1", "-q", 1.0),
    ("ARGPI4", 10, 81, "t-1", "inc", 100.0), ("P2R", 10, 81, 64, "+q", 20.0),
    ("I16C", 16, 129, "t+1", "+q", 0.2), ("I8R", 16, 129, "t", "-q", 1.0), ("P2C", 16, 129, "3t+7", "inc", 20.0),
    ("I8C", 64, 513, "t+1", "inc", 1.0), ("P2R", 64, 1023, "3t+7", "-q", 20.0), ("ARGPI4", 64, 513, "t-1", 0, 100.0),
    ("I16R", 64, 1, 2, 0, 1.0),
)


def _if_hz(spec):
    return {0: 0.0, "+q": FS / 4, "-q": -FS / 4, "inc": INCOMMENSURATE * FS}[spec]


def _count(spec, tile):
    return spec if isinstance(spec, int) else {"t-1": tile - 1, "t": tile, "t+1": tile + 1, "3t+7": 3 * tile + 7}[spec]


def make_case(fmt, D, T, out_first, out_count, f_if, gain, seed, record_length=None, amp16=2047, h=None):
    """A record of random samples that holds exactly what the outputs need (from the byte boundary below), and its reference."""
    h = taps(D, T) if h is None else np.asarray(h, dtype=np.float64)
    T0 = (T - 1) // 2
    lo = max(out_first * D - T0, 0)
    hi = (out_first + out_count - 1) * D + T - T0
    if record_length is not None:
        hi = min(hi, record_length)
    den = fe_ref.BYTES[fmt][1]
    raw_first = lo - lo % den
    raw_count = hi - raw_first
    rng = np.random.Generator(np.random.PCG64(seed))
    raw = fe_ref.random_record(fmt, raw_count, rng, amp16)
    x = fe_ref.decode(fmt, raw, 0, raw_count)
    d = fe_ref.delta(f_if, FS)
    y = fe_ref.convert(x, raw_first, record_length, out_first, out_count, D, h, gain, d)
    return dict(fmt=fmt, D=D, T=T, h=h, gain=gain, f_if=f_if, delta=d, raw=raw, raw_first=raw_first, raw_count=raw_count,
                record_length=record_length, out_first=out_first, out_count=out_count, y=y,
                tol=fe_ref.tolerance(h, gain, float(np.abs(x).max())))


@functools.lru_cache(maxsize=None)
def parity_case(i):
    fmt, D, T, count, f_if, gain = PARITY[i]
    tile = tile_outputs(D, T, fmt in fe_ref.REAL)
    return make_case(fmt, D, T, 1000 + 37 * i, _count(count, tile), _if_hz(f_if), gain, seed=100 + i)


@functools.lru_cache(maxsize=None)
def saturation_case():
    """int16 samples through a gain of 3 that drives both rails.  Taps [1] at D = 1 and IF 0 make every output 3 x exactly:
    |x| <= 8999 stays below 26 997, |x| >= 11 600 gives at least 34 800, so no value lies within 1 of a rail's threshold."""
    rng = np.random.Generator(np.random.PCG64(77))
    n = 3000
    mag = rng.integers(0, 2, 2 * n) * 11500 + rng.integers(100, 9000, 2 * n)          # 100 .. 8999 stays, 11600 .. 20499 clips
    v = (mag * (2 * rng.integers(0, 2, 2 * n) - 1)).astype("<i2")
    raw = v.view(np.uint8)
    x = fe_ref.decode("I16C", raw, 0, n)
    y = fe_ref.convert(x, 0, None, 0, n, 1, [1.0], 3.0, 0)
    return dict(fmt="I16C", D=1, T=1, h=np.array([1.0]), gain=3.0, f_if=0.0, delta=0, raw=raw, raw_first=0, raw_count=n, record_length=None,
                out_first=0, out_count=n, y=y, tol=fe_ref.tolerance([1.0], 3.0, float(np.abs(x).max())))


# ---- the end-to-end world
WORLD_FS_OUT, WORLD_D, WORLD_GAIN, WORLD_IF, WORLD_SIGMA = 2.5e6, 4, 400.0, 2.5e6, 300.0
WORLD_BINS = 100.0 * (np.arange(125) - 62)


@functools.lru_cache(maxsize=None)
def world():
    """synth.gen_iq at 10 Msps (4 SVs, amp 60, sigma 300, no DC, no bit flip) -> real IF 2.5 MHz by the specification's own phase
    word -> 2 bits at +-1 sigma, offset binary, four samples per byte (P2R) -> the reference's 2.5 Msps int16 record."""
    ch = synth.random_channels(7, 4)
    S = 100000
    iq = synth.gen_iq(5, FS, S, ch, amp=60.0, sigma=WORLD_SIGMA, dc=(0.0, 0.0), flip=np.zeros(4, dtype=bool))
    x = iq[0::2].astype(np.float64) + 1j * iq[1::2].astype(np.float64)
    d = fe_ref.delta(WORLD_IF, FS)
    up = (x * np.exp(2j * np.pi * (fe_ref.phase_words(np.arange(S), d).astype(np.float64) / 4294967296.0))).real
    codes = (up >= -WORLD_SIGMA).astype(np.uint8) + (up >= 0.0) + (up >= WORLD_SIGMA)
    raw = fe_ref.pack2(codes)
    h = frontend.design_lowpass(WORLD_D)
    xq = fe_ref.decode("P2R", raw, 0, S)
    n_out = S // WORLD_D
    y = fe_ref.convert(xq, 0, S, 0, n_out, WORLD_D, h, WORLD_GAIN, d)
    # truth per SV: the delay index of the code period's start and the nearest Doppler bin
    t_start = (synth.L_CA - ch["rc"]) / ch["fc"]
    truth_idx = np.mod(t_start * WORLD_FS_OUT, 2500.0)
    truth_bin = np.array([int(np.argmin(np.abs(WORLD_BINS - f))) for f in ch["fi"]])
    return dict(ch=ch, S=S, raw=raw, h=h, delta=d, y=y, n_out=n_out, iq=fe_ref.quantise(y), truth_idx=truth_idx, truth_bin=truth_bin,
                tol=fe_ref.tolerance(h, WORLD_GAIN, 3.0))
