"""Cases for the front end's tests (tests/test_fe_ref_cpu.py proves them on the CPU, tests/test_gpu_fe.py runs them on the device):
the parity table, the saturation case and the end-to-end world -- a 10 Msps synthetic record taken to a real IF of 2.5 MHz,
quantised to 2 bits and brought back to 2.5 Msps complex baseband for acquisition -- and the table BEYOND of what the parity
table holds constant (tests/test_fe_beyond_cpu.py, tests/test_gpu_fe_beyond.py).  Every reference is computed once per process.

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


def asym_taps(D, T, seed):
    """taps(D, T) times a ramp over the taps plus a small seeded perturbation: no symmetry, so h[t] and h[T-1-t] cannot stand
    for one another, and no dyadic values."""
    rng = np.random.Generator(np.random.PCG64(seed))
    h = taps(D, T)
    return h * (1.0 + 0.8 * np.linspace(-1.0, 1.0, T)) + 1e-3 * np.abs(h).max() * rng.standard_normal(T)


def make_case(fmt, D, T, out_first, out_count, f_if, gain, seed, record_length=None, amp16=2047, h=None, levels=fe_ref.LEVELS,
              pad_before=0, pad_after=0):
    """A record of random samples and its reference.  The buffer holds what the outputs need (from the byte boundary below:
    need_first, need_count), pad_before samples before that and pad_after samples beyond it -- beyond record_length when there is
    one -- random like the rest.  y is the reference of the true record: what lies at or beyond record_length counts as zero."""
    h = taps(D, T) if h is None else np.asarray(h, dtype=np.float64)
    T0 = (T - 1) // 2
    lo = max(out_first * D - T0, 0)
    hi = (out_first + out_count - 1) * D + T - T0
    if record_length is not None:
        hi = min(hi, record_length)
    den = fe_ref.BYTES[fmt][1]
    need_first = lo - lo % den
    assert pad_before % den == 0 and 0 <= pad_before <= need_first and pad_after >= 0
    raw_first = need_first - pad_before
    raw_count = hi + pad_after - raw_first
    rng = np.random.Generator(np.random.PCG64(seed))
    raw = fe_ref.random_record(fmt, raw_count, rng, amp16)
    x = fe_ref.decode(fmt, raw, 0, raw_count, levels)
    d = fe_ref.delta(f_if, FS)
    y = fe_ref.convert(x, raw_first, record_length, out_first, out_count, D, h, gain, d)
    return dict(fmt=fmt, D=D, T=T, h=h, gain=gain, f_if=f_if, delta=d, raw=raw, raw_first=raw_first, raw_count=raw_count,
                record_length=record_length, out_first=out_first, out_count=out_count, y=y, levels=tuple(float(v) for v in levels),
                need_first=need_first, need_count=hi - need_first, pad_before=pad_before, pad_after=pad_after,
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


# ---- beyond the parity table: what it holds constant (tests/test_fe_beyond_cpu.py proves the cases, tests/test_gpu_fe_beyond.py
# runs them).  name -> fmt, D, T, count (outputs, or "t+1", "t+3", "2t+3", "3t+7" of the plan's tile), IF, gain, and optionally
#   asym      asym_taps instead of taps                    levels    the four 2-bit values
#   first     the first output (default 1000 + 37 i)       length    the record's length: "in tile 1" = (tile + 300) D + 1,
#   pad       (pad_before, pad_after) in input samples               "cut" = T0 + 2 samples short of what the outputs read
#   accept    False: not a case for the acceptance rule (it clips)
# IF beyond _if_hz: "+n" / "-n" = +-fs/2 (both the word 2^31), "+fs" / "-fs" (both the word 0), "+1" / "-1" = the words 1 and
# 2^32 - 1, "odd" = the incommensurate word made odd.
GAIN = {"I16C": 0.5, "I8C": 1.0, "I16R": 0.5, "I8R": 1.0, "ARGPI4": 100.0, "P2R": 20.0, "P2C": 20.0}
SIGN_MAGNITUDE = (1.0, 3.0, -1.0, -3.0)
QUARTER_TURN_FIRST = (2 ** 33 + 2 ** 30) // 4 + 3        # D = 4: the input index modulo 2^32 is near 2^30, one word per sample a quarter turn
TOP_FIRST = 2 ** 55 - 200
WIDE_PAD_BEFORE = 4 * 517


def _beyond_table():
    B = {}
    # 1. asymmetric taps, every kernel mode: real input, complex input with real taps (IF 0), complex input with complex taps
    for fmt, D, T, f_if, gain in (("I8C", 3, 25, "inc", 1.0), ("P2R", 10, 81, "+q", 20.0), ("I16R", 1, 9, "inc", 0.5), ("I16C", 4, 33, 0, 0.5),
                                  ("ARGPI4", 2, 17, "-q", 100.0)):
        B["asym %s D%d" % (fmt, D)] = dict(fmt=fmt, D=D, T=T, count="t+3", f_if=f_if, gain=gain, asym=True)
    # 2. levels other than (-3, -1, 1, 3)
    for fmt, D, T, f_if, gain, lv in (("P2R", 4, 33, "inc", 20.0, SIGN_MAGNITUDE), ("P2C", 3, 25, "-q", 20.0, SIGN_MAGNITUDE),
                                      ("P2C", 2, 17, "+q", 15.0, (-2.75, -0.5, 1.25, 4.5)), ("P2R", 1, 9, "inc", 10.0, (0.25, -7.0, 2.5, 1.0))):
        B["levels %s D%d" % (fmt, D)] = dict(fmt=fmt, D=D, T=T, count="t+3", f_if=f_if, gain=gain, levels=lv)
    # 3. phases of up to 1023 taps, and the smallest tile the plan makes (45 outputs, 9 busy lanes)
    for fmt, D, T, f_if, gain in (("I8R", 1, 1023, "inc", 0.3), ("P2C", 1, 1023, "inc", 10.0), ("I16R", 4, 1023, "-q", 0.02), ("I16C", 2, 255, "+q", 0.05),
                                  ("I8C", 64, 1023, "inc", 0.5), ("I16C", 64, 1023, 0, 0.03)):
        B["long %s D%d T%d" % (fmt, D, T)] = dict(fmt=fmt, D=D, T=T, count="2t+3", f_if=f_if, gain=gain)
    # 4. the IF words 2^31, 0 from +-fs, 1 and 2^32 - 1
    for fmt in ("I8C", "I16R"):
        for f_if in ("+n", "-n", "+fs", "-fs", "+1", "-1"):
            B["if %s %s" % (f_if, fmt)] = dict(fmt=fmt, D=4, T=33, count=300, f_if=f_if, gain=GAIN[fmt],
                                               **(dict(first=QUARTER_TURN_FIRST) if f_if in ("+1", "-1") else {}))
    # 5. the last outputs the interface takes
    B["top"] = dict(fmt="I8C", D=64, T=513, count=200, f_if="odd", gain=1.0, first=TOP_FIRST)
    # 6. both record edges in one call; the end inside tile 1, tiles 2 and 3 wholly beyond it
    B["edges I16C"] = dict(fmt="I16C", D=4, T=33, count="3t+7", f_if="inc", gain=0.5, first=0, length="in tile 1")
    B["edges P2R"] = dict(fmt="P2R", D=3, T=25, count="3t+7", f_if="inc", gain=20.0, first=0, length="in tile 1")
    # 7. buffers wider than needed: two shapes of the parity table, with and without the record's end
    for fmt, D, T, count, f_if, gain in (("P2R", 4, 33, "3t+7", 0, 20.0), ("I16C", 2, 17, "t+1", "inc", 0.5)):
        for length in (None, "cut"):
            B["wide %s%s" % (fmt, " cut" if length else "")] = dict(fmt=fmt, D=D, T=T, count=count, f_if=f_if, gain=gain, first=5000, length=length,
                                                                   pad=(WIDE_PAD_BEFORE, 2 * T + 13))
    # 8. one case per format for the alignment test
    for fmt in fe_ref.FORMATS:
        B["align %s" % fmt] = dict(fmt=fmt, D=3, T=25, count="t+1", f_if="inc", gain=GAIN[fmt])
    # 9. filtered, mixed and clipping.  Per component the output's deviation is about gain sqrt(sum h^2) 74 = 300 x 0.47 x 74 = 10 400
    # (int8 over every bit pattern: 74), so the rails lie more than three deviations out and few components pass them: about 3 in
    # 10 000 on the reference.  300 000 outputs give some 170 of them, which the CPU test holds above 100.
    B["clip I8C"] = dict(fmt="I8C", D=4, T=33, count=300000, f_if="inc", gain=300.0, accept=False)
    # 11. negative gain
    B["negative gain"] = dict(fmt="P2C", D=3, T=25, count="t+3", f_if="inc", gain=-20.0)
    return B


BEYOND = _beyond_table()


def _beyond_if(spec):
    inc_odd = (fe_ref.delta(INCOMMENSURATE * FS, FS) | 1) * FS / 4294967296.0
    extra = {"+n": FS / 2, "-n": -FS / 2, "+fs": FS, "-fs": -FS, "+1": FS / 4294967296.0, "-1": -FS / 4294967296.0, "odd": inc_odd}
    return extra[spec] if spec in extra else _if_hz(spec)


@functools.lru_cache(maxsize=None)
def beyond_case(name):
    s = BEYOND[name]
    i = list(BEYOND).index(name)
    fmt, D, T = s["fmt"], s["D"], s["T"]
    tile = tile_outputs(D, T, fmt in fe_ref.REAL)
    count = s["count"] if isinstance(s["count"], int) else {"t+1": tile + 1, "t+3": tile + 3, "2t+3": 2 * tile + 3, "3t+7": 3 * tile + 7}[s["count"]]
    first = s.get("first", 1000 + 37 * i)
    length = {None: None, "in tile 1": (tile + 300) * D + 1, "cut": (first + count - 1) * D + T - (T - 1) // 2 - ((T - 1) // 2 + 2)}[s.get("length")]
    pad_before, pad_after = s.get("pad", (0, 0))
    c = make_case(fmt, D, T, first, count, _beyond_if(s["f_if"]), s["gain"], seed=2000 + i, record_length=length,
                  h=asym_taps(D, T, 3000 + i) if s.get("asym") else None, levels=s.get("levels", fe_ref.LEVELS), pad_before=pad_before, pad_after=pad_after)
    c.update(name=name, tile=tile, asym=bool(s.get("asym")), accept=s.get("accept", True), if_spec=s["f_if"])
    return c


def clip_bounds(c):
    """(lower, upper): the components of the reference that lie more than tol beyond a rail's threshold, and those that lie beyond
    it or within tol of it.  rint(v) leaves the int16 range from 32767.5 up and from -32768.5 down."""
    v, tol = fe_ref.interleave(c["y"]), c["tol"]
    return int(((v > 32767.5 + tol) | (v < -32768.5 - tol)).sum()), int(((v > 32767.5 - tol) | (v < -32768.5 + tol)).sum())


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
