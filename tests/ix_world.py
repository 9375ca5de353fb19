"""Cases for the excisor's tests (tests/test_ix_ref_cpu.py proves them on the CPU, tests/test_gpu_ix.py runs them on the device).
A case's input is int16 noise within +-2047 per component plus the interferers its row names; every case and every reference is
computed once per process.  HOPS_PER_BLOCK restates the launch plan's figure (csrc/dpe_ix_plan.h: kIxHopsPerBlock);
tests/test_ix_plan_cpu.py holds the C++ to it and the GPU test holds the handle's own figure to it."""
import functools

import numpy as np

from navlab_dpe_sdr_amd import synth
from tests import ix_ref

HOPS_PER_BLOCK = 16
AMP = 2047
TONE = 0.1837            # cycles per sample: the jammer of the end-to-end world
SIZES = (64, 256, 1024, 4096)


def noise(seed, n, amp=AMP):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.integers(-amp, amp + 1, n).astype(np.float64) + 1j * rng.integers(-amp, amp + 1, n).astype(np.float64)


def tone(first, n, freq, amplitude, phase=0.3):
    return amplitude * np.exp(2j * np.pi * (freq * (first + np.arange(n, dtype=np.float64)) + phase))


def chirp(first, n, f0, f1, span, amplitude):
    """frequency f0 at sample 0 rising linearly to f1 at sample `span`"""
    t = first + np.arange(n, dtype=np.float64)
    return amplitude * np.exp(2j * np.pi * (f0 * t + 0.5 * (f1 - f0) / span * t * t))


def to_i16(x):
    """complex -> rounded complex (integers in both parts), asserted inside int16"""
    v = np.rint(x.real) + 1j * np.rint(x.imag)
    assert max(np.abs(v.real).max(), np.abs(v.imag).max()) <= 32767
    return v


def i16_bytes(x):
    out = np.empty(2 * x.size, dtype="<i2")
    out[0::2], out[1::2] = x.real, x.imag
    return out


def f32_pairs(x):
    out = np.empty(2 * x.size, dtype=np.float32)
    out[0::2], out[1::2] = x.real, x.imag
    return out


def needed(out_first, out_count, N, record_length=None):
    H = N // 2
    lo, hi = max((out_first // H - 1) * H, 0), ((out_first + out_count - 1) // H + 2) * H
    if record_length is not None:
        hi = min(hi, record_length)
    return lo, max(hi, lo)


def _static(N, seed, count=10):
    m = np.zeros(N, dtype=np.uint8)
    m[np.random.Generator(np.random.PCG64(seed)).choice(N, count, replace=False)] = 1
    return m


# name -> N, first output, output count ("cross": 17 hops and 9 outputs from a block's third hop on, so two blocks), and optionally
#   kappa (10), guard (1), gain (1), blank (0), static (a seed), f32 (fp32 input), length (the record's), pad (samples of the buffer
#   before and beyond the needed range), and the interferer: ("tone", cycles per sample or "bin b", amplitude), ("tones", ...),
#   ("chirp", f0, f1, amplitude), ("pulse", offset into the outputs, length, amplitude)
def _table():
    T = {"single output N64": dict(N=64, first=1000 + 13, count=1, add=("tone", TONE, 6000))}
    for N in SIZES:
        T["cross N%d" % N] = dict(N=N, first=3 * (N // 2) + 5, count="cross", add=("tone", TONE, 6000))
    T["wrap bins 0 and N-1"] = dict(N=256, first=777, count=700, guard=2, add=("tones", ("bin", 0, 5000), ("bin", 255, 5000)))
    T["tone between bins"] = dict(N=256, first=777, count=700, add=("tone", 37.5 / 256, 6000))
    T["chirp"] = dict(N=256, first=0, count=3000, add=("chirp", 0.1, 0.3, 6000))
    T["static mask alone"] = dict(N=256, first=777, count=700, kappa=1.0e6, static=5)
    T["pulse"] = dict(N=256, first=777, count=700, blank=4.0 * AMP * AMP, add=("pulse", 300, 37, 20000))
    T["nothing excised"] = dict(N=1024, first=777, count=2500, kappa=1.0e6, gain=1.25)
    T["negative gain"] = dict(N=256, first=777, count=700, gain=-0.75, add=("tone", TONE, 6000))
    T["fp32 input"] = dict(N=256, first=777, count=700, f32=True, add=("tone", TONE, 6000.25))
    # record edges
    T["record shorter than a hop"] = dict(N=256, first=0, count=300, length=50, add=("tone", TONE, 6000))
    T["record ends inside a frame"] = dict(N=256, first=100, count=900, length=777, add=("tone", TONE, 6000))
    T["frames beyond the record"] = dict(N=64, first=0, count=40 * 32 + 5, length=333, add=("tone", TONE, 6000))
    T["first output 0"] = dict(N=1024, first=0, count=1500, add=("tone", TONE, 6000))
    T["wide buffer"] = dict(N=256, first=2000, count=700, length=2600, pad=(391, 517), add=("tone", TONE, 6000))
    T["large indices"] = dict(N=256, first=2 ** 55 - 700 - 3, count=700, add=("tone", TONE, 6000))
    return T


CASES = _table()
PARITY = ("single output N64", "cross N64", "cross N256", "cross N1024", "cross N4096", "wrap bins 0 and N-1", "tone between bins", "chirp",
          "static mask alone", "pulse", "nothing excised", "negative gain", "fp32 input")
EDGES = ("record shorter than a hop", "record ends inside a frame", "frames beyond the record", "first output 0", "wide buffer")


@functools.lru_cache(maxsize=None)
def case(name):
    s = CASES[name]
    i = list(CASES).index(name)
    N = s["N"]
    H = N // 2
    first = s["first"]
    count = 17 * H + 9 if s["count"] == "cross" else s["count"]
    length = s.get("length")
    lo, hi = needed(first, count, N, None)
    before, beyond = s.get("pad", (0, 0))
    x_first = lo - before
    n = hi + beyond - x_first                    # the buffer runs over the record's end where there is one: those samples do not count
    base = noise(500 + i, n)
    x = base.copy()
    add = s.get("add")
    phase_first = x_first % 2 ** 20                # (a tone's phase from a small index: fp64 keeps it exact at 2^55 too)
    if add and add[0] == "tone":
        x += tone(phase_first, n, add[1], add[2])
    elif add and add[0] == "tones":
        for _, b, amp in add[1:]:
            x += tone(phase_first, n, b / N, amp)
    elif add and add[0] == "chirp":
        x += chirp(x_first, n, add[1], add[2], hi, add[3])
    elif add and add[0] == "pulse":
        at = first + add[1] - x_first
        x[at:at + add[2]] += tone(0, add[2], 0.05, add[3])
    x = x if s.get("f32") else to_i16(x)
    if s.get("f32"):
        x = f32_pairs(x).astype(np.float64)
        x = x[0::2] + 1j * x[1::2]
    return dict(name=name, N=N, H=H, kappa=s.get("kappa", 10.0), guard=s.get("guard", 1), gain=s.get("gain", 1.0), blank_power=s.get("blank", 0.0),
                static=_static(N, s["static"]) if "static" in s else None, in_f32=bool(s.get("f32")), x=x, base=base, x_first=x_first,
                record_length=length, out_first=first, out_count=count, needed=needed(first, count, N, length))


def reference(c, masks=None):
    """(out, tol, F) of ix_ref.excise for a case, by the reference's own masks or the given ones"""
    return ix_ref.excise(c["x"], c["x_first"], c["record_length"], c["out_first"], c["out_count"], c["N"], c["kappa"], c["guard"], c["static"],
                         c["blank_power"], c["gain"], masks=masks, detail=True)


def blanked_count(c):
    """the input samples among the case's outputs and inside the record that the blanker zeroes"""
    a, b = c["out_first"], c["out_first"] + c["out_count"]
    if c["record_length"] is not None:
        b = min(b, c["record_length"])
    seg = c["x"][a - c["x_first"]:max(b, a) - c["x_first"]]
    return int(ix_ref.blanked(seg, c["blank_power"]).sum())


# ---- analysis: six frames per size, the tone of the end-to-end world
ANALYSIS_FRAMES, ANALYSIS_FIRST = 6, 3


@functools.lru_cache(maxsize=None)
def analysis_case(N):
    H = N // 2
    x_first = (ANALYSIS_FIRST - 1) * H
    n = (ANALYSIS_FRAMES + 1) * H
    x = to_i16(noise(900 + N, n) + tone(x_first, n, TONE, 6000))
    static = _static(N, 40 + N, 3)
    F = ix_ref.frames(x, x_first, None, ANALYSIS_FIRST, ANALYSIS_FRAMES, N, 10.0, 1, static)
    return dict(N=N, x=x, x_first=x_first, static=static, kappa=10.0, guard=1, F=F)


# ---- the clipping case: a gain of 20 takes components beyond +-1638 over the rails
@functools.lru_cache(maxsize=None)
def clip_case():
    N, first, count = 256, 500, 1200
    lo, hi = needed(first, count, N)
    x = to_i16(noise(77, hi - lo))
    return dict(name="clip", N=N, H=N // 2, kappa=10.0, guard=1, gain=20.0, blank_power=0.0, static=None, in_f32=False, x=x, x_first=lo,
                record_length=None, out_first=first, out_count=count)


# ---- the end-to-end world: 4 SVs at 2.5 Msps under a tone of amplitude 4000
WORLD_FS, WORLD_S = 2.5e6, 25000
WORLD_BINS = 100.0 * (np.arange(125) - 62)


@functools.lru_cache(maxsize=None)
def world():
    ch = synth.random_channels(7, 4)
    iq = synth.gen_iq(5, WORLD_FS, WORLD_S, ch, amp=60.0, sigma=300.0, dc=(0.0, 0.0), flip=np.zeros(4, dtype=bool))
    clean = ix_ref.from_i16(iq)
    jammed = to_i16(clean + tone(0, WORLD_S, TONE, 4000.0))
    excised = ix_ref.excise(jammed, 0, WORLD_S, 0, WORLD_S, 1024, 10.0, 1)
    t_start = (synth.L_CA - ch["rc"]) / ch["fc"]
    truth_idx = np.mod(t_start * WORLD_FS, 2500.0)
    truth_bin = np.array([int(np.argmin(np.abs(WORLD_BINS - f))) for f in ch["fi"]])
    return dict(ch=ch, clean=np.asarray(iq, dtype=np.int16), jammed=i16_bytes(jammed), excised=ix_ref.quantise(ix_ref.interleave(excised)),
                truth_idx=truth_idx, truth_bin=truth_bin)
