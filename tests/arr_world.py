"""Cases for the array combiner's tests (tests/test_arr_ref_cpu.py proves them on the CPU, tests/test_gpu_arr.py runs them on the
device).  A case's input is, per element, int16 noise within +-2047 per component (ix_world.noise) plus, where its row names a
steering, one wide-band interferer of sigma 6000 per component common to the elements with a phase per element; every case and
every reference is computed once per process.  UNIT_SAMPLES restates the launch plan's figure (csrc/dpe_arr_plan.h:
kArrUnitSamples); tests/test_arr_plan_cpu.py holds the C++ to it and the GPU test holds the handle's own figure to it."""
import functools

import numpy as np

from navlab_dpe_sdr_amd import engine, synth
from tests import arr_ref, ix_ref, ix_world

UNIT_SAMPLES = 4096
JAM_SIGMA = 6000.0


def unit_blocks(L):
    return max(1, UNIT_SAMPLES // L)


def needed(first, count, L, record_length=None):
    lo, hi = first // L * L, ((first + count - 1) // L + 1) * L
    if record_length is not None:
        hi = min(hi, record_length)
    return lo, max(hi, lo)


def elements(seed, M, n, steering=None):
    """complex [M, n] with integer parts inside int16: independent noise per element, plus the common interferer times
    exp(j steering[a])"""
    x = np.stack([ix_world.noise(1000 * seed + a, n) for a in range(M)])
    if steering is not None:
        rng = np.random.Generator(np.random.PCG64(7000 + seed))
        g = JAM_SIGMA * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        x = x + np.exp(1j * np.asarray(steering, dtype=np.float64))[:, None] * g[None, :]
    return np.stack([ix_world.to_i16(row) for row in x])


def i16_rows(x):
    """complex [M, n] -> int16 [M, 2 n]"""
    return np.stack([ix_world.i16_bytes(row) for row in x])


def random_constraints(seed, B, M):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.standard_normal((B, M)) + 1j * rng.standard_normal((B, M))


def _steer(M, k=1.0):
    return 2.0 * np.pi * 0.37 * k * np.arange(M) + 0.2 * np.arange(M) ** 2


# name -> M, L, first output, output count ("cross": from the third sample of a unit's last-but-one block over a whole unit more, so
#   two workgroups), and optionally cons (a seed and B for random complex constraints), reference (0), loading (1e-3), gain (1),
#   length (the record's), pad (samples of the buffers before and beyond the needed range), jam (False: noise alone), zero (a block,
#   counted from the first needed one, set to zero)
def _table():
    T = {}
    T["M2 L256 cross"] = dict(M=2, L=256, count="cross")
    T["M4 L1024 last reference, no loading"] = dict(M=4, L=1024, count="cross", reference=3, loading=0.0)
    T["M8 L256 three constraints, loading 1"] = dict(M=8, L=256, count="cross", cons=(31, 3), loading=1.0)
    T["M4 L256 negative gain"] = dict(M=4, L=256, first=777, count=700, gain=-0.75)
    T["M8 L1024 last reference"] = dict(M=8, L=1024, first=1024 + 5, count=2100, reference=7, jam=False)     # (with the interferer 1.8 % of its components are undecided)
    T["M2 L65536"] = dict(M=2, L=65536, first=65536 - 50, count=200)
    T["M2 L4096 cross"] = dict(M=2, L=4096, count="cross", loading=0.0)
    T["M3 L256 noise alone"] = dict(M=3, L=256, first=100, count=600, jam=False, gain=3.0)
    # edges
    T["first output 0"] = dict(M=4, L=1024, first=0, count=1500)
    T["record shorter than 2M"] = dict(M=4, L=256, first=0, count=300, length=7)
    T["record ends inside a block"] = dict(M=4, L=256, first=100, count=900, length=777)
    T["record ends 2M-1 into a block"] = dict(M=4, L=256, first=0, count=600, length=512 + 7)
    T["wide buffer"] = dict(M=2, L=256, first=2000, count=700, length=2600, pad=(391, 517))
    T["large indices"] = dict(M=4, L=256, first=2 ** 55 - 700 - 3, count=700)
    T["zero block"] = dict(M=4, L=256, first=256, count=768, zero=1)
    return T


CASES = _table()
PARITY = ("M2 L256 cross", "M4 L1024 last reference, no loading", "M8 L256 three constraints, loading 1", "M4 L256 negative gain",
          "M8 L1024 last reference", "M2 L65536", "M2 L4096 cross", "M3 L256 noise alone")
EDGES = ("first output 0", "record shorter than 2M", "record ends inside a block", "record ends 2M-1 into a block", "wide buffer", "large indices",
         "zero block")


@functools.lru_cache(maxsize=None)
def case(name):
    s = CASES[name]
    i = list(CASES).index(name)
    M, L = s["M"], s["L"]
    ub = unit_blocks(L)
    if s["count"] == "cross":
        first, count = (2 * ub - 2) * L + 3, (ub + 1) * L + 9
    else:
        first, count = s["first"], s["count"]
    length = s.get("length")
    lo, hi = needed(first, count, L, None)
    before, beyond = s.get("pad", (0, 0))
    x_first = lo - before
    n = hi + beyond - x_first                    # the buffers run over the record's end where there is one: those samples do not count
    x = elements(50 + i, M, n, _steer(M) if s.get("jam", True) else None)
    if "zero" in s:
        a = lo - x_first + s["zero"] * L
        x[:, a:a + L] = 0.0
    if "cons" in s:
        cons = random_constraints(*s["cons"], M)
    else:
        cons = arr_ref.unit_vector(M, s.get("reference", 0))
    return dict(name=name, M=M, L=L, B=cons.shape[0], cons=cons, explicit="cons" in s, reference=s.get("reference", 0), loading=s.get("loading", 1e-3),
                gain=s.get("gain", 1.0), x=x, x_first=x_first, record_length=length, out_first=first, out_count=count,
                needed=needed(first, count, L, length))


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    return arr_ref.process(c["x"], c["x_first"], c["record_length"], c["out_first"], c["out_count"], c["L"], c["cons"], c["loading"], c["gain"])


# ---- covariance: three blocks per (M, L), the last cut by the record, and the extreme inputs
COV_SHAPES = [(M, L) for M in (2, 3, 5, 8) for L in (256, 4096)]


@functools.lru_cache(maxsize=None)
def cov_case(M, L):
    first = 2
    x = elements(300 + M + L, M, 3 * L, _steer(M, 0.5))
    return dict(M=M, L=L, x=x, x_first=first * L, block_first=first, block_count=3, record_length=(first + 3) * L - L // 3)


def extreme(kind):
    if kind == "floor":          # one block at L = 65536, every component -32768: every entry of S is 2^47 (its imaginary parts 0)
        return dict(M=2, L=65536, x=np.full((2, 65536), -32768.0 - 32768.0j), x_first=0, block_first=0, block_count=1, record_length=None)
    n = np.arange(512)           # alternating +32767 / -32768, the two elements and the two parts in different phases of it
    alt = np.where(n % 2 == 0, 32767.0, -32768.0)
    x = np.stack([alt + 1j * alt[::-1], alt + 1j * alt, alt[::-1] - 1j * (alt + 1.0)])
    return dict(M=3, L=256, x=x, x_first=0, block_first=0, block_count=2, record_length=None)


# ---- the clipping case: a gain that takes 10-50 % of the components over the rails
@functools.lru_cache(maxsize=None)
def clip_case():
    M, L, first, count = 4, 256, 500, 1200
    lo, hi = needed(first, count, L)
    x = elements(77, M, hi - lo, _steer(M))
    return dict(name="clip", M=M, L=L, B=1, cons=arr_ref.unit_vector(M, 0), explicit=False, reference=0, loading=1e-3, gain=30.0, x=x, x_first=lo,
                record_length=None, out_first=first, out_count=count)


# ---- the end-to-end world: 4 SVs at 2.5 Msps on a 2 x 2 half-wavelength square under a broadband jammer 20 dB above the noise
WORLD_FS, WORLD_S = 2.5e6, 25000
WORLD_BINS = 100.0 * (np.arange(125) - 62)
WORLD_POS = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.5, 0.0], [0.5, 0.5, 0.0]])      # wavelengths
WORLD_SV = ((0.3, 1.0), (2.0, 0.6), (4.0, 0.9), (5.5, 0.4))                                     # (azimuth, elevation), rad
WORLD_JAMMER = (1.1, 0.05)


def los(az, el):
    return np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])


@functools.lru_cache(maxsize=None)
def world():
    ch = synth.random_channels(7, 4)
    x = np.zeros((4, WORLD_S), dtype=np.complex128)
    for k in range(4):
        one = {key: val[k:k + 1] for key, val in ch.items()}
        sv = ix_ref.from_i16(synth.gen_iq(5, WORLD_FS, WORLD_S, one, amp=60.0, sigma=0.0, dc=(0.0, 0.0), flip=np.zeros(1, dtype=bool)))
        x += engine.steering_vectors(WORLD_POS, los(*WORLD_SV[k]), wavelength=1.0)[0][:, None] * sv[None, :]
    rng = np.random.Generator(np.random.PCG64(11))
    x += 300.0 * (rng.standard_normal((4, WORLD_S)) + 1j * rng.standard_normal((4, WORLD_S)))
    jam = 3000.0 * (rng.standard_normal(WORLD_S) + 1j * rng.standard_normal(WORLD_S))
    x += engine.steering_vectors(WORLD_POS, los(*WORLD_JAMMER), wavelength=1.0)[0][:, None] * jam[None, :]
    x = np.stack([ix_world.to_i16(row) for row in x])
    t_start = (synth.L_CA - ch["rc"]) / ch["fc"]
    truth_idx = np.mod(t_start * WORLD_FS, 2500.0)
    truth_bin = np.array([int(np.argmin(np.abs(WORLD_BINS - f))) for f in ch["fi"]])
    return dict(ch=ch, x=x, rows=i16_rows(x), truth_idx=truth_idx, truth_bin=truth_bin)


def world_combined(L, loading):
    """the reference's power-inversion output of the world as interleaved int16"""
    w = world()
    r = arr_ref.process(w["x"], 0, WORLD_S, 0, WORLD_S, L, arr_ref.unit_vector(4, 0), loading, 1.0)
    return arr_ref.quantise(arr_ref.interleave(r["y"][0])), r
