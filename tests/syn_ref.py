"""Numpy restatement of the synthesiser's model (include/dpe_hip.h, "Signal synthesiser"): the fp64 PRE-ROUNDING value x_ref of
every sample, for the window form and the record form, with its own Philox4x32-10 and an fp64 Box-Muller.  The chip index, the nav
sign and the sample-to-counter mapping are written as synth.py writes them (numpy fp64, floor modulus); tests/test_syn_ref_cpu.py
pins clip(rint(x_ref)) at sigma = 0 to synth.gen_iq / synth.gen_iq_record element for element, the generator to its known answers
and the noise to its moments.  Test infrastructure only: nothing of the package imports it."""
import numpy as np

from navlab_dpe_sdr_amd import synth

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or scalars) of one shape, key: two uint32 scalars.  Returns the four output words (uint32 arrays)."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & MASK for x in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                      # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def gauss(seed, stream, n):
    """(gI, gQ) in fp64 for the sample indices n (uint64 array) of one stream under one seed."""
    n = np.asarray(n, dtype=np.uint64)
    seed, stream = int(seed) & (2 ** 64 - 1), int(stream) & (2 ** 64 - 1)
    w = philox4x32_10((n & MASK, n >> np.uint64(32), np.uint64(stream & 0xFFFFFFFF), np.uint64(stream >> 32)),
                      (seed & 0xFFFFFFFF, seed >> 32))
    u1 = ((w[0] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (w[1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)


def _signal(t, ch, k, amp, sign):
    chips = synth.ca_code(int(ch["prn"][k])).astype(np.float64)
    ci = np.floor(t * ch["fc"][k] + ch["rc"][k]).astype(np.int64)
    ph = ch["fi"][k] * t + ch["ri"][k]
    return ci, amp * sign(ci) * chips[np.mod(ci, synth.L_CA)] * np.exp(2j * np.pi * (ph - np.floor(ph)))


def window(fs, S, ch, amp, sigma, dc, flip, seed, stream):
    """x_ref (complex128 [S]) of one window: synth.gen_iq's signal, noise stream `stream` with the in-window index as counter."""
    K = len(ch["prn"])
    t = synth.time_idx(S, fs)
    amp = np.broadcast_to(np.asarray(amp, dtype=np.float64), (K,))
    x = np.zeros(S, dtype=np.complex128)
    for k in range(K):
        nb = synth.nav_bit_boundary(ch["cp"][k], ch["cp_ref"][k], ch["rc"][k], ch["fc"][k], fs)
        d = np.ones(S)
        if flip is not None and flip[k] and 0 < nb < S:
            d[nb:] = -1.0
        x += _signal(t, ch, k, amp[k], lambda ci: d)[1]
    if sigma:
        gi, gq = gauss(seed, stream, np.arange(S, dtype=np.uint64))
        x += sigma * (gi + 1j * gq)
    return x + complex(dc[0], dc[1])


def record(fs, first, n_samples, ch, amp, sigma, nav_bits, seed, stream, dc=(0.0, 0.0)):
    """x_ref (complex128 [n_samples]) of samples [first, first + n_samples) of a record: synth.gen_iq_record's signal, noise
    stream `stream` with the absolute index as counter."""
    K = len(ch["prn"])
    n = np.arange(first, first + n_samples, dtype=np.int64)
    t = n.astype(np.float64) / fs
    amp = np.broadcast_to(np.asarray(amp, dtype=np.float64), (K,))
    x = np.zeros(n_samples, dtype=np.complex128)
    for k in range(K):
        bits = np.asarray(nav_bits[k], dtype=np.int8)
        fe = int(ch["cp_ref"][k]) % 20 if "cp_ref" in ch else 0

        def sign(ci, bits=bits, fe=fe):
            idx = (ci // synth.L_CA - fe + 20) // 20
            assert idx.min() >= 0 and idx.max() < bits.size
            return bits[idx]
        x += _signal(t, ch, k, amp[k], sign)[1]
    if sigma:
        gi, gq = gauss(seed, stream, n.astype(np.uint64))
        x += sigma * (gi + 1j * gq)
    return x + complex(dc[0], dc[1])


def quantise(x):
    """clip(rint(x)) per component as interleaved int16 [2 len(x)]."""
    iq = np.empty(2 * x.size, dtype=np.int16)
    iq[0::2] = np.clip(np.rint(x.real), -32768, 32767).astype(np.int16)
    iq[1::2] = np.clip(np.rint(x.imag), -32768, 32767).astype(np.int16)
    return iq


def n_bits_needed(fs, last_sample, ch):
    """Per channel: how many nav bits a record needs whose last sample is `last_sample`."""
    t = np.float64(last_sample) / fs
    out = []
    for k in range(len(ch["prn"])):
        ci = int(np.floor(t * ch["fc"][k] + ch["rc"][k]))
        fe = int(ch["cp_ref"][k]) % 20 if "cp_ref" in ch else 0
        out.append((ci // synth.L_CA - fe + 20) // 20 + 1)
    return out


# ---- the shapes of tests/test_gpu_syn.py, shared with tests/test_syn_ref_cpu.py (which pins the restatement at every one of them)
def channels(seed, K, fs, rc_edge=False, fi_sign=None):
    """synth.random_channels with the edge cases the tests ask for: code phases within 1e-9 of 0 and of 1023, fi of either sign."""
    ch = synth.random_channels(seed, K)
    if fi_sign is not None:
        ch["fi"] = fi_sign * np.abs(ch["fi"])
        ch["fc"] = synth.F_CA * (1.0 + ch["fi"] / synth.F_L1)
    if rc_edge:
        ch["rc"][0] = 5e-10
        ch["rc"][-1] = 1023.0 - 5e-10
    return ch


WINDOW_SHAPES = [   # (name, fs, S, K, W, sigma, dc, flip mode, rc_edge, fi_sign)
    ("S12500_K8", 2.5e6, 12500, 8, 1, 300.0, (3.0, -2.0), "predicted", False, None),
    ("S4093_K12_W5", 25e6, 4093, 12, 5, 300.0, (3.0, -2.0), "predicted", True, -1.0),
    ("S4093_K1_clean", 2.5e6, 4093, 1, 1, 0.0, (0.0, 0.0), "none", True, 1.0),
    ("S7_K8_W5", 2.5e6, 7, 8, 5, 300.0, (-1.5, 0.5), "predicted", False, None),
    ("S12500_K12_clean", 25e6, 12500, 12, 1, 0.0, (3.0, -2.0), "edges", False, None),
]


def window_case(shape):
    """Channels [W] (each window its own seed), amplitudes (sum <= 400), flip flags [W][K] for a row of WINDOW_SHAPES.
    flip mode "edges": channel 0 flips at sample 1, channel 1 at S - 1, channel 2's boundary lies outside the window (its flag is set
    and must do nothing); the code phases are chosen so that synth.nav_bit_boundary gives exactly these."""
    name, fs, S, K, W, sigma, dc, mode, rc_edge, fi_sign = shape
    chs = [channels(100 + 7 * w, K, fs, rc_edge, fi_sign) for w in range(W)]
    amp = np.linspace(20.0, 40.0, K) if K > 1 else np.array([400.0])
    amp = amp * min(1.0, 400.0 / amp.sum())
    flips = np.zeros((W, K), dtype=bool)
    if mode == "predicted":
        flips[:] = np.random.Generator(np.random.PCG64(5)).integers(0, 2, (W, K)).astype(bool)
        flips[:, 0] = True
    elif mode == "edges":
        for ch in chs:
            for k, want in ((0, 1), (1, S - 1), (2, S + 10)):
                ch["cp"][k], ch["cp_ref"][k] = 1019, 1000          # one code period to the boundary
                # boundary = floor((1023 - rc) fs / fc) + 1 = want  <=  (1023 - rc) fs / fc = want - 0.5
                ch["rc"][k] = 1023.0 - (want - 0.5) * ch["fc"][k] / fs
                assert synth.nav_bit_boundary(ch["cp"][k], ch["cp_ref"][k], ch["rc"][k], ch["fc"][k], fs) == want
            flips[:, :3] = True
    return chs, amp, flips


RECORD = dict(fs=2.5e6, n=40000, K=8, sigma=300.0, seed=77)


def record_case(first=0, n=None):
    """Channels, amplitudes and nav bits of the record tests: cp_ref spread over 0..19 so that bit edges fall inside 40 000 samples
    (16 code periods) for most channels."""
    fs, K = RECORD["fs"], RECORD["K"]
    ch = channels(31, K, fs)
    ch["cp_ref"] = (1000 + np.array([1, 3, 5, 8, 10, 12, 15, 0])[:K]).astype(np.int32)
    amp = np.linspace(30.0, 60.0, K)
    last = first + (RECORD["n"] if n is None else n) - 1
    rng = np.random.Generator(np.random.PCG64(9))
    bits = [(2 * rng.integers(0, 2, nb + 2) - 1).astype(np.int8) for nb in n_bits_needed(fs, last, ch)]
    return ch, amp, bits
