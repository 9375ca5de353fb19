"""Test-side synthesis for the scalar navigation stage: a GPS LNAV subframe ENCODER (IS-GPS-200, 20.3.3 and 20.3.5) -- ephemeris
fields and a time of week -> 300 bits with TLM, HOW and parity, subframes 4 and 5 as parity-valid filler -- and the cp_sign
stream (20 entries per bit) the decoder under test reads.  Written from the interface specification, independent of the decoder:
what the encoder lays down, the decoder (and, in tests/golden/make_golden_o15.py, the reference twin) must read back."""
import numpy as np

PI = 3.1415926535898
EPH_FIELDS = ["sqrt_A", "e", "i_0", "OMEGA_0", "omega", "M_0", "delta_n", "OMEGADOT", "IDOT", "C_rc", "C_rs", "C_uc", "C_us", "C_ic",
              "C_is", "t_oe", "t_oc", "a_f0", "a_f1", "a_f2", "T_GD"]
# name: (bits, signed, power of two of the LSB, times pi)
SCALE = {"sqrt_A": (32, False, -19, False), "e": (32, False, -33, False), "i_0": (32, True, -31, True),
         "OMEGA_0": (32, True, -31, True), "omega": (32, True, -31, True), "M_0": (32, True, -31, True),
         "delta_n": (16, True, -43, True), "OMEGADOT": (24, True, -43, True), "IDOT": (14, True, -43, True),
         "C_rc": (16, True, -5, False), "C_rs": (16, True, -5, False), "C_uc": (16, True, -29, False), "C_us": (16, True, -29, False),
         "C_ic": (16, True, -29, False), "C_is": (16, True, -29, False), "t_oe": (16, False, 4, False), "t_oc": (16, False, 4, False),
         "a_f0": (22, True, -31, False), "a_f1": (16, True, -43, False), "a_f2": (8, True, -55, False), "T_GD": (8, True, -31, False)}
# IS-GPS-200 table 20-XIV: which data bits (1-based) enter D25 .. D30, besides D29* / D30*
PARITY_BITS = [(1, 2, 3, 5, 6, 10, 11, 12, 13, 14, 17, 18, 20, 23), (2, 3, 4, 6, 7, 11, 12, 13, 14, 15, 18, 19, 21, 24),
               (1, 3, 4, 5, 7, 8, 12, 13, 14, 15, 16, 19, 20, 22), (2, 4, 5, 6, 8, 9, 13, 14, 15, 16, 17, 20, 21, 23),
               (1, 3, 5, 6, 7, 9, 10, 14, 15, 16, 17, 18, 21, 22, 24), (3, 5, 6, 8, 9, 10, 11, 13, 15, 19, 22, 23, 24)]
PARITY_STAR = [0, 1, 0, 1, 1, 0]     # D29* (0) or D30* (1) enters D25 .. D30


def quantise(eph):
    """{name: value} -> {name: integer}: the value in units of its LSB (two's complement where signed)."""
    q = {}
    for name, (bits, signed, p2, pi) in SCALE.items():
        v = float(eph[name]) / (PI if pi else 1.0) / 2.0 ** p2
        n = int(round(v))
        assert (-(1 << (bits - 1)) <= n < (1 << (bits - 1))) if signed else (0 <= n < (1 << bits)), (name, n)
        q[name] = n
    return q


def dequantise(q):
    """The doubles a decoder must give for the integers q: integer x 2^p, then (for the angles) one product with pi."""
    return {name: (q[name] * 2.0 ** p2) * PI if pi else q[name] * 2.0 ** p2 for name, (bits, signed, p2, pi) in SCALE.items()}


def _field(n, bits):
    return [(n >> (bits - 1 - i)) & 1 for i in range(bits)]       # two's complement for negative n, MSB first


def _word(d, d29s, d30s, solve_t=False):
    """24 source bits -> 30 transmitted bits (data bits complemented by D30*, then the six parity bits).  solve_t: choose the
    two last data bits so that D29 = D30 = 0 (words 2 and 10)."""
    d = list(d)
    star = (d29s, d30s)

    def par(i):
        return (star[PARITY_STAR[i]] + sum(d[j - 1] for j in PARITY_BITS[i])) & 1
    if solve_t:
        d[22] = d[23] = 0
        if par(4):
            d[23] = 1              # d24 enters D29, d23 does not
        if par(5):
            d[22] = 1              # d23 enters D30
        assert par(4) == 0 and par(5) == 0
    return [b ^ d30s for b in d] + [par(i) for i in range(6)]


def subframe_words(sf_id, tow, q, week=2008, accuracy=0, health=0, iode=77, iodc=77, filler_seed=0):
    """The ten 24-bit source words of subframe sf_id whose first bit leaves at time of week `tow` (a multiple of 6 s).  The HOW
    carries the count of the NEXT subframe's start, tow / 6 + 1 (20.3.3.2)."""
    rng = np.random.default_rng(1000 * filler_seed + sf_id)
    tlm = [1, 0, 0, 0, 1, 0, 1, 1] + [int(b) for b in rng.integers(0, 2, 14)] + [0, 0]
    how = _field((tow // 6 + 1) % (1 << 17), 17) + [0, 0] + _field(sf_id, 3) + [0, 0]
    w = [tlm, how]
    if sf_id == 1:
        w.append(_field(week % 1024, 10) + [0, 1] + _field(accuracy, 4) + _field(health << 5, 6) + _field(iodc >> 8, 2))
        w += [[int(b) for b in rng.integers(0, 2, 24)] for _ in range(3)]
        w.append([int(b) for b in rng.integers(0, 2, 16)] + _field(q["T_GD"], 8))
        w.append(_field(iodc & 255, 8) + _field(q["t_oc"], 16))
        w.append(_field(q["a_f2"], 8) + _field(q["a_f1"], 16))
        w.append(_field(q["a_f0"], 22) + [0, 0])
    elif sf_id == 2:
        w.append(_field(iode, 8) + _field(q["C_rs"], 16))
        m0, e, sa = _field(q["M_0"], 32), _field(q["e"], 32), _field(q["sqrt_A"], 32)
        w.append(_field(q["delta_n"], 16) + m0[:8])
        w.append(m0[8:])
        w.append(_field(q["C_uc"], 16) + e[:8])
        w.append(e[8:])
        w.append(_field(q["C_us"], 16) + sa[:8])
        w.append(sa[8:])
        w.append(_field(q["t_oe"], 16) + [0] + [0, 0, 0, 0, 0] + [0, 0])
    elif sf_id == 3:
        om0, i0, om = _field(q["OMEGA_0"], 32), _field(q["i_0"], 32), _field(q["omega"], 32)
        w.append(_field(q["C_ic"], 16) + om0[:8])
        w.append(om0[8:])
        w.append(_field(q["C_is"], 16) + i0[:8])
        w.append(i0[8:])
        w.append(_field(q["C_rc"], 16) + om[:8])
        w.append(om[8:])
        w.append(_field(q["OMEGADOT"], 24))
        w.append(_field(iode, 8) + _field(q["IDOT"], 14) + [0, 0])
    else:
        w += [[int(b) for b in rng.integers(0, 2, 24)] for _ in range(8)]
    assert len(w) == 10 and all(len(x) == 24 for x in w)
    return w


def encode_bits(sf_ids, tow0, q, **kw):
    """Transmitted bits (0 / 1) of consecutive subframes sf_ids, the first one starting at tow0.  The words are chained through
    D29* / D30*; before the first subframe both are 0, as after any word 10."""
    bits, d29s, d30s = [], 0, 0
    for n, sf in enumerate(sf_ids):
        for i, d in enumerate(subframe_words(sf, tow0 + 6 * n, q, **kw)):
            t = _word(d, d29s, d30s, solve_t=i in (1, 9))
            d29s, d30s = t[28], t[29]
            bits += t
    return np.array(bits, dtype=np.int8)


def sign_stream(bits, polarity=1):
    """cp_sign entries, 20 per bit: a 0 bit is +polarity, a 1 bit -polarity (the twin's preamble reads -1 1 1 1 -1 1 -1 -1)."""
    return np.repeat(polarity * (1 - 2 * bits.astype(np.int8)), 20).astype(np.int8)


def eph_row_to_dict(row):
    return {name: float(row[j]) for j, name in enumerate(EPH_FIELDS)}
