"""The front end's specification in fp64 numpy (include/dpe_hip.h, "Front end"), written from the formulas and from
nothing of the device code:

    y[m] = gain sum_{t<T} h[t] z[m D + t - T0],  T0 = (T - 1) / 2
    z[n] = x[n] exp(-2 pi j ((n delta) mod 2^32) / 2^32)  for 0 <= n < record_length, else 0
    delta = rint(f_IF / fs_in 2^32) mod 2^32
    out  = clip(rint(y), -32768, 32767) per component

plus the decoders of the seven input formats, encoders for building test records, and the derived tolerance."""
import numpy as np

FORMATS = ("I16C", "I8C", "I16R", "I8R", "ARGPI4", "P2R", "P2C")
BYTES = {"I16C": (4, 1), "I8C": (2, 1), "I16R": (2, 1), "I8R": (1, 1), "ARGPI4": (1, 1), "P2R": (1, 4), "P2C": (1, 2)}   # num / den per sample
REAL = {"I16R", "I8R", "P2R"}
LEVELS = (-3.0, -1.0, 1.0, 3.0)


def delta(f_if, fs_in):
    """The phase increment per input sample as a Python integer in [0, 2^32)."""
    return int(np.rint(np.float64(f_if) / np.float64(fs_in) * 4294967296.0)) % (1 << 32)


def phase_words(n, d):
    """(n delta) mod 2^32 for int64 indices n (any sign): the product wraps modulo 2^64, of which 2^32 is a divisor."""
    n = np.asarray(n, dtype=np.int64)
    with np.errstate(over="ignore"):
        return (n.view(np.uint64) * np.uint64(d)) & np.uint64(0xFFFFFFFF)


def decode(fmt, raw, first, count, levels=LEVELS):
    """x[first .. first + count) of a record whose sample 0 begins at byte 0 of `raw` (uint8 array), complex128."""
    raw = np.asarray(raw, dtype=np.uint8)
    n = np.arange(first, first + count, dtype=np.int64)
    lv = np.asarray(levels, dtype=np.float64)
    if fmt == "I16C":
        v = raw[4 * first:4 * (first + count)].view("<i2").astype(np.float64)
        return v[0::2] + 1j * v[1::2]
    if fmt == "I8C":
        v = raw[2 * first:2 * (first + count)].view(np.int8).astype(np.float64)
        return v[0::2] + 1j * v[1::2]
    if fmt == "I16R":
        return raw[2 * first:2 * (first + count)].view("<i2").astype(np.complex128)
    if fmt == "I8R":
        return raw[first:first + count].view(np.int8).astype(np.complex128)
    if fmt == "ARGPI4":
        return np.exp(1j * ((raw[first:first + count] & 7).astype(np.float64) * (np.pi / 4.0)))
    if fmt == "P2R":
        return lv[(raw[n >> 2] >> (2 * (n & 3)).astype(np.uint8)) & 3].astype(np.complex128)
    if fmt == "P2C":
        b = raw[n >> 1] >> (4 * (n & 1)).astype(np.uint8)
        return lv[b & 3] + 1j * lv[(b >> 2) & 3]
    raise ValueError(fmt)


def pack2(codes):
    """2-bit codes (0..3), four per byte, the first in the least significant bits; padded with code 0 to a whole byte."""
    c = np.asarray(codes, dtype=np.uint8)
    c = np.concatenate([c, np.zeros(-c.size % 4, dtype=np.uint8)]).reshape(-1, 4)
    return (c[:, 0] | (c[:, 1] << 2) | (c[:, 2] << 4) | (c[:, 3] << 6)).astype(np.uint8)


def random_record(fmt, n, rng, amp16=2047):
    """n samples of format fmt as bytes: int16 values within +-amp16, everything else every bit pattern."""
    num, den = BYTES[fmt]
    if fmt in ("I16C", "I16R"):
        return rng.integers(-amp16, amp16 + 1, n * num // 2).astype("<i2").view(np.uint8)
    return rng.integers(0, 256, -(-n * num // den), dtype=np.uint8)


def convert(x, x_first, record_length, out_first, out_count, D, h, gain, d):
    """y[out_first .. out_first + out_count) in complex128.  x holds the record's samples [x_first, x_first + len(x)); what the
    outputs need of [0, record_length) has to lie inside (record_length None: no end)."""
    h = np.asarray(h, dtype=np.float64)
    T = h.size
    T0 = (T - 1) // 2
    lo = out_first * D - T0
    hi = (out_first + out_count - 1) * D + T - T0
    n = np.arange(lo, hi, dtype=np.int64)
    inside = n >= 0
    if record_length is not None:
        inside &= n < record_length
    assert not inside.any() or (n[inside][0] >= x_first and n[inside][-1] < x_first + len(x)), "the reference's input does not hold the range"
    z = np.zeros(n.size, dtype=np.complex128)
    z[inside] = np.asarray(x)[n[inside] - x_first] * np.exp(-2j * np.pi * (phase_words(n[inside], d).astype(np.float64) / 4294967296.0))
    win = np.lib.stride_tricks.sliding_window_view(z, T)[::D]
    assert win.shape[0] == out_count
    return gain * (win @ h)


def quantise(y):
    """clip(rint(y)) per component as interleaved int16."""
    out = np.empty(2 * y.size, dtype=np.int16)
    out[0::2] = np.clip(np.rint(y.real), -32768, 32767).astype(np.int16)
    out[1::2] = np.clip(np.rint(y.imag), -32768, 32767).astype(np.int16)
    return out


def interleave(y):
    return np.stack([y.real, y.imag], axis=1).ravel()


def clip_count(y):
    v = np.rint(interleave(y))
    return int(((v < -32768) | (v > 32767)).sum())


def tolerance(h, gain, x_max):
    """(2 T + 16) 2^-24 A with A = gain sum|h| max|x|: 2 T for the fp32 multiply-adds of the two components, 16 for a mixer value
    within 2^-22 and the rotation."""
    h = np.asarray(h, dtype=np.float64)
    return (2 * h.size + 16) * 2.0 ** -24 * abs(gain) * np.abs(h).sum() * x_max


def band(y, tol):
    """Per interleaved component: the fp64 value lies within tol of a half-integer, where rounding may go either way."""
    v = interleave(y)
    return np.abs(v - np.floor(v) - 0.5) <= tol
