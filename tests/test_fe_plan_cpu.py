"""The front end's host-side planning (csrc/dpe_fe_plan.h) without a GPU: host/test_fe_plan.cpp, built with the host compiler,
checks the tile geometry's properties itself (every output of a call has exactly one owner, the staged tile covers what its outputs
read, every index stays inside the LDS allocation and the exact range of the division, at the extreme D and T too) and evaluates
the mappings -- phase increment, phase word, needed range, geometry, owner, modulated taps, refusals, the int16 output word -- for the
cases written here, which are held to Python integers and to numpy exactly."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import fe_ref, fe_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "navlab-dpe-sdr_amd", "host", "test_fe_plan.cpp")
FMT = {n: i for i, n in enumerate(fe_ref.FORMATS)}


def _cxx():
    for c in ("g++", "c++", "clang++"):
        if shutil.which(c):
            return shutil.which(c)
    return None


def _tap(d, t):
    """The mode-2 table entry of tap t for gain 1, h = 1: (cr, ci, -ci, cr) with cr + j ci = exp(-2 pi j ((t d) mod 2^32) / 2^32),
    as fp32.  cos and sin may differ from the C library's in the last bit of the fp64 value: compared to one fp32 ulp."""
    w = (t * d) % (1 << 32)
    a = 2.0 * np.pi * w / 4294967296.0
    return np.array([np.cos(a), -np.sin(a), np.sin(a), np.cos(a)])


def _table(D, T, mode):
    """The whole table [D][ceil(T / D)][4] for gain 1, delta 0 and the distinct taps h[t] = t + 1: entry (t mod D, t div D) carries
    t + 1 -- (h, 0, 0, 0) for real input, (h, h, 0, 0) for real taps, (h, 0, 0, h) for complex taps -- and every other entry is zero."""
    tab = np.zeros((D, -(-T // D), 4))
    for t in range(T):
        tab[t % D, t // D] = ((t + 1, 0, 0, 0), (t + 1, t + 1, 0, 0), (t + 1, 0, 0, t + 1))[mode]
    return tab.ravel()


def _quant(re, im):
    """The int16 I/Q word of an fp32 pair and the components clipped: rounded half to even in fp32, clipped to the rails, I in the low
    half of the little-endian word."""
    r = np.rint(np.array([re, im], dtype=np.float32))
    q = np.clip(r, -32768.0, 32767.0)
    return "%d %d" % (q.astype("<i2").view("<u4")[0], np.count_nonzero(q != r))


def _cases():
    rng = np.random.Generator(np.random.PCG64(21))
    h = float.hex
    out = []
    for fs, f in ((10e6, 2.5e6), (10e6, -2.5e6), (25e6, 0.0), (10e6, 1234567.8), (16.368e6, 4.092e6), (16.368e6, -4.092e6), (5e6, 5e6), (5e6, -5e6),
                  (4e6, 1.0), (4e6, -1.0)):
        d = fe_ref.delta(f, fs)
        real = d * fs / 4294967296.0
        out.append(("delta %s %s" % (h(f), h(fs)), ("%d" % d, real - fs if d > 2 ** 31 else real)))
    for d in (1, 2 ** 30, 3 * 2 ** 30, 530243895, 2 ** 32 - 1):
        for n in [0, 1, -1, -511, 2 ** 33 + 1, 2 ** 33 - 1, 2 ** 40 + 12345, 2 ** 40 - 1, 2 ** 61 + 3] + rng.integers(2 ** 33, 2 ** 41, 6).tolist():
            out.append(("phase %d %d" % (n, d), "%d" % ((n * d) % (1 << 32))))
    for D, T in ((1, 1), (4, 33), (10, 81), (64, 1023), (3, 25)):
        T0 = (T - 1) // 2
        for first, count, length in ((0, 1, -1), (0, 100, 50), (5, 7, -1), (2 ** 33 // D + 9, 1285, -1), (1000, 10, 1000 * D + 2), (1000, 10, 3)):
            lo, hi = max(first * D - T0, 0), (first + count - 1) * D + T - T0
            if length >= 0:
                hi = min(hi, length)
            out.append(("needed %d %d %d %d %d" % (first, count, D, T, length), "%d %d" % (lo, max(hi, lo))))
        for real in (0, 1):
            tile = fe_world.tile_outputs(D, T, bool(real))
            Q = -(-T // D)
            out.append(("geom %d %d %d" % (D, T, real), "%d %d %d %d %d %d" % (tile, tile + Q - 1, tile + Q, fe_world.lds_bytes(D, T, bool(real)), Q, T - (Q - 1) * D)))
            for i in [0, 1, 4, 5, tile - 1, tile, tile + 1, 3 * tile + 6, 2 ** 30 - 1]:
                out.append(("owner %d %d %d %d" % (D, T, real, i), "%d %d %d" % (i // tile, i % tile // 5, i % tile % 5)))
        for d in (2 ** 30, 3 * 2 ** 30, 530243895):
            for t in sorted({0, min(1, T - 1), T // 2, T - 1}):
                out.append(("tap %d %d 0 %d %d" % (D, T, d, t), _tap(d, t)))
        for mode in (0, 1, 2):
            out.append(("taps %d %d %d" % (D, T, mode), _table(D, T, mode)))
    I16C, P2R, P2C = FMT["I16C"], FMT["P2R"], FMT["P2C"]
    for line, pat in (("cfg %d 0 4 33 %s %s" % (I16C, h(1e7), h(0.0)), "ok"), ("cfg %d 1 64 1023 %s %s" % (P2C, h(1e7), h(-1e7)), "ok"),
                      ("cfg %d 0 4 32 %s %s" % (I16C, h(1e7), h(0.0)), "T = 32 taps is even"), ("cfg %d 0 0 33 %s %s" % (I16C, h(1e7), h(0.0)), "D = 0 outside 1..64"),
                      ("cfg %d 0 65 33 %s %s" % (I16C, h(1e7), h(0.0)), "D = 65 outside 1..64"), ("cfg %d 0 4 1025 %s %s" % (I16C, h(1e7), h(0.0)), "T = 1025 taps outside 1..1023"),
                      ("cfg %d 0 4 0 %s %s" % (I16C, h(1e7), h(0.0)), "T = 0 taps outside"), ("cfg 7 0 4 33 %s %s" % (h(1e7), h(0.0)), "input format 7"),
                      ("cfg %d 2 4 33 %s %s" % (I16C, h(1e7), h(0.0)), "output format 2"), ("cfg %d 0 4 33 %s %s" % (I16C, h(0.0), h(0.0)), "sampling frequency"),
                      ("cfg %d 0 4 33 %s %s" % (I16C, h(1e7), h(2e7)), "intermediate frequency"),
                      # conv fmt D T rawFirst rawCount len outFirst outCount rawAlign outAlign: outputs 100..109 at D 4 T 33 need 384..452
                      ("conv %d 4 33 384 69 -1 100 10 0 0" % I16C, "ok"), ("conv %d 4 33 385 68 -1 100 10 0 0" % I16C, "need the input samples 384..452, the buffer holds 385..452"),
                      ("conv %d 4 33 384 68 -1 100 10 0 0" % I16C, "the buffer holds 384..451"), ("conv %d 4 33 384 68 452 100 10 0 0" % I16C, "ok"),
                      ("conv %d 4 33 0 4 -1 0 1 0 0" % I16C, "need the input samples 0..16"), ("conv %d 4 33 0 17 -1 0 1 0 0" % I16C, "ok"),
                      ("conv %d 4 33 382 71 -1 100 10 0 0" % P2R, "not on a byte boundary (4 samples per byte)"), ("conv %d 4 33 380 73 -1 100 10 0 0" % P2R, "ok"),
                      ("conv %d 4 33 383 70 -1 100 10 0 0" % P2C, "not on a byte boundary (2 samples per byte)"),
                      ("conv %d 4 33 384 69 -1 100 10 2 0" % I16C, "input is not aligned to a sample (4 bytes)"), ("conv %d 4 33 384 69 -1 100 10 0 2" % I16C, "output is not aligned"),
                      ("conv %d 4 33 384 69 -1 100 0 0 0" % I16C, "0 outputs outside"), ("conv %d 4 33 384 69 -1 -1 10 0 0" % I16C, "first output -1"),
                      ("conv %d 4 33 384 69 -2 100 10 0 0" % I16C, "record length -2"), ("conv %d 4 33 0 0 0 100 10 0 0" % I16C, "ok"),
                      # every output index below 2^55: D 64 T 513, the buffer holds what 201 outputs from 2^55 - 200 would read
                      ("conv %d 64 513 %d 14000 -1 %d 200 0 0" % (FMT["I8C"], 2 ** 61 - 13056, 2 ** 55 - 200), "ok"),
                      ("conv %d 64 513 %d 14000 -1 %d 201 0 0" % (FMT["I8C"], 2 ** 61 - 13056, 2 ** 55 - 200), "with 201 outputs outside 0..2^55"),
                      ("conv %d 64 513 %d 14000 -1 %d 1 0 0" % (FMT["I8C"], 2 ** 61 - 13056, 2 ** 55 - 1), "ok"),
                      ("conv %d 64 513 %d 14000 -1 %d 1 0 0" % (FMT["I8C"], 2 ** 61 - 13056, 2 ** 55), "first output 36028797018963968 with 1 outputs outside 0..2^55")):
        out.append((line, pat))
    # ties, the signed zero, either side of both rails (32767.5 rounds to 32768 and clips, -32768.5 to -32768 and does not), far
    # outside, both components clipped
    pairs = [(0.5, 1.5), (2.5, -0.5), (-1.5, -0.0), (-0.0, 0.0), (32767.49, 32767.5), (32768.0, 32767.0), (-32768.5, -32769.0), (-32768.0, -32768.49),
             (1e9, -1e9), (-1e9, 12345.0), (40000.0, -40000.0), (32767.5, -32769.0), (-1.0, 1.0), (-32767.5, 32766.5)]
    pairs += [tuple(v) for v in (rng.integers(-2 ** 17, 2 ** 17, (12, 2)) / 4.0).tolist()]
    for re, im in pairs:
        re, im = float(np.float32(re)), float(np.float32(im))
        out.append(("quant %s %s" % (h(re), h(im)), _quant(re, im)))
    return out


def test_plan_properties_and_mappings(tmp_path):
    if _cxx() is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "test_fe_plan")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", exe], check=True)
    cases = _cases()
    path = tmp_path / "cases.txt"
    path.write_text("".join(line + "\n" for line, _ in cases))
    p = subprocess.run([exe, str(path)], check=True, stdout=subprocess.PIPE, text=True)     # (exit 1: a property failed, message on stderr)
    got = p.stdout.splitlines()
    assert len(got) == len(cases) > 200
    for (line, want), have in zip(cases, got):
        kind = line.split()[0]
        if kind == "delta":
            d, real = have.split()
            assert d == want[0] and float.fromhex(real) == want[1], line
            f, fs = (float.fromhex(v) for v in line.split()[1:])
            assert abs(float.fromhex(real) - f) <= fs / 2 ** 33 or abs(f) == fs, line     # (+-fs is the alias of 0)
        elif kind == "tap":
            e = np.array([float.fromhex(v) for v in have.split()])
            assert np.all(np.abs(e - want) <= 2.0 ** -24) and e[2] == -e[1] and e[3] == e[0], line
            assert np.all(e == e.astype(np.float32)), line
        elif kind == "taps":
            assert np.array_equal(np.array([float.fromhex(v) for v in have.split()]), want), line      # (-0.0 equals 0.0)
        elif kind in ("cfg", "conv"):
            assert (have == "ok") if want == "ok" else (have.startswith("[FrontEnd] ") and want in have), (line, have)
        else:
            assert have == want, line
