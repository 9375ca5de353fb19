"""The array combiner's host-side planning (csrc/dpe_arr_plan.h) without a GPU: host/test_arr_plan.cpp, built with the host compiler,
checks the launch plan's properties itself (every output has one owner whose blocks hold it, what a unit reads lies in the needed
range, the LDS regions stay inside the allocation for every (M, L), counted blocks over any split sum to those of one call, the
packed covariance gives the Hermitian matrix back) and evaluates the mappings -- needed ranges, blocks and units, counted blocks,
owner, samples inside the record, LDS layout, the apply chain, refusals -- for the cases written here, which are held to Python
integers and to numpy's fp32 FMA chain."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import arr_ref, arr_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "navlab-dpe-sdr_amd", "host", "test_arr_plan.cpp")


def _cxx():
    for c in ("g++", "c++", "clang++"):
        if shutil.which(c):
            return shutil.which(c)
    return None


def _padded(M):
    v = 4
    while v < M * M:
        v *= 2
    return v


def _fma32(a, b, c):
    """fp32 fma(a, b, c) for the values of _apply_case: the product and the sum are exact in fp64 (multiples of 2^-8 below 2^22), so
    the cast rounds once, as the FMA does"""
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


def _apply_case(seed, M):
    rng = np.random.Generator(np.random.PCG64(seed))
    v = rng.integers(-2 ** 10, 2 ** 10, 2 * M).astype(np.float32) / np.float32(256.0)      # multiples of 2^-8 below 4
    x = rng.integers(-32768, 32768, 2 * M).astype(np.float32)
    re = im = np.float32(0.0)
    for a in range(M):
        re = _fma32(v[2 * a], x[2 * a], re)
        re = _fma32(-v[2 * a + 1], x[2 * a + 1], re)
        im = _fma32(v[2 * a], x[2 * a + 1], im)
        im = _fma32(v[2 * a + 1], x[2 * a], im)
    line = "apply %d %s %s" % (M, " ".join(float(t).hex() for t in v), " ".join(float(t).hex() for t in x))
    return line, (re, im)


def _cases():
    h = float.hex
    out = []
    for L in (256, 1024, 65536):
        ub = arr_world.unit_blocks(L)
        for first, count, length in ((0, 1, -1), (0, 100, 50), (5, 7, -1), (3 * L + 5, 17 * L + 9, -1), (2 ** 55 - 703, 700, -1), (1000, 10, 1003), (1000, 10, 3),
                                     (L - 1, 2 * L + 2, 2 * L)):
            rl = None if length < 0 else length
            lo, hi = arr_world.needed(first, count, L, rl)
            out.append(("needed %d %d %d %d" % (first, count, L, length), "%d %d" % (lo, hi)))
            k0, k1 = first // L, (first + count - 1) // L
            out.append(("launch %d %d %d %d" % (first, count, L, length), "%d %d %d %d" % (k0, k1, (k1 - k0) // ub + 1, len(arr_ref.counted(first, count, L, rl)))))
            n = first + count - 1
            u = (n // L - k0) // ub
            out.append(("owner %d %d %d" % (n, first, L), "%d %d %d" % (u, k0 + u * ub, min(k0 + u * ub + ub - 1, k1))))
        for bf, bc, length in ((0, 1, -1), (3, 6, -1), (3, 6, 4 * L + 1), (2 ** 55 // L - 6, 6, -1), (5, 2, 3)):
            lo, hi = bf * L, (bf + bc) * L
            if length >= 0:
                hi = min(hi, length)
            out.append(("blocks %d %d %d %d" % (bf, bc, L, length), "%d %d" % (lo, max(hi, lo))))
        for k, length in ((0, -1), (3, 3 * L), (3, 3 * L + 7), (3, 4 * L), (3, 4 * L + 1), (3, 5), (2 ** 55 // L - 1, -1)):
            out.append(("samples %d %d %d" % (k, L, length), "%d" % (L if length < 0 else min(max(length - k * L, 0), L))))
    for M in range(2, 9):
        for L in (256, 512, 2048, 4096, 65536):
            ub = arr_world.unit_blocks(L)
            cov, part = 0, 8 * ub * M * M
            applied = part + 16 * 4 * _padded(M)
            fallback = applied + 8 * ub * 4 * M
            out.append(("lds %d %d" % (M, L), "0 %d %d %d %d %d" % (part, applied, fallback, fallback + 4 * ub, fallback + 4 * ub + 16)))
        out.append(_apply_case(40 + M, M))
    ok = "cfg 4 1024 1 %s %s 0 0 none" % (h(1e-3), h(1.0))
    for line, pat in ((ok, "ok"), ("cfg 8 65536 4 %s %s 1 0 ok" % (h(0.0), h(-2.0)), "ok"), ("cfg 2 256 1 %s %s 0 1 none" % (h(1.0), h(0.0)), "ok"),
                      (ok.replace("cfg 4", "cfg 1"), "1 elements outside 2..8"), (ok.replace("cfg 4", "cfg 9"), "9 elements outside 2..8"),
                      (ok.replace("1024", "1000"), "block length L = 1000 is no power of two in 256..65536"), (ok.replace("1024", "128"), "L = 128 is no power of two"),
                      (ok.replace("1024", "131072"), "L = 131072 is no power of two"), ("cfg 4 1024 0 %s %s 0 0 ok" % (h(1e-3), h(1.0)), "0 constraints outside 1..4"),
                      ("cfg 4 1024 5 %s %s 0 0 ok" % (h(1e-3), h(1.0)), "5 constraints outside 1..4"),
                      ("cfg 4 1024 2 %s %s 0 0 none" % (h(1e-3), h(1.0)), "2 constraints without constraint vectors"),
                      ("cfg 4 1024 1 %s %s 0 4 none" % (h(1e-3), h(1.0)), "reference element 4 outside 0..3"),
                      ("cfg 4 1024 1 %s %s 0 -1 none" % (h(1e-3), h(1.0)), "reference element -1 outside 0..3"),
                      ("cfg 4 1024 1 %s %s 0 0 none" % (h(-1e-3), h(1.0)), "loading not finite or negative"), ("cfg 4 1024 1 nan %s 0 0 none" % h(1.0), "loading not finite"),
                      ("cfg 4 1024 1 inf %s 0 0 none" % h(1.0), "loading not finite"), ("cfg 4 1024 1 %s nan 0 0 none" % h(1e-3), "gain not finite"),
                      ("cfg 4 1024 1 %s inf 0 0 none" % h(1e-3), "gain not finite"), ("cfg 4 1024 1 %s %s 2 0 none" % (h(1e-3), h(1.0)), "output format 2 is neither"),
                      ("cfg 4 1024 3 %s %s 0 0 zero" % (h(1e-3), h(1.0)), "constraint 2 is zero"), ("cfg 4 1024 3 %s %s 0 0 nan" % (h(1e-3), h(1.0)), "constraint 0 is not finite"),
                      # proc M L B out xFirst xCount len outFirst outCount xAddr0 xStride outAddr0 outStride: outputs 777..1476 at L 256 need 768..1535
                      ("proc 4 256 1 0 768 768 -1 777 700 4096 4096 65536 4096", "ok"),
                      ("proc 4 256 1 0 769 767 -1 777 700 4096 4096 65536 4096", "need the input samples 768..1535, the buffers hold 769..1535"),
                      ("proc 4 256 1 0 768 767 -1 777 700 4096 4096 65536 4096", "the buffers hold 768..1534"), ("proc 4 256 1 0 768 767 1535 777 700 4096 4096 65536 4096", "ok"),
                      ("proc 4 256 1 0 0 0 0 777 700 4096 4096 65536 4096", "ok"), ("proc 4 256 1 0 0 255 -1 0 1 4096 4096 65536 4096", "need the input samples 0..255"),
                      ("proc 4 256 1 0 0 256 -1 0 1 4096 4096 65536 4096", "ok"), ("proc 4 256 1 0 768 768 -1 777 700 4098 4096 65536 4096", "input of element 0 is not aligned to an I/Q pair (4 bytes)"),
                      ("proc 4 256 2 0 768 768 -1 777 700 4096 4096 65536 4098", "output of constraint 1 is not aligned to an I/Q pair (4 bytes)"),
                      ("proc 4 256 2 1 768 768 -1 777 700 4096 4096 65536 4100", "output of constraint 1 is not aligned to an I/Q pair (8 bytes)"),
                      ("proc 4 256 2 1 768 768 -1 777 700 4096 4096 65536 8000", "ok"), ("proc 4 256 1 0 768 768 -1 777 700 0 4096 65536 4096", "null input buffer of element 0"),
                      ("proc 4 256 1 0 768 768 -1 777 700 4096 -4 65536 4096", "null input buffer of element 3"), ("proc 4 256 1 0 768 768 -1 777 700 4096 4096 0 4096", "null output buffer of constraint 0"),
                      ("proc 4 256 1 0 768 768 -1 777 700 4096 4096 65536 4096", "ok"), ("proc 4 256 1 0 768 768 -1 777 0 4096 4096 65536 4096", "0 outputs outside 1..2^30"),
                      ("proc 4 256 1 0 768 768 -1 777 %d 4096 4096 65536 4096" % (2 ** 30 + 1), "outputs outside 1..2^30"), ("proc 4 256 1 0 768 768 -1 -1 700 4096 4096 65536 4096", "first output -1"),
                      ("proc 4 256 1 0 -1 768 -1 777 700 4096 4096 65536 4096", "input range -1 + 768 negative"), ("proc 4 256 1 0 768 768 -2 777 700 4096 4096 65536 4096", "record length -2"),
                      # the inputs hold 3072 bytes each from 4096 + 4096 a; outputs of 2800 bytes
                      ("proc 4 256 1 0 768 768 -1 777 700 4096 4096 19452 4096", "output of constraint 0 overlaps the input of element 3"),
                      ("proc 4 256 1 0 768 768 -1 777 700 4096 4096 19456 4096", "ok"), ("proc 4 256 1 0 768 768 -1 777 700 4096 4096 1300 4096", "overlaps the input of element 0"),
                      ("proc 4 256 1 0 768 768 -1 777 700 4096 4096 1296 4096", "ok"), ("proc 4 256 2 0 768 768 -1 777 700 4096 4096 1296 4096", "output of constraint 1 overlaps the input of element 0"),
                      ("proc 4 256 1 0 %d 768 -1 %d 700 4096 4096 65536 4096" % (2 ** 55 - 768, 2 ** 55 - 700), "ok"),
                      ("proc 4 256 1 0 %d 768 -1 %d 700 4096 4096 65536 4096" % (2 ** 55 - 768, 2 ** 55 - 699), "with 700 outputs outside 0..2^55"),
                      ("ana 4 256 768 1536 -1 3 6", "ok"), ("ana 4 256 769 1535 -1 3 6", "blocks 3..8 need the input samples 768..2303, the buffers hold 769..2303"),
                      ("ana 4 256 768 1536 -1 3 0", "0 blocks outside 1..2^24"), ("ana 4 256 768 1536 -1 -1 6", "first block -1"),
                      ("ana 4 256 %d 1536 -1 %d 6" % (2 ** 55 - 1536, 2 ** 55 // 256 - 6), "ok"), ("ana 4 256 %d 1536 -1 %d 6" % (2 ** 55 - 1536, 2 ** 55 // 256 - 5), "first block")):
        out.append((line, pat))
    return out


def test_plan_properties_and_mappings(tmp_path):
    if _cxx() is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "test_arr_plan")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", exe], check=True)
    cases = _cases()
    path = tmp_path / "cases.txt"
    path.write_text("".join(line + "\n" for line, _ in cases))
    p = subprocess.run([exe, str(path)], check=True, stdout=subprocess.PIPE, text=True)     # (exit 1: a property failed, message on stderr)
    got = p.stdout.splitlines()
    assert len(got) == len(cases) > 150
    for (line, want), have in zip(cases, got):
        kind = line.split()[0]
        if kind == "apply":
            e = [np.float32(float.fromhex(v)) for v in have.split()]
            assert e[0] == want[0] and e[1] == want[1], (line, have, want)
        elif kind in ("cfg", "proc", "ana"):
            assert (have == "ok") if want == "ok" else (have.startswith("[ArrayCombiner] ") and want in have), (line, have)
        else:
            assert have == want, (line, have, want)
