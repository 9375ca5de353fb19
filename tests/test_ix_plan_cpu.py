"""The excisor's host-side planning (csrc/dpe_ix_plan.h) without a GPU: host/test_ix_plan.cpp, built with the host compiler, checks
the launch plan's properties itself (every output has one owner whose frames are the ones it is made of, what a block reads lies in
the needed range, every LDS and transform index stays inside the allocation from N = 64 to N = 4096, counted frames over any split
sum to those of one call) and evaluates the mappings -- needed ranges, hops and blocks, counted frames, owner, LDS layout, tables,
refusals -- for the cases written here, which are held to Python integers and to numpy."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import ix_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "navlab-dpe-sdr_amd", "host", "test_ix_plan.cpp")
HPB = ix_world.HOPS_PER_BLOCK


def _cxx():
    for c in ("g++", "c++", "clang++"):
        if shutil.which(c):
            return shutil.which(c)
    return None


def _cases():
    h = float.hex
    out = []
    for N in (64, 256, 4096):
        H = N // 2
        for first, count, length in ((0, 1, -1), (0, 100, 50), (5, 7, -1), (3 * H + 5, 17 * H + 9, -1), (2 ** 55 - 703, 700, -1), (1000, 10, 1003), (1000, 10, 3)):
            lo, hi = ix_world.needed(first, count, N, None if length < 0 else length)
            out.append(("needed %d %d %d %d" % (first, count, N, length), "%d %d" % (lo, hi)))
            h0, h1 = first // H, (first + count - 1) // H
            counted = sum(1 for k in range(h0, h1 + 1) if first <= k * H < first + count)
            out.append(("launch %d %d %d" % (first, count, N), "%d %d %d %d" % (h0, h1, (h1 - h0) // HPB + 1, counted)))
            n = first + count - 1
            b = (n // H - h0) // HPB
            out.append(("owner %d %d %d" % (n, first, N), "%d %d %d" % (b, h0 + b * HPB, min(h0 + b * HPB + HPB - 1, h1))))
        for ff, fc, length in ((0, 1, -1), (3, 6, -1), (3, 6, 4 * H + 1), (2 ** 55 // H - 5, 6, -1)):
            lo, hi = max((ff - 1) * H, 0), (ff + fc) * H
            if length >= 0:
                hi = min(hi, length)
            out.append(("frames %d %d %d %d" % (ff, fc, N, length), "%d %d" % (lo, max(hi, lo))))
        out.append(("lds %d" % N, "0 %d %d %d %d %d %d" % (8 * N, 12 * N, 13 * N, 13 * N + 1024, 13 * N + 1032, 13 * N + 1048)))
        for m, i in ((0, 0), (1, 1), (N // 8, N // 2), (N // 4 + 3, N - 1), (N // 2 - 1, 17)):
            out.append(("tables %d %d %d" % (N, m, i), np.array([np.cos(2 * np.pi * m / N), -np.sin(2 * np.pi * m / N), np.sin(np.pi * (i + 0.5) / N)])))
    for p, word in ((0.0, 0), (0.99, 0), (16760836.0, 16760836), (16760836.9, 16760836), (2.0 ** 31, 2 ** 31), (1e300, 2 ** 32 - 1)):
        out.append(("blank %s" % h(p), "%d" % word))
    ok = "cfg 1024 %s 1 %s %s 0 0" % (h(10.0), h(0.0), h(1.0))
    for line, pat in ((ok, "ok"), ("cfg 64 %s 31 %s %s 1 1" % (h(1e-3), h(5.0), h(-2.0)), "ok"), ("cfg 4096 %s 0 %s %s 0 1" % (h(1e6), h(0.0), h(0.0)), "ok"),
                      (ok.replace("1024", "1000"), "frame length N = 1000 is no power of two in 64..4096"), (ok.replace("1024", "32"), "N = 32 is no power of two"),
                      (ok.replace("1024", "8192"), "N = 8192 is no power of two"), (ok.replace("1024", "0"), "N = 0 is no power"),
                      ("cfg 1024 %s 1 %s %s 0 0" % (h(0.0), h(0.0), h(1.0)), "threshold not finite or not positive"),
                      ("cfg 1024 %s 1 %s %s 0 0" % (h(-1.0), h(0.0), h(1.0)), "threshold not finite or not positive"),
                      ("cfg 1024 nan 1 %s %s 0 0" % (h(0.0), h(1.0)), "threshold not finite"), ("cfg 1024 inf 1 %s %s 0 0" % (h(0.0), h(1.0)), "threshold not finite"),
                      ("cfg 1024 %s -1 %s %s 0 0" % (h(10.0), h(0.0), h(1.0)), "guard -1 outside 0..511"),
                      ("cfg 64 %s 32 %s %s 0 0" % (h(10.0), h(0.0), h(1.0)), "guard 32 outside 0..31"),
                      ("cfg 1024 %s 1 %s %s 0 0" % (h(10.0), h(-1.0), h(1.0)), "blanking power not finite or negative"),
                      ("cfg 1024 %s 1 inf %s 0 0" % (h(10.0), h(1.0)), "blanking power not finite"), ("cfg 1024 %s 1 %s nan 0 0" % (h(10.0), h(0.0)), "gain not finite"),
                      ("cfg 1024 %s 1 %s %s 2 0" % (h(10.0), h(0.0), h(1.0)), "input format 2"), ("cfg 1024 %s 1 %s %s 0 2" % (h(10.0), h(0.0), h(1.0)), "output format 2"),
                      # proc N in out xFirst xCount len outFirst outCount xAlign outAlign: outputs 777..1476 at N 256 need 640..1663
                      ("proc 256 0 0 640 1024 -1 777 700 0 0", "ok"), ("proc 256 0 0 641 1023 -1 777 700 0 0", "need the input samples 640..1663, the buffer holds 641..1663"),
                      ("proc 256 0 0 640 1023 -1 777 700 0 0", "the buffer holds 640..1662"), ("proc 256 0 0 640 1023 1663 777 700 0 0", "ok"),
                      ("proc 256 0 0 0 0 0 777 700 0 0", "ok"), ("proc 256 0 0 0 255 -1 0 1 0 0", "need the input samples 0..255"), ("proc 256 0 0 0 256 -1 0 1 0 0", "ok"),
                      ("proc 256 0 0 640 1024 -1 777 700 2 0", "input is not aligned to an I/Q pair (4 bytes)"), ("proc 256 1 0 640 1024 -1 777 700 4 0", "input is not aligned to an I/Q pair (8 bytes)"),
                      ("proc 256 0 0 640 1024 -1 777 700 4 0", "ok"), ("proc 256 0 0 640 1024 -1 777 700 0 2", "output is not aligned to an I/Q pair (4 bytes)"),
                      ("proc 256 0 1 640 1024 -1 777 700 0 4", "output is not aligned to an I/Q pair (8 bytes)"), ("proc 256 0 0 640 1024 -1 777 0 0 0", "0 outputs outside 1..2^30"),
                      ("proc 256 0 0 640 1024 -1 777 %d 0 0" % (2 ** 30 + 1), "outputs outside 1..2^30"), ("proc 256 0 0 640 1024 -1 -1 700 0 0", "first output -1"),
                      ("proc 256 0 0 -1 1024 -1 777 700 0 0", "input range -1 + 1024 negative"), ("proc 256 0 0 640 1024 -2 777 700 0 0", "record length -2"),
                      ("proc 256 0 0 %d 1024 -1 %d 700 0 0" % (2 ** 55 - 896, 2 ** 55 - 700), "ok"),
                      ("proc 256 0 0 %d 1024 -1 %d 700 0 0" % (2 ** 55 - 896, 2 ** 55 - 699), "with 700 outputs outside 0..2^55"),
                      ("ana 256 256 896 -1 3 6", "ok"), ("ana 256 257 895 -1 3 6", "frames 3..8 need the input samples 256..1151, the buffer holds 257..1151"),
                      ("ana 256 256 896 -1 3 0", "0 frames outside 1..2^24"), ("ana 256 256 896 -1 -1 6", "first frame -1"),
                      ("ana 256 %d 896 -1 %d 6" % (2 ** 55 - 768, 2 ** 55 // 128 - 5), "ok"), ("ana 256 %d 896 -1 %d 6" % (2 ** 55 - 768, 2 ** 55 // 128 - 4), "first frame")):
        out.append((line, pat))
    return out


def test_plan_properties_and_mappings(tmp_path):
    if _cxx() is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "test_ix_plan")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", exe], check=True)
    cases = _cases()
    path = tmp_path / "cases.txt"
    path.write_text("".join(line + "\n" for line, _ in cases))
    p = subprocess.run([exe, str(path)], check=True, stdout=subprocess.PIPE, text=True)     # (exit 1: a property failed, message on stderr)
    got = p.stdout.splitlines()
    assert len(got) == len(cases) > 120
    for (line, want), have in zip(cases, got):
        kind = line.split()[0]
        if kind == "tables":
            e = np.array([float.fromhex(v) for v in have.split()])
            assert np.all(np.abs(e - want) <= 2.0 ** -24) and np.all(e == e.astype(np.float32)), line
        elif kind in ("cfg", "proc", "ana"):
            assert (have == "ok") if want == "ok" else (have.startswith("[Excisor] ") and want in have), (line, have)
        else:
            assert have == want, line
