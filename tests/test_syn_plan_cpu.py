"""The synthesiser's host-side planning (csrc/dpe_syn_plan.h) without a GPU: host/test_syn_plan.cpp, built with the host compiler,
checks the launch geometry's properties itself (every sample of a segment belongs to exactly one block at every 16-byte phase, no
lane's group is split between blocks, the floor division is exact up to 2^51) and evaluates the fp64 mappings -- sample times, chip
index and code period, nav-bit boundary, nav-bit span of a record, the parameter block -- for the cases written here, which are held
to numpy and synth.py bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from navlab_dpe_sdr_amd import synth
from tests import syn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "navlab-dpe-sdr_amd", "host", "test_syn_plan.cpp")


def _cxx():
    for c in ("g++", "c++", "clang++"):
        if shutil.which(c):
            return shutil.which(c)
    return None


def _cases():
    """(line, expected answer) pairs."""
    rng = np.random.Generator(np.random.PCG64(11))
    out = []
    h = float.hex
    for fs in (2.5e6, 25e6, 4.0e6):
        for i in [0, 1, 2, 3, 7, 4092, 12499, 49999, 499999] + rng.integers(0, 500000, 20).tolist():
            t = np.round(np.float64(i) / fs * 1.0e9) / 1.0e9
            out.append(("tw %d %s" % (i, h(fs)), h(float(t))))
        for n in [0, 1, 39999, 2 ** 32 - 100, 2 ** 32, 2 ** 32 + 3993, 2 ** 40 + 1] + rng.integers(0, 2 ** 33, 20).tolist():
            out.append(("tr %d %s" % (n, h(fs)), h(float(np.float64(n) / fs))))
    ch = syn_ref.channels(5, 12, 2.5e6, rc_edge=True)
    for k in range(12):
        fc, rc = float(ch["fc"][k]), float(ch["rc"][k])
        for t in [0.0, 4e-7, 1e-3, 0.016, 1717.986, 1717.9869184] + rng.uniform(0, 2000, 10).tolist():
            ci = int(np.floor(np.float64(t) * fc + rc))
            out.append(("chip %s %s %s" % (h(t), h(fc), h(rc)), "%d %d" % (ci % 1023, ci // 1023)))
        out.append(("chip %s %s %s" % (h(0.0), h(fc), h(-0.25)), "1022 -1"))          # floor modulus below zero
        for fs in (2.5e6, 25e6):
            for cp, ref in ((1000, 1000 + k), (1019, 1000), (5, 17), (40, 1)):
                out.append(("flip %d %d %s %s %s" % (cp, ref, h(rc), h(fc), h(fs)), "%d" % synth.nav_bit_boundary(cp, ref, rc, fc, fs)))
        for first, n in ((0, 40000), (13001, 16001), (2 ** 32 - 100, 4093), (0, 1)):
            one = dict(prn=ch["prn"][k:k + 1], rc=ch["rc"][k:k + 1], fc=ch["fc"][k:k + 1], cp_ref=ch["cp_ref"][k:k + 1])
            b0 = syn_ref.n_bits_needed(2.5e6, first, one)[0] - 1
            b1 = syn_ref.n_bits_needed(2.5e6, first + n - 1, one)[0] - 1
            out.append(("bits %d %d %s %s %s %d" % (first, n, h(2.5e6), h(rc), h(fc), int(ch["cp_ref"][k])), "1 %d %d" % (b0, b1)))
    out.append(("bits 0 1000 %s %s %s 0" % (h(1.0), h(0.0), h(1e16)), "0 0 0"))         # the code phase leaves the exact range
    for at, S, want in ((1, 100, 1), (99, 100, 99), (0, 100, 0x7fffffff), (100, 100, 0x7fffffff), (-5, 100, 0x7fffffff), (2 ** 40, 100, 0x7fffffff)):
        out.append(("chan %s %s %d %d %d %d" % (h(1.5), h(1.023e6), 1013, 37, at, S), "%d 13 36" % want))
    out.append(("chan %s %s %d %d %d %d" % (h(1.5), h(1.023e6), -7, 1, 0, 0), "%d 13 0" % 0x7fffffff))   # floor modulus of cpReference
    return out


def test_plan_properties_and_mappings(tmp_path):
    if _cxx() is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "test_syn_plan")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", SRC, "-o", exe], check=True)
    cases = _cases()
    path = tmp_path / "cases.txt"
    path.write_text("".join(line + "\n" for line, _ in cases))
    p = subprocess.run([exe, str(path)], check=True, stdout=subprocess.PIPE, text=True)     # (exit 1: a property failed, message on stderr)
    got = p.stdout.splitlines()
    assert len(got) == len(cases) > 500
    for (line, want), have in zip(cases, got):
        if line.startswith("t"):
            assert float.fromhex(have) == float.fromhex(want), line
        else:
            assert have == want, line
