"""The orbit arithmetic (csrc/dpe_sat.h) and the channel manager's arithmetic (csrc/dpe_chm_arith.h) as plain C++, without a GPU
and without a HIP header: host/test_sat_headers.cpp is built three times with the host compiler -- dpe_sat.h alone, dpe_chm_arith.h
alone, and dpe_cd_plan.h followed by the two (whatever order a unit includes them in, it gets the same functions) -- and evaluates
sat_state, sat_state_t with ModFloor, rotate_state and propagate on channel 0 of the handoff that tests/chm_world.py builds its
worlds from.  The three forms print the same doubles, string for string, and those are the doubles of
tests/golden/sat_headers_parent.txt: the same calls on the same arguments, compiled with the same flags against the single header
(dpe_chm_dev.h, with the HIP headers it then needed) that held this arithmetic before it was split.  No tolerance is involved."""
import os
import shutil
import subprocess

import pytest

from tests import chm_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "navlab-dpe-sdr_amd", "host", "test_sat_headers.cpp")
PARENT = os.path.join(ROOT, "tests", "golden", "sat_headers_parent.txt")
FORMS = {1: "dpe_sat.h", 2: "dpe_chm_arith.h", 3: "dpe_cd_plan.h, dpe_sat.h, dpe_chm_arith.h"}


def _cxx():
    for c in ("g++", "c++", "clang++"):
        if shutil.which(c):
            return shutil.which(c)
    return None


def arguments():
    """Channel 0 of the handoff: its ephemeris at its own transmit time, a time of flight of 70 ms, and the measurement update
    from a fix 30 m and 0.2 m/s off the handoff's."""
    ho = chm_world.base_handoff()
    tx = float(ho["TOW"][0]) + (int(ho["cp"][0]) - int(ho["cp_timestamp"][0])) * 1e-3 + float(ho["rc"][0]) / chm_world.FCA
    x = ho["X_ECEF"].astype(float).copy()
    x[:3] += (30.0, -20.0, 10.0)
    x[4:7] += (0.2, -0.1, 0.05)
    vals = [float(v) for v in ho["eph"][0]] + [tx, 0.07]
    vals += [float(ho["cp"][0]), float(ho["cp_timestamp"][0]), float(ho["TOW"][0]), float(ho["rc"][0]), float(ho["ri"][0]),
             float(ho["fc"][0]), float(ho["fi"][0])]
    vals += [float(v) for v in x] + [float(ho["rxTime"]), 0.02, 1.0]
    assert len(vals) == 41
    return [float.hex(v) for v in vals]


def test_split_headers_build_alone_and_print_the_parents_doubles(tmp_path):
    if _cxx() is None:
        pytest.skip("no host C++ compiler")
    out = {}
    for form in FORMS:
        exe = str(tmp_path / ("test_sat_headers_%d" % form))
        subprocess.run([_cxx(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-DSAT_HEADERS=%d" % form,
                        "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe], check=True)
        out[form] = subprocess.run([exe] + arguments(), check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    for form in FORMS:
        print(FORMS[form] + ":\n  " + "\n  ".join(out[form]))
    with open(PARENT) as f:
        parent = f.read().splitlines()
    assert [line.split()[0] for line in parent] == ["sat_state", "sat_state_floor", "rotate_state", "propagate"]
    assert parent[3].split()[1] == "0"                                   # propagate's status: both Kepler solves converged
    assert parent[0] != parent[1]                                        # (np.mod and fmod do differ on this ephemeris: the lines are not copies)
    assert out[2] == out[3]
    assert out[1] == out[2][:3] and len(out[2]) == 4
    assert out[2] == parent
