"""Stage 1's launch plan (csrc/dpe_bcs_plan.h) without a GPU: host/test_bcs_plan.cpp, built with the host compiler, must give for every
row of tests/golden/bcs_plan_parent.json the create-time shape and the plan that the library chose for that row when the plan was
still part of dpe_bcs_update (recorded on an MI355X from the commit before the header existed: per row the configuration, the
switches, the device's CU count and occupancy answers, the call's flags and what the channel values said -- and the plan).  Every
field of every row is compared for equality; nothing is left out."""
import json
import os
import shutil
import subprocess

import pytest

from tests import stage1_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "bcs_plan_parent.json")
SRC = os.path.join(ROOT, "navlab-dpe-sdr_amd", "host", "test_bcs_plan.cpp")


def _cxx():
    for c in ("g++", "c++", "clang++"):
        if shutil.which(c):
            return shutil.which(c)
    return None


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    if _cxx() is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("bcs_plan") / "test_bcs_plan")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", SRC, "-o", exe], check=True)
    p = subprocess.run([exe, TABLE], check=True, stdout=subprocess.PIPE, text=True)     # (exit 1: a bcs_chan_facts check failed)
    with open(TABLE) as f:
        table = json.load(f)
    return table, [json.loads(line) for line in p.stdout.splitlines()]


def test_every_row_gives_the_recorded_shape_and_plan(plans):
    table, got = plans
    assert len(table) == len(got) == 142
    for want, have in zip(table, got):
        assert have["name"] == want["name"]
        assert have["shape"] == want["shape"], want["name"]
        assert have["plan"] == want["plan"], want["name"]


def test_the_rerun_behind_a_hinted_launch_is_dense_or_wide(plans):
    table, got = plans
    reruns = [have for want, have in zip(table, got) if want["in"]["rerun"]]
    assert len(reruns) == 3     # hinted, hinted with a broken promise, hinted without the second chip form
    for have in reruns:
        assert have["plan"]["kernel"] in ("bcs_bank_kernel", "bcs_bank_wide_kernel"), have["name"]
        assert not have["plan"]["sumLaunch"] and not have["plan"]["chip"]


def test_the_table_covers_every_form_and_every_gpu_row(plans):
    table, _ = plans
    by_name = {t["name"]: t for t in table}
    for row in stage1_rows.ROWS:       # the rows tests/test_gpu_stage1_forms.py runs: the kernel each expects, checked here first
        t = by_name[row["name"]]
        assert t["plan"]["kernel"] == row["kernel"], row["name"]
        assert (t["in"]["S"], t["in"]["L"], t["in"]["B"], t["in"]["nWindows"], t["in"]["nChan"], t["in"]["fs"]) == \
            (row["S"], row["L"], row["B"], row["W"], row["K"], row["fs"]), row["name"]
        assert t["env"] == row.get("env", {})
    kernels = {t["plan"]["kernel"] for t in table}
    assert kernels == {"bcs_bank_kernel", "bcs_bank_wide_kernel", "bcs_bank16_kernel", "bcs_bank_chip_kernel", "bcs_bank_chip2_kernel",
                       "rocfft full-lag path (bcs_fft_*_kernel)"}
    plans_ = [t["plan"] for t in table if "fuse" in t["plan"]]
    for flag in ("fuse", "coRide", "inl", "upInSum", "useGraph", "ride", "fatFinalize", "sumLaunch"):
        assert {p[flag] for p in plans_} == {0, 1}, flag
    assert {t["shape"]["nMom"] for t in table} == {4, 6} and {t["shape"]["useTable"] for t in table} == {0, 1}
    assert max(p["nSideChunks"] for p in plans_) >= 4 and max(p["nBinBlk"] for p in plans_) > 4
