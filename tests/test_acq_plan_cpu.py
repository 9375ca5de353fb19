"""The acquisition search's plan (csrc/dpe_acq_plan.h) without a GPU: host/test_acq_plan.cpp, built with the host compiler, must give
for every row of tests/golden/acq_plan_parent.json the create-time shape and the launch list that the library chose for that row when
both were still spread over dpe_acq_create and dpe_acq_search (recorded at create on an MI355X from the commit before the header
existed: per row the configuration, the switches, the device's answers -- and the shape and every launch of one search).  Rows the
device at hand cannot give (an LDS opt-in refused, 32 and 6 compute units) are written from the same expressions by hand and marked
"derived".  Every field of every row is compared for equality; nothing is left out."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import acq_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "acq_plan_parent.json")
SRC = os.path.join(ROOT, "navlab-dpe-sdr_amd", "host", "test_acq_plan.cpp")
CORR = {"rocfft-chain", "fused-2500", "fused-mixed", "alias-packed", "alias-radix10-2500", "alias-radix10-mixed"}
FWD = {"wipe+rocfft", "wipe-fold+rocfft", "acq_wipe_fft2500_kernel", "acq_fwd25k_pack_kernel"}
KERNELS = {"acq_wipe_kernel", "acq_wipe_fold_kernel", "acq_wipe_fft2500_kernel", "acq_fwd25k_pack_kernel", "rocfft forward",
           "acq_corr2500_kernel<false>", "acq_corr_mixed_kernel<4000, 10, 8, 5, false>", "acq_corr_mixed_kernel<5000, 10, 10, 5, false>",
           "acq_decimate10_kernel", "acq_corr25k_pack_kernel", "acq_radix10_kernel", "acq_corr2500_kernel<true>",
           "acq_corr_mixed_kernel<4000, 10, 8, 5, true>", "acq_corr_mixed_kernel<5000, 10, 10, 5, true>", "acq_mul_kernel", "rocfft inverse",
           "acq_fold_kernel", "acq_stats_small_kernel", "acq_stats_kernel"}
MODES = {"coherent": 0, "noncoherent": 1, "textbook": 2}


def _cxx():
    for c in ("g++", "c++", "clang++"):
        if shutil.which(c):
            return shutil.which(c)
    return None


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    if _cxx() is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("acq_plan") / "test_acq_plan")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", SRC, "-o", exe], check=True)
    p = subprocess.run([exe, TABLE], check=True, stdout=subprocess.PIPE, text=True)
    with open(TABLE) as f:
        table = json.load(f)
    return table, [json.loads(line) for line in p.stdout.splitlines()]


def test_every_row_gives_the_recorded_shape_and_launches(plans):
    table, got = plans
    assert len(table) == len(got)
    kinds = {True: 0, False: 0}
    for want, have in zip(table, got):
        assert have["name"] == want["name"]
        assert have["shape"] == want["shape"], want["name"]
        assert have["launches"] == want["launches"], want["name"]
        assert have["createOk"] == want["createOk"], want["name"]
        kinds[bool(want.get("derived", False))] += 1
    print("rows recorded on the device: %d, derived by hand: %d" % (kinds[False], kinds[True]))
    assert kinds[False] >= 100 and kinds[True] >= 4


def test_the_table_reaches_every_form_kernel_and_item_order(plans):
    table, _ = plans
    assert {t["shape"]["corr"] for t in table} == CORR
    assert {t["shape"]["fwd"] for t in table} == FWD
    assert {l["kernel"] for t in table for l in t["launches"]} == KERNELS
    assert {l["order"] for t in table for l in t["launches"] if l["kernel"] == "acq_corr25k_pack_kernel"} == {0, 1}
    assert {t["in"]["mode"] for t in table} == {0, 1, 2}
    assert {2500, 4000, 5000, 2000, 12000, 16368} <= {t["shape"]["M"] for t in table}
    assert {10, 1, 5} <= {t["in"]["N"] for t in table}
    for t in table:     # the alias forms are those of ten code periods
        if t["in"]["mode"] == 1 and t["in"]["N"] != 10:
            assert t["shape"]["corr"] == "rocfft-chain", t["name"]
    assert {0, 1, 5, 8, 32} <= {t["in"]["prnChunk"] for t in table if t["in"]["P"] == 32} and 3 in {t["in"]["P"] for t in table}
    # prnChunk = 0 on both sides of the 1 GiB rule of the packed form's stage buffer
    gib = {t["in"]["B"]: t["shape"]["chunk"] for t in table
           if t["in"]["mode"] == 1 and t["in"]["prnChunk"] == 0 and t["in"]["P"] == 32 and t["shape"]["M"] == 2500 and t["in"]["N"] == 10}
    assert gib[125] == 32 and gib[200] == 8
    assert {25, 31, 125} <= {t["in"]["B"] for t in table}
    for sw in ("noFused", "noPack", "noFwdPack"):     # each switch alone
        assert any(t["in"]["sw"][sw] and sum(t["in"]["sw"].values()) == 1 for t in table), sw
    stats = {(t["shape"]["statsSmall"], t["shape"]["rowInLds"]) for t in table}
    assert {(1, 1), (0, 1), (0, 0)} <= stats
    derived = [t for t in table if t.get("derived")]
    assert {t["in"]["dev"]["cus"] for t in derived} >= {32, 6}
    assert any(t["in"]["dev"]["cus"] >= 8 and t["in"]["dev"]["cus"] % 8 for t in derived)      # the rounding to whole eights
    assert any(t["in"]["sw"]["noFusedFwd"] for t in derived) and any(t["in"]["sw"]["statsLds"] for t in derived)
    assert any(not t["in"]["dev"]["packLds"] for t in derived) and any(not t["createOk"] for t in derived)


def test_the_gpu_tests_configurations_take_the_forms_their_docstrings_claim(plans):
    table, _ = plans
    by_name = {t["name"]: t for t in table}
    rows = {r["name"]: r for r in acq_rows.ROWS}
    golden = os.path.join(ROOT, "tests", "golden")      # the fixture rows are the fixtures' own shapes
    o8, o9 = np.load(os.path.join(golden, "o8_acquisition.npz")), np.load(os.path.join(golden, "o9_scalar_acquisition.npz"))
    for name, g, bins in (("o8-coherent", o8, o8["bins_coh"]), ("o8-noncoherent", o8, o8["bins_non"]), ("o9-search-signal", o9, o9["bins"])):
        assert (rows[name]["fs"], rows[name]["S"]) == (float(g["fs"]), int(g["S"])) and np.array_equal(acq_rows.bins_of(rows[name]), bins), name
    assert acq_rows.prns_of(rows["o9-search-signal"]) == [int(p) for p in o9["prn_list"]]
    for row in acq_rows.ROWS:
        t = by_name[row["name"]]
        i = t["in"]
        assert (i["S"], i["fs"], i["B"], i["P"], i["mode"], i["prnChunk"]) == \
            (row["S"], row["fs"], row["B"], row["P"], MODES[row["mode"]], row["chunk"]), row["name"]
        assert t["env"] == row.get("env", {}) and not t.get("derived")
        assert (t["shape"]["corr"], t["shape"]["fwd"]) == (row["corr"], row["fwd"]), row["name"]
        launched = {l["kernel"] for l in t["launches"]}
        assert set(row["kernels"]) <= launched, row["name"]
        want = {"registers": (1, 1), "lds": (0, 1), "memory": (0, 0)}[row["stats"]]
        assert (t["shape"]["statsSmall"], t["shape"]["rowInLds"]) == want, row["name"]
