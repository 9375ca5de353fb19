"""Every path through stage 1's launches (bcs_launch, csrc/dpe_bcs.hip) at the smallest shape that reaches it (tests/stage1_rows.py):
the kernel the plan names is the one that ran, and its banks are the fp64 oracle's (batchcorrscores.cu:1043-1180 semantics) to 2e-6
of the bank's peak, nav-bit decisions and DC mean exact -- the standard of tests/test_gpu_chip.py and tests/test_gpu_parity.py.
The hinted device-parameter call and its guarded re-run are held the same way by
tests/test_gpu_chip.py::test_device_ports_at_a_high_sampling_rate_take_the_chip_kernel."""
import numpy as np
import pytest

from tests import stage1_rows

pytestmark = pytest.mark.gpu
TOL = 2e-6


@pytest.mark.parametrize("row", stage1_rows.ROWS, ids=[r["name"] for r in stage1_rows.ROWS])
def test_form_is_selected_and_its_banks_are_the_oracles(row):
    from oracle import oracle as o
    case = stage1_rows.case_of(row)
    code, carr, info, kernel = stage1_rows.run_row(row, case)
    assert kernel == row["kernel"]
    L, B = row["L"], row["B"]
    worst = 0.0
    for wi, w in enumerate(case["wins"]):
        s = w["start"]
        for k in range(row["K"]):
            c, f, inf = o.bcs_sv(w["iq"], case["fs"], int(s["prn"][k]), s["rc"][k], s["ri"][k], s["fc"][k], s["fi"][k],
                                 int(s["cp"][k]), int(s["cp_ref"][k]), -L, L, -B, B, case["C"])
            for name, got, ref in (("code", code[wi][k], c), ("carr", carr[wi][k], f)):
                err = np.abs(got - ref).max() / np.abs(ref).max()
                worst = max(worst, err)
                assert err < TOL, "%s window %d SV %d: rel err %.3g" % (name, wi, k, err)
            assert info[0][wi, k] == inf["idx_next"] and bool(info[1][wi, k]) == inf["no_flip_larger"]
        assert info[2][wi] == inf["mean"]
    print("%s: %s, worst rel err %.3g" % (row["name"], kernel, worst))
