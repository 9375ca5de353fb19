"""GPU: pipeline.run_monte_carlo -- realisations made by the device synthesiser, one stage-1 and one manifold update over the batch --
gives for every realisation of tests/mc_world.py the arg-max the oracle gives on the numpy restatement's samples, and the same result
when called twice."""
import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import helpers, mc_world

pytestmark = pytest.mark.gpu


def _run():
    ho = dpe.handoff.read_handoff(helpers.HANDOFF)
    return dpe.pipeline.run_monte_carlo(ho, mc_world.FS, mc_world.S, mc_world.K, mc_world.POS, mc_world.VEL, mc_world.LEVELS, mc_world.N_REAL,
                                        mc_world.SEED, init_delta=mc_world.init_delta(), sigma=mc_world.SIGMA, weighted_mean=True,
                                        lag_half_width=mc_world.L, bin_half_width=mc_world.B), ho


def test_monte_carlo_matches_the_oracle_and_repeats():
    import __graft_entry__ as ge
    ge.build()
    (a, ho), (b, _) = _run(), _run()
    ref = mc_world.oracle_run()
    assert len(a) == len(ref) == 2
    for ra, rb, rr in zip(a, b, ref):
        assert ra["cn0_dbhz"] == rr["cn0"]
        assert np.array_equal(ra["pos_index"], rr["pos_index"]) and np.array_equal(ra["vel_index"], rr["vel_index"]), rr["cn0"]
        assert not ra["pos_out_of_window"].any() and not ra["vel_out_of_window"].any()
        assert np.abs(ra["fixes"] - rr["fixes"]).max() < 1e-6                       # the same grid points give the same fixes
        assert abs(ra["rmse_3d"] - rr["rmse_3d"]) < 1e-6 * max(1.0, rr["rmse_3d"])
        for k in ("fixes", "pos_index", "vel_index", "rmse_enu"):
            assert np.array_equal(ra[k], rb[k]), k
        assert ra["rmse_3d"] == rb["rmse_3d"]
        assert np.abs(ra["mean_fixes"] - rb["mean_fixes"]).max() < 1e-6             # (sums over the grid: their order may differ)
        assert abs(np.sqrt(np.sum(ra["rmse_enu"] ** 2)) - ra["rmse_3d"]) < 1e-9 * max(1.0, ra["rmse_3d"])
        assert abs(dpe.synth.amp_to_cn0(ra["amp"], mc_world.SIGMA, mc_world.FS) - ra["cn0_dbhz"]) < 1e-9
    assert a[1]["rmse_3d"] > a[0]["rmse_3d"] and a[0]["rmse_vel"] < 1e-6
    assert np.isfinite(a[0]["mean_fixes"]).all() and a[0]["mean_rmse_3d"] > 0
