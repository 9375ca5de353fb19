"""CPU: the Monte-Carlo world of tests/mc_world.py through the oracle alone -- the realisations come from the numpy restatement of the
synthesiser (tests/syn_ref.py), the scores and fixes from oracle/.  What the GPU test then holds pipeline.run_monte_carlo to is
proven meaningful here: at the high C/N0 level every ML fix is the grid point nearest the truth (which is not the grid's centre), at
the low level the 3-D RMSE is strictly larger, and no realisation's peak can lie outside the banks (no pair of any grid point does)."""
import numpy as np

import navlab_dpe_sdr_amd as dpe
from tests import helpers, mc_world


def test_the_truth_is_a_grid_point_away_from_the_centre():
    off = -np.asarray(mc_world.CENTRE_OFFSET)
    d = np.linalg.norm(mc_world.POS - off[None, :], axis=1)
    assert int(np.argmin(d)) == mc_world.true_index() and d.min() < 1e-9
    assert np.linalg.norm(mc_world.POS[mc_world.true_index()]) > 60.0            # beyond half a sample (60 m at 2.5 Msps) from the centre
    ho = dpe.handoff.read_handoff(helpers.HANDOFF)
    from oracle import oracle as o
    R0 = o.enu2ecef(o.ecef2ll(ho["X_ECEF"])).reshape(3, 3)
    assert np.allclose(R0.T @ mc_world.init_delta()[:3], mc_world.CENTRE_OFFSET[:3], atol=1e-9)


def test_high_level_fixes_are_the_nearest_grid_point_and_the_low_level_is_worse():
    hi, lo = mc_world.oracle_run()
    assert hi["cn0"] > lo["cn0"] + 20
    assert (hi["pos_index"] == mc_world.true_index()).all()
    centre_vel = int(np.argmin(np.linalg.norm(mc_world.VEL, axis=1)))
    assert (hi["vel_index"] == centre_vel).all()
    ho = dpe.handoff.read_handoff(helpers.HANDOFF)
    assert np.abs(hi["fixes"][:, :3] - ho["X_ECEF"][None, :3]).max() < 0.01       # the fix is the truth to the manifold's second-order term
    assert lo["rmse_3d"] > hi["rmse_3d"] and lo["rmse_3d"] > 10.0
    assert len(set(lo["pos_index"].tolist())) > 4                                  # the low level really wanders
    assert not hi["oob"].any() and not lo["oob"].any()
    # the arg-max of every realisation is clear of fp32 rounding (2e-5 of the peak, tests/test_gpu_parity.py): the seed was chosen on
    # the CPU for this margin among eight tried
    assert hi["margin"].min() > 1e-3 and lo["margin"].min() > 1e-4
