"""The filter inside the measurement kernel (ekf_dev_step / ekf_lu_column, csrc/dpe_ekf_dev.h) against the host filter
(csrc/dpe_ekf.hip) with the LU inverse OFF the diagonal-pivot path.  P_k|k-1 starts as I in both forms and every run of the suite
keeps S = P + I diagonally dominant, so p == C in every column of every window: the row-swap half of ekf_lu_column -- the shuffle
sources, the pivot permutation, diagOld, ownOdd / ownEven, the unsigned-magnitude pivot search -- and the singular exit never ran.
Here P_k|k-1 is loaded into both forms before a window (dpe_chm_dev_ekf_load / dpe_ekf_load), the host filter is fed the measurement
the device formed (its zVal port), and x_k|k, x_k+1|k, P_k|k, P_k+1|k, K and Q are required to be equal BIT FOR BIT
(dpe_chm_dev_ekf_state / dpe_ekf_state).  The loads and what each reaches: tests/chm_world.py::filter_case, proven by the numpy copy of
the pivot rule in tests/test_chm_world_cpu.py.  Small attached loop: S = 8192, K = 6, 5^4 uniform grids."""
import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import chm_world as cw

pytestmark = pytest.mark.gpu

FS, S, K, W = 2.5e6, 8192, 6, 20


@pytest.fixture(scope="module")
def windows():
    iq, _, _, _ = dpe.workload.build_windows(W, FS, S, K, seed=11, amp=200.0, velocity=np.array([4.0, -3.0, 2.0]))
    return np.ascontiguousarray(iq)


class Loop:
    def __init__(self, iq, couple):
        import torch
        ho = dpe.handoff.read_handoff(dpe.workload.HANDOFF_CSV)
        g = dpe.synth.uniform_grid(5, 1.0)
        L, B = dpe.pipeline.bank_half_widths(g, g, FS, dpe.engine.carr_fft_len(S))
        self.bcs = dpe.engine.BatchCorrScores(FS, samples_per_window=S, lag_half_width=L, bin_half_width=B, max_channels=K)
        self.bcs.Start()
        self.bcm = dpe.engine.BatchCorrManifold(FS, S, self.bcs.NumFFTPoints, g, g, LPower=1, lag_half_width=L, bin_half_width=B, max_channels=K)
        self.bcm.Start()
        self.cm = dpe.engine.ChanMgrDev.from_handoff(ho, S / FS, K, (0.0,))
        self.cm.attach(self.bcs, self.bcm, 32)
        x = np.array(ho["X_ECEF"], dtype=np.float64).copy()
        with pytest.raises(dpe.DpeError, match="ekf_load: no filter"):        # refused before set_ekf
            self.cm.ekf_load(None, np.eye(8))
        self.cm.set_ekf(S / FS, x, couple_velocity=couple)
        self.host = dpe.engine.cuEKF(x, SampleLength=S / FS, EnableEKF=True, couple_velocity=couple)
        self.z_dev = self.cm.ports()[5]
        self.xk_dev = self.cm.ports()[4]
        self.iq_d = torch.from_numpy(iq).to("cuda:0")
        self.cm.Start(x)
        self.w = 0

    def step(self):
        """One window of the device loop: -> (fix record, the measurement the filter consumed)."""
        self.bcs.UpdatePrepared(self.iq_d[self.w], K)
        self.bcm.UpdatePrepared(self.bcs.CodeScores, self.bcs.CarrScores, K)
        self.cm.step()
        r = self.cm.fix(self.w)
        self.w += 1
        return r, dpe.engine.d2h(self.z_dev, 64, np.float64)

    def load(self, P):
        self.cm.ekf_load(None, P)
        self.host.load(None, P)

    def assert_equal(self, tag):
        d, h = self.cm.ekf_state(), self.host.state()
        for k in cw.EKF_KEYS:
            assert d[k].tobytes() == h[k].tobytes(), (tag, k, np.abs(d[k] - h[k]).max())

    def nominal(self, tag):
        r, z = self.step()
        self.host.Update(z, np.eye(8))
        assert r["zVal"].tobytes() == self.host.xCurrk1k1.tobytes(), tag
        self.assert_equal(tag)
        return r

    def close(self):
        self.host.Stop(); self.cm.Stop(); self.bcm.Stop(); self.bcs.Stop()


@pytest.mark.parametrize("couple", [True, False], ids=["coupled", "uncoupled"])
@pytest.mark.parametrize("name", ["swaps", "tie", "negative"])
def test_loaded_covariance_takes_the_inverse_off_the_diagonal(windows, name, couple):
    """Two nominal windows, then P_k|k-1 = the case's matrix in both forms, a window, and two more nominal ones: every member of the
    filter bit-equal after each.  `swaps`: row swaps in >= 4 columns, columns 0 and 6 among them, p = 7 and p = C + 1; `tie`: the
    first of two candidates of equal magnitude and opposite sign; `negative`: negative pivots chosen over smaller positive candidates."""
    lp = Loop(windows, couple)
    for i in range(2):
        assert lp.nominal(("before", i))["status"] == 0
    lp.load(cw.filter_case(name))
    assert lp.cm.ekf_state()["Pkk1"].tobytes() == cw.filter_case(name).tobytes()
    r = lp.nominal("loaded")
    assert not r["status"] & 32 and np.isfinite(r["zVal"]).all()
    for i in range(2):
        assert not lp.nominal(("after", i))["status"] & 32
    lp.close()


@pytest.mark.parametrize("couple", [True, False], ids=["coupled", "uncoupled"])
@pytest.mark.parametrize("name", ["singular0", "singular5"])
def test_singular_s_holds_the_state_and_is_flagged(windows, name, couple):
    """S with column 0, respectively column 5 after five clean eliminations, zero at and below the diagonal: ekf_lu_column<C> returns
    false.  The window's fix carries bit 32 and its zVal and both state ports are x_k|k-1; no member of the filter changes; the host
    filter's StepUpdate refuses the same S.  The next window, after a fresh SPD load into both, is bit-equal again, and bit 32 stays."""
    lp = Loop(windows, couple)
    assert lp.nominal("before")["status"] == 0
    lp.load(cw.filter_case(name))
    before = lp.cm.ekf_state()
    xk_port = dpe.engine.d2h(lp.xk_dev, 64, np.float64)
    assert xk_port.tobytes() == before["xkk1"].tobytes()
    r, z = lp.step()
    assert r["status"] & 32 and not r["status"] & 4, r["status"]
    assert r["zVal"].tobytes() == xk_port.tobytes()
    s, e, win = lp.cm.outputs()
    assert win["xCurrkk1"][0].tobytes() == xk_port.tobytes()
    after = lp.cm.ekf_state()
    for k in cw.EKF_KEYS:
        assert after[k].tobytes() == before[k].tobytes(), k
    with pytest.raises(dpe.DpeError, match="S inversion failed"):
        lp.host.step_update(z, np.eye(8))
    lp.assert_equal("held")
    lp.load(cw.filter_case("fresh"))
    for i in range(2):
        r = lp.nominal(("after", i))
        assert r["status"] & 32 and not r["status"] & 4, r["status"]
    lp.close()


@pytest.mark.parametrize("couple", [True, False], ids=["coupled", "uncoupled"])
def test_nominal_run_is_bit_equal_in_every_member(windows, couple):
    """No load, 20 windows: the full matrices -- P_k|k, P_k+1|k, K, Q -- and both states, not only x_k|k, bit-equal in every window."""
    lp = Loop(windows, couple)
    for w in range(W):
        assert lp.nominal(w)["status"] == 0
    lp.close()
