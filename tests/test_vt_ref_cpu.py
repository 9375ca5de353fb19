"""CPU: the vector-tracking restatement (tests/vt_ref.py) against the physical truth of the synthetic world (tests/vt_world.py).
A filtered loop that cannot beat the single-epoch least squares on its own measurements is wrong: the yardstick is the RMS of
those per-epoch fixes, computed on the same record -- no fixed metre figure."""
import numpy as np
import pytest

from tests import vt_ref, vt_world

N_EPOCHS, N, S = 40, 20, 2500
N_SAMPLES = N_EPOCHS * N * S                    # 0.8 s
OUT_CH, OUT_FIRST, OUT_LEN = 2, 15, 10          # the outage: channel 2 has no signal during epochs 15 .. 24


def outage_profile():
    return {OUT_CH: [(OUT_FIRST * N * S, (OUT_FIRST + OUT_LEN) * N * S, 0.0)]}


def run_world(oracle, profile=None, **kw):
    w = vt_world.build(oracle, N_SAMPLES)
    iq = vt_world.record(w, profile=profile)
    cfg = vt_ref.Config(vt_world.FS, w["start"]["prns"])
    out = vt_ref.run(iq, cfg, oracle, w["start"], vt_world.perturbed(w), vt_world.sigma0(), N_EPOCHS, **kw)
    return w, iq, cfg, out


def ls_rms(w, out):
    err = out["ls"][:, :3] - w["start"]["X"][:3]
    return float(np.sqrt(np.mean(np.sum(err ** 2, axis=1))))


@pytest.fixture(scope="module")
def nominal(oracle):
    return run_world(oracle, with_ls=True)


@pytest.fixture(scope="module")
def outage(oracle):
    return run_world(oracle, profile=outage_profile())


def test_filter_beats_single_epoch_least_squares(nominal, capsys):
    w, _, cfg, out = nominal
    t = vt_ref.table(out["recs"])
    err = np.linalg.norm(t["X"][:, :3] - w["start"]["X"][:3], axis=1)
    verr = np.linalg.norm(t["X"][:, 4:7] - w["start"]["X"][4:7], axis=1)
    rms = ls_rms(w, out)
    with capsys.disabled():
        print("\nvt_ref on the world: position error %.2f m at epoch 1 -> %.2f m at epoch %d (velocity %.3f m/s); single-epoch LS RMS %.2f m"
              % (err[0], err[-1], N_EPOCHS, verr[-1], rms))
        print("  error by epoch (m): %s" % np.round(err, 2))
    assert np.all(t["status"] == 0)
    assert err[-1] < rms, (err[-1], rms)


def test_lock_gate_on_present_signal(nominal):
    w, _, cfg, out = nominal
    t = vt_ref.table(out["recs"])
    assert np.all(t["mask"] == (1 << cfg.K) - 1), t["mask"]          # present signal at the tests' amplitude: never excluded
    assert np.all(t["lock"] > cfg.lock_thr)


def test_outage_and_return(outage, capsys):
    w, _, cfg, out = outage
    t = vt_ref.table(out["recs"])
    inc = (t["mask"] >> OUT_CH) & 1
    with capsys.disabled():
        print("\noutage of channel %d, epochs %d .. %d: included %s" % (OUT_CH, OUT_FIRST, OUT_FIRST + OUT_LEN - 1, "".join(str(int(v)) for v in inc)))
        print("  lock metric %s" % np.round(t["lock"][:, OUT_CH], 1))
        print("  dpc at return %.4f chip" % t["dpc"][OUT_FIRST + OUT_LEN, OUT_CH])
    assert np.all(inc[OUT_FIRST + 1:OUT_FIRST + OUT_LEN] == 0)       # excluded in every outage epoch, except possibly the first
    assert np.all(inc[OUT_FIRST + OUT_LEN + 1:] == 1)                # included again from the second epoch after return
    assert np.all(inc[:OUT_FIRST] == 1)
    others = t["mask"] | (1 << OUT_CH)
    assert np.all(others == (1 << cfg.K) - 1)                        # nobody else is ever excluded
    assert abs(t["dpc"][OUT_FIRST + OUT_LEN, OUT_CH]) < 0.25
    assert np.all(t["status"] == 0)
