"""GPU: vt_filter_kernel (csrc/dpe_vt.hip, body vt_filter_epoch of csrc/dpe_vt_dev.h) one epoch at a time, through every branch it
has.  Teacher-forced: before each epoch the whole device state is read (VectorTracker.state_rec), the device runs that one epoch, and
tests/vt_ref.py repeats it from the device's own before-state on the device's own sums -- so a deviation is that epoch's and the
filter's alone, and the bound can sit at the level of a maths library's last bits instead of the closed loop's fp32 yardstick
(tests/test_gpu_vt.py).  Classes, bounds and worlds: tests/vt_cases.py; that the worlds show what they are built for and that the
bounds are attainable: tests/test_vt_filter_worlds_cpu.py.  The exact class is held against the host form too (one source, two
forms: DESIGN.md 7e)."""
import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import vt_cases, vt_ref

pytestmark = pytest.mark.gpu
VT = dpe.engine.VectorTracker


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return dpe.engine.lib()


def to_dev(iq):
    import torch
    return torch.from_numpy(iq).to("cuda:0")


def make_vt(c, log_capacity):
    cfg, s = c["cfg"], c["w"]["start"]
    vt = dpe.VectorTracker(cfg.fs, cfg.prns, T=cfg.T, N=cfg.N, num_prev=cfg.num_prev, log_capacity_epochs=log_capacity)
    vt.set_ephemerides(s["eph"], s["tow"], s["cps"])
    vt.init(c["X0"], c["Sigma0"], s["rxTime0"], c["chan"])
    return vt


def clone(rec):
    return dpe.engine.VtStateRec.from_buffer_copy(rec)


def step_through(c, oracle, capsys):
    """The case on the device, epoch by epoch, each held by vt_cases.check_epoch and against the host form.  -> per epoch (state
    before, sums, log record, state after) and the device's sticky status."""
    cfg, s = c["cfg"], c["w"]["start"]
    ccfg = VT.config(cfg.fs, cfg.prns, T=cfg.T, N=cfg.N, num_prev=cfg.num_prev)
    iq_d = to_dev(c["iq"])
    per = 2 * cfg.N * cfg.S
    vt = make_vt(c, c["n_epochs"])
    lines, steps, worst = [], [], {}
    try:
        for e in range(c["n_epochs"]):
            b = vt.state_rec()
            vt.track(iq_d[e * per:(e + 1) * per], 1)
            sums, row, a = vt.read_corr(), vt.read_log_rows(e, 1)[0], vt.state_rec()
            got = {k: v[0] for k, v in VT.unpack_log(row[None, :], cfg.K).items()}
            before, after = vt_ref.state_from_rec(cfg, b), vt_ref.state_from_rec(cfg, a)
            assert b.satValid == (1 if e else 0) and a.satValid == 1
            out = vt_cases.check_epoch(c, oracle, e, before, sums, got, after, raw_row=row, lines=lines)
            for n, (d, bound) in out.items():
                if d > 0.0 and d / bound >= worst.get(n, (0.0,))[0]:
                    worst[n] = (d / bound, d, bound, e)
            h = clone(b)                                                                           # one source, two forms: the exact class
            host = VT.filter_step_host(ccfg, s["eph"], s["tow"], s["cps"], h, sums)
            for n in vt_cases.EXACT:
                assert vt_cases.same(got[n], host[n]), (c["name"], e, n, got[n], host[n])
            ha = vt_ref.state_from_rec(cfg, h)
            for n in ("epochs", "status", "rxTime0", "histN", "histPos", "histR", "rc", "ri", "cp"):
                assert vt_cases.same(after[n], ha[n]), (c["name"], e, n)
            steps.append((before, sums, got, after))
        status = vt.dev_status()
    finally:
        vt.close()
        with capsys.disabled():
            print("\n%s: device against vt_ref on the device's own before-state and sums" % c["name"])
            print("\n".join(lines))
            print("  worst ratios: %s" % ", ".join("%s %.2f (%.2e / %.2e, epoch %d)" % ((n,) + worst[n]) for n in vt_cases.BOUNDED if n in worst))
    return steps, status


def test_nominal(built, oracle, capsys):
    """Epoch 0 computes its own satellite states; the measured W is in use from epoch 3 on; the history ring wraps."""
    c = vt_cases.case(oracle, "nominal")
    steps, status = step_through(c, oracle, capsys)
    assert status == 0
    for e, (before, _, got, after) in enumerate(steps):
        assert np.all((got["wR"] != c["cfg"].init_var[0]) == (e >= vt_cases.NUM_PREV)) and np.all((got["wV"] != c["cfg"].init_var[1]) == (e >= vt_cases.NUM_PREV))
        assert np.all(after["histPos"] == (e + 1) % vt_cases.NUM_PREV) and np.all(after["histN"] == min(e + 1, vt_cases.NUM_PREV))


def test_sixteen_channels_partly_included(built, oracle, capsys):
    """chanOf off the identity, n = 32, 30, 26, 28, 32: rows of A and S beyond the first 64 elements, with holes."""
    c = vt_cases.case(oracle, "k16_partial")
    steps, status = step_through(c, oracle, capsys)
    assert status == 0 and [2 * int(g["n_incl"]) for _, _, g, _ in steps] == [32, 30, 26, 28, 32]
    assert [int(g["mask"]) for _, _, g, _ in steps] == c["masks"]


def test_too_few_channels(built, oracle, capsys):
    c = vt_cases.case(oracle, "too_few")
    steps, status = step_through(c, oracle, capsys)
    before, _, got, after = steps[2]
    assert got["mask"] == 0b010101 and got["status"] == VT.NO_UPDATE and got["n_incl"] == 3
    NT = c["cfg"].NT
    assert np.array_equal(got["X"][:4], before["X"][:4] + NT * before["X"][4:]) and np.array_equal(got["X"][4:], before["X"][4:])   # X = F X
    P = 0.5 * (before["Sigma"] + before["Sigma"].T)
    F = np.eye(8)
    F[:4, 4:] = NT * np.eye(4)
    assert np.allclose(after["Sigma"], F @ P @ F.T + np.diag(c["cfg"].q), rtol=1e-14, atol=0.0)                                    # (bit for bit against vt_ref: check_epoch)
    assert [int(g["status"]) for _, _, g, _ in steps] == [0, 0, VT.NO_UPDATE, 0, 0, 0] and [int(g["n_incl"]) for _, _, g, _ in steps[3:]] == [5, 6, 6]
    assert status == VT.NO_UPDATE                                                                   # sticky


@pytest.mark.parametrize("name", ["pivot_first", "pivot_late"])
def test_pivot_not_positive(built, oracle, capsys, name):
    """Sigma = -1e4 I: the first pivot fails.  Sigma = diag(1e4 x 4, 1, 1, 1, -1e3): the range rows factor, the first rate row fails --
    the break between barriers after factored columns."""
    c = vt_cases.case(oracle, name)
    steps, status = step_through(c, oracle, capsys)
    assert status == VT.PIVOT
    for before, _, got, after in steps:
        assert got["status"] == VT.PIVOT and got["n_incl"] == 6
        assert np.array_equal(got["X"][4:], before["X"][4:]) and np.array_equal(got["X"][:4], before["X"][:4] + c["cfg"].NT * before["X"][4:])   # predict only
        assert np.all(np.isfinite(got["X"])) and np.all(np.isfinite(after["Sigma"]))
        assert all(np.all(np.isfinite(got[n])) for n in VT.CHAN_NAMES)


def test_bad_window(built, oracle, capsys):
    """fi = NaN on channel 1: vt_correlate_kernel's own test gives case -1 and zero sums, in every epoch (ri stays NaN)."""
    c = vt_cases.case(oracle, "bad_window")
    steps, status = step_through(c, oracle, capsys)
    assert status == VT.BAD_WINDOW
    others = [0, 2, 3, 4, 5]
    for _, sums, got, after in steps:
        assert np.all(sums[:, 1, 6] == -1.0) and np.all(sums[:, 1, :6] == 0.0)
        assert got["mask"] == 0b111101 and got["status"] == VT.BAD_WINDOW and got["n_incl"] == 5
        assert all(np.all(np.isfinite(got[n][others])) for n in VT.CHAN_NAMES)
        assert np.all(np.isfinite(got["X"])) and np.all(np.isfinite(after["Sigma"]))


def test_bad_window_and_too_few(built, oracle, capsys):
    c = vt_cases.case(oracle, "bad_and_few")
    steps, status = step_through(c, oracle, capsys)
    assert status == (VT.BAD_WINDOW | VT.NO_UPDATE)
    for _, _, got, _ in steps:
        assert got["mask"] == 0b1110 and got["status"] == (VT.BAD_WINDOW | VT.NO_UPDATE)


def test_epoch_off_the_millisecond_grid(built, oracle, capsys):
    """N T = 3.2 ms: vt_next_rx_time's roundMs = 0 branch; rxTime0 = rxBase + epochs N T in one rounding."""
    c = vt_cases.case(oracle, "off_grid")
    steps, status = step_through(c, oracle, capsys)
    assert status == 0 and not c["cfg"].round_ms
    rx0 = c["w"]["start"]["rxTime0"]
    for e, (_, _, got, _) in enumerate(steps):
        assert got["rxTime0"] == rx0 + float(e + 1) * c["cfg"].NT


def test_log_ring(built, oracle):
    """Capacity 4, track(3) then track(7): slots wrap; a read that crosses the wrap comes in two pieces; what has left is refused."""
    c = vt_cases.case(oracle, "nominal")
    iq_d = to_dev(c["iq"])
    per = 2 * c["cfg"].N * c["cfg"].S
    full = make_vt(c, 10)
    full.track(iq_d, 10)
    want = full.read_log_rows(0, 10)
    full.close()
    vt = make_vt(c, 4)
    try:
        vt.track(iq_d, 3)
        assert np.array_equal(vt.read_log_rows(0, 3).view(np.int64), want[0:3].view(np.int64))
        vt.track(iq_d[3 * per:], 7)
        assert np.array_equal(vt.read_log_rows(6, 4).view(np.int64), want[6:10].view(np.int64))
        assert np.array_equal(vt.read_log_rows(7, 3).view(np.int64), want[7:10].view(np.int64))   # slots 3, 0, 1
        got = vt.read_log(7, 3)
        assert np.array_equal(got["X"], want[7:10, 0:8])
        with pytest.raises(dpe.engine.DpeError, match="has left the log"):
            vt.read_log(5, 1)
        with pytest.raises(dpe.engine.DpeError, match="have not been tracked"):
            vt.read_log(8, 3)
    finally:
        vt.close()
