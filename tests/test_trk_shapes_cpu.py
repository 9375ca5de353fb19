"""CPU: the inputs of tests/test_gpu_trk_shapes.py (tests/trk_shapes.py), checked with the fp64 reference tests/trk_ref.py alone --
that the window shapes leave 16-byte alignment and end in a partial quad, that the reference visits the boundary cases the shapes
were chosen for, that no sign is decided on less than 1 % of the median prompt magnitude (so the GPU test's allowance for such
signs is never used), that the teacher-forced rows sit where they claim to (the exact-boundary pair, the fourth branch) and that
none of them asks which chip a sample exactly on a chip edge belongs to.

Measured (fp64 numpy on x86-64): case 0 in 80 of 160 windows at T = 0.5 ms, case 2 in 40 of 80 at T = 1.5 ms, case 1 everywhere
else; smallest |Re p_s| / median prompt 0.137 (T = 1.5 ms, PRN 27); smallest distance of a sample's tap from a chip edge over
the teacher-forced rows 1.8e-7 chip."""
import numpy as np
import pytest

from tests import trk_ref, trk_shapes as ts


@pytest.mark.parametrize("shape", ts.SHAPES, ids=ts.SHAPE_IDS)
def test_shapes_cases_and_sign_margins(shape):
    fs, T, M, ds = shape
    r, x = ts.record(*shape), ts.reference(*shape)
    S = r["S"]
    assert S == int(round(T * fs)) and S <= 3750 and M <= 160 and r["iq"].size == 2 * (M + 1) * S
    if ds > 0:
        assert S % 4 != 0 and (4 * S) % 16 != 0          # odd windows off the 16-byte boundary, a partial quad at every window's end
    else:
        assert (fs, T) == (2.5e6, 1e-3)                  # ds = -1 runs at the shape the other tests use
    case = x["case"]
    assert case.shape == (M, 2) and (case >= 0).all()    # the fourth branch nowhere
    print("%s: windows per case %s" % (ts.SHAPE_IDS[ts.SHAPES.index(shape)], {c: int((case == c).sum(axis=0).min()) for c in (0, 1, 2)}))
    if T == 0.5e-3:
        assert ((case == 0).sum(axis=0) >= M / 3).all()  # a boundary-less window every second time: p_a is carried
    if T == 1.5e-3:
        assert ((case == 2).sum(axis=0) >= M / 3).all()  # two boundaries, two signs, three non-empty segments
    margin = ts.sign_margin(x)
    print("smallest |Re p_s| / median prompt per channel: %s" % ["%.3f" % v for v in margin])
    assert min(margin) > 0.01
    for k in range(2):
        assert x["signs"][k].size == x["ref"]["cp"][M, k] == case[:, k].sum() and set(x["signs"][k]) <= {-1.0, 1.0}
    # the start is off the truth, and the ds = -1 record really has the code Doppler the other way round
    assert np.array_equal(np.sign(r["truth"]["fc"] - trk_ref.F_CA), ds * np.sign(ts.FI))
    assert np.array_equal(np.sign(r["start"][:, 2] - trk_ref.F_CA), ds * np.sign(ts.FI))


def test_ds_changes_the_reference():
    """ds is not a no-op in the reference the GPU test compares with: on the ds = -1 record the ds = +1 loop ends elsewhere."""
    fs, T, M, ds = ts.SHAPES[3]
    r, x = ts.record(fs, T, M, ds), ts.reference(fs, T, M, ds)
    other = trk_ref.track(r["iq"], fs, T, ts.PRNS, r["start"], M, ds=1.0)[0]
    assert np.abs(other["fc"][M] - x["ref"]["fc"][M]).min() > 1e-3 and not np.array_equal(other["fc_bias"], x["ref"]["fc_bias"])


def test_ring_record():
    """The ring tests' record: one sign per window, so that after 100 windows the 50 newest signs fill the ring of a 24-window
    tracker from its first slot (no wrap inside the range) and after 7 more they wrap."""
    fs, T, M, ds = ts.RING_SHAPE
    x = ts.reference(fs, T, M, ds, extra=ts.RING_EXTRA + 1)
    assert (x["case"] == 1).all() and all(s.size == M + ts.RING_EXTRA for s in x["signs"])
    assert M % 50 == 0 and 3 <= (M + ts.RING_EXTRA) % 50 <= 47


@pytest.mark.parametrize("fs,T", [(2.5e6, 1e-3), (2.5e6, 0.5e-3)], ids=["S2500", "S1250"])
def test_edge_rows(fs, T):
    S = int(round(T * fs))
    p, clean = ts.edge_params(fs, T)
    r = ts.record(fs, T, ts.N_EDGE, 1.0)
    o = ts.correlate_ref(r["iq"], fs, S, p)
    row = ts.EDGE_ROWS.index
    assert p.shape == (ts.N_EDGE, 2, 4) and r["iq"].size >= 2 * S * ts.N_EDGE
    # the exact-boundary pair: neighbouring doubles, idxs1 = S (case 1, empty last segment) against S + 1 (case 0)
    a, b = p[row("idxs1=S"), :, 0], p[row("idxs1=S+1"), :, 0]
    assert (np.nextafter(b, a) == a).all() and (0.0 < b).all() and (a < 1023.0).all()
    assert (o["idxs1"][row("idxs1=S")] == S).all() and (o["case"][row("idxs1=S")] == 1).all()
    assert (o["idxs1"][row("idxs1=S+1")] == S + 1).all() and (o["case"][row("idxs1=S+1")] == 0).all()
    assert (o["seg"][row("idxs1=S"), :, 1:] == 0).all()
    # the ends of the code phase
    assert (p[row("rc=0"), :, 0] == 0.0).all() and (p[row("rc=1023"), :, 0] == 1023.0).all()
    assert (p[row("rc=1023-1e-9"), :, 0] < 1023.0).all() and (1023.0 - p[row("rc=1023-1e-9"), :, 0] < 2e-9).all()
    assert (o["idxs1"][row("rc=1023")] == 1).all() and (o["idxs1"][row("rc=1023-1e-9")] == 1).all()
    # the fourth branch: negative fc in the reference itself; NaN has no reference
    assert o["case"][row("fc<0"), 1] == -1 and o["case"][row("fc<0"), 0] >= 0
    assert np.isnan(p[row("fc=nan"), 0, 2]) and o["case"][row("fc=nan"), 1] >= 0
    bad = np.zeros((ts.N_EDGE, 2), dtype=bool)
    bad[row("fc<0"), 1] = bad[row("fc=nan"), 0] = True
    assert np.array_equal(o["case"] < 0, bad) and np.array_equal(clean != p, np.broadcast_to(bad[:, :, None] & (np.arange(4) == 2), p.shape))
    assert (ts.correlate_ref(r["iq"], fs, S, clean)["case"] >= 0).all()
    print("S = %d: cases per row %s" % (S, o["case"].tolist()))
    assert {0, 1} <= set(o["case"][~bad]) and (S != 2500 or 2 in o["case"])
    # the rows are what they say: the signal is there at the truth and gone 10 kHz away
    peak = np.abs(o["epl"][:, :, 1]).max(axis=0)
    assert (np.abs(o["epl"][row("truth"), :, 1]) > 0.5 * peak).all() and (np.abs(o["epl"][row("fi=+10k"), :, 1]) < 0.3 * peak).all()
    # no sample of any row lies on a chip edge of any tap (sample 0 of the rc = 0 / 1023 rows apart, where both sides hold rc
    # exactly): the device's fixed-point code phase is good to S 2^-53 + 2^-42 < 1e-12 chip, the reference's fp64 to 2e-13
    tie = min(ts.tie_margin(fs, S, p[m, k, 0], p[m, k, 2]) for m in range(ts.N_EDGE) for k in range(2) if not bad[m, k])
    print("S = %d: smallest distance of a tap from a chip edge %.2e chip" % (S, tie))
    assert tie > 1e-9
