"""Shared by tests/test_vt_filter_worlds_cpu.py and tests/test_gpu_vt_filter.py: the worlds that take vt_filter_epoch (csrc/dpe_vt_dev.h)
through every branch it has, and the check of ONE epoch of it -- host or device form -- against tests/vt_ref.py on the same
before-state and the same sums.

Two classes of quantities:
  exact    mask status n_incl rxTime0 cp rc ri wR wV dpc lock eR, the history rings and counters, the sticky status: no operation
           behind them but + - * / floor fmod sqrt, each correctly rounded on both sides, contraction off -- bit for bit;
  bounded  dfi eV X diag fc fi: behind them stand atan2, sin and cos, which differ between maths libraries.  The bound is measured
           from vt_ref alone, per quantity and per epoch, on the same inputs: 4 x the larger of its spread over six row orders (the
           rule of test_vt_host_cpu.compare) and its spread over sixteen runs in which every atan2 / sin / cos result is moved by up to
           2 ulps (vt_ref.Nudge; in an epoch that computes the satellite states of its start, those are moved too, by the bounds
           tests/test_gpu_chm_dev.py holds sat_state to).
The satellite states at steering are given to vt_ref as the form under test computed them (SatStandin), and are held on their own to
the oracle at the same transmit time: fc and fi then test the geometry and the steering, not Kepler's equation."""
import numpy as np

import navlab_dpe_sdr_amd as dpe
from tests import helpers, vt_ref, vt_world

FS, NUM_PREV = vt_world.FS, 3
BAD_WINDOW, NO_UPDATE, PIVOT = vt_ref.BAD_WINDOW, vt_ref.NO_UPDATE, vt_ref.PIVOT
EXACT = ("mask", "status", "n_incl", "rxTime0", "cp", "rc", "ri", "wR", "wV", "dpc", "lock", "eR")
BOUNDED = ("dfi", "eV", "X", "diag", "fc", "fi")
SAT_REL, SAT_CLK = 1e-12, 1e-17                   # of 2.6e7 m and 3e3 m/s; clock terms absolutely (tests/test_gpu_chm_dev.py)
N_ORDERS, N_NUDGES = 6, 16
LOCK_MARGIN = 0.5
NAMES = ("nominal", "k16_partial", "too_few", "pivot_first", "pivot_late", "bad_window", "bad_and_few", "off_grid")
_cache = {}


def _world(oracle, K, T, N, n_epochs, profile=None):
    key = (K, T, N, n_epochs, repr(profile))
    if key not in _cache:
        ho, chans = None, vt_world.CHANS[:K]
        if K > len(vt_world.CHANS):
            ho, chans = vt_world.synthetic_handoff(dpe.handoff.read_handoff(helpers.HANDOFF), K), list(range(K))
        S = int(round(T * FS))
        w = vt_world.build(oracle, n_epochs * N * S, chans=chans, ho=ho)
        _cache[key] = (w, vt_world.record(w, profile=profile))
    return _cache[key]


def case(oracle, name):
    """-> dict(name, w, iq, cfg, X0, Sigma0, chan, n_epochs, masks, status): the world, its record, the loop's start and the included
    masks and status words every epoch must show."""
    K, T, N, n, profile = 6, 1e-3, 20, 6, None
    E = 20 * 2500                                  # samples per epoch at T = 1 ms, N = 20
    full = lambda k: (1 << k) - 1
    if name == "nominal":
        n_rec, masks, status = 10, [full(6)] * 6, [0] * 6                     # (the log-ring test tracks all ten epochs of this record)
    elif name == "k16_partial":
        K, n = 16, 5
        profile = {2: [(E, 4 * E, 0.0)], 9: [(2 * E, 4 * E, 0.0)], 15: [(2 * E, 3 * E, 0.0)]}
        n_rec, masks, status = n, [0xFFFF, 0xFFFB, 0b0111110111111011, 0b1111110111111011, 0xFFFF], [0] * 5
    elif name == "too_few":
        profile = {1: [(2 * E, 4 * E, 0.0)], 3: [(2 * E, 3 * E, 0.0)], 5: [(2 * E, 3 * E, 0.0)]}
        n_rec, masks, status = n, [full(6), full(6), 0b010101, 0b111101, full(6), full(6)], [0, 0, NO_UPDATE, 0, 0, 0]
    elif name in ("pivot_first", "pivot_late"):
        n = 2
        n_rec, masks, status = 10, [full(6)] * 2, [PIVOT] * 2
    elif name == "bad_window":
        n = 3
        n_rec, masks, status = 10, [0b111101] * 3, [BAD_WINDOW] * 3
    elif name == "bad_and_few":
        K, n = 4, 2
        n_rec, masks, status = n, [0b1110] * 2, [BAD_WINDOW | NO_UPDATE] * 2
    elif name == "off_grid":
        T, N, n = 0.8e-3, 4, 10
        n_rec, masks, status = n, [full(6)] * 10, [0] * 10
    else:
        raise KeyError(name)
    w, iq = _world(oracle, K, T, N, n_rec, profile)
    cfg = vt_ref.Config(FS, w["start"]["prns"], T=T, N=N, num_prev=NUM_PREV)
    Sigma0, chan = vt_world.sigma0(), w["start"]["chan"].copy()
    if name == "pivot_first":
        Sigma0 = -1.0e4 * np.eye(8)
    if name == "pivot_late":
        Sigma0 = np.diag([1.0e4, 1.0e4, 1.0e4, 1.0e4, 1.0, 1.0, 1.0, -1.0e3])
    if name == "bad_window":
        chan[1, 3] = np.nan
    if name == "bad_and_few":
        chan[0, 3] = np.nan
    return dict(name=name, w=w, iq=iq, cfg=cfg, X0=vt_world.perturbed(w), Sigma0=Sigma0, chan=chan, n_epochs=n, masks=masks, status=status)


def copy_state(st):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}


def closed_loop(c, oracle, nudge=None):
    """vt_ref's own closed loop on the case.  -> [(state before, sums, record)] per epoch."""
    cfg, s = c["cfg"], c["w"]["start"]
    st = vt_ref.new_state(cfg, c["X0"], c["Sigma0"], s["rxTime0"], c["chan"])
    chips = [dpe.synth.ca_code(p).astype(np.float64) for p in cfg.prns]
    steps = []
    with np.errstate(invalid="ignore"):
        for e in range(c["n_epochs"]):
            sums = vt_ref.correlate_epoch(c["iq"], e * cfg.N * cfg.S, cfg, st, chips)
            before = copy_state(st)
            steps.append((before, sums, vt_ref.filter_step(cfg, oracle, s["eph"], s["tow"], s["cps"], st, sums, nudge=nudge)))
    return steps


class SatStandin:
    """Stands in for the oracle in vt_ref.filter_step: the first n_real calls (an epoch's start states, asked for only while the state
    holds none) go to the real oracle, every later one returns the state the form under test left for that channel."""

    def __init__(self, oracle, eph, after_sat, n_real):
        self.oracle, self.eph, self.after_sat, self.n_real = oracle, np.asarray(eph), np.asarray(after_sat, dtype=np.float64), int(n_real)

    def sat_pos(self, eph_k, tt):
        if self.n_real > 0:
            self.n_real -= 1
            return self.oracle.sat_pos(eph_k, tt)
        k = [i for i in range(self.eph.shape[0]) if np.array_equal(self.eph[i], eph_k)]
        assert len(k) == 1
        return self.after_sat[k[0]].copy(), 0


def deviation(a, b):
    """max |a - b|; NaN against NaN counts as equal, NaN against a number as infinite."""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b)
    d[(a == b) | (np.isnan(a) & np.isnan(b))] = 0.0
    d[np.isnan(d)] = np.inf
    return float(d.max())


def same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def reference(c, oracle, before, sums, after_sat, step=vt_ref.filter_step):
    """vt_ref's epoch from `before` on `sums` with the steering-time satellite states `after_sat`.  -> record, state after, and per
    bounded quantity the bound: 4 x the larger of the spread over row orders and the spread over nudged runs."""
    cfg, s = c["cfg"], c["w"]["start"]

    def run(**kw):
        st = copy_state(before)
        o = SatStandin(oracle, s["eph"], after_sat, cfg.K if before["sat"] is None else 0)
        with np.errstate(invalid="ignore"):
            return step(cfg, o, s["eph"], s["tow"], s["cps"], st, sums, **kw), st

    ref, ref_st = run()
    spread = {n: [0.0, 0.0] for n in BOUNDED}
    rng = np.random.default_rng(7)
    for i in range(N_ORDERS + N_NUDGES):
        alt, _ = run(order=list(rng.permutation(cfg.K))) if i < N_ORDERS else run(nudge=vt_ref.Nudge(1000 + i))
        assert alt["mask"] == ref["mask"] and alt["status"] == ref["status"]
        for n in BOUNDED:
            spread[n][i >= N_ORDERS] = max(spread[n][i >= N_ORDERS], deviation(alt[n], ref[n]))
    return ref, ref_st, {n: 4.0 * max(spread[n]) for n in BOUNDED}


def sat_errors(c, oracle, after):
    """The form's satellite states after an epoch against the oracle at the transmit time of the channel's new NCO state."""
    s = c["w"]["start"]
    pos = vel = clk = 0.0
    for k in range(c["cfg"].K):
        tt, _ = vt_ref.transmit(s["tow"][k], s["cps"][k], after["cp"][k], after["rc"][k], after["rxTime0"])
        want, rc_ = oracle.sat_pos(s["eph"][k], tt)
        assert rc_ == 0
        d = np.abs(after["sat"][k] - np.asarray(want))
        pos, vel, clk = max(pos, d[:3].max() / 2.6e7), max(vel, d[4:7].max() / 3.0e3), max(clk, d[3], d[7])
    return pos, vel, clk


def check_epoch(c, oracle, e, before, sums, got, after, raw_row=None, lines=None, step=vt_ref.filter_step):
    """One epoch of the form under test: `got` its log record (VectorTracker.unpack_log's, one row), `after` its state after the epoch
    (vt_ref.state_from_rec's dict), raw_row the log row as stored.  Asserts the exact class, the bounds, the satellite states and the
    expected mask and status of the case.  -> {quantity: (deviation, bound)}."""
    cfg = c["cfg"]
    K = cfg.K
    assert after["sat"] is not None                                                                # satValid == 1
    ref, ref_st, bound = reference(c, oracle, before, sums, after["sat"], step=step)
    label = "%s, epoch %d" % (c["name"], e)
    assert ref["mask"] == c["masks"][e] and ref["status"] == c["status"][e], (label, bin(ref["mask"]), ref["status"])
    for n in EXACT:
        assert same(got[n], ref[n]), (label, n, got[n], ref[n])
    # the state after the epoch
    assert after["epochs"] == before["epochs"] + 1 == ref_st["epochs"], label
    assert after["status"] == (before["status"] | c["status"][e]) == ref_st["status"], label     # sticky
    assert after["rxTime0"] == ref["rxTime0"] and after["rxBase"] == before["rxBase"], label
    for n in ("histN", "histPos", "histR", "rc", "ri", "cp"):
        assert same(after[n], ref_st[n]), (label, n, after[n], ref_st[n])
    # the rate ring holds eV, a bounded quantity: every old entry is the one before, the new entry is the logged eV, bit for bit
    for k in range(K):
        want = before["histV"][k].copy()
        if (ref["mask"] >> k) & 1:
            want[before["histPos"][k]] = got["eV"][k]
        assert same(after["histV"][k], want), (label, "histV", k)
    assert same(got["X"], after["X"]) and same(got["diag"], np.diag(after["Sigma"])), label        # the log row is the state
    assert same(after["fc"], got["fc"]) and same(after["fi"], got["fi"]), label
    if raw_row is not None:
        head, lc = dpe.engine.VectorTracker.LOG_HEAD, dpe.engine.VectorTracker.LOG_CHAN
        assert raw_row.shape == (head + 16 * lc,) and np.all(raw_row[head + K * lc:] == 0.0), label   # channels K .. 15 zeroed
    pos, vel, clk = sat_errors(c, oracle, after)
    assert pos < SAT_REL and vel < SAT_REL and clk < SAT_CLK, (label, pos, vel, clk)
    out = {}
    for n in BOUNDED:
        d = deviation(got[n], ref[n])
        out[n] = (d, bound[n])
        if lines is not None:
            lines.append("  %-12s e%-2d %-5s deviation %.3e   bound %.3e   ratio %s" % (c["name"], e, n, d, bound[n], "%.2f" % (d / bound[n]) if bound[n] else ("0/0" if d == 0 else "inf")))
    bad = [(n, v) for n, v in out.items() if not v[0] <= v[1]]
    assert not bad, (label, bad)
    return out
