#!/usr/bin/env python3
"""Fixture O15: the reference twin's own nav-message decode and scalar navigation solution.

Run where the reference tree is available (as make_golden.py, whose harness this imports and which stays as it is):

    python tests/golden/make_golden_o15.py

  O15 parse_ephemerides with Word / Subframe / Ephemerides        libgnss/dataparser.py:10-70; libgnss/ephemeris.py:16-297
      calculate_nav_soln(pOut=True) with perform_least_sqrs       scalar/naveng.py:10-224

Decode: cp_sign streams encoded by tests/nav_synth.py from the shipped handoff's ephemerides -- five PRNs, both polarities, first
subframes 1, 3, 5, 2 and 4 -- are laid into a stub channel's cp / cp_sign, which is all parse_ephemerides reads; one stream with a
single flipped bit in a data word of subframe 2 (the twin raises there: a failed word has no bit string), one with three subframes
only.  Solution: the shipped handoff's eight channels propagated over 24 epochs at constant code and carrier frequency, filled
into stub channels' cp / rc / fi; every epoch solved in the list's order and in six more orders of the satellites, the spread
over which is the yardstick a second implementation of the same arithmetic is held to.
Only DATA is written: the streams, the twin's outputs and the spreads."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (import_pygnss; puts the repository root on sys.path)
import nav_synth as ns  # noqa: E402

dpe = mg.dpe
HANDOFF = os.path.join(mg.ROOT, "navlab-dpe-sdr_amd", "data", "handoff_params_usrp6.csv")

O15_CHANS = (0, 1, 2, 3, 4)                 # rows of the handoff
O15_FIRST_SF = (1, 3, 5, 2, 4)              # subframe ID of the first subframe inside each stream
O15_POL = (1, -1, 1, -1, 1)
O15_LEAD = (437, 52, 3011, 40, 1999)        # entries before the first decoded subframe
O15_CP0 = (1000, 12, 0, 777, 31000)         # code-period count of the stream's first entry
O15_TOW0 = 414000                           # start of the frame's subframe 1
O15_EPOCHS, O15_STEP = 24, 0.5
N_PERM = 6


class StubChannel:
    pass


def make_stream(q, first_sf, lead, pol, n_sub=5, tail=200, iode=77):
    """Entries [start, ...) of two frames' bits: `lead` entries of the subframe before first_sf, n_sub subframes, `tail` more."""
    ids = [5] + [1, 2, 3, 4, 5] * 2 + [1]
    bits = ns.encode_bits(ids, O15_TOW0 - 6, q, iode=iode, iodc=iode)
    s = ns.sign_stream(bits, pol)
    first = 1 + (first_sf - 1)                                # index in ids of the first decoded subframe
    a = first * 6000 - lead
    return s[a:a + lead + n_sub * 6000 + tail].copy(), O15_TOW0 + 6 * (first - 1)


def twin_decode(pg, stream, cp0):
    """parse_ephemerides on a stub channel.  Returns dict(found, raised, fields ..., parity [5, 10], polarity [5], ids [5])."""
    dp, eph = pg.dataparser, pg.ephemeris
    ch = StubChannel()
    n = stream.size
    ch.cp = np.arange(cp0, cp0 + n + 1, dtype=np.float64)
    ch.cp_sign = np.zeros(cp0 + n + 1)
    ch.cp_sign[cp0:cp0 + n] = stream
    ch.ephemerides = None
    captured = []
    orig = eph.Subframe.__init__

    def spy(self, cp, words):            # HARNESS: keep the words of every subframe the twin forms, also when it then raises
        captured.append((cp, words))
        orig(self, cp, words)
    eph.Subframe.__init__ = spy
    raised = 0
    try:
        dp.parse_ephemerides(ch, 0, n)
    except TypeError:
        raised = 1
    finally:
        eph.Subframe.__init__ = orig
    out = dict(raised=raised, found=int(len(captured) > 0), parity=np.full((5, 10), -1), polarity=np.zeros(5, dtype=np.int64),
               subframe_cp=np.full(5, -1, dtype=np.int64), ids=np.full(5, -1), eph=np.full(21, np.nan),
               ints=np.full(5, -1, dtype=np.int64), timestamp=np.full(2, -1, dtype=np.int64))
    for f, (cp, words) in enumerate(captured):
        out["parity"][f] = [int(bool(w.paritypass)) for w in words]
        out["polarity"][f] = int(words[0].polarity)
        out["subframe_cp"][f] = int(cp)
    e = ch.ephemerides
    if e is not None:
        for f, sf in enumerate(e.subframes):
            out["ids"][f] = sf.ID
        out["eph"] = np.array([float(getattr(e, name)) for name in dpe.handoff.EPH_FIELDS])
        out["ints"] = np.array([e.weeknumber, e.accuracy, e.health, e.IODE, e.IODC], dtype=np.int64)
        out["timestamp"] = np.array([e.timestamp["TOW"], e.timestamp["cp"]], dtype=np.int64)
    return out


def make_o15(pg):
    np.product = np.prod                                   # HARNESS: removed in NumPy 2 (ephemeris.py:56)
    pg.dataparser.reload = lambda m: m                     # HARNESS: dataparser.py:53 reloads the module it has already imported;
    pg.dataparser.importlib = types.SimpleNamespace(reload=lambda m: m)   # (as lib2to3 rewrites the call) -- kept, so that the spy below stays
    ho = dpe.handoff.read_handoff(HANDOFF)
    out = {}
    streams, cp0s, names = [], [], []
    for j, k in enumerate(O15_CHANS):
        q = ns.quantise(ns.eph_row_to_dict(ho["eph"][k]))
        s, tow = make_stream(q, O15_FIRST_SF[j], O15_LEAD[j], O15_POL[j], iode=60 + j)
        streams.append(s); cp0s.append(O15_CP0[j]); names.append("prn%d" % ho["prn_list"][k])
    q0 = ns.quantise(ns.eph_row_to_dict(ho["eph"][0]))
    s, _ = make_stream(q0, 1, 300, 1, iode=91)
    s = s.copy()
    b = 300 + 6000 + (5 * 30 + 7) * 20                     # subframe 2, word 6 (e, low bits), data bit 8
    s[b:b + 20] = -s[b:b + 20]
    streams.append(s); cp0s.append(5); names.append("corrupt")
    s, _ = make_stream(q0, 1, 300, -1, n_sub=3, iode=92)
    streams.append(s); cp0s.append(9); names.append("short")
    dec = [twin_decode(pg, s, c) for s, c in zip(streams, cp0s)]
    nmax = max(s.size for s in streams)
    S = np.zeros((len(streams), nmax), dtype=np.int8)
    for i, s in enumerate(streams):
        S[i, :s.size] = s
    out.update(dec_streams=S, dec_n=np.array([s.size for s in streams]), dec_cp0=np.array(cp0s), dec_names=np.array(names),
               dec_src_chan=np.array(list(O15_CHANS) + [0, 0]))
    for key in dec[0]:
        out["dec_" + key] = np.array([d[key] for d in dec])
    for d, name in zip(dec, names):
        print(name, "found", d["found"], "raised", d["raised"], "ids", d["ids"], "timestamp", d["timestamp"])

    # ---- navigation solution
    K = ho["prn_list"].size
    prns = [int(p) for p in ho["prn_list"]]
    rng = np.random.default_rng(1515)
    M = O15_EPOCHS
    t = np.arange(M) * O15_STEP
    chips = ho["rc"][None, :] + ho["fc"][None, :] * t[:, None] + rng.normal(0.0, 0.01, (M, K))   # +- 3 m of code noise
    cp = ho["cp"][None, :] + np.floor(chips / 1023.0)
    rc = chips - 1023.0 * np.floor(chips / 1023.0)
    fi = ho["fi"][None, :] + rng.normal(0.0, 0.3, (M, K)) + 0.4 * t[:, None]
    rx = types.SimpleNamespace(channels={}, rawfile=types.SimpleNamespace(ds=1.0), _mcount=0)
    for k, p in enumerate(prns):
        c = StubChannel()
        c.cp, c.rc, c.fi = cp[:, k].copy(), rc[:, k].copy(), fi[:, k].copy()
        c.ephemerides = mg.Eph(ho, k)
        rx.channels[p] = c
    orders = [list(prns)] + [[prns[i] for i in rng.permutation(K)] for _ in range(N_PERM)]
    res = np.zeros((len(orders), M, 10))                   # rxTime_a, rxTime, posvel_ECEF[8]
    for o, order in enumerate(orders):
        for m in range(M):
            rxTime_a, rxTime, X_ECEF, X_ECI, sats, pr, prate = pg.naveng.calculate_nav_soln(rx, prn_list=order, mc=m, pOut=True)
            res[o, m, 0], res[o, m, 1] = rxTime_a, rxTime
            res[o, m, 2:] = np.asarray(X_ECEF)[:, 0]
    sched = np.zeros((M, 10))                              # the rxTime0 schedule of receiver.py:561-569
    rxTime0 = np.round(res[0, 0, 1] * 1000.0) / 1000.0
    for m in range(M):
        rxTime_a, rxTime, X_ECEF, X_ECI, sats = pg.naveng.calculate_nav_soln(rx, prn_list=prns, mc=m, rxTime0=rxTime0 + m * O15_STEP)
        sched[m, 0], sched[m, 1] = rxTime_a, rxTime
        sched[m, 2:] = np.asarray(X_ECEF)[:, 0]
    spread = res.max(axis=0) - res.min(axis=0)             # [M, 10]
    out.update(sol_prn=np.array(prns), sol_cp=cp, sol_rc=rc, sol_fi=fi, sol_eph=ho["eph"], sol_tow=ho["TOW"], sol_cp_timestamp=ho["cp_timestamp"],
               sol_twin=res[0], sol_spread=spread, sol_yardstick=spread.max(axis=0), sol_orders=np.array(orders),
               sol_sched_rxTime0=rxTime0, sol_sched_step=O15_STEP, sol_sched=sched)
    print("yardstick (rxTime_a, rxTime, X_ECEF[8]):", out["sol_yardstick"])
    path = os.path.join(HERE, "o15_scalar_nav.npz")
    np.savez_compressed(path, **out)
    print("o15_scalar_nav.npz %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    pg = mg.import_pygnss()
    from pythonreceiver.libgnss import dataparser, ephemeris
    from pythonreceiver.scalar import naveng
    pg.dataparser, pg.ephemeris, pg.naveng = dataparser, ephemeris, naveng
    make_o15(pg)
