"""Test-side: a +1 record and its handoff as a DopplerSign = -1 receiver's.

A front end whose spectrum runs the other way delivers the complex conjugate of the samples: every carrier rotates the other way
(fi -> -fi) from the conjugate phase (ri -> -ri, a fraction of a cycle: (1 - ri) mod 1), code phase, code frequency, counters and
ephemerides as they are.  So a +1 record mirrored and a +1 handoff mirrored are the record and the handoff of a -1 receiver on the
same trajectory -- for records built elsewhere (workload.build_windows, fixture logs), whose generators take no sign."""
import numpy as np


def mirror_iq(iq):
    """Interleaved int16 I/Q of any shape [..., 2 n]: Q -> -Q.  -32768 has no int16 negative; no record here holds it."""
    iq = np.asarray(iq)
    assert iq.dtype == np.int16 and iq.shape[-1] % 2 == 0
    assert not np.any(iq[..., 1::2] == -32768), "a sample of -32768 cannot be negated in int16"
    out = iq.copy()
    out[..., 1::2] = -iq[..., 1::2]
    return out


def mirror_handoff(ho):
    """fi -> -fi, ri -> (1 - ri) mod 1; every other entry is shared with `ho`."""
    out = dict(ho)
    out["fi"] = -np.asarray(ho["fi"], dtype=np.float64)
    out["ri"] = np.mod(1.0 - np.asarray(ho["ri"], dtype=np.float64), 1.0)
    return out


def mirror_log(log):
    """A tracker's log rows {cp, rc, fi}: fi -> -fi."""
    out = dict(log)
    out["fi"] = -np.asarray(log["fi"], dtype=np.float64)
    return out
