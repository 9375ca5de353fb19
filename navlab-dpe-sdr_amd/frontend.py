"""Helpers around engine.FrontEnd (dpe_fe_*): a low-pass designer for the decimator, the input format of the
reference's raw-file dtypes (pygnss rawfile.py:102-108, 152-158), and a generator that takes a raw file through the front end
piece by piece, with an excisor behind the front end where one is wanted (Excised).  No device is needed to import this module or
to design a filter."""
import numpy as np


def design_lowpass(D, taps_per_phase=8, beta=8.0, cutoff=0.9):
    """Kaiser-windowed sinc for decimation by D: odd length T = taps_per_phase D + 1 (made odd when it is not), cut-off at
    `cutoff` times the output Nyquist frequency fs_in / (2 D), unit gain at DC.  Symmetric, so its group delay is (T - 1) / 2."""
    D = int(D)
    T = int(taps_per_phase) * D + 1
    T += 1 - T % 2
    n = np.arange(T, dtype=np.float64) - (T - 1) // 2
    h = np.sinc(float(cutoff) / D * n) * np.kaiser(T, float(beta))
    return h / h.sum()


def format_from_dtype(dtype):
    """The FrontEnd format name of a numpy dtype: the reference's structured dtypes with the fields ('i', 'q') (int8 or int16) or
    ('arg_pi4',), and plain int8 / int16 for a real-sampled record."""
    dt = np.dtype(dtype)
    if dt.names is not None:
        if tuple(dt.names) == ("i", "q") and dt["i"] == dt["q"] and dt.itemsize == 2 * dt["i"].itemsize:
            if dt["i"] == np.dtype("<i2"):
                return "I16C"
            if dt["i"] == np.dtype("i1"):
                return "I8C"
        if tuple(dt.names) == ("arg_pi4",) and dt.itemsize == 1:
            return "ARGPI4"
    elif dt == np.dtype("<i2"):
        return "I16R"
    elif dt == np.dtype("i1"):
        return "I8R"
    raise ValueError("no front-end input format for dtype %r" % (dt,))


def convert_file(path, fe, chunk_out, record_length=None):
    """The whole record in the file `path` through `fe` (an engine.FrontEnd with int16 output), chunk_out outputs per piece: reads
    the bytes each piece needs (consecutive pieces overlap by T - 1 input samples), uploads them, converts, and yields the device
    int16 tensors [2 n] in order.  record_length (input samples; default: what the file holds) ends the record; the outputs are
    m = 0 .. ceil(record_length / D) - 1.  By the front end's split property the pieces are the bytes one call would give."""
    import os
    import torch
    num, den = fe.bytes_num, fe.bytes_den
    n_file = os.path.getsize(path) * den // num
    record_length = n_file if record_length is None else int(record_length)
    if record_length > n_file:
        raise ValueError("the file holds %d samples, record_length is %d" % (n_file, record_length))
    n_out = -(-record_length // fe.D)
    with open(path, "rb") as f:
        for first in range(0, n_out, int(chunk_out)):
            count = min(int(chunk_out), n_out - first)
            lo, hi = fe.needed(first, count, record_length)
            lo -= lo % den                                   # a packed format's buffer starts on a byte boundary
            f.seek(lo * num // den)
            raw = np.frombuffer(f.read(-(-(hi - lo) * num // den)), dtype=np.uint8)
            dev = torch.from_numpy(raw.copy()).to("cuda")
            yield fe.convert(dev, lo, first, count, record_length=record_length, raw_count=hi - lo)


class Excised:
    """An engine.FrontEnd followed by an engine.Excisor, with the face convert_file reads a front end by: convert_file(path,
    Excised(fe, excisor), chunk_out) yields each chunk of the front end's output excised.  A chunk of excised outputs needs front-end
    outputs on both sides of it (Excisor.needed), so `needed` asks for the raw samples of that wider range and `convert` takes the
    wider range through the front end before it excises the chunk.  By the split property of both stages the pieces are the bytes
    of one FrontEnd.convert call over the whole record put through one Excisor.process call.  Both stages give int16."""

    def __init__(self, fe, excisor):
        if fe.out_f32 or excisor.in_f32:
            raise ValueError("Excised joins a front end with int16 output to an excisor with int16 input")
        self.fe, self.excisor = fe, excisor
        self.D, self.bytes_num, self.bytes_den = fe.D, fe.bytes_num, fe.bytes_den

    def _mid(self, out_first, out_count, record_length):
        """The front-end outputs the excised outputs read; the front end's record of n_in input samples holds ceil(n_in / D)."""
        n_mid = None if record_length is None else -(-int(record_length) // self.D)
        lo, hi = self.excisor.needed(out_first, out_count, n_mid)
        return lo, hi, n_mid

    def needed(self, out_first, out_count, record_length=None):
        lo, hi, _ = self._mid(out_first, out_count, record_length)
        if hi <= lo:
            return 0, 0
        return self.fe.needed(lo, hi - lo, record_length)

    def convert(self, raw, raw_first, out_first, out_count, record_length=None, raw_count=None, out=None, stream=None):
        import torch
        lo, hi, n_mid = self._mid(out_first, out_count, record_length)
        if hi > lo:
            mid = self.fe.convert(raw, raw_first, lo, hi - lo, record_length=record_length, raw_count=raw_count, stream=stream)
        else:                                                # (outputs wholly beyond the record read nothing)
            mid = torch.zeros(2, dtype=torch.int16, device="cuda")
        return self.excisor.process(mid, lo, out_first, out_count, record_length=n_mid, x_count=hi - lo, out=out, stream=stream)
