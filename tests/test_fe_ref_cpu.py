"""CPU: the front end's fp64 specification (tests/fe_ref.py) against a direct np.convolve form on one case per input format, its
phase-word arithmetic against Python integers at indices near 2^33 and 2^40, the designer and the dtype map of
navlab_dpe_sdr_amd.frontend, and every condition the GPU cases of tests/fe_world.py rest on, proven on the reference alone before
the device sees them: tol <= 0.02 and at most 5 % of the values in the rounding band per case, no clipping in the parity table,
no saturation value within 1 of a rail's threshold, and the end-to-end world -- all four PRNs found by the oracle's coarse
acquisition on the converted 2-bit record, each delay within one output sample of the truth, each Doppler at the nearest bin."""
import numpy as np
import pytest

from navlab_dpe_sdr_amd import frontend, synth
from oracle import oracle
from tests import fe_ref, fe_world


@pytest.mark.parametrize("fmt", fe_ref.FORMATS)
def test_reference_against_convolve(fmt):
    rng = np.random.Generator(np.random.PCG64(3))
    D, h, gain, n = 3, frontend.design_lowpass(3), 1.7, 900
    T, T0 = h.size, (h.size - 1) // 2
    raw = fe_ref.random_record(fmt, n, rng)
    x = fe_ref.decode(fmt, raw, 0, n)
    d = fe_ref.delta(1.1e6, 10e6)
    z = x * np.exp(-2j * np.pi * ((np.arange(n) * d) % (1 << 32)) / 4294967296.0)
    full = gain * np.convolve(z, h)                   # full[i] = gain sum_t h[t] z[i - t]; h is symmetric: y[m] = full[m D + T0]
    assert np.allclose(h, h[::-1], rtol=0, atol=1e-18)
    n_out = -(-n // D)
    y = fe_ref.convert(x, 0, n, 0, n_out, D, h, gain, d)
    assert np.abs(y - full[np.arange(n_out) * D + T0]).max() <= 1e-9 * np.abs(full).max()
    # a piece from the middle, from a buffer that starts at its own first needed sample
    lo = 100 * D - T0
    lo -= lo % 4
    y2 = fe_ref.convert(fe_ref.decode(fmt, raw, lo, n - lo), lo, n, 100, 50, D, h, gain, d)
    assert np.array_equal(y2, y[100:150])
    if fmt in fe_ref.REAL:
        assert np.all(x.imag == 0)


def test_decoders_bit_layout():
    assert np.array_equal(fe_ref.decode("P2R", np.array([0b11100100], np.uint8), 0, 4), np.array([-3, -1, 1, 3]))
    assert np.array_equal(fe_ref.decode("P2C", np.array([0b01001110], np.uint8), 0, 2), np.array([1 + 3j, -3 - 1j]))
    assert np.allclose(fe_ref.decode("ARGPI4", np.array([1, 0xFA], np.uint8), 0, 2), [np.exp(0.25j * np.pi), 1j])
    assert np.array_equal(fe_ref.decode("I8C", np.array([0x80, 0x7F], np.uint8), 0, 1), [-128 + 127j])
    assert np.array_equal(fe_ref.decode("I16C", np.array([0x00, 0x80, 0xFF, 0x7F], np.uint8), 0, 1), [-32768 + 32767j])
    assert np.array_equal(fe_ref.pack2([0, 1, 2, 3, 3]), [0b11100100, 0b00000011])


def test_phase_words_against_python_integers():
    for f, fs in ((2.5e6, 10e6), (-2.5e6, 10e6), (1234567.8, 10e6), (-4.092e6, 16.368e6), (0.0, 5e6)):
        d = fe_ref.delta(f, fs)
        assert 0 <= d < 2 ** 32 and abs(((d + 2 ** 31) % 2 ** 32 - 2 ** 31) * fs / 2 ** 32 - f) <= fs / 2 ** 33
    assert fe_ref.delta(2.5e6, 10e6) == 2 ** 30 and fe_ref.delta(-2.5e6, 10e6) == 3 * 2 ** 30
    for d in (1, 2 ** 30 + 1, 530243895, 2 ** 32 - 1):
        n = np.array([-3, 0, 5, 2 ** 33 - 1, 2 ** 33, 2 ** 33 + 77, 2 ** 40 - 5, 2 ** 40, 2 ** 40 + 123457], dtype=np.int64)
        assert [int(v) for v in fe_ref.phase_words(n, d)] == [(int(v) * d) % 2 ** 32 for v in n]


def test_designer_and_dtype_map():
    for D in (1, 2, 3, 4, 10, 16, 64):
        h = frontend.design_lowpass(D)
        assert h.size == 8 * D + 1 and abs(h.sum() - 1.0) < 1e-12 and np.allclose(h, h[::-1], rtol=0, atol=1e-18)
        H = np.abs(np.fft.rfft(h, 64 * h.size))
        f = np.arange(H.size) / (64.0 * h.size)                 # cycles per input sample
        # Kaiser's formulas for beta = 8: 81 dB of attenuation, transition 72 / (2.285 (T - 1)) rad = 0.63 / D cycles about the
        # cut-off 0.45 / D -- the stop band begins at 0.76 / D
        if D > 1:
            assert H[f >= 0.8 / D].max() < 10 ** (-70 / 20.0)
        assert np.abs(H[f <= 0.1 / D] - 1.0).max() < 0.01
    assert frontend.design_lowpass(4, taps_per_phase=7).size == 29
    assert frontend.format_from_dtype(np.dtype([("i", "<i2"), ("q", "<i2")])) == "I16C"
    assert frontend.format_from_dtype(np.dtype([("i", "i1"), ("q", "i1")])) == "I8C"
    assert frontend.format_from_dtype(np.dtype([("arg_pi4", "u1")])) == "ARGPI4"
    assert frontend.format_from_dtype(np.int16) == "I16R" and frontend.format_from_dtype(np.int8) == "I8R"
    for bad in (np.float32, np.dtype([("q", "<i2"), ("i", "<i2")]), np.dtype([("i", "<i2"), ("q", "i1")])):
        with pytest.raises(ValueError):
            frontend.format_from_dtype(bad)


def test_parity_table_covers_what_it_should():
    P = fe_world.PARITY
    assert 38 <= len(P) <= 44
    for fmt in fe_ref.FORMATS:
        assert sum(1 for c in P if c[0] == fmt) >= 2, fmt
    assert {c[1] for c in P} == {1, 2, 3, 4, 10, 16, 64}
    assert {c[2] for c in P} >= {1, 3, 1023} and sum(1 for c in P if c[2] == 1023) == 1
    assert all(c[2] in (1, 3, 1023, 8 * c[1] + 1) for c in P) and {c[1] for c in P if c[2] == 8 * c[1] + 1} == {1, 2, 3, 4, 10, 16, 64}
    assert {c[3] for c in P} == {1, 2, 63, 64, 65, "t-1", "t", "t+1", "3t+7"}
    assert {c[4] for c in P} == {0, "+q", "-q", "inc"}


@pytest.mark.parametrize("i", range(len(fe_world.PARITY)))
def test_parity_case_conditions(i):
    c = fe_world.parity_case(i)
    assert c["tol"] <= 0.02, c["tol"]
    assert fe_ref.band(c["y"], c["tol"]).mean() <= 0.05
    assert fe_ref.clip_count(c["y"]) == 0
    assert np.abs(fe_ref.interleave(c["y"])).max() > 0


def test_saturation_case_conditions():
    c = fe_world.saturation_case()
    v = fe_ref.interleave(c["y"])
    assert np.all(np.minimum(np.abs(v - 32767.5), np.abs(v + 32768.5)) > 1.0)
    q = fe_ref.quantise(c["y"])
    assert (q == 32767).sum() > 100 and (q == -32768).sum() > 100 and 1000 < fe_ref.clip_count(c["y"]) < v.size
    assert fe_ref.clip_count(c["y"]) == int(((v > 32767) | (v < -32768)).sum())


def test_world_on_the_reference():
    w = fe_world.world()
    assert w["h"].size == 33 and w["tol"] <= 0.02
    assert fe_ref.band(w["y"], w["tol"]).mean() <= 0.05
    assert fe_ref.clip_count(w["y"]) == 0
    rms = np.sqrt(np.mean(np.abs(w["y"]) ** 2) / 2)
    assert 200 < rms < 600, rms
    for k, prn in enumerate(w["ch"]["prn"]):
        a = oracle.coarse_acquisition(w["iq"], fe_world.WORLD_FS_OUT, int(prn), fe_world.WORLD_BINS, coherent=True, wrap_mask=True)
        assert a["found"] and a["cppm"] > 2.0, (prn, a["cppm"])
        dist = abs((a["max_code_idx"] - w["truth_idx"][k] + 1250.0) % 2500.0 - 1250.0)
        assert dist <= 1.0, (prn, a["max_code_idx"], w["truth_idx"][k])
        rc_err = abs((a["rc"] - w["ch"]["rc"][k] + 511.5) % synth.L_CA - 511.5)
        assert rc_err <= synth.F_CA / fe_world.WORLD_FS_OUT + 1e-9, (prn, a["rc"], w["ch"]["rc"][k])
        assert a["max_dopp_idx"] == w["truth_bin"][k], (prn, a["fi"], w["ch"]["fi"][k])
