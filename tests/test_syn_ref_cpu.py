"""CPU: the numpy restatement the synthesiser's GPU tests compare against (tests/syn_ref.py) is itself pinned -- its Philox4x32-10
to the generator's known answers, its signal at sigma = 0 to the shipped host generators synth.gen_iq and synth.gen_iq_record element
for element at every shape the GPU tests use, its Gaussian pair to its moments over 2^20 samples -- and synth.cn0_to_amp to its
definition and its inverse."""
import numpy as np
import pytest

from navlab_dpe_sdr_amd import synth
from tests import syn_ref

KNOWN = [   # counter, key, output (Random123's known-answer vectors for philox4x32-10)
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KNOWN)
def test_philox_known_answers(ctr, key, want):
    got = syn_ref.philox4x32_10(ctr, key)
    assert tuple(int(w[0]) for w in got) == want


def test_philox_is_elementwise():
    n = np.arange(5, dtype=np.uint64) + np.uint64(0xfffffffe)        # crosses into the counter's second word
    w = syn_ref.philox4x32_10((n & syn_ref.MASK, n >> np.uint64(32), 7, 0), (1, 2))
    for i in range(5):
        one = syn_ref.philox4x32_10((int(n[i]) & 0xffffffff, int(n[i]) >> 32, 7, 0), (1, 2))
        assert [int(x[i]) for x in w] == [int(x[0]) for x in one]


@pytest.mark.parametrize("shape", syn_ref.WINDOW_SHAPES, ids=[s[0] for s in syn_ref.WINDOW_SHAPES])
def test_window_form_at_sigma_0_is_gen_iq(shape):
    name, fs, S, K, W, _, dc, mode, _, _ = shape
    chs, amp, flips = syn_ref.window_case(shape)
    assert amp.sum() <= 400.0 + 1e-9
    for w in range(W):
        x = syn_ref.window(fs, S, chs[w], amp, 0.0, dc, flips[w], 1, w)
        want = synth.gen_iq(0, fs, S, chs[w], amp=amp, sigma=0.0, dc=dc, flip=flips[w])
        assert np.array_equal(syn_ref.quantise(x), want), (name, w)
    if mode == "edges":      # the flips the shape promises: at sample 1, at S - 1, and none for the boundary outside the window
        x0 = syn_ref.window(fs, S, chs[0], amp, 0.0, dc, np.zeros(K, dtype=bool), 1, 0)
        x1 = syn_ref.window(fs, S, chs[0], amp, 0.0, dc, np.array([True] + [False] * (K - 1)), 1, 0)
        assert x1[0] == x0[0] and np.all(x1[1:] != x0[1:])
        x2 = syn_ref.window(fs, S, chs[0], amp, 0.0, dc, np.array([False, True] + [False] * (K - 2)), 1, 0)
        assert np.all(x2[:S - 1] == x0[:S - 1]) and x2[S - 1] != x0[S - 1]
        x3 = syn_ref.window(fs, S, chs[0], amp, 0.0, dc, np.array([False, False, True] + [False] * (K - 3)), 1, 0)
        assert np.array_equal(x3, x0)


def test_edge_code_phases_are_what_the_shapes_say():
    chs, _, _ = syn_ref.window_case(syn_ref.WINDOW_SHAPES[1])
    assert all(0 < c["rc"][0] < 1e-9 and 0 < 1023.0 - c["rc"][-1] < 1e-9 and np.all(c["fi"] < 0) for c in chs)
    chs, _, _ = syn_ref.window_case(syn_ref.WINDOW_SHAPES[2])
    assert np.all(chs[0]["fi"] > 0)


def test_record_form_at_sigma_0_is_gen_iq_record():
    fs, n = syn_ref.RECORD["fs"], syn_ref.RECORD["n"]
    ch, amp, bits = syn_ref.record_case()
    want, used = synth.gen_iq_record(0, fs, n, ch, amp=amp, sigma=0.0, nav_bits=bits)
    assert sum(int(np.any(np.diff(b.astype(int)))) for b in used) >= 3     # sign changes inside the record
    assert np.array_equal(syn_ref.quantise(syn_ref.record(fs, 0, n, ch, amp, 0.0, bits, 1, 0)), want)
    # a sub-range is the slice of the whole: the restatement has no state either
    part = syn_ref.record(fs, 13001, 16001, ch, amp, 300.0, bits, 5, 2)
    whole = syn_ref.record(fs, 0, n, ch, amp, 300.0, bits, 5, 2)
    assert np.array_equal(part, whole[13001:29002])
    assert syn_ref.n_bits_needed(fs, n - 1, ch) == [b.size for b in used]


def test_noise_moments_over_two_to_the_20_samples():
    N = 1 << 20
    gi, gq = syn_ref.gauss(0xfeedfacecafebeef, 3, np.arange(N, dtype=np.uint64))
    se = 1.0 / np.sqrt(N)
    assert abs(gi.mean()) < 5 * se and abs(gq.mean()) < 5 * se
    assert abs(gi.var() - 1.0) < 5 * np.sqrt(2.0) * se and abs(gq.var() - 1.0) < 5 * np.sqrt(2.0) * se
    assert abs(np.mean(gi * gq)) < 5 * se
    assert max(np.abs(gi).max(), np.abs(gq).max()) <= np.sqrt(48.0 * np.log(2.0)) + 1e-12      # the tail ends at 5.77 sigma
    g2, _ = syn_ref.gauss(0xfeedfacecafebeef, 4, np.arange(N, dtype=np.uint64))
    assert abs(np.mean(gi * g2)) < 5 * se                                                       # streams are independent


def test_cn0_to_amp_round_trip():
    fs, sigma = 2.5e6, 300.0
    for cn0 in (25.0, 38.5, 45.0, 60.0):
        amp = synth.cn0_to_amp(cn0, sigma, fs)
        assert abs(amp ** 2 * fs / (2 * sigma ** 2) - 10 ** (cn0 / 10)) < 1e-9 * 10 ** (cn0 / 10)
        assert abs(synth.amp_to_cn0(amp, sigma, fs) - cn0) < 1e-10
    assert abs(synth.amp_to_cn0(48.0, 300.0, 2.5e6) - 10 * np.log10(48.0 ** 2 * 2.5e6 / (2 * 300.0 ** 2))) < 1e-12
    a = synth.cn0_to_amp(np.array([30.0, 40.0]), 300.0, 2.5e6)
    assert a.shape == (2,) and abs(a[1] / a[0] - np.sqrt(10.0)) < 1e-12
