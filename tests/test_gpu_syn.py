"""GPU: the synthesiser (dpe_syn_*, engine.Synthesizer) against the numpy restatement tests/syn_ref.py.

The acceptance rule: every device sample d satisfies |d - clip(x_ref)| <= 0.5 + eps per component, x_ref the fp64 pre-rounding value.
Chips, nav signs, sample times and noise counters are exact by construction on both sides, so an error in any of them moves a sample
by whole units and fails; eps bounds only what the device does in fp32.  Term by term, with u = 2^-24 (the unit roundoff of fp32,
half an ulp) and the error bounds the OpenCL / HIP math specification gives the device functions (sincospi 4 ulp = 8 u absolute on
values <= 1, log 3 ulp = 6 u relative, sqrt taken as 1 ulp = 2 u), for amplitudes amp_k, A = sum amp_k, K channels, noise sigma:

  signal, per channel, relative to amp_k:
      amp_k rounded to fp32                                                  1 u
      the cycle fraction in [-0.5, 0.5] rounded to fp32: 2^-26 cycles,
          i.e. 2 pi 2^-26 rad on a unit phasor                              1.58 u
      sincospif                                                              8 u
      (the product of amp_k and the +-1 chip and sign is exact)
  accumulation: K fused multiply-adds, each rounding a partial sum <= A      K u A
  noise, relative to sigma, with r = sqrt(-2 ln u1) <= 5.77:
      ln: 6 u on L = -2 ln u1, halved by the root: 3 u; the root itself 2 u   5 u r
      sincospif 8 u, the product r cos / r sin 1 u                           9 u r
      sigma rounded to fp32                                                  1 u r
  the last two operations (sigma g + acc, + dc), each rounding |x| <= A + 5.77 sigma + |dc|, and dc rounded to fp32

  eps = u [ A (10.58 + K) + 15 * 5.77 sigma + 2 (A + 5.77 sigma + |dc|) + |dc| ]

At the test amplitudes (A <= 400, K <= 12, sigma <= 300, |dc| <= 3) that is 2.3e-3, far below the 0.05 the issue allows; the
saturation test (A = 40 000) uses the same formula (0.03).  Samples whose x_ref lies farther than eps from a half-integer -- all
but a fraction of about 2 eps -- are thereby held to exact equality with rint(x_ref); the test asserts that too, and prints the
measured worst |d - x_ref| - 0.5 (DESIGN.md 7f records it)."""
import ctypes as C

import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import helpers, syn_ref

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
GUARD = 12345


def eps_of(A, K, sigma, dc):
    d = float(np.max(np.abs(dc)))
    return U * (A * (10.58 + K) + 15 * 5.77 * sigma + 2 * (A + 5.77 * sigma + d) + d)


def accept(d, x_ref, eps, what):
    """d: interleaved int16 from the device; x_ref: complex128.  Returns the worst |d - x_ref| - 0.5."""
    d = d.astype(np.float64)
    worst = -1.0
    for comp, got in ((x_ref.real, d[0::2]), (x_ref.imag, d[1::2])):
        ref = np.clip(comp, -32768.0, 32767.0)
        err = np.abs(got - ref)
        worst = max(worst, float(err.max()) - 0.5)
        assert err.max() <= 0.5 + eps, "%s: sample %d off by %.6f (eps %.2e)" % (what, int(err.argmax()), err.max(), eps)
        clear = np.abs(comp - np.floor(comp) - 0.5) > eps
        assert np.array_equal(got[clear], np.clip(np.rint(comp), -32768, 32767)[clear]), what
        assert clear.mean() > 0.9, what
    print("%s: worst |d - x_ref| - 0.5 = %.3e (eps %.3e)" % (what, worst, eps))
    return worst


@pytest.fixture(scope="module")
def syn():
    import __graft_entry__ as ge
    ge.build()
    s = {}

    def get(fs):
        if fs not in s:
            s[fs] = dpe.Synthesizer(fs, max_segments=8, max_channels=12, max_nav_bits=1 << 17)
        return s[fs]
    yield get
    for h in s.values():
        h.close()


def chan_array(chs):
    return np.stack([dpe.engine.chan_start_array(c["prn"], c["rc"], c["ri"], c["fc"], c["fi"], c["cp"], c["cp_ref"]) for c in chs])


@pytest.mark.parametrize("shape", syn_ref.WINDOW_SHAPES, ids=[s[0] for s in syn_ref.WINDOW_SHAPES])
def test_windows_against_the_restatement(syn, shape):
    import torch
    name, fs, S, K, W, sigma, dc, mode, rc_edge, fi_sign = shape
    chs, amp, flips = syn_ref.window_case(shape)
    gap = next(g for g in range(S + 1, S + 5) if (S + g) % 4 == 1)          # pairs between windows: the stride exceeds 2 S, and
    stride = 2 * (S + gap)                                                   # consecutive windows start at every 16-byte phase
    buf = torch.full((W * stride + 2,), GUARD, dtype=torch.int16, device="cuda")
    out = buf[2:]                                                            # 4-byte aligned, not 16
    seed, first = 0x1234567887654321, (1 << 40) + 3
    syn(fs).windows(S, chan_array(chs), amp=amp, sigma=sigma, dc=dc, flip=flips, seed=seed, first_stream=first, stride=stride, out=out)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:2] == GUARD).all()
    eps = eps_of(amp.sum(), K, sigma, dc)
    assert eps <= 0.05
    for w in range(W):
        row = got[2 + w * stride: 2 + (w + 1) * stride]
        assert (row[2 * S:] == GUARD).all(), "window %d: the values behind it were overwritten" % w
        x = syn_ref.window(fs, S, chs[w], amp, sigma, dc, flips[w], seed, first + w)
        accept(row[:2 * S], x, eps, "%s window %d" % (name, w))


def test_windows_do_not_depend_on_batch_position_or_stride(syn):
    """Window 3 of a batch of five equals the same window generated alone with its stream id, at another stride and alignment."""
    import torch
    shape = syn_ref.WINDOW_SHAPES[1]
    _, fs, S, K, W, sigma, dc, _, _, _ = shape
    chs, amp, flips = syn_ref.window_case(shape)
    a = syn(fs).windows(S, chan_array(chs), amp=amp, sigma=sigma, dc=dc, flip=flips, seed=9, first_stream=100, stride=2 * S + 2)
    b = syn(fs).windows(S, chan_array(chs[3:4]), amp=amp, sigma=sigma, dc=dc, flip=flips[3:4], seed=9, first_stream=103)
    c = syn(fs).windows(S, chan_array(chs[3:4]), amp=amp, sigma=sigma, dc=dc, flip=flips[3:4], seed=9, first_stream=104)
    torch.cuda.synchronize()
    assert torch.equal(a[3, :2 * S], b[0]) and not torch.equal(b[0], c[0])


def test_record_against_the_restatement_and_in_pieces(syn):
    import torch
    fs, n, K, sigma, seed = (syn_ref.RECORD[k] for k in ("fs", "n", "K", "sigma", "seed"))
    ch, amp, bits = syn_ref.record_case()
    s = syn(fs)
    s.set_nav_bits(bits)
    whole = s.record(0, n, ch, amp=amp, sigma=sigma, seed=seed, stream_id=5)
    again = s.record(0, n, ch, amp=amp, sigma=sigma, seed=seed, stream_id=5)
    other = s.record(0, n, ch, amp=amp, sigma=sigma, seed=seed, stream_id=6)
    pieces = torch.full((2 * n,), GUARD, dtype=torch.int16, device="cuda")
    for a, b in ((29002, n), (0, 13001), (13001, 29002)):                   # three unequal pieces, out of order, odd boundaries
        s.record(a, b - a, ch, amp=amp, sigma=sigma, seed=seed, stream_id=5, out=pieces[2 * a:2 * b])
    torch.cuda.synchronize()
    assert torch.equal(whole, again), "the same seed twice gives the same bytes"
    assert torch.equal(whole, pieces), "a range generated in pieces gives the bytes of one call"
    eps = eps_of(amp.sum(), K, sigma, (0.0, 0.0))
    assert eps <= 0.05
    x5 = syn_ref.record(fs, 0, n, ch, amp, sigma, bits, seed, 5)
    edges = sum(int(np.any(np.diff((np.floor(np.arange(n) / fs * ch["fc"][k] + ch["rc"][k]).astype(np.int64) // 1023
                                    - int(ch["cp_ref"][k]) % 20 + 20) // 20))) for k in range(K))
    assert edges >= 4, "nav-bit edges must fall inside the record"
    accept(whole.cpu().numpy(), x5, eps, "record 40000")
    x6 = syn_ref.record(fs, 0, n, ch, amp, sigma, bits, seed, 6)
    accept(other.cpu().numpy(), x6, eps, "record 40000, stream 6")          # same signal, other noise
    assert not torch.equal(whole, other)


def test_record_beyond_two_to_the_32_samples(syn):
    """firstSample = 2^32 - 100: the counter's high word, a chip count beyond 2^31 in places, nav-bit indices in the ten thousands."""
    import torch
    fs, K, sigma, seed = (syn_ref.RECORD[k] for k in ("fs", "K", "sigma", "seed"))
    first, n = (1 << 32) - 100, 4093
    ch, amp, bits = syn_ref.record_case(first, n)
    s = syn(fs)
    s.set_nav_bits(bits)
    got = s.record(first, n, ch, amp=amp, sigma=sigma, seed=seed, stream_id=1 << 33)
    torch.cuda.synchronize()
    x = syn_ref.record(fs, first, n, ch, amp, sigma, bits, seed, 1 << 33)
    accept(got.cpu().numpy(), x, eps_of(amp.sum(), K, sigma, (0.0, 0.0)), "record from 2^32 - 100")


def test_saturation_clips_where_the_restatement_does(syn):
    import torch
    fs, S = 2.5e6, 4093
    ch = syn_ref.channels(3, 1, fs)
    amp, sigma, dc = np.array([40000.0]), 300.0, (3.0, -2.0)
    got = syn(fs).windows(S, ch, amp=amp, sigma=sigma, dc=dc, flip=None, seed=4, first_stream=0)
    torch.cuda.synchronize()
    d = got[0].cpu().numpy()
    x = syn_ref.window(fs, S, ch, amp, sigma, dc, None, 4, 0)
    eps = eps_of(40000.0, 1, sigma, dc)
    accept(d, x, eps, "saturation")
    for comp, g in ((x.real, d[0::2]), (x.imag, d[1::2])):
        hi, lo = comp > 32767.5 + eps, comp < -32768.5 - eps
        assert hi.sum() > 100 and lo.sum() > 100
        assert (g[hi] == 32767).all() and (g[lo] == -32768).all()
        assert (g[comp < 32766.5 - eps] < 32767).all() and (g[comp > -32767.5 + eps] > -32768).all()


def test_refusals_each_with_a_message(syn):
    import torch
    fs = 2.5e6
    s = syn(fs)
    ch = syn_ref.channels(1, 12, fs)
    with pytest.raises(dpe.DpeError, match=r"nChan 13 outside 1\.\.12"):
        s.windows(64, {k: np.r_[v, v[:1]] for k, v in ch.items()})            # K above the handle's maximum
    with pytest.raises(dpe.DpeError, match="odd stride"):
        s.windows(64, ch, stride=131)
    with pytest.raises(dpe.DpeError, match="stride 100 below 2 S"):
        s.windows(64, chan_array([ch, ch]), stride=100)
    with pytest.raises(dpe.DpeError, match="nWindows 9 outside"):
        s.windows(64, chan_array([ch] * 9))
    buf = torch.zeros(128, dtype=torch.int16, device="cuda")
    cs = chan_array([ch])
    amp = np.full(12, 10.0)
    sig = dpe.engine.SynSignal(1.0, 0.0, 0.0, 1)
    lib = dpe.engine.lib()
    args = (C.c_int64(128), C.c_int32(1), C.c_int32(64), C.c_int32(12), cs.ctypes.data_as(C.POINTER(dpe.engine.ChanStart)),
            amp.ctypes.data_as(C.POINTER(C.c_double)), C.byref(sig), None, C.c_uint64(0), None)
    assert lib.dpe_syn_windows(s._h, None, *args) != 0 and "null output" in lib.dpe_last_error().decode()
    assert lib.dpe_syn_windows(s._h, C.c_void_p(buf.data_ptr() + 2), *args) != 0 and "not aligned" in lib.dpe_last_error().decode()
    s.set_nav_bits([np.ones(3, dtype=np.int8)] * 12)
    with pytest.raises(dpe.DpeError, match=r"channel \d+ needs \d+ nav bits for its last sample, has 3"):
        s.record(0, 2_500_000, ch, out=buf)                                  # one second: some fifty bits (nothing is launched)
    with pytest.raises(dpe.DpeError, match="not \\+-1"):
        s.set_nav_bits([np.zeros(3, dtype=np.int8)])
    bad = dict(ch, fc=ch["fc"].copy())
    bad["fc"][5] = float("nan")
    with pytest.raises(dpe.DpeError, match="channel 5: a parameter is not finite"):
        s.windows(64, bad)
    torch.cuda.synchronize()
    assert not buf.any()


def test_generated_windows_run_downstream_as_they_are(syn):
    """Windows made on the device go into BatchCorrScores / BatchCorrManifold without leaving it; the same bytes, read back, go
    through the oracle: parity at the tolerance smoke() uses for this shape."""
    import torch
    case = helpers.make_case(seed=3, fs=2.5e6, S=12500, K=4, G=4096, amp=200.0)
    L, B = 8, 32
    w = case["wins"][0]
    iq_d = syn(case["fs"]).windows(case["S"], w["start"], amp=200.0, sigma=300.0, flip=w["flip"], seed=3, first_stream=0)
    _, cs, ce, bw = helpers.pack_gpu_inputs(case)
    bcs = dpe.BatchCorrScores(case["fs"], samples_per_window=case["S"], lag_half_width=L, bin_half_width=B, max_windows=1, max_channels=4)
    bcs.Start()
    bcm = dpe.BatchCorrManifold(case["fs"], case["S"], bcs.NumFFTPoints, case["pos"], case["vel"], lag_half_width=L, bin_half_width=B,
                                max_windows=1, max_channels=4, write_scores=True, weighted_mean=True)
    bcm.Start()
    bcs.Update(iq_d, cs)
    bcm.Update(bcs.CodeScores, bcs.CarrScores, bw, ce)
    res = bcm.results()
    code, carr = bcs.read_banks()
    idx_next, no_flip, mean = bcs.read_info()
    ps, vs = bcm.read_scores()
    out = dict(code=list(code), carr=list(carr), res=res, idx_next=idx_next, no_flip=no_flip, mean=mean, pos=list(ps), vel=list(vs))
    bcm.Stop()
    bcs.Stop()
    w["iq"] = iq_d[0].cpu().numpy().copy()
    assert np.abs(w["iq"].astype(np.int32)).max() > 500                       # (a window of zeros would agree with itself)
    helpers.assert_parity(out, helpers.run_oracle(case, L=L, B=B), tol=2e-5)
