"""GPU: the front end (dpe_fe_*, engine.FrontEnd) against its fp64 specification tests/fe_ref.py, on the cases of tests/fe_world.py
(proven on the reference alone by tests/test_fe_ref_cpu.py).

The acceptance rule.  With A = gain sum|h| max|x| and tol = (2 T + 16) 2^-24 A (2 T: the fp32 multiply-adds of the two components;
16: a mixer value within 2^-22 and the rotation):
  fp32 output   |device - reference| <= tol at every value;
  int16 output  equal to the reference's outside the band (the values whose fp64 y lies within tol of a half-integer), at most 1
                off inside it, and in every case exactly clip(rint(.)) of the device's own fp32 output.
Each comparison prints the worst residual as a fraction of tol before it asserts."""
import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from navlab_dpe_sdr_amd import frontend, synth
from tests import fe_ref, fe_world

pytestmark = pytest.mark.gpu
GUARD = 12345


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


def _fe(c, out_f32, fs=fe_world.FS):
    return dpe.FrontEnd(fs, c["fmt"], c["D"], c["h"], gain=c["gain"], f_if=c["f_if"], levels=c.get("levels", fe_ref.LEVELS), out_f32=out_f32)


def _device(raw):
    import torch
    return torch.from_numpy(np.ascontiguousarray(raw).view(np.uint8).copy()).to("cuda")


def _convert(c, out_f32, raw_dev=None):
    """-> (host array of the call's output, clip count)"""
    fe = _fe(c, out_f32)
    raw_dev = _device(c["raw"]) if raw_dev is None else raw_dev
    out = fe.convert(raw_dev, c["raw_first"], c["out_first"], c["out_count"], record_length=c["record_length"], raw_count=c["raw_count"])
    clipped = fe.clipped()
    res = out.cpu().numpy()
    fe.close()
    return res, clipped


def _accept(c, what, raw_dev=None):
    f32, _ = _convert(c, True, raw_dev)
    i16, clipped = _convert(c, False, raw_dev)
    ref, tol = fe_ref.interleave(c["y"]), c["tol"]
    worst = float(np.abs(f32.astype(np.float64) - ref).max())
    print("%s: worst |fp32 - reference| = %.3e = %.3f of tol %.3e" % (what, worst, worst / tol, tol))
    assert worst <= tol, what
    own = np.clip(np.rint(f32), -32768, 32767).astype(np.int16)
    assert np.array_equal(i16, own), what
    want, band = fe_ref.quantise(c["y"]), fe_ref.band(c["y"], tol)
    assert np.array_equal(i16[~band], want[~band]), what
    assert np.abs(i16.astype(np.int32) - want.astype(np.int32)).max() <= 1, what
    assert clipped == fe_ref.clip_count(c["y"]) == 0, what
    return worst / tol


# ---- 1. exact pass-through
def test_passthrough_i16c_bytes_identical():
    rng = np.random.Generator(np.random.PCG64(1))
    v = rng.integers(-32768, 32768, 2 * 3001).astype("<i2")
    v[:6] = [32767, -32768, -32768, 32767, 32767, 32767]
    v[-2:] = [-32768, -32768]
    fe = dpe.FrontEnd(25e6, "I16C", 1, [1.0])
    out = fe.convert(_device(v), 0, 0, 3001)
    assert fe.clipped() == 0
    assert np.array_equal(out.cpu().numpy(), v)
    fe.close()


def test_passthrough_i8c_gain_256():
    rng = np.random.Generator(np.random.PCG64(2))
    v = rng.integers(-128, 128, 2 * 2999).astype(np.int8)
    v[:4] = [127, -128, -128, 127]
    fe = dpe.FrontEnd(25e6, "I8C", 1, [1.0], gain=256.0)
    out = fe.convert(_device(v), 0, 0, 2999)
    assert np.array_equal(out.cpu().numpy(), v.astype(np.int16) * 256) and fe.clipped() == 0
    fe.close()


# ---- 2. the parity table
@pytest.mark.parametrize("i", range(len(fe_world.PARITY)))
def test_parity(i):
    c = fe_world.parity_case(i)
    fe = _fe(c, False)
    assert fe.tile_outputs == fe_world.tile_outputs(c["D"], c["T"], c["fmt"] in fe_ref.REAL)
    assert fe.lds_bytes == fe_world.lds_bytes(c["D"], c["T"], c["fmt"] in fe_ref.REAL) and fe.delta == c["delta"]
    fe.close()
    _accept(c, "parity %d %s" % (i, fe_world.PARITY[i],))


def test_parity_from_a_synthesizer_record():
    """The input is the tensor Synthesizer.record left on the device; it comes to the host for the reference alone."""
    ch = synth.random_channels(11, 4)
    n = 40000
    syn = dpe.Synthesizer(10e6, max_segments=1, max_channels=4, max_nav_bits=64)
    syn.set_nav_bits([np.ones(64, dtype=np.int8)] * 4)
    rec = syn.record(0, n, ch, amp=60.0, sigma=300.0, seed=9)
    raw = rec.cpu().numpy().view(np.uint8)
    h, D, gain = frontend.design_lowpass(4), 4, 0.5
    x = fe_ref.decode("I16C", raw, 0, n)
    assert np.abs(x).max() <= 2047 * np.sqrt(2.0)
    c = dict(fmt="I16C", D=D, T=h.size, h=h, gain=gain, f_if=0.0, delta=0, raw=raw, raw_first=0, raw_count=n, record_length=n, out_first=0,
             out_count=n // D, y=fe_ref.convert(x, 0, n, 0, n // D, D, h, gain, 0), tol=fe_ref.tolerance(h, gain, float(np.abs(x).max())))
    assert c["tol"] <= 0.02 and fe_ref.band(c["y"], c["tol"]).mean() <= 0.05
    _accept(c, "synthesizer record", raw_dev=rec)
    syn.close()


# ---- 3. record edges
@pytest.mark.parametrize("fmt,D,T,first,count,length", [("I8C", 4, 33, 0, 40, None), ("P2R", 3, 25, 0, 1300, None), ("I16C", 4, 33, 231, 20, 1003),
                                                         ("P2C", 10, 81, 90, 11, 1001), ("I8R", 1, 9, 0, 7, 7)])
def test_record_edges(fmt, D, T, first, count, length):
    """Zeros before sample 0 (first = 0), zeros from the record's length on (the last outputs), and both at once; the buffer holds
    exactly the samples of the record that the outputs need."""
    gain = {"I8C": 1.0, "P2R": 20.0, "I16C": 0.5, "P2C": 20.0, "I8R": 1.0}[fmt]
    c = fe_world.make_case(fmt, D, T, first, count, fe_world.INCOMMENSURATE * fe_world.FS, gain, seed=500 + D, record_length=length)
    assert c["tol"] <= 0.02
    if length is not None:
        assert (first + count - 1) * D + T - (T - 1) // 2 > length and c["raw_first"] + c["raw_count"] == length
    _accept(c, "edges %s D %d first %d length %s" % (fmt, D, first, length))


# ---- 4. large indices
def test_large_indices():
    """outFirst D just above 2^33 with an odd phase increment: a 32-bit slip or a drifting phase turns the outputs."""
    D, T = 4, 33
    d = fe_ref.delta(fe_world.INCOMMENSURATE * fe_world.FS, fe_world.FS) | 1
    f_if = d * fe_world.FS / 4294967296.0
    assert fe_ref.delta(f_if, fe_world.FS) == d and d % 2 == 1
    first = 2 ** 33 // D + 3
    c = fe_world.make_case("I8C", D, T, first, 1500, f_if, 1.0, seed=900)
    assert c["raw_first"] > 2 ** 33 - T and c["tol"] <= 0.02
    _accept(c, "large indices")


# ---- 5. the split property
@pytest.mark.parametrize("fmt,D,T,f_if,gain", [("P2C", 3, 25, "inc", 20.0), ("I16R", 10, 81, "+q", 0.5), ("I16C", 2, 17, 0, 0.5)])
def test_split_property(fmt, D, T, f_if, gain):
    import torch
    tile = fe_world.tile_outputs(D, T, fmt in fe_ref.REAL)
    count = 2 * tile + 211
    c = fe_world.make_case(fmt, D, T, 777, count, fe_world._if_hz(f_if), gain, seed=600 + D)
    raw = _device(c["raw"])
    for out_f32 in (False, True):
        fe = _fe(c, out_f32)
        one = fe.convert(raw, c["raw_first"], c["out_first"], count, raw_count=c["raw_count"])
        parts, at = [], 0
        for n in (1, 7, tile + 3, count - tile - 11):
            parts.append(fe.convert(raw, c["raw_first"], c["out_first"] + at, n, raw_count=c["raw_count"]))
            at += n
        assert at == count
        pieces = torch.cat(parts)
        bits = torch.int32 if out_f32 else torch.int16
        assert torch.equal(one.view(bits), pieces.view(bits)), (fmt, out_f32)
        fe.close()


def test_convert_file_equals_one_call(tmp_path):
    import torch
    rng = np.random.Generator(np.random.PCG64(8))
    n, D = 10007, 4
    raw = fe_ref.random_record("P2R", n, rng)[: -(-n // 4)]
    path = tmp_path / "record.bin"
    path.write_bytes(raw.tobytes())
    n_file = raw.size * 4
    fe = dpe.FrontEnd(10e6, "P2R", D, frontend.design_lowpass(D), gain=20.0, f_if=2.5e6)
    pieces = list(frontend.convert_file(str(path), fe, 997, record_length=n))
    assert [p.numel() // 2 for p in pieces] == [997, 997, 508]
    one = fe.convert(_device(raw), 0, 0, -(-n // D), record_length=n, raw_count=n_file)
    assert torch.equal(one, torch.cat(pieces))
    want = fe_ref.quantise(fe_ref.convert(fe_ref.decode("P2R", raw, 0, n), 0, n, 0, -(-n // D), D, fe.taps, 20.0, fe.delta))
    assert np.abs(one.cpu().numpy().astype(np.int32) - want).max() <= 1
    fe.close()


# ---- 6. saturation
def test_saturation_and_clip_count():
    c = fe_world.saturation_case()
    i16, clipped = _convert(c, False)
    want = fe_ref.quantise(c["y"])
    assert np.array_equal(i16, want) and i16.max() == 32767 and i16.min() == -32768
    assert clipped == fe_ref.clip_count(c["y"]) > 1000
    f32, _ = _convert(c, True)
    assert np.array_equal(f32.astype(np.float64), fe_ref.interleave(c["y"]))            # 3 x is exact in fp32: nothing is clipped here


# ---- 7. refusals
def test_refusals_launch_nothing():
    import torch
    h = frontend.design_lowpass(4)
    fe = dpe.FrontEnd(10e6, "I16C", 4, h)
    raw = torch.zeros(2 * 69, dtype=torch.int16, device="cuda")
    out = torch.full((20,), GUARD, dtype=torch.int16, device="cuda")

    def refused(pattern, *args, **kw):
        with pytest.raises(dpe.DpeError, match=pattern) as e:
            kw.pop("fe", fe).convert(*args, out=out, **kw)
        assert str(e.value).startswith("[FrontEnd] ")
        torch.cuda.synchronize()
        assert bool((out == GUARD).all())

    fe.convert(raw, 384, 100, 10, out=out.clone())                                             # outputs 100..109 need 384..452: accepted
    refused(r"need the input samples 384\.\.452, the buffer holds 385\.\.453", raw, 385, 100, 10)
    refused(r"need the input samples 384\.\.452, the buffer holds 383\.\.451", raw, 383, 100, 10)
    refused(r"need the input samples 384\.\.452, the buffer holds 384\.\.451", raw, 384, 100, 10, raw_count=68)
    refused(r"null input buffer", 0, 384, 100, 10, raw_count=69)
    refused(r"0 outputs outside", raw, 384, 100, 0)
    refused(r"first output -1", raw, 384, -1, 10)
    with pytest.raises(dpe.DpeError, match=r"\[FrontEnd\] convert: null output buffer"):
        fe.convert(raw, 384, 100, 10, out=0)
    p2 = dpe.FrontEnd(10e6, "P2R", 4, h)
    refused(r"not on a byte boundary \(4 samples per byte\)", raw, 382, 100, 10, fe=p2)
    p2.close()
    p2c = dpe.FrontEnd(10e6, "P2C", 4, h)
    refused(r"not on a byte boundary \(2 samples per byte\)", raw, 383, 100, 10, fe=p2c)
    p2c.close()
    fe.close()
    for kw, pat in ((dict(D=4, taps=np.ones(32)), "T = 32 taps is even"), (dict(D=0, taps=h), r"decimation D = 0 outside 1\.\.64"),
                    (dict(D=65, taps=h), r"decimation D = 65 outside 1\.\.64"), (dict(D=4, taps=np.ones(1025)), r"T = 1025 taps outside 1\.\.1023")):
        with pytest.raises(dpe.DpeError, match=r"\[FrontEnd\] create: " + pat):
            dpe.FrontEnd(10e6, "I16C", kw["D"], kw["taps"])
    assert dpe.engine.lib().dpe_fe_create(None, None, None) != 0
    assert dpe.engine.lib().dpe_last_error().decode().startswith("[FrontEnd] create: null argument")


# ---- 8. end to end
def test_world_acquired_at_2p5_msps():
    """A 2-bit real-IF record at 10 Msps, which nothing else in the package can read, through the front end into Acquisition."""
    w = fe_world.world()
    fe = dpe.FrontEnd(fe_world.FS, "P2R", fe_world.WORLD_D, w["h"], gain=fe_world.WORLD_GAIN, f_if=fe_world.WORLD_IF)
    assert fe.fs_out == fe_world.WORLD_FS_OUT and fe.realised_if == fe_world.WORLD_IF
    iq = fe.convert(_device(w["raw"]), 0, 0, w["n_out"], record_length=w["S"])
    assert fe.clipped() == 0
    got = iq.cpu().numpy()
    band = fe_ref.band(w["y"], w["tol"])
    assert np.array_equal(got[~band], w["iq"][~band]) and np.abs(got.astype(np.int32) - w["iq"]).max() <= 1
    prns = [int(p) for p in w["ch"]["prn"]]
    acq = dpe.Acquisition(fe_world.WORLD_FS_OUT, w["n_out"], prns, fe_world.WORLD_BINS, mode="coherent")
    acq.search(iq)
    res = acq.results()
    for k, r in enumerate(res):
        assert r["prn"] == prns[k] and r["found"], r
        dist = abs((r["max_code_idx"] - w["truth_idx"][k] + 1250.0) % 2500.0 - 1250.0)
        assert dist <= 1.0, (r, w["truth_idx"][k])
        assert r["max_dopp_idx"] == w["truth_bin"][k], (r, w["ch"]["fi"][k])
    acq.close()
    fe.close()
