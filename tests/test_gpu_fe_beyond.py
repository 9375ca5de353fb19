"""GPU: the front end beyond what tests/test_gpu_fe.py holds constant, on the cases of fe_world.BEYOND (proven on the reference alone
by tests/test_fe_beyond_cpu.py): taps without symmetry, 2-bit levels other than the default, phases of up to 1023 taps and the
smallest tile, the IF words 2^31, 0 from +-fs, 1 and 2^32 - 1, the last output indices the interface takes, a record that ends in a
later tile with whole tiles beyond it, buffers wider than needed on both sides, every promised alignment of input and output with
guard values around the output, the clip count call after call, a side stream, and a negative and a zero gain.

The acceptance rule is tests/test_gpu_fe.py's (_accept): fp32 within the derived tol, int16 equal outside the rounding band and
within 1 inside it, int16 exactly clip(rint(.)) of the device's own fp32.  Each case prints its worst residual as a fraction of tol."""
import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import fe_ref, fe_world
from tests.test_gpu_fe import GUARD, _accept, _convert, _device, _fe

pytestmark = pytest.mark.gpu
INC = fe_world.INCOMMENSURATE * fe_world.FS


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


def _names(prefix):
    return [n for n in fe_world.BEYOND if n.startswith(prefix)]


def _bits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _guarded(count, out_f32, offset_bytes=0):
    """-> (buffer of guard values, the slice for 2 count output values that starts offset_bytes past a 16-byte boundary, its start)"""
    import torch
    dt = torch.float32 if out_f32 else torch.int16
    buf = torch.full((2 * count + 128,), GUARD, dtype=dt, device="cuda")
    at = 64 + offset_bytes // buf.element_size()
    out = buf[at:at + 2 * count]
    assert buf.data_ptr() % 16 == 0 and out.data_ptr() % 16 == offset_bytes % 16
    return buf, out, at


def _guard_intact(buf, at, count):
    return bool((buf[:at] == GUARD).all()) and bool((buf[at + 2 * count:] == GUARD).all())


# ---- 1 .. 5, 11: cases for the acceptance rule as they stand
@pytest.mark.parametrize("name", _names("asym ") + _names("levels ") + _names("long ") + _names("if ") + ["top", "negative gain"])
def test_beyond_accepted(name):
    c = fe_world.beyond_case(name)
    fe = _fe(c, False)
    assert fe.tile_outputs == c["tile"] and fe.lds_bytes == fe_world.lds_bytes(c["D"], c["T"], c["fmt"] in fe_ref.REAL)
    if name.startswith("long ") and c["D"] == 64:
        assert fe.tile_outputs == 45
    d = c["delta"]
    assert fe.delta == d and fe.realised_if == d * fe_world.FS / 4294967296.0 - (fe_world.FS if d > 2 ** 31 else 0.0)
    if c["if_spec"] in ("+fs", "-fs"):
        assert fe.delta == 0
    if c["if_spec"] in ("+n", "-n"):
        assert fe.delta == 2 ** 31 and fe.realised_if == fe_world.FS / 2
    if c["if_spec"] == "-1":
        assert fe.delta == 2 ** 32 - 1 and fe.realised_if == -fe_world.FS / 4294967296.0
    fe.close()
    _accept(c, "beyond: " + name)


def test_one_output_past_the_top_is_refused():
    import torch
    c = fe_world.beyond_case("top")
    assert c["out_first"] + c["out_count"] == 2 ** 55
    fe = _fe(c, False)
    buf, out, at = _guarded(c["out_count"] + 1, False)
    with pytest.raises(dpe.DpeError, match=r"\[FrontEnd\] convert: first output \d+ with 201 outputs outside 0\.\.2\^55"):
        fe.convert(_device(c["raw"]), c["raw_first"], c["out_first"], c["out_count"] + 1, raw_count=c["raw_count"], out=out)
    torch.cuda.synchronize()
    assert bool((buf == GUARD).all())
    fe.close()


# ---- 6. record edges across tiles
@pytest.mark.parametrize("name", _names("edges "))
def test_record_edges_across_tiles(name):
    """Zeros before sample 0, the record's end inside tile 1, tiles 2 and 3 wholly beyond it: one call."""
    c = fe_world.beyond_case(name)
    assert c["out_first"] == 0 and c["raw_first"] + c["raw_count"] == c["record_length"]
    _accept(c, "beyond: " + name)
    beyond = np.repeat(np.arange(c["out_count"]) * c["D"] - (c["T"] - 1) // 2 >= c["record_length"], 2)
    assert beyond[4 * c["tile"]:].all() and not beyond[:2 * c["tile"]].any()                      # tiles 2 and 3 wholly, tile 0 not at all
    f32, _ = _convert(c, True)
    i16, clipped = _convert(c, False)
    assert np.all(i16[beyond] == 0) and np.all(f32[beyond] == 0) and clipped == 0                  # (-0.0 equals 0)


@pytest.mark.parametrize("fmt,D,T", [("I16C", 4, 33), ("P2R", 3, 25)])
def test_all_outputs_beyond_the_record(fmt, D, T):
    """Every output's window begins at or beyond the record's length: whatever valid buffer comes with the call, nothing of it is
    read, the output is zeros and nothing clips -- also where the buffer holds samples at the very indices the windows cover."""
    import torch
    length, T0 = 1000, (T - 1) // 2
    first = -(-(length + T0) // D)
    tile = fe_world.tile_outputs(D, T, fmt in fe_ref.REAL)
    count = tile + 7
    assert first * D - T0 >= length
    rng = np.random.Generator(np.random.PCG64(17))
    for out_f32 in (False, True):
        fe = dpe.FrontEnd(fe_world.FS, fmt, D, fe_world.taps(D, T), gain=fe_world.GAIN[fmt], f_if=INC, out_f32=out_f32)
        for raw_first, n in ((0, 16), (length + 4000, 64), (first * D - first * D % 4, (count + 8) * D)):
            raw = _device(fe_ref.random_record(fmt, n, rng, amp16=30000))
            buf, out, at = _guarded(count, out_f32)
            fe.convert(raw, raw_first, first, count, record_length=length, raw_count=n, out=out)
            assert fe.clipped() == 0
            assert bool((out == 0).all()) and _guard_intact(buf, at, count), (out_f32, raw_first)
        fe.close()


# ---- 7. buffers wider than needed
@pytest.mark.parametrize("name", _names("wide "))
def test_buffers_wider_than_needed(name):
    import torch
    c = fe_world.beyond_case(name)
    num, den = fe_ref.BYTES[c["fmt"]]
    raw = _device(c["raw"])
    b0 = c["pad_before"] * num // den
    tight = raw[b0:b0 + -(-c["need_count"] * num // den)]
    assert c["pad_before"] == 4 * 517 and c["pad_after"] == 2 * c["T"] + 13 and c["raw_count"] == c["need_count"] + c["pad_before"] + c["pad_after"]
    for out_f32 in (False, True):
        fe = _fe(c, out_f32)
        wide = fe.convert(raw, c["raw_first"], c["out_first"], c["out_count"], record_length=c["record_length"], raw_count=c["raw_count"])
        exact = fe.convert(tight, c["need_first"], c["out_first"], c["out_count"], record_length=c["record_length"], raw_count=c["need_count"])
        assert torch.equal(_bits(wide), _bits(exact)), (name, out_f32)
        fe.close()
    _accept(c, "beyond: " + name)


# ---- 8. alignment and stray stores
ALIGN_IN = {"I8R": (1, 2, 3, 5), "ARGPI4": (1, 2, 3, 5), "P2R": (1, 2, 3, 5), "P2C": (1, 2, 3, 5), "I8C": (2, 6), "I16R": (2, 6), "I16C": (4, 8, 12)}


def _shifted(raw_dev, offset):
    """The same bytes, offset bytes past a 16-byte boundary."""
    import torch
    n = raw_dev.numel()
    buf = torch.zeros(n + 32, dtype=torch.uint8, device="cuda")
    buf[offset:offset + n] = raw_dev
    assert buf.data_ptr() % 16 == 0
    return buf[offset:offset + n]


@pytest.mark.parametrize("fmt", fe_ref.FORMATS)
def test_alignment_and_stray_stores(fmt):
    """Input at every offset a sample may start at, output at every offset an I/Q pair may start at, guard values on both sides of
    the output: the bytes of the aligned call, and nothing stored outside the 2 out_count values."""
    import torch
    c = fe_world.beyond_case("align " + fmt)
    assert c["out_count"] == c["tile"] + 1 and c["out_count"] % 5 != 0
    base = _device(c["raw"])
    moved = [(off, _shifted(base, off)) for off in ALIGN_IN[fmt]]
    for count in (c["out_count"], 13):
        for out_f32 in (False, True):
            fe = _fe(c, out_f32)
            want = fe.convert(base, c["raw_first"], c["out_first"], count, raw_count=c["raw_count"])
            for off_in, raw in moved:
                for off_out in ((8,) if out_f32 else (4, 8, 12)):
                    buf, out, at = _guarded(count, out_f32, off_out)
                    fe.convert(raw, c["raw_first"], c["out_first"], count, raw_count=c["raw_count"], out=out)
                    assert torch.equal(_bits(out), _bits(want)), (fmt, count, out_f32, off_in, off_out)
                    assert _guard_intact(buf, at, count), (fmt, count, out_f32, off_in, off_out)
            fe.close()
    _accept(c, "beyond: align " + fmt)


def test_misaligned_buffers_are_refused():
    import torch
    c = fe_world.beyond_case("align I16C")
    count = 13
    base = _device(c["raw"])

    def refused(fe, pattern, raw, buf, out):
        with pytest.raises(dpe.DpeError, match=pattern) as e:
            fe.convert(raw, c["raw_first"], c["out_first"], count, raw_count=c["raw_count"], out=out)
        assert str(e.value).startswith("[FrontEnd] convert: ")
        torch.cuda.synchronize()
        assert bool((buf == GUARD).all())

    for out_f32 in (False, True):
        fe = _fe(c, out_f32)
        buf, out, at = _guarded(count, out_f32)
        refused(fe, r"the input is not aligned to a sample \(4 bytes\)", _shifted(base, 2), buf, out)
        refused(fe, r"the input is not aligned to a sample \(4 bytes\)", _shifted(base, 13), buf, out)
        refused(fe, r"the output is not aligned to an I/Q pair \(%d bytes\)" % (8 if out_f32 else 4), base, buf, buf[at + 1:at + 1 + 2 * count])
        fe.close()
    c8 = fe_world.beyond_case("align I8C")
    fe = _fe(c8, False)
    buf, out, at = _guarded(count, False)
    with pytest.raises(dpe.DpeError, match=r"the input is not aligned to a sample \(2 bytes\)"):
        fe.convert(_shifted(_device(c8["raw"]), 3), c8["raw_first"], c8["out_first"], count, raw_count=c8["raw_count"], out=out)
    torch.cuda.synchronize()
    assert bool((buf == GUARD).all())
    fe.close()


# ---- 9. the clip counter
def test_clip_count_is_per_call():
    """One handle, a clipping call, a quiet one, the clipping one again: the count is the last call's own."""
    c = fe_world.saturation_case()
    n, want = c["out_count"], fe_ref.clip_count(c["y"])
    loud = _device(c["raw"])
    quiet = _device((c["raw"].view("<i2") // 8).astype("<i2"))                  # |3 x| <= 7 690
    fe = _fe(c, False)
    counts = []
    for raw in (loud, quiet, loud):
        fe.convert(raw, 0, 0, n)
        counts.append(fe.clipped())
    assert want > 0 and counts == [want, 0, want], counts
    fe.close()
    fe = _fe(c, True)
    fe.convert(loud, 0, 0, n)
    assert fe.clipped() == 0
    fe.close()


def test_clip_count_of_a_filtered_mixed_case():
    """The count equals the components of the device's own fp32 output whose rint lies beyond a rail, and lies between the
    reference's counts taken tol outside and tol inside the rails (the only things compared to the reference here)."""
    c = fe_world.beyond_case("clip I8C")
    f32, none = _convert(c, True)
    i16, clipped = _convert(c, False)
    r = np.rint(f32)
    lower, upper = fe_world.clip_bounds(c)
    print("clip case: the device counts %d, the reference between %d and %d" % (clipped, lower, upper))
    assert none == 0 and clipped == int(((r < -32768) | (r > 32767)).sum()) and lower <= clipped <= upper
    assert np.array_equal(i16, np.clip(r, -32768, 32767).astype(np.int16)) and i16.max() == 32767 and i16.min() == -32768


# ---- 10. a side stream
def test_side_stream():
    """Upload and conversion on a stream of their own; clipped() synchronises with it."""
    import torch
    c = fe_world.saturation_case()
    n = c["out_count"]
    fe = _fe(c, False)
    want = fe.convert(_device(c["raw"]), 0, 0, n)
    count = fe.clipped()
    out = torch.full((2 * n,), GUARD, dtype=torch.int16, device="cuda")
    host = torch.from_numpy(c["raw"].copy())
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.current_stream().cuda_stream
    with torch.cuda.stream(side):
        raw = host.to("cuda", non_blocking=True)
    fe.convert(raw, 0, 0, n, out=out, stream=side)
    assert fe.clipped() == count > 0
    assert torch.equal(out, want)
    fe.close()


# ---- 11. gain zero (the negative gain is among the accepted cases)
def test_gain_zero_gives_zeros():
    c = dict(fe_world.beyond_case("negative gain"), gain=0.0)
    for out_f32 in (False, True):
        fe = _fe(c, out_f32)
        buf, out, at = _guarded(c["out_count"], out_f32)
        fe.convert(_device(c["raw"]), c["raw_first"], c["out_first"], c["out_count"], raw_count=c["raw_count"], out=out)
        assert fe.clipped() == 0 and bool((out == 0).all()) and _guard_intact(buf, at, c["out_count"])
        fe.close()
