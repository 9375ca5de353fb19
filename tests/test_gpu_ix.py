"""GPU: the excisor (dpe_ix_*, engine.Excisor) against its fp64 specification tests/ix_ref.py, on the cases of tests/ix_world.py
(proven on the reference alone by tests/test_ix_ref_cpu.py).

Detection is tested on the device's own values through dpe_ix_analyse: P^ within delta of the reference, m^ the exact lower median
of P^, the mask exactly what P^, m^, the guard and the static mask give, and equal to the reference's at every decided bin.  The
output is tested against the reference synthesis given the device's masks: |device - reference| <= tol[n] at every value
(ix_ref: the two tolerance rules).  Each comparison prints the worst residual as a fraction of its bound before it asserts."""
import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from navlab_dpe_sdr_amd import frontend
from tests import ix_ref, ix_world

pytestmark = pytest.mark.gpu
GUARD = 12345


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


def _device(c):
    import torch
    host = ix_world.f32_pairs(c["x"]) if c["in_f32"] else ix_world.i16_bytes(c["x"])
    return torch.from_numpy(host).to("cuda")


def _excisor(c, out_f32, **kw):
    args = dict(guard=c["guard"], blank_power=c["blank_power"], gain=c["gain"], static_mask=c["static"], in_f32=c["in_f32"], out_f32=out_f32)
    args.update(kw)
    ix = dpe.Excisor(c["N"], c["kappa"], **args)
    assert ix.hop == c["N"] // 2 and ix.hops_per_block == ix_world.HOPS_PER_BLOCK and (ix.lead_hops, ix.tail_hops) == (1, 2)
    assert ix.lds_bytes <= 80 * 1024                                         # two blocks to a CU at every frame length
    return ix


def _masks(ix, c, x_dev):
    """the device's own e for the frames the case's outputs read"""
    H = c["H"]
    k0, k1 = c["out_first"] // H, (c["out_first"] + c["out_count"] - 1) // H + 1
    # (analyse needs the frames' whole input range, which is the needed range of the outputs)
    _, _, e = ix.analyse(x_dev, c["x_first"], k0, k1 - k0 + 1, record_length=c["record_length"])
    return e.cpu().numpy()


def _parity(c):
    """-> (fp32 output as float64, the excisor's stats): held to the reference given the device's masks"""
    x_dev = _device(c)
    ix = _excisor(c, True)
    assert ix.needed(c["out_first"], c["out_count"], c["record_length"]) == c["needed"]
    out = ix.process(x_dev, c["x_first"], c["out_first"], c["out_count"], record_length=c["record_length"])
    st = ix.stats()
    e = _masks(ix, c, x_dev)
    ix.close()
    ref, tol, F = ix_world.reference(c, masks=e)
    got = out.cpu().numpy().astype(np.float64)
    err = np.abs((got[0::2] + 1j * got[1::2]) - ref)
    # each component lies within tol of the reference's: |.| of the complex difference bounds both
    worst = float((err / np.maximum(tol, 1e-300)).max()) if np.any(tol > 0) else 0.0
    print("%s: worst |fp32 - reference| = %.3f of tol (tol up to %.3e)" % (c["name"], worst, tol.max()))
    assert np.all(err <= tol), c["name"]
    # statistics over the counted frames: those whose centre k H is an output
    H, k0 = c["H"], c["out_first"] // c["H"]
    ks = np.arange(k0, k0 + e.shape[0])
    counted = (ks * H >= c["out_first"]) & (ks * H < c["out_first"] + c["out_count"])
    assert st["frames"] == int(counted.sum()) and st["excisedBins"] == int(e[counted].sum()), (c["name"], st)
    assert np.array_equal(st["excisedPerBin"], e[counted].sum(axis=0)), c["name"]
    assert st["blanked"] == ix_world.blanked_count(c) and st["clipped"] == 0, (c["name"], st)
    return got, st, e, F


# ---- 1. analysis
@pytest.mark.parametrize("N", ix_world.SIZES)
def test_analysis(N):
    import torch
    a = ix_world.analysis_case(N)
    F = a["F"]
    ix = dpe.Excisor(N, a["kappa"], guard=a["guard"], static_mask=a["static"])
    x_dev = torch.from_numpy(ix_world.i16_bytes(a["x"])).to("cuda")
    P, m, e = (t.cpu().numpy() for t in ix.analyse(x_dev, a["x_first"], ix_world.ANALYSIS_FIRST, ix_world.ANALYSIS_FRAMES))
    ix.close()
    delta = ix_ref.power_tolerance(F, N)
    frac = np.abs(P.astype(np.float64) - F["P"]) / delta
    print("N %d: worst |P^ - P| = %.3f of delta" % (N, frac.max()))
    assert frac.max() <= 1.0
    assert P.dtype == np.float32 and np.array_equal(m, np.sort(P, axis=-1)[:, N // 2 - 1])
    own = ix_ref.widen(P > np.float32(a["kappa"]) * m[:, None], a["guard"], a["static"])
    assert np.array_equal(e != 0, own) and set(np.unique(e)) <= {0, 1}
    dec, _ = ix_ref.decided(F, N, a["kappa"], a["guard"], a["static"])
    assert np.array_equal((e != 0)[dec], F["e"][dec]) and dec.mean() >= 0.99


# ---- 2. parity of process
@pytest.mark.parametrize("name", ix_world.PARITY)
def test_parity(name):
    c = ix_world.case(name)
    got, st, e, F = _parity(c)
    if name.startswith("cross"):
        H = c["H"]
        assert (c["out_first"] + c["out_count"] - 1) // H - c["out_first"] // H + 1 > ix_world.HOPS_PER_BLOCK       # two blocks
    if name == "wrap bins 0 and N-1":
        assert e[:, [253, 254, 255, 0, 1, 2]].all()
    if name == "static mask alone":
        assert np.array_equal(e != 0, np.broadcast_to(c["static"] != 0, e.shape)) and st["excisedBins"] == 10 * st["frames"]
    if name == "pulse":
        assert st["blanked"] == 37
    if name == "nothing excised":
        assert not e.any() and st["excisedBins"] == 0
        a = c["out_first"] - c["x_first"]
        want = c["gain"] * ix_ref.interleave(c["x"][a:a + c["out_count"]])
        tol = ix_world.reference(c, masks=e)[1]
        assert np.all(np.abs(got - want) <= np.repeat(tol, 2))
    if name in ("tone between bins", "chirp", "negative gain", "fp32 input"):
        assert e.any(axis=-1).mean() > 0.5


# ---- 3. int16 output
def test_int16_output_is_the_rounded_fp32_output_and_clips_are_counted():
    c = ix_world.clip_case()
    x_dev = _device(c)
    res = {}
    for out_f32 in (True, False):
        ix = _excisor(c, out_f32)
        res[out_f32] = ix.process(x_dev, c["x_first"], c["out_first"], c["out_count"]).cpu().numpy()
        st = ix.stats()
        ix.close()
    f32, i16 = res[True], res[False]
    assert i16.dtype == np.int16 and np.array_equal(i16, ix_ref.quantise(f32))
    r = np.rint(f32)
    clipped = int(((r > 32767) | (r < -32768)).sum())
    assert st["clipped"] == clipped > 100 and i16.max() == 32767 and i16.min() == -32768


# ---- 4. record edges
@pytest.mark.parametrize("name", ix_world.EDGES)
def test_record_edges(name):
    c = ix_world.case(name)
    got, _, _, _ = _parity(c)
    ix = _excisor(c, False)
    i16 = ix.process(_device(c), c["x_first"], c["out_first"], c["out_count"], record_length=c["record_length"]).cpu().numpy()
    ix.close()
    assert np.array_equal(i16, ix_ref.quantise(got.astype(np.float32)))
    if name == "frames beyond the record":                   # frames 12 on hold nothing of the 333 samples: exact zeros from output 12 x 32 on
        assert np.all(got[2 * 384:] == 0.0) and np.all(i16[2 * 384:] == 0) and np.abs(got[:600]).max() > 1000
    if name == "record shorter than a hop":
        assert np.all(got[2 * 256:] == 0.0) and np.all(i16[2 * 256:] == 0)


# ---- 5. split property
@pytest.mark.parametrize("N", [64, 1024, 4096])
def test_split_property(N):
    import torch
    c = ix_world.case("cross N%d" % N)
    x_dev = _device(c)
    a, n, H = c["out_first"], c["out_count"], c["H"]
    edge = (a // H + ix_world.HOPS_PER_BLOCK) * H - a           # the first output of the second block, counted from a
    splits = ([0, 2 * H - a % H, n], [0, 2 * H - a % H + H // 3, n], [0] + list(range(edge - 2, edge + 3)) + [n])
    for out_f32 in (True, False):
        ix = _excisor(c, out_f32)
        one = ix.process(x_dev, c["x_first"], a, n)
        whole = ix.stats()
        assert whole["frames"] == ix_world.HOPS_PER_BLOCK + 1 and whole["excisedBins"] > 0
        for cuts in splits:
            parts, total = [], None
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                parts.append(ix.process(x_dev, c["x_first"], a + lo, hi - lo))
                st = ix.stats()
                total = st if total is None else {k: total[k] + st[k] for k in st}
            assert torch.equal(one.view(torch.int32), torch.cat(parts).view(torch.int32)), (N, out_f32, cuts)
            assert all(np.array_equal(total[k], whole[k]) for k in whole), (N, out_f32, cuts)
        ix.close()


# ---- 6. large indices
def test_large_indices():
    c = ix_world.case("large indices")
    assert c["out_first"] + c["out_count"] == 2 ** 55 - 3
    _parity(c)
    ix = _excisor(c, True)
    with pytest.raises(dpe.DpeError, match=r"\[Excisor\] process: first output \d+ with 700 outputs outside 0\.\.2\^55"):
        ix.process(_device(c), c["x_first"], 2 ** 55 - 699, 700)
    ix.close()


# ---- 7. side stream, stray stores, refusals
@pytest.mark.parametrize("out_f32", [True, False])
def test_side_stream_and_guard_values(out_f32):
    import torch
    c = ix_world.case("tone between bins")
    x_dev = _device(c)
    ix = _excisor(c, out_f32)
    dtype = torch.float32 if out_f32 else torch.int16
    want = ix.process(x_dev, c["x_first"], c["out_first"], c["out_count"])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    n = 2 * c["out_count"]
    for pair in range(2 if out_f32 else 4):                  # every offset within 16 bytes an I/Q pair may start at
        buf = torch.full((n + 64,), GUARD, dtype=dtype, device="cuda")
        torch.cuda.synchronize()
        off = 16 + 2 * pair
        ix.process(x_dev, c["x_first"], c["out_first"], c["out_count"], out=buf[off:off + n], stream=side)
        side.synchronize()
        assert torch.equal(buf[off:off + n], want) and bool((buf[:off] == GUARD).all()) and bool((buf[off + n:] == GUARD).all()), pair
    before = ix.stats()
    out = torch.full((n + 8,), GUARD, dtype=dtype, device="cuda")

    def refused(pattern, *args, **kw):
        with pytest.raises(dpe.DpeError, match=pattern) as e:
            ix.process(*args, **kw)
        assert str(e.value).startswith("[Excisor] ")
        torch.cuda.synchronize()
        assert bool((out == GUARD).all())
        after = ix.stats()
        assert all(np.array_equal(after[k], before[k]) for k in before)

    lo, hi = c["needed"]
    refused(r"need the input samples %d\.\.%d, the buffer holds %d\.\.%d" % (lo, hi - 1, lo + 1, lo + c["x"].size), x_dev, c["x_first"] + 1, c["out_first"],
            c["out_count"], out=out)
    refused(r"the buffer holds %d\.\.%d" % (lo, hi - 2), x_dev, c["x_first"], c["out_first"], c["out_count"], x_count=c["x"].size - 1, out=out)
    refused(r"output is not aligned to an I/Q pair", x_dev, c["x_first"], c["out_first"], c["out_count"], out=out[1:])
    refused(r"input is not aligned to an I/Q pair", x_dev[1:], c["x_first"], c["out_first"], c["out_count"], x_count=c["x"].size, out=out)
    refused(r"0 outputs outside 1\.\.2\^30", x_dev, c["x_first"], c["out_first"], 0, out=out)
    refused(r"null input buffer", 0, c["x_first"], c["out_first"], c["out_count"], x_count=c["x"].size, out=out)
    refused(r"record length -2", x_dev, c["x_first"], c["out_first"], c["out_count"], record_length=-2, out=out)
    with pytest.raises(dpe.DpeError, match=r"\[Excisor\] analyse: frames 0\.\.0 need the input samples 0\.\.127"):
        ix.analyse(x_dev, c["x_first"], 0, 1)
    ix.close()


# ---- 8. behind the front end, piece by piece
def test_convert_file_excised_equals_one_call_each(tmp_path):
    import torch
    rng = np.random.Generator(np.random.PCG64(8))
    n, D = 20011, 2
    x = ix_world.to_i16(ix_world.noise(9, n, 1500) + ix_world.tone(0, n, 0.0731, 9000.0))
    raw = ix_world.i16_bytes(x)
    path = tmp_path / "record.bin"
    path.write_bytes(raw.tobytes())
    fe = dpe.FrontEnd(5e6, "I16C", D, frontend.design_lowpass(D), gain=0.9)
    ix = dpe.Excisor(256, 10.0, guard=1)
    n_out = -(-n // D)
    plain = list(frontend.convert_file(str(path), fe, 997))
    mid = fe.convert(torch.from_numpy(raw).to("cuda"), 0, 0, n_out, record_length=n)
    assert torch.equal(torch.cat(plain), mid)                                     # without an excisor: the bytes of before
    pieces = list(frontend.convert_file(str(path), frontend.Excised(fe, ix), 997))
    assert [p.numel() // 2 for p in pieces] == [997] * 10 + [n_out - 9970]
    one = ix.process(mid, 0, 0, n_out, record_length=n_out)
    st = ix.stats()
    assert torch.equal(one, torch.cat(pieces)) and st["excisedBins"] > st["frames"] > 70
    assert not torch.equal(one, mid)
    ix.close()
    fe.close()


# ---- 9. end to end
def _acquire(iq_dev, w):
    prns = [int(p) for p in w["ch"]["prn"]]
    acq = dpe.Acquisition(ix_world.WORLD_FS, ix_world.WORLD_S, prns, ix_world.WORLD_BINS, mode="coherent")
    acq.search(iq_dev)
    good = []
    for k, r in enumerate(acq.results()):
        dist = abs((r["max_code_idx"] - w["truth_idx"][k] + 1250.0) % 2500.0 - 1250.0)
        good.append(bool(r["found"]) and dist <= 1.0 and r["max_dopp_idx"] == w["truth_bin"][k])
    acq.close()
    return good


def test_jammed_world_is_acquired_after_excision():
    import torch
    from tests import fe_world
    assert np.array_equal(ix_world.WORLD_BINS, fe_world.WORLD_BINS)
    w = ix_world.world()
    jammed = torch.from_numpy(w["jammed"]).to("cuda")
    assert sum(_acquire(jammed, w)) <= 1
    ix = dpe.Excisor(1024, 10.0, guard=1)
    clean = ix.process(jammed, 0, 0, ix_world.WORLD_S, record_length=ix_world.WORLD_S)
    st = ix.stats()
    ix.close()
    assert all(_acquire(clean, w))
    # the tone's bin is excised in every frame (so are its neighbours under the window's skirt: the maximum is a plateau)
    per, peak = st["excisedPerBin"], round(ix_world.TONE * 1024)
    assert st["frames"] == -(-ix_world.WORLD_S // 512) and per[peak] == per.max() == st["frames"]
    assert 0.005 < st["excisedBins"] / (st["frames"] * 1024.0) < 0.05
