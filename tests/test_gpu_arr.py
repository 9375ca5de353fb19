"""GPU: the array combiner (dpe_arr_*, engine.ArrayCombiner) against its specification tests/arr_ref.py, on the cases of
tests/arr_world.py (proven on the reference alone by tests/test_arr_ref_cpu.py).

The covariance is tested exactly through dpe_arr_analyse: every int64 entry equals numpy's integer sum.  The weights are tested on
the device's own S: ||w^ - w||_2 <= 100 M^2 kappa_2(R) 2^-53 ||w||_2 against numpy.linalg.solve, and v^ = fp32(gain conj(w^))
exactly.  The output is tested against the reference apply given the device's v: |y^ - y| <= tol per component (arr_ref: the FMA
chain's bound), and the int16 output equals rint of the reference wherever that is farther than tol from a rounding boundary and is
within 1 elsewhere.  Each comparison prints the worst residual as a fraction of its bound before it asserts."""
import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests import arr_ref, arr_world

pytestmark = pytest.mark.gpu
GUARD = 12345


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


def _device(x):
    import torch
    return torch.from_numpy(arr_world.i16_rows(x)).to("cuda")


def _combiner(c, output, **kw):
    args = dict(constraints=c["cons"] if c["explicit"] else None, reference=c["reference"], loading=c["loading"], gain=c["gain"], output=output)
    args.update(kw)
    arr = dpe.ArrayCombiner(c["M"], c["L"], **args)
    info = arr.info()
    assert info == dict(block_length=c["L"], blocks_per_unit=arr_world.unit_blocks(c["L"]), lds_bytes=arr.lds_bytes, min_samples=2 * c["M"])
    assert arr.lds_bytes <= 64 * 1024 and arr.B == c["B"]
    return arr


def _check_weights(name, S, w, v, count, cons, loading, gain):
    """the device's w and v [blocks, B, M, 2] against numpy's solve on the device's own S; -> the worst fraction of the bound"""
    M = S.shape[1]
    ref, fb, kappa = arr_ref.weights(S, count, cons, loading)
    wc = w[..., 0] + 1j * w[..., 1]
    worst = 0.0
    for k in range(S.shape[0]):
        for b in range(ref.shape[1]):
            if fb[k, b]:
                assert np.allclose(wc[k, b], ref[k, b], rtol=4 * (M + 1) * arr_ref.U64, atol=0.0), (name, k, b)      # c / (c^H c): a 2 M-term sum and a division on either side
                continue
            bound = 100.0 * M * M * kappa[k] * arr_ref.U64 * np.linalg.norm(ref[k, b])
            worst = max(worst, np.linalg.norm(wc[k, b] - ref[k, b]) / bound)
    print("%s: worst ||w^ - w|| = %.4f of the bound (kappa up to %.1f)" % (name, worst, np.nanmax(kappa) if np.any(~np.isnan(kappa)) else 0.0))
    assert worst <= 1.0, name
    assert v.dtype == np.float32 and np.array_equal(v, arr_ref.applied(wc, gain)), name
    return fb


def _parity(c):
    """both output formats of a case held to the reference apply given the device's v; -> (fp32 output, stats, fallback [blocks, B])"""
    x_dev = _device(c["x"])
    L, a, n = c["L"], c["out_first"], c["out_count"]
    k0, k1 = a // L, (a + n - 1) // L
    res = {}
    for output in ("f32", "i16"):
        arr = _combiner(c, output)
        assert arr.needed(a, n, c["record_length"]) == c["needed"]
        out = arr.process(x_dev, c["x_first"], a, n, record_length=c["record_length"])
        res[output] = (np.stack([t.cpu().numpy() for t in out]), arr.stats())
        if output == "f32":
            S, w, v = (t.cpu().numpy() for t in arr.analyse(x_dev, c["x_first"], k0, k1 - k0 + 1, record_length=c["record_length"]))
        arr.close()
    xb, count = arr_ref.blocks_of(c["x"], c["x_first"], c["record_length"], k0, k1 - k0 + 1, L)
    assert S.dtype == np.int64 and np.array_equal(S, arr_ref.covariance(xb)), c["name"]
    fb = _check_weights(c["name"], S, w, v, count, c["cons"], c["loading"], c["gain"])
    y, tol = arr_ref.combine(c["x"], c["x_first"], c["record_length"], a, n, L, v)
    want = np.stack([arr_ref.interleave(row) for row in y])
    tol = tol.reshape(tol.shape[0], -1)
    f32, st = res["f32"]
    err = np.abs(f32.astype(np.float64) - want)
    worst = float((err[tol > 0] / tol[tol > 0]).max()) if np.any(tol > 0) else 0.0
    print("%s: worst |fp32 - reference| = %.3f of tol (tol up to %.3e)" % (c["name"], worst, tol.max()))
    assert f32.dtype == np.float32 and np.all(err <= tol), c["name"]
    i16, st16 = res["i16"]
    decided = arr_ref.boundary_distance(want) > tol
    exact = arr_ref.quantise(want)
    assert i16.dtype == np.int16 and np.array_equal(i16[decided], exact[decided]) and np.abs(i16.astype(np.int64) - exact).max() <= 1, c["name"]
    assert np.array_equal(i16, arr_ref.quantise(f32))                    # the int16 output is the rounded fp32 output
    blocks = arr_ref.counted(a, n, L, c["record_length"])
    want_st = dict(blocks=len(blocks), fallbackBlocks=int(sum(fb[k - k0].any() for k in blocks)), clipped=0)
    assert st == want_st and st16 == want_st, (c["name"], st, st16, want_st)
    return f32, st, fb


# ---- 1. covariance, exactly
def _analyse(c, **kw):
    arr = dpe.ArrayCombiner(c["M"], c["L"], **kw)
    S, w, v = (t.cpu().numpy() for t in arr.analyse(_device(c["x"]), c["x_first"], c["block_first"], c["block_count"], record_length=c["record_length"]))
    arr.close()
    xb, count = arr_ref.blocks_of(c["x"], c["x_first"], c["record_length"], c["block_first"], c["block_count"], c["L"])
    return S, w, v, arr_ref.covariance(xb), count


@pytest.mark.parametrize("M,L", arr_world.COV_SHAPES)
def test_covariance_exact_and_weights(M, L):
    c = arr_world.cov_case(M, L)
    for loading in (0.0, 1e-3):
        S, w, v, want, count = _analyse(c, loading=loading, reference=M - 1, gain=-1.5)
        assert S.dtype == np.int64 and np.array_equal(S, want)
        assert count[-1] == L - L // 3                                   # the record ends inside the last block
        _check_weights("cov M%d L%d loading %g" % (M, L, loading), S, w, v, count, arr_ref.unit_vector(M, M - 1), loading, -1.5)


@pytest.mark.parametrize("kind", ["floor", "alternating"])
def test_covariance_exact_at_the_extremes(kind):
    c = arr_world.extreme(kind)
    S, w, v, want, count = _analyse(c)
    assert np.array_equal(S, want)
    if kind == "floor":
        assert np.all(S[..., 0] == 2 ** 47) and np.all(S[..., 1] == 0)
    else:
        assert np.abs(S).max() > 2 ** 38 and S[..., 1].any()
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(v))


# ---- 2. weights and output
@pytest.mark.parametrize("name", arr_world.PARITY)
def test_parity(name):
    c = arr_world.case(name)
    f32, st, fb = _parity(c)
    assert not fb.any() and st["blocks"] >= 1
    if "cross" in name:
        assert (c["out_first"] + c["out_count"] - 1) // c["L"] - c["out_first"] // c["L"] + 1 > arr_world.unit_blocks(c["L"])      # two workgroups
    if name == "M4 L1024 last reference, no loading":                    # the interferer is gone from the output
        a = c["out_first"] - c["x_first"]
        assert np.sqrt(np.mean(np.abs(c["x"][3, a:a + c["out_count"]]) ** 2)) > 8000 and np.sqrt(2.0 * np.mean(f32.astype(np.float64) ** 2)) < 2500


# ---- 3. clipping
def test_clipped_components_are_counted():
    c = arr_world.clip_case()
    x_dev = _device(c["x"])
    res = {}
    for output in ("f32", "i16"):
        arr = _combiner(c, output)
        res[output] = arr.process(x_dev, c["x_first"], c["out_first"], c["out_count"])[0].cpu().numpy()
        st = arr.stats()
        arr.close()
    f32, i16 = res["f32"], res["i16"]
    assert np.array_equal(i16, arr_ref.quantise(f32))
    r = np.rint(f32)
    clipped = int(((r > 32767) | (r < -32768)).sum())
    assert st["clipped"] == clipped and 0.1 < clipped / r.size < 0.5 and i16.max() == 32767 and i16.min() == -32768


# ---- 4. edges
@pytest.mark.parametrize("name", arr_world.EDGES)
def test_edges(name):
    c = arr_world.case(name)
    f32, st, fb = _parity(c)
    L, M = c["L"], c["M"]
    if name == "record shorter than 2M":                      # everything is fallback: the reference element alone, zeros beyond the record
        assert fb.all() and st == dict(blocks=1, fallbackBlocks=1, clipped=0)
        assert np.array_equal(f32[0, :14], arr_ref.interleave(c["x"][0, :7]).astype(np.float32)) and np.all(f32[:, 14:] == 0.0)
    if name == "record ends inside a block":
        assert not fb.any() and np.all(f32[:, 2 * (777 - 100):] == 0.0) and st["blocks"] == 3
    if name == "record ends 2M-1 into a block":
        assert fb[:, 0].tolist() == [False, False, True] and st == dict(blocks=3, fallbackBlocks=1, clipped=0)
    if name == "large indices":
        assert c["out_first"] + c["out_count"] == 2 ** 55 - 3
        arr = _combiner(c, "f32")
        with pytest.raises(dpe.DpeError, match=r"\[ArrayCombiner\] process: first output \d+ with 700 outputs outside 0\.\.2\^55"):
            arr.process(_device(c["x"]), c["x_first"], 2 ** 55 - 699, 700)
        arr.close()
    if name == "zero block":                                  # fallback, counted, and the neighbours as without it
        assert fb[:, 0].tolist() == [False, True, False] and st == dict(blocks=3, fallbackBlocks=1, clipped=0)
        assert np.all(f32[:, 2 * L:4 * L] == 0.0) and np.abs(f32[:, :2 * L]).max() > 100 and np.abs(f32[:, 4 * L:]).max() > 100


# ---- 5. split property and additive statistics
@pytest.mark.parametrize("name", ["M2 L256 cross", "M8 L256 three constraints, loading 1", "M2 L4096 cross", "zero block"])
def test_split_property(name):
    import torch
    c = arr_world.case(name)
    x_dev = _device(c["x"])
    a, n, L = c["out_first"], c["out_count"], c["L"]
    ub = arr_world.unit_blocks(L)
    edge = (a // L + 1) * L - a                                 # the first output of the call's second block, counted from a
    share = (a // L + ub) * L - a                               # the first output of the second workgroup's share
    splits = [[0, edge, n], [0, edge + L // 3, n], [0] + list(range(edge - 2, edge + 3)) + [n]]
    if share < n:
        splits += [[0, share, n], [0] + list(range(share - 2, share + 3)) + [n]]
    for output in ("f32", "i16"):
        arr = _combiner(c, output, gain=c["gain"] * (9.0 if output == "i16" else 1.0))       # (a gain at which int16 components of the M2 cases clip)
        one = arr.process(x_dev, c["x_first"], a, n)
        whole = arr.stats()
        assert whole["blocks"] == len(arr_ref.counted(a, n, L)) and (output == "f32" or not name.startswith("M2") or whole["clipped"] > 0)
        for cuts in splits:
            parts, total = [[] for _ in range(c["B"])], None
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                for b, t in enumerate(arr.process(x_dev, c["x_first"], a + lo, hi - lo)):
                    parts[b].append(t)
                st = arr.stats()
                total = st if total is None else {k: total[k] + st[k] for k in st}
            for b in range(c["B"]):
                assert torch.equal(one[b].view(torch.int32), torch.cat(parts[b]).view(torch.int32)), (name, output, cuts, b)
            assert total == whole, (name, output, cuts, total, whole)
        arr.close()


# ---- 6. side stream, stray stores, refusals
@pytest.mark.parametrize("output", ["f32", "i16"])
def test_side_stream_guard_values_and_refusals(output):
    import torch
    c = arr_world.case("M8 L256 three constraints, loading 1")
    x_dev = _device(c["x"])
    arr = _combiner(c, output)
    dtype = torch.float32 if output == "f32" else torch.int16
    a, n = c["out_first"], c["out_count"]
    want = arr.process(x_dev, c["x_first"], a, n)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    bufs = [torch.full((2 * n + 64,), GUARD, dtype=dtype, device="cuda") for _ in range(c["B"])]
    torch.cuda.synchronize()
    offs = [16 + 2 * b for b in range(c["B"])]
    arr.process(x_dev, c["x_first"], a, n, out=[buf[off:off + 2 * n] for buf, off in zip(bufs, offs)], stream=side)
    side.synchronize()
    for b, (buf, off) in enumerate(zip(bufs, offs)):
        assert torch.equal(buf[off:off + 2 * n], want[b]) and bool((buf[:off] == GUARD).all()) and bool((buf[off + 2 * n:] == GUARD).all()), b
    before = arr.stats()
    outs = [torch.full((2 * n + 8,), GUARD, dtype=dtype, device="cuda") for _ in range(c["B"])]
    rows = list(x_dev)

    def refused(pattern, *args, **kw):
        kw.setdefault("out", [o[:2 * n] for o in outs])
        with pytest.raises(dpe.DpeError, match=pattern) as e:
            arr.process(*args, **kw)
        assert str(e.value).startswith("[ArrayCombiner] ")
        torch.cuda.synchronize()
        assert all(bool((o == GUARD).all()) for o in outs) and arr.stats() == before

    lo, hi = c["needed"]
    size = c["x"].shape[1]
    refused(r"need the input samples %d\.\.%d, the buffers hold %d\.\.%d" % (lo, hi - 1, lo + 1, lo + size), rows, c["x_first"] + 1, a, n)
    refused(r"the buffers hold %d\.\.%d" % (lo, hi - 2), rows, c["x_first"], a, n, x_count=size - 1)
    refused(r"null input buffer of element 5", rows[:5] + [0] + rows[6:], c["x_first"], a, n, x_count=size)
    refused(r"null output buffer of constraint 1", rows, c["x_first"], a, n, out=[outs[0][:2 * n], 0, outs[2][:2 * n]])
    refused(r"input of element 2 is not aligned to an I/Q pair", rows[:2] + [rows[2][1:]] + rows[3:], c["x_first"], a, n, x_count=size - 1)
    refused(r"output of constraint 0 is not aligned to an I/Q pair", rows, c["x_first"], a, n, out=[outs[0][1:2 * n + 1]] + [o[:2 * n] for o in outs[1:]])
    refused(r"0 outputs outside 1\.\.2\^30", rows, c["x_first"], a, 0)
    refused(r"record length -2", rows, c["x_first"], a, n, record_length=-2)
    # an output range inside an input buffer: out-of-place only
    inside = rows[4].view(dtype)[: (2 * n if output == "i16" else 2 * 200)]
    refused(r"output of constraint 2 overlaps the input of element 4", rows, c["x_first"], a, n if output == "i16" else 200,
            out=[outs[0][:2 * n], outs[1][:2 * n], inside])
    with pytest.raises(dpe.DpeError, match=r"\[ArrayCombiner\] analyse: blocks 0\.\.0 need the input samples 0\.\.255"):
        arr.analyse(rows, c["x_first"], 0, 1)
    with pytest.raises(dpe.DpeError, match=r"\[ArrayCombiner\] 7 input buffers for 8 elements"):
        arr.process(rows[:7], c["x_first"], a, n)
    assert arr.stats() == before and bool(torch.equal(_device(c["x"]), x_dev))
    arr.close()


# ---- 7. end to end
def _acquire(iq_dev, w):
    prns = [int(p) for p in w["ch"]["prn"]]
    acq = dpe.Acquisition(arr_world.WORLD_FS, arr_world.WORLD_S, prns, arr_world.WORLD_BINS, mode="coherent")
    acq.search(iq_dev)
    good = []
    for k, r in enumerate(acq.results()):
        dist = abs((r["max_code_idx"] - w["truth_idx"][k] + 1250.0) % 2500.0 - 1250.0)
        good.append(bool(r["found"]) and dist <= 1.0 and r["max_dopp_idx"] == w["truth_bin"][k])
    acq.close()
    return good


def test_jammed_world_is_acquired_behind_the_array():
    import torch
    w = arr_world.world()
    rows = torch.from_numpy(w["rows"]).to("cuda")
    assert sum(_acquire(rows[0].contiguous(), w)) <= 1
    arr = dpe.ArrayCombiner(4, 1024, loading=1e-3)
    out = arr.process(rows, 0, 0, arr_world.WORLD_S, record_length=arr_world.WORLD_S)[0]
    st = arr.stats()
    arr.close()
    assert all(_acquire(out, w))
    assert st == dict(blocks=-(-arr_world.WORLD_S // 1024), fallbackBlocks=0, clipped=0)
    rms = float(torch.sqrt(2.0 * torch.mean(out.double() ** 2)))
    assert rms < 700                                            # against 4 236 on one element
