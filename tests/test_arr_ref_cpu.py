"""CPU: the array combiner's specification tests/arr_ref.py on its own -- the split property, the w^H c = 1 identity, the fallback
rules -- and the conditions the cases of tests/arr_world.py must meet for the GPU tests to mean what they say: every parity case
has kappa_2(R_k) <= 10^6 and at least 99 % of its int16 output components farther than tol from a rounding boundary; the clipping
case clips 10-50 %; and the end-to-end world's premise by the CPU oracle's acquisition."""
import numpy as np
import pytest

from navlab_dpe_sdr_amd import engine
from oracle import oracle
from tests import arr_ref, arr_world, ix_world


@pytest.mark.parametrize("name", ["M2 L256 cross", "M8 L256 three constraints, loading 1", "record ends inside a block", "zero block"])
def test_split_property_of_the_reference(name):
    c = arr_world.case(name)
    one = arr_world.reference(name)
    a, n, L = c["out_first"], c["out_count"], c["L"]
    edge = (a // L + 1) * L - a
    for cuts in ([0, edge, n], [0, edge + L // 3, n], [0] + list(range(edge - 2, edge + 3)) + [n]):
        parts = [arr_ref.process(c["x"], c["x_first"], c["record_length"], a + lo, hi - lo, L, c["cons"], c["loading"], c["gain"])["y"]
                 for lo, hi in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(np.concatenate(parts, axis=1), one["y"]), (name, cuts)
        total = sum(len(arr_ref.counted(a + lo, hi - lo, L, c["record_length"])) for lo, hi in zip(cuts[:-1], cuts[1:]))
        assert total == len(arr_ref.counted(a, n, L, c["record_length"]))


@pytest.mark.parametrize("name", arr_world.PARITY)
def test_constraint_identity_and_case_conditions(name):
    c, r = arr_world.case(name), arr_world.reference(name)
    assert not r["fallback"].any() and np.nanmax(r["kappa"]) <= 1.0e6, (name, np.nanmax(r["kappa"]))
    unit = np.einsum("kba,ba->kb", np.conj(r["w"]), c["cons"])          # w^H c
    assert np.abs(unit - 1.0).max() <= 1e-9
    if not c["explicit"]:                                               # power inversion: the reference element passes with unit weight
        assert np.abs(r["w"][:, 0, c["reference"]] - 1.0).max() <= 1e-9
    y = np.stack([arr_ref.interleave(row) for row in r["y"]])
    tol = r["tol"].reshape(r["tol"].shape[0], -1)
    decided = arr_ref.boundary_distance(y) > tol
    print("%s: kappa up to %.1f, %.4f of the int16 components decided, |y| up to %.0f" % (name, np.nanmax(r["kappa"]), decided.mean(), np.abs(y).max()))
    assert decided.mean() >= 0.99 and np.abs(y).max() < 32767


def test_jammed_cases_are_nulled():
    c, r = arr_world.case("M4 L1024 last reference, no loading"), arr_world.reference("M4 L1024 last reference, no loading")
    a = c["out_first"] - c["x_first"]
    before = np.sqrt(np.mean(np.abs(c["x"][3, a:a + c["out_count"]]) ** 2))
    after = np.sqrt(np.mean(np.abs(r["y"][0]) ** 2))
    assert before > 8000 and after < 2500          # the interferer of sigma 6000 is gone; what is left is the elements' noise


def test_fallback_rules():
    M, L = 4, 256
    cons = arr_world.random_constraints(3, 2, M)
    x = arr_world.elements(9, M, 3 * L)
    x[:, L:2 * L] = 0.0
    r = arr_ref.process(x, 0, None, 0, 3 * L, L, cons, 1e-3, 1.0)
    assert r["fallback"].tolist() == [[False, False], [True, True], [False, False]]
    want = cons / np.sum(np.abs(cons) ** 2, axis=1, keepdims=True)
    assert np.array_equal(r["w"][1], want) and np.all(r["y"][:, L:2 * L] == 0.0)
    for length, fb in ((2 * L + 2 * M - 1, True), (2 * L + 2 * M, False)):      # fewer than 2 M samples of the last block inside the record
        r = arr_ref.process(x, 0, length, 0, 3 * L, L, cons, 1e-3, 1.0)
        assert bool(r["fallback"][2].all()) == fb and r["count"].tolist() == [L, L, length - 2 * L]
        assert np.all(r["y"][:, length:] == 0.0)
    # a rank-one block with loading > 0 does not take the fallback, and keeps w^H c = 1
    g = arr_world.elements(10, 1, L, None)[0]
    steer = np.array([1.0, 1j, -1.0, -1j])
    one = np.stack([ix_world.to_i16(s * g) for s in steer])
    r = arr_ref.process(one, 0, None, 0, L, L, arr_ref.unit_vector(M, 0), 1e-3, 1.0)
    assert not r["fallback"].any() and abs(np.vdot(r["w"][0, 0], arr_ref.unit_vector(M, 0)[0]) - 1.0) < 1e-12 and r["kappa"][0] < 1e4
    assert np.linalg.matrix_rank(r["S"][0, :, :, 0] + 1j * r["S"][0, :, :, 1]) == 1


def test_covariance_is_exact_at_the_extremes():
    c = arr_world.extreme("floor")
    xb, _ = arr_ref.blocks_of(c["x"], 0, None, 0, 1, c["L"])
    S = arr_ref.covariance(xb)
    assert np.all(S[..., 0] == 2 ** 47) and np.all(S[..., 1] == 0)
    c = arr_world.extreme("alternating")
    xb, _ = arr_ref.blocks_of(c["x"], 0, None, 0, 2, c["L"])
    S = arr_ref.covariance(xb)
    I, Q = [[int(v) for v in row] for row in c["x"].real[:, :256]], [[int(v) for v in row] for row in c["x"].imag[:, :256]]
    for a in range(3):
        for b in range(3):      # Python integers
            assert S[0, a, b, 0] == sum(I[a][n] * I[b][n] + Q[a][n] * Q[b][n] for n in range(256))
            assert S[0, a, b, 1] == sum(Q[a][n] * I[b][n] - I[a][n] * Q[b][n] for n in range(256))
    assert np.array_equal(S[..., 0], S[..., 0].transpose(0, 2, 1)) and np.array_equal(S[..., 1], -S[..., 1].transpose(0, 2, 1))


def test_clip_case_clips_a_tenth_to_a_half():
    c = arr_world.clip_case()
    r = arr_ref.process(c["x"], c["x_first"], None, c["out_first"], c["out_count"], c["L"], c["cons"], c["loading"], c["gain"])
    v = np.rint(arr_ref.interleave(r["y"][0]))
    assert 0.1 < ((v > 32767) | (v < -32768)).mean() < 0.5


def test_steering_vectors():
    pos = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.25, 0.0]])
    s = engine.steering_vectors(pos, [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], wavelength=1.0)
    assert s.shape == (3, 3) and np.allclose(s, [[1, -1, 1], [1, 1, 1j], [1, 1, 1]])
    d = engine.steering_vectors(pos * engine.L1_WAVELENGTH, [1.0, 0.0, 0.0])
    assert np.allclose(d, [[1, -1, 1]]) and abs(engine.L1_WAVELENGTH - 299792458.0 / 1575.42e6) < 1e-15


def _acquire(iq, w):
    found = []
    for k, prn in enumerate(w["ch"]["prn"]):
        a = oracle.coarse_acquisition(iq, arr_world.WORLD_FS, int(prn), arr_world.WORLD_BINS, coherent=True, wrap_mask=True)
        dist = abs((a["max_code_idx"] - w["truth_idx"][k] + 1250.0) % 2500.0 - 1250.0)
        found.append(bool(a["found"]) and dist <= 1.0 and a["max_dopp_idx"] == w["truth_bin"][k])
    return found


def test_premise_the_jammer_hides_the_satellites_and_the_array_brings_them_back():
    w = arr_world.world()
    assert sum(_acquire(w["rows"][0], w)) <= 1
    iq, r = arr_world.world_combined(1024, 1e-3)
    assert all(_acquire(iq, w))
    rms = np.sqrt(np.mean(iq.astype(np.float64) ** 2) * 2)
    jammed = np.sqrt(np.mean(np.abs(w["x"][0]) ** 2))
    print("output rms %.0f against %.0f jammed, kappa up to %.0f" % (rms, jammed, np.nanmax(r["kappa"])))
    assert jammed > 4000 and rms < 700 and not r["fallback"].any()
