"""CPU: the excisor's fp64 specification (tests/ix_ref.py) on its own -- reconstruction, cyclic guard and static masks, the frame of
zeros, its own split property -- the conditions the GPU cases (tests/ix_world.py) rest on, and the premise of the stage: a tone
that hides every satellite from acquisition, and the excised record in which all are found again."""
import numpy as np
import pytest

from oracle import oracle
from tests import ix_ref, ix_world


def test_engine_has_the_stage():
    import navlab_dpe_sdr_amd as dpe
    assert dpe.Excisor is dpe.engine.Excisor and dpe.frontend.Excised


@pytest.mark.parametrize("N", [64, 256, 4096])
def test_reconstruction_when_nothing_is_excised(N):
    x = ix_world.noise(1, 6 * N)
    out = ix_ref.excise(x, 0, None, 0, 5 * N, N, 1.0e6, 1, gain=-1.5)
    assert np.abs(out - (-1.5) * x[:5 * N]).max() <= 1e-9
    out = ix_ref.excise(x, 0, 2 * N + 7, N - 3, 2 * N, N, 1.0e6, 1)                 # the record's end: zeros beyond it
    want = np.concatenate([x[N - 3:2 * N + 7], np.zeros(N - 10)])
    assert np.abs(out - want).max() <= 1e-9


def test_guard_and_static_wrap_cyclically():
    det = np.zeros((2, 64), dtype=bool)
    det[0, 0] = det[1, 63] = True
    e = ix_ref.widen(det, 2)
    assert np.flatnonzero(e[0]).tolist() == [0, 1, 2, 62, 63] and np.flatnonzero(e[1]).tolist() == [0, 1, 61, 62, 63]
    static = np.zeros(64, dtype=np.uint8)
    static[[5, 63]] = 1
    e = ix_ref.widen(det, 0, static)
    assert np.flatnonzero(e[0]).tolist() == [0, 5, 63] and np.flatnonzero(e[1]).tolist() == [5, 63]
    # a tone on bin 0 and one on bin N - 1 are excised with their neighbours on the far side
    c = ix_world.case("wrap bins 0 and N-1")
    _, _, F = ix_world.reference(c)
    assert F["e"][:, [253, 254, 255, 0, 1, 2]].all() and F["e"].mean() < 0.06


def test_a_frame_of_zeros_excises_nothing():
    F = ix_ref.frames(np.zeros(512, dtype=complex), 0, None, 1, 2, 256, 10.0, 3)
    assert not F["detected"].any() and not F["e"].any() and np.all(F["m"] == 0.0)
    c = ix_world.case("frames beyond the record")
    out, _, F = ix_world.reference(c)
    assert not F["e"][13:].any() and np.all(out[384:] == 0.0) and np.abs(out[:333]).max() > 1000


@pytest.mark.parametrize("name", ["cross N64", "cross N1024", "pulse"])
def test_split_of_the_reference(name):
    c = ix_world.case(name)
    whole, _, _ = ix_world.reference(c)
    a, n, H = c["out_first"], c["out_count"], c["H"]
    for cut in ((a // H + 2) * H - a, (a // H + 2) * H - a + H // 3, 1, n - 1):
        parts = [ix_ref.excise(c["x"], c["x_first"], c["record_length"], f, k, c["N"], c["kappa"], c["guard"], c["static"], c["blank_power"], c["gain"])
                 for f, k in ((a, cut), (a + cut, n - cut))]
        assert np.array_equal(np.concatenate(parts), whole), (name, cut)


@pytest.mark.parametrize("name", list(ix_world.CASES))
def test_case_conditions(name):
    c = ix_world.case(name)
    assert np.abs(c["base"].real).max() <= ix_world.AMP and np.abs(c["base"].imag).max() <= ix_world.AMP
    if not c["in_f32"]:
        assert np.array_equal(c["x"], np.rint(c["x"].real) + 1j * np.rint(c["x"].imag)) and np.abs(ix_world.i16_bytes(c["x"])).max() <= 32767
    lo, hi = c["needed"]
    assert c["x_first"] >= 0 and c["x_first"] <= lo and hi <= c["x_first"] + c["x"].size
    out, tol, F = ix_world.reference(c)
    assert np.isfinite(out).all() and np.all(tol >= 0) and tol.max() <= 1e-4 * max(np.abs(c["x"]).max() * abs(c["gain"]) * c["N"] ** 0.5, 1.0), (name, tol.max())
    if name in ("static mask alone", "nothing excised"):
        assert not F["detected"].any()
    elif "add" in ix_world.CASES[name] and ix_world.CASES[name]["add"][0] != "pulse":
        inside = F["fr"].any(axis=-1)
        assert F["detected"][inside].any(axis=-1).mean() > 0.5, name                 # the interferer is found in most frames that hold samples
    if name == "pulse":
        assert ix_world.blanked_count(c) == 37
        bare = dict(c, blank_power=0.0)
        assert np.abs(ix_world.reference(bare)[0] - out).max() > 1000                # without the blanker the pulse comes through
    if name == "large indices":
        assert c["out_first"] + c["out_count"] == 2 ** 55 - 3


@pytest.mark.parametrize("N", ix_world.SIZES)
def test_analysis_cases_are_decided(N):
    a = ix_world.analysis_case(N)
    dec, unsure = ix_ref.decided(a["F"], N, a["kappa"], a["guard"], a["static"])
    assert unsure.mean() <= 0.01 and (~dec).mean() <= 0.01, (N, unsure.mean(), (~dec).mean())
    assert a["F"]["detected"].any(axis=-1).all() and a["F"]["e"][:, a["static"] != 0].all()
    d = ix_ref.power_tolerance(a["F"], N)
    assert np.all(d > 0) and np.median(d / a["F"]["P"]) < 1e-2


def test_clip_case_clips():
    c = ix_world.clip_case()
    out, tol, _ = ix_world.reference(c)
    v = ix_ref.interleave(out)
    assert 0.1 < (np.abs(v) > 32768).mean() < 0.5


def _acquire(iq, w):
    found = []
    for k, prn in enumerate(w["ch"]["prn"]):
        a = oracle.coarse_acquisition(iq, ix_world.WORLD_FS, int(prn), ix_world.WORLD_BINS, coherent=True, wrap_mask=True)
        dist = abs((a["max_code_idx"] - w["truth_idx"][k] + 1250.0) % 2500.0 - 1250.0)
        found.append(bool(a["found"]) and dist <= 1.0 and a["max_dopp_idx"] == w["truth_bin"][k])
    return found


def test_premise_the_tone_hides_the_satellites_and_excision_brings_them_back():
    w = ix_world.world()
    assert all(_acquire(w["clean"], w))
    assert sum(_acquire(w["jammed"], w)) <= 1
    assert all(_acquire(w["excised"], w))
