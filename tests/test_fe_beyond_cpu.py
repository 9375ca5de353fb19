"""CPU: the cases of fe_world.BEYOND proven on the fp64 reference alone, before the device sees them (tests/test_gpu_fe_beyond.py).

The reference's own direction: fe_ref.convert against a direct sum over t written here, with taps that have no symmetry, and not
equal to it with the taps reversed.  The conditions of the acceptance rule for every case that goes through it (tol <= 0.02, at
most 5 % of the values in the rounding band, no clipping, not all zero: what test_parity_case_conditions asserts for the parity
table).  And the discriminating power of the cases: each differs from its wrong twin -- taps reversed, the default 2-bit levels, the
record's end ignored, the IF word's sign turned -- by more than 100 tol, so no kernel that computes the twin passes."""
import numpy as np
import pytest

from tests import fe_ref, fe_world

ACCEPTED = [n for n, s in fe_world.BEYOND.items() if s.get("accept", True)]
ASYM = [n for n, s in fe_world.BEYOND.items() if s.get("asym")]
LEVELS = [n for n, s in fe_world.BEYOND.items() if "levels" in s]
UNENDED = [n for n, s in fe_world.BEYOND.items() if s.get("length") and s.get("pad", (0, 0))[1] > 0]
UNIT_WORDS = [n for n, s in fe_world.BEYOND.items() if s["f_if"] in ("+1", "-1")]


def _direct(x, D, h, gain, d, n_out):
    """y[m] = gain sum_t h[t] z[m D + t - T0] over a record x[0 .. len) that ends at len(x): one term per t, in Python integers
    for the phase word."""
    T, T0, n = len(h), (len(h) - 1) // 2, len(x)
    w = np.array([(k * d) % (1 << 32) for k in range(n)], dtype=np.float64)
    z = np.concatenate([np.zeros(T0, dtype=np.complex128), x * np.exp(-2j * np.pi * w / 4294967296.0), np.zeros(T + D, dtype=np.complex128)])
    y = np.zeros(n_out, dtype=np.complex128)
    for t in range(T):
        y += h[t] * z[t:t + n_out * D:D]                    # z index m D + t is the record's m D + t - T0
    return gain * y


@pytest.mark.parametrize("fmt", fe_ref.FORMATS)
def test_reference_direction(fmt):
    rng = np.random.Generator(np.random.PCG64(31))
    D, T, gain, n = 3, 25, 1.7, 900
    h = fe_world.asym_taps(D, T, 41)
    assert np.abs(h - h[::-1]).max() > 0.1 * np.abs(h).max()
    x = fe_ref.decode(fmt, fe_ref.random_record(fmt, n, rng), 0, n)
    d = fe_ref.delta(1.1e6, 10e6)
    n_out = -(-n // D)
    want = _direct(x, D, h, gain, d, n_out)
    scale = np.abs(want).max()
    assert np.abs(fe_ref.convert(x, 0, n, 0, n_out, D, h, gain, d) - want).max() <= 1e-9 * scale
    assert np.abs(fe_ref.convert(x, 0, n, 0, n_out, D, h[::-1], gain, d) - want).max() > 1e-2 * scale
    # the same with np.correlate (which slides h over z without turning it), on the outputs clear of both edges
    z = x * np.exp(-2j * np.pi * ((np.arange(n) * d) % (1 << 32)) / 4294967296.0)
    corr = gain * np.correlate(z, h, mode="valid")          # corr[i] = sum_t z[i + t] h[t]
    m = np.arange(-(-(T - 1) // 2 // D), (n - T + (T - 1) // 2) // D + 1)
    assert m.size > 250 and np.abs(want[m] - corr[m * D - (T - 1) // 2]).max() <= 1e-9 * scale


def test_asym_taps_have_no_symmetry_and_no_dyadic_values():
    for D, T in ((1, 9), (2, 17), (3, 25), (4, 33), (10, 81)):
        h = fe_world.asym_taps(D, T, 5)
        assert h.size == T and np.abs(h - h[::-1]).max() > 0.02 * np.abs(h).max()        # (D = 1: nearly one tap, the ramp moves its neighbours)
        assert not np.any(h * 1024.0 == np.rint(h * 1024.0))
        assert np.array_equal(h, fe_world.asym_taps(D, T, 5)) and not np.array_equal(h, fe_world.asym_taps(D, T, 6))


def test_beyond_table_holds_what_it_should():
    B = fe_world.BEYOND
    assert {B[n]["fmt"] for n in ASYM} >= {"I8C", "P2R", "I16R", "I16C", "ARGPI4"} and any(B[n]["f_if"] == 0 for n in ASYM)
    assert len(LEVELS) == 4 and len(UNENDED) == 2 and len(UNIT_WORDS) == 4
    assert sum(1 for s in B.values() if s["T"] == 1023 and s["D"] == 1) == 2
    for n in ("long I8C D64 T1023", "long I16C D64 T1023"):
        assert fe_world.beyond_case(n)["tile"] == 45
    for spec, word in (("+n", 2 ** 31), ("-n", 2 ** 31), ("+fs", 0), ("-fs", 0), ("+1", 1), ("-1", 2 ** 32 - 1)):
        for fmt in ("I8C", "I16R"):
            assert fe_world.beyond_case("if %s %s" % (spec, fmt))["delta"] == word
    top = fe_world.beyond_case("top")
    assert top["delta"] % 2 == 1 and top["out_first"] + top["out_count"] == 2 ** 55 and 2 ** 61 - 64 * 205 <= top["raw_first"] < 2 ** 61
    for n in ("edges I16C", "edges P2R"):
        c = fe_world.beyond_case(n)
        beyond = np.arange(c["out_count"]) * c["D"] - (c["T"] - 1) // 2 >= c["record_length"]
        assert c["out_count"] == 3 * c["tile"] + 7 and c["tile"] * c["D"] < c["record_length"] < 2 * c["tile"] * c["D"] - c["T"]
        assert beyond[2 * c["tile"]:].all() and not beyond[:c["tile"] + 300].any() and np.all(c["y"][beyond] == 0) and np.all(c["y"][:c["tile"]] != 0)
    for n in UNENDED + [u[:-4] for u in UNENDED]:
        c = fe_world.beyond_case(n)
        assert c["pad_before"] == 4 * 517 and c["pad_after"] == 2 * c["T"] + 13 and c["raw_first"] % fe_ref.BYTES[c["fmt"]][1] == 0
        assert c["raw_count"] == c["need_count"] + c["pad_before"] + c["pad_after"] and c["raw_first"] + c["pad_before"] == c["need_first"]
        if c["record_length"] is not None:
            assert c["need_first"] + c["need_count"] == c["record_length"] < (c["out_first"] + c["out_count"] - 1) * c["D"] + c["T"] - (c["T"] - 1) // 2


@pytest.mark.parametrize("name", ACCEPTED)
def test_beyond_case_conditions(name):
    c = fe_world.beyond_case(name)
    assert c["tol"] <= 0.02, c["tol"]
    assert fe_ref.band(c["y"], c["tol"]).mean() <= 0.05
    assert fe_ref.clip_count(c["y"]) == 0
    assert np.abs(fe_ref.interleave(c["y"])).max() > 0


def _x(c, levels=None):
    return fe_ref.decode(c["fmt"], c["raw"], 0, c["raw_count"], c["levels"] if levels is None else levels)


def _twin(c, x=None, record_length="same", h=None, d=None):
    return fe_ref.convert(_x(c) if x is None else x, c["raw_first"], c["record_length"] if record_length == "same" else record_length,
                          c["out_first"], c["out_count"], c["D"], c["h"] if h is None else h, c["gain"], c["delta"] if d is None else d)


@pytest.mark.parametrize("name", ASYM)
def test_reversed_taps_are_another_answer(name):
    c = fe_world.beyond_case(name)
    assert np.array_equal(_twin(c), c["y"])
    diff = np.abs(_twin(c, h=c["h"][::-1]) - c["y"])
    print("%s: reversed taps differ by %.0f tol at the median" % (name, np.median(diff) / c["tol"]))
    assert (diff > 100 * c["tol"]).mean() >= 0.9


@pytest.mark.parametrize("name", LEVELS)
def test_default_levels_are_another_answer(name):
    c = fe_world.beyond_case(name)
    diff = np.abs(_twin(c, x=_x(c, fe_ref.LEVELS)) - c["y"])
    print("%s: default levels differ by %.0f tol at the median" % (name, np.median(diff) / c["tol"]))
    assert np.median(diff) > 100 * c["tol"]


@pytest.mark.parametrize("name", UNENDED)
def test_a_record_without_its_end_is_another_answer(name):
    c = fe_world.beyond_case(name)
    diff = np.abs(_twin(c, record_length=None) - c["y"])
    print("%s: %d outputs differ by more than 100 tol when the record does not end" % (name, (diff > 100 * c["tol"]).sum()))
    assert (diff > 100 * c["tol"]).sum() >= 1


@pytest.mark.parametrize("name", UNIT_WORDS)
def test_the_unit_words_sign_is_another_answer(name):
    c = fe_world.beyond_case(name)
    assert c["delta"] in (1, 2 ** 32 - 1) and abs(int(fe_ref.phase_words(c["out_first"] * c["D"], 1)) - 2 ** 30) < 2 ** 12
    diff = np.abs(_twin(c, d=2 ** 32 - c["delta"]) - c["y"])
    print("%s: the other sign differs by %.0f tol at the median" % (name, np.median(diff) / c["tol"]))
    assert np.median(diff) > 100 * c["tol"]


def test_clip_case_conditions():
    """The filtered clipping case: the reference's counts taken tol outside and tol inside the rails bound the device's count."""
    c = fe_world.beyond_case("clip I8C")
    lower, upper = fe_world.clip_bounds(c)
    print("clip case: between %d and %d components beyond a rail, tol %.3f" % (lower, upper, c["tol"]))
    assert 100 < lower <= fe_ref.clip_count(c["y"]) <= upper < c["y"].size // 10
