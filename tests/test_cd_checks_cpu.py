"""What the collective-detection cases reject, shown on the CPU (tests/cd_checks.py): the assertions the GPU test makes are fed
the outputs of numpy scans that are wrong on purpose.  No GPU.

Mutant A scores every j != 0 at half its value -- a stand-in for a scan that reads the wrong bin row for jj != J, decodes jj wrongly
or drops the wrong SV at a raster edge, with wrong scores that stay below the j = 0 ones.  RANDOM_CASES' seven shapes put SV 0 at
the raster's low edge and SV 1 at its high edge, so any j != 0 drops an SV and j = 0 wins nearly everywhere: at least six of the seven
accept the mutant.  Every drift case of the second table rejects it.  Mutant B keeps the last maximum instead of the first wherever
scores are equal: the tie cases' exact comparison rejects it.  The specification's own scan, rounded to fp32, passes everywhere."""
import numpy as np
import pytest

from tests import cd_checks, cd_world


def _halve_off_zero(J):
    def mutate(sc):
        out = sc * 0.5
        out[J] = sc[J]
        return out
    return mutate


def _accepts(check, *args, **kw):
    try:
        check(*args, **kw)
    except AssertionError:
        return False
    return True


def test_the_old_cases_accept_mutant_a():
    accepted = []
    for name in cd_world.RANDOM_CASES:
        c = cd_world.random_case(name)
        fix, per, score, jm = cd_checks.numpy_scan(c, mutate=_halve_off_zero(c["J"]))
        if _accepts(cd_checks.check_parity, c, fix, per, score, jm, name=name + " (mutant A)"):
            accepted.append(name)
    print("mutant A passes check_parity on %d of %d cases: %s" % (len(accepted), len(cd_world.RANDOM_CASES), ", ".join(accepted)))
    assert len(accepted) >= 6


@pytest.mark.parametrize("name", list(cd_world.DRIFT_CASES))
def test_drift_case_rejects_mutant_a(name):
    c = cd_world.new_case(name)
    fix, per, score, jm = cd_checks.numpy_scan(c, mutate=_halve_off_zero(c["J"]))
    with pytest.raises(AssertionError):
        cd_checks.check_parity(c, fix, per, score, jm, name=name + " (mutant A)")


@pytest.mark.parametrize("name", list(cd_world.TIE_CASES))
def test_tie_case_rejects_mutant_b(name):
    c = cd_world.new_case(name)
    fix, per, score, jm = cd_checks.numpy_scan(c, last=True)
    assert np.array_equal(score.astype(np.float64), c["ref"]["map_score"])          # the scores are right; only the choice among ties is not
    with pytest.raises(AssertionError):
        cd_checks.check_exact(c, fix, score, jm)
    fix["point"] = 0                          # a scan wrong in (j, m) alone
    with pytest.raises(AssertionError):
        cd_checks.check_exact(c, fix, score, jm)
    fix, per, score, jm = cd_checks.numpy_scan(c)
    cd_checks.check_exact(c, fix, score, jm)
    fix["point"] = c["P"] - 1                 # ... and one wrong in the point alone
    with pytest.raises(AssertionError):
        cd_checks.check_exact(c, fix, score, jm)


@pytest.mark.parametrize("name", list(cd_world.RANDOM_CASES) + list(cd_world.NEW_CASES))
def test_the_reference_itself_passes(name):
    c = cd_world.any_case(name)
    for ds in (1.0, -1.0):
        fix, per, score, jm = cd_checks.numpy_scan(c, ds=ds)
        assert cd_checks.check_parity(c, fix, per, score, jm, ds=ds, name=name) <= 0.05      # fp32 rounding: 2^-25 of the score against 2e-6
        if ds == 1.0 and (fix["j"] != 0 or any(r["fi"] != 0.0 for r in per)):
            with pytest.raises(AssertionError):                                             # the sign is looked at
                cd_checks.check_parity(c, fix, per, score, jm, ds=-1.0, name=name)
    if name in cd_world.TIE_CASES:
        cd_checks.check_exact(c, fix, score, jm)
