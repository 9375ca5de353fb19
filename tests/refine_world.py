"""Worlds for the coarse-to-fine scan (dpe_bcm_create_refine), built on tests/epoch_world.py.

The batch: four one-window worlds, epoch_world.build(N=1, K=8, seed=s) for s in SEEDS, as the windows of ONE batch (own SV
selection, own noise, own centre each).  Their truth sits on a point of the world's 7^4 grid at 40 m / 12 m/s steps; the
COARSE level here is that grid displaced by SHIFT_POS / SHIFT_VEL, so the truth is OFF the coarse grid, and the FINE level has
a third of the step (13.33 m / 4 m/s) over +-`half` coarse steps (13 entries at +-2, 7 at +-1).  The comparator is the dense
uniform grid of the fine step over the coarse extent plus the fine half-span (31^4 at +-2): the point (coarse index ic, fine
index jf) of an axis is dense entry 3 ic + jf.

L and B are widened from pipeline.bank_half_widths_refine until the oracle counts no pair outside the banks at the 16 corners
of the dense grids of every window (the index is linear in the offset up to a second-order term of millimetres, so the
corners bound the grid); tests/test_refine_world_cpu.py then counts the whole dense grids."""
import functools

import numpy as np

import navlab_dpe_sdr_amd as dpe
from tests import epoch_world as ew
from tests import refine_ref as rr

SEEDS = (0, 1, 2, 3)
SHIFT_POS = (13.0, -9.0, 6.0, -15.0)       # m: the coarse grid's displacement from the world's grid
SHIFT_VEL = (4.0, -2.5, 1.5, -5.0)         # m/s
COARSE_DIM, RATIO = 7, 3
ORACLE_TOL = ew.ORACLE_TOL


def _uniform(n, step, shift=(0.0, 0.0, 0.0, 0.0)):
    return dpe.GridAxes(*[step * (np.arange(n) - (n - 1) // 2).astype(np.float64) + s for s in shift])


def coarse():
    return _uniform(COARSE_DIM, ew.POS_STEP, SHIFT_POS), _uniform(COARSE_DIM, ew.VEL_STEP, SHIFT_VEL)


def fine(half=2):
    n = 2 * RATIO * half + 1
    return _uniform(n, ew.POS_STEP / RATIO), _uniform(n, ew.VEL_STEP / RATIO)


def levels(half=2):
    return [coarse(), fine(half)]


def dense(half=2):
    n = RATIO * (COARSE_DIM - 1) + 2 * RATIO * half + 1
    return _uniform(n, ew.POS_STEP / RATIO, SHIFT_POS), _uniform(n, ew.VEL_STEP / RATIO, SHIFT_VEL)


def dense_index(coarse_index, fine_index, half=2):
    """The dense grid's index of the refined point: integer arithmetic on (coarse index, fine index), axis by axis."""
    nf, nd = 2 * RATIO * half + 1, RATIO * (COARSE_DIM - 1) + 2 * RATIO * half + 1
    ic, jf = rr.decode(coarse_index, [COARSE_DIM] * 4), rr.decode(fine_index, [nf] * 4)
    return rr.encode([RATIO * i + j for i, j in zip(ic, jf)], [nd] * 4)


def _corners(ax):
    return rr.points([np.array([a.min(), a.max()]) for a in ax.axes])


@functools.lru_cache(maxsize=None)
def build(widen=True):
    """-> world dict in epoch_world's form (N = 4 windows, K = 8), L and B widened as the module header says.
    widen False / "L" / "B": deliberately narrow banks (L = 1, B = 2) on both sides / the lag side / the bin side only."""
    if widen is not True:
        world = dict(build(True))
        if widen in (False, "L"):
            world["L"] = 1
        if widen in (False, "B"):
            world["B"] = 2
        return world
    parts = [ew.build(N=1, K=8, seed=s) for s in SEEDS]
    p0 = parts[0]
    world = dict(fs=p0["fs"], S=p0["S"], C=p0["C"], N=len(parts), K=p0["K"], wins=[p["wins"][0] for p in parts], R=p0["R"],
                 truth=np.stack([p["truth"][0] for p in parts]), offset=p0["offset"])
    L, B = dpe.pipeline.bank_half_widths_refine(levels(2), world["fs"], world["C"])
    L, B = max([L] + [p["L"] for p in parts]), max([B] + [p["B"] for p in parts])
    dp, dv = dense(2)
    cp, cv = _corners(dp), _corners(dv)
    while True:
        world["L"], world["B"] = L, B
        n = 0
        for w in range(world["N"]):
            n += scorer(world, w, 0)(cp, count=True)[1] + scorer(world, w, 1)(cv, count=True)[1]
        if n == 0:
            break
        L, B = L + 1, B + 2
    return world


_BANKS = {}


def oracle_banks(world, w):
    """The oracle's code and carrier banks of window w at the world's L, B (cached)."""
    key = (id(world["wins"][w]), world["L"], world["B"])
    if key not in _BANKS:
        o = ew._o()
        win, L, B = world["wins"][w], world["L"], world["B"]
        s = win["start"]
        code, carr = [], []
        for k in range(world["K"]):
            c, f, _inf = o.bcs_sv(win["iq"], world["fs"], int(s["prn"][k]), s["rc"][k], s["ri"][k], s["fc"][k], s["fi"][k], int(s["cp"][k]),
                                  int(s["cp_ref"][k]), -L, L, -B, B, world["C"])
            code.append(c)
            carr.append(f)
        _BANKS[key] = (np.stack(code), np.stack(carr))
    return _BANKS[key]


def scorer(world, w, manifold, lpower=1, code=None, carr=None):
    """score(points [G, 4]) -> the oracle's row of window w (extended-precision position rows, velocity rows) on the oracle's
    banks, or on the banks given (the GPU's own).  score(points, count=True) -> (row, pairs outside the banks)."""
    o = ew._o()
    win, L, B = world["wins"][w], world["L"], world["B"]
    if code is None:
        code, carr = oracle_banks(world, w)

    def score(pts, count=False):
        if manifold == 0:
            row, oob = o.bcm_pos(win["sat"], code, world["S"] // 2 - L, win["centre"], pts, win["R"], win["fc"], win["cpRefTOW"], win["cpElaEnd"],
                                 win["cpRef"], win["rcEnd"], win["rxTime"], world["fs"], world["S"], lpower, extended=True)
        else:
            row, oob = o.bcm_vel(win["sat"], carr, world["C"] // 2 - B, win["centre"], pts, win["R"], win["fi"], win["rxTime"], world["fs"],
                                 world["C"], 1, lpower)
        return (row, oob) if count else row
    return score


_DENSE = {}


def dense_rows(world, half=2):
    """Per window (position row, velocity row, pairs outside the banks) of the oracle on the dense grids (cached)."""
    key = (id(world["wins"][0]), world["L"], world["B"], half)
    if key not in _DENSE:
        dp, dv = dense(half)
        pp, pv = dp.points(), dv.points()
        out = []
        for w in range(world["N"]):
            p, np_ = scorer(world, w, 0)(pp, count=True)
            v, nv = scorer(world, w, 1)(pv, count=True)
            out.append((p, v, np_ + nv))
        _DENSE[key] = out
    return _DENSE[key]


def axes_of(lv, manifold):
    """Per level the four axes of one manifold."""
    return [l[manifold].axes for l in lv]


def margin(row):
    """(first maximum, (max - runner-up) / max) of a row."""
    i = rr.first_max(row)
    rest = np.delete(row, i)
    return i, float((row[i] - np.nanmax(rest)) / row[i])
