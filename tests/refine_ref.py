"""A numpy restatement of the coarse-to-fine level chain (dpe_bcm_create_refine, csrc/dpe_bcm_refine.h): fp32 centres, the
decode of a flattened index against a level's dims, and the key-0 rule.  It knows nothing about scores: a caller hands it
`score(manifold, points)`, which returns the row of a [G, 4] fp64 point list (the oracle on generated or on the GPU's banks).

A level's grid is the tensor product of its four axes, flattened ((ix ny + iy) nz + iz) nt + it.  Level l >= 1 is scored at
the fp32 points fl32(c + a_i), where c is the fp32 point level l - 1 scored at its first maximum (its own centre, 0 at level
0, plus its axis values, each sum rounded once to fp32).  A level none of whose points has a score (every sum NaN) has key 0:
index -1 there, and no later level is scanned."""
import numpy as np


def decode(index, dims):
    """Flattened index -> (ix, iy, iz, it)."""
    out = []
    for d in reversed(dims):
        out.append(int(index) % int(d))
        index = int(index) // int(d)
    return tuple(reversed(out))


def encode(coords, dims):
    i = 0
    for c, d in zip(coords, dims):
        i = i * int(d) + int(c)
    return i


def scored_axes(centre, axes):
    """The fp32 axis values a level scores: np.float32(c) + a.astype(np.float32), one rounding per sum."""
    return [np.float32(c) + np.asarray(a, dtype=np.float64).astype(np.float32) for c, a in zip(centre, axes)]


def points(axes):
    """[G, 4] fp64 point list of four axes in the flattened order (t fastest)."""
    g = np.meshgrid(*[np.asarray(a, dtype=np.float64) for a in axes], indexing="ij")
    return np.stack([x.reshape(-1) for x in g], axis=1)


def first_max(row):
    """First maximum by strict 'greater' from -1 (scores are >= 0; a NaN never compares greater) -> index or -1 (key 0)."""
    row = np.asarray(row)
    ok = ~np.isnan(row)
    if not ok.any():
        return -1
    return int(np.argmax(np.where(ok, row, -np.inf)))


def make_key(score, index):
    return 0 if index < 0 else (int(np.float32(score).view(np.uint32)) << 32) | (0xFFFFFFFF - int(index))


def chain(level_axes, score):
    """level_axes: per level the four axes of ONE manifold; score(points [G, 4]) -> row.  Returns per level a dict
    (index, centre = the fp32 centre the level was scored around, axes = the fp32 values it scored, row) -- index -1 and
    row None from the first level without a score on -- and the final fp32 point (NaN when the chain stopped)."""
    c = np.zeros(4, dtype=np.float32)
    out, alive = [], True
    for axes in level_axes:
        if not alive:
            out.append(dict(index=-1, centre=None, axes=None, row=None))
            continue
        ax = scored_axes(c, axes)
        row = score(points(ax))
        i = first_max(row)
        out.append(dict(index=i, centre=c.copy(), axes=ax, row=row))
        if i < 0:
            alive = False
            continue
        c = np.array([a[j] for a, j in zip(ax, decode(i, [a.size for a in ax]))], dtype=np.float32)
    return out, (c.astype(np.float64) if alive else np.full(4, np.nan))


def point_of(level_axes, indices):
    """The fp32 point a chain of per-level indices ends at (every index >= 0), by the device's own additions."""
    c = np.zeros(4, dtype=np.float32)
    for axes, i in zip(level_axes, indices):
        ax = scored_axes(c, axes)
        c = np.array([a[j] for a, j in zip(ax, decode(i, [a.size for a in ax]))], dtype=np.float32)
    return c
