"""Tensor-product manifold grids given by their four axes (dpe_grid_axes, dpe_bcm_create_axes).

Every grid the reference builds for itself is a tensor product: Uniform and ArthurBasis (BCM_InitPosGrid,
batchcorrmanifold.cu:160-246) and PyGNSS' spread grids (receiver.py:995-1026).  Point i of such a grid is
((ix * ny + iy) * nz + iz) * nt + it, t fastest (batchcorrmanifold.cu:165-170) -- the order of synth.uniform_grid /
spread_grid and host/grids.hpp.  A GridAxes may stand for a contiguous slice [begin, end) of that flattened index (one rank's
shard, sharding.shard_range); BatchCorrManifold and Pipe take it wherever they take a [G, 4] point list.
"""
import ctypes as C

import numpy as np


class GridAxesC(C.Structure):     # dpe_grid_axes
    _fields_ = [("dim", C.c_int32 * 4), ("axis", C.POINTER(C.c_double) * 4)]


def _axis(kind, dim, spacing):
    """One axis of BCM_InitPosGrid (host/grids.hpp grid_axis): index -> offset from the centre."""
    half = (dim - 1) // 2
    i = np.arange(dim)
    a = spacing * (i - half).astype(np.float64)
    if kind == "arthur":
        # outer quarters: three times the spacing, shifted so that the axis stays continuous (:192-199)
        outer = (i < half // 2) | ((dim - i) < half // 2)
        shift = spacing * ((half // 2) + 1) * 2
        a = np.where(outer, 3 * spacing * (i - half) + np.where(i < half, shift, -shift), a)
    return a


def _four(v):
    v = np.atleast_1d(v)
    return list(v) * 4 if v.size == 1 else list(v)


class GridAxes:
    """Axes x, y, z, delta_t (m; m/s for the velocity manifold) and the slice [begin, end) of the flattened index."""

    def __init__(self, x, y, z, t, begin=0, end=None):
        self.axes = tuple(np.ascontiguousarray(np.ravel(a), dtype=np.float64) for a in (x, y, z, t))
        self.dim = tuple(int(a.size) for a in self.axes)
        self.global_size = int(np.prod(self.dim, dtype=np.int64))
        self.begin = int(begin)
        self.end = self.global_size if end is None else int(end)
        if not 0 <= self.begin < self.end <= self.global_size:
            raise ValueError("GridAxes: slice [%d, %d) outside the %d-point grid" % (self.begin, self.end, self.global_size))

    @classmethod
    def uniform(cls, dim, spacing):
        """Uniform grid (ManifoldGridTypes::Uniform); dim / spacing: one value for all four axes, or four."""
        return cls(*[_axis("uniform", int(d), float(s)) for d, s in zip(_four(dim), _four(spacing))])

    @classmethod
    def arthur_basis(cls, dim, spacing):
        """ArthurBasis position grid (outer quarters at three times the spacing); the reference's velocity grid is uniform."""
        return cls(*[_axis("arthur", int(d), float(s)) for d, s in zip(_four(dim), _four(spacing))])

    @classmethod
    def pygnss_spread(cls):
        """PyGNSS spread grids (receiver.py:995-1026) as (pos, vel): synth.spread_grid without the point lists."""
        a = np.array([-22, -19, -16, -13, -10, -7, -6, -5, -4, -3, -2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 10, 13, 16, 19, 22],
                     dtype=np.float64)
        b = np.arange(-12, 13, dtype=np.float64)
        return cls(a * 5, a * 5, a * 5, a * 6), cls(b * 0.5, b * 0.5, b * 0.5, b * 0.25)

    @property
    def size(self):
        """Points in this slice."""
        return self.end - self.begin

    def __len__(self):
        return self.size

    @property
    def shape(self):   # the [G, 4] shape of the point list it stands for
        return (self.size, 4)

    def shard(self, begin, end):
        """The slice [begin, end) of the GLOBAL flattened index (sharding.shard_range); it must lie inside this slice."""
        if not self.begin <= begin < end <= self.end:
            raise ValueError("GridAxes.shard: [%d, %d) outside [%d, %d)" % (begin, end, self.begin, self.end))
        return GridAxes(*self.axes, begin=begin, end=end)

    def full(self):
        """The whole grid these axes span (the global grid of a shard)."""
        return GridAxes(*self.axes)

    def _points(self, idx):
        idx = np.asarray(idx, dtype=np.int64)
        out = np.empty(idx.shape + (4,), dtype=np.float64)
        r = idx.copy()
        for c in (3, 2, 1, 0):
            out[..., c] = self.axes[c][r % self.dim[c]]
            r //= self.dim[c]
        return out

    def point(self, i):
        """Row i of this slice, {x, y, z, delta_t}."""
        if not 0 <= i < self.size:
            raise IndexError(i)
        return self._points(self.begin + int(i))

    def global_point(self, index):
        """The point of GLOBAL index `index` (what a key decodes to)."""
        return self._points(int(index))

    def points(self):
        """The slice materialised as a [size, 4] point list, in the flattened order."""
        return self._points(np.arange(self.begin, self.end, dtype=np.int64))

    def c_struct(self):
        """dpe_grid_axes pointing at this object's arrays (keep the object alive while it is used)."""
        s = GridAxesC()
        for c in range(4):
            s.dim[c] = self.dim[c]
            s.axis[c] = self.axes[c].ctypes.data_as(C.POINTER(C.c_double))
        return s
