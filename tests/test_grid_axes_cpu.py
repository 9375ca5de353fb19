"""GridAxes (grid_axes.py): the point lists it stands for equal the project's grid builders (synth.uniform_grid / spread_grid and
host/grids.hpp through `dpe_flow --dump-grid`), point(i) equals points()[i], and shards follow sharding.shard_range."""
import os
import subprocess

import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("dim,sp", [(5, 1.0), (6, 0.5), (25, 1.0)])
def test_uniform_points_match_synth(dim, sp):
    assert np.array_equal(dpe.GridAxes.uniform(dim, sp).points(), dpe.synth.uniform_grid(dim, sp))


def test_spread_points_match_synth():
    pa, va = dpe.GridAxes.pygnss_spread()
    p, v = dpe.synth.spread_grid()
    assert np.array_equal(pa.points(), p) and np.array_equal(va.points(), v)


@pytest.mark.parametrize("gtype,dim,sp", [(0, 5, 1.0), (0, 6, 0.5), (2, 9, 1.5), (2, 25, 1.0), (2, 12, 0.75)])
def test_points_match_host_builder(tmp_path, gtype, dim, sp):
    import __graft_entry__ as ge
    ge.build()
    out = str(tmp_path / "g.bin")
    subprocess.check_call([os.path.join(ROOT, "navlab-dpe-sdr_amd", "dpe_flow"), "--dump-grid", str(gtype), str(dim), str(sp), out])
    G = dim ** 4
    raw = np.fromfile(out)[:4 * G].reshape(G, 4)
    ga = (dpe.GridAxes.uniform if gtype == 0 else dpe.GridAxes.arthur_basis)(dim, sp)
    assert ga.size == G and np.array_equal(ga.points(), raw)


def test_point_and_odd_shapes():
    rng = np.random.default_rng(7)
    ga = dpe.GridAxes(rng.normal(size=3), rng.normal(size=5), rng.normal(size=7), rng.normal(size=1))
    pts = ga.points()
    assert pts.shape == (105, 4) and ga.dim == (3, 5, 7, 1)
    for i in (0, 1, 34, 104):
        assert np.array_equal(ga.point(i), pts[i])
    ix, iy, iz, it = np.unravel_index(np.arange(105), ga.dim)
    assert np.array_equal(pts, np.stack([ga.axes[0][ix], ga.axes[1][iy], ga.axes[2][iz], ga.axes[3][it]], axis=1))
    with pytest.raises(IndexError):
        ga.point(105)


@pytest.mark.parametrize("world", [1, 3, 5, 7])
def test_shards_follow_shard_range(world):
    ga = dpe.GridAxes.uniform((6, 5, 4, 33), (1.0, 2.0, 0.5, 0.25))
    full = ga.points()
    parts = []
    for r in range(world):
        b, e = dpe.sharding.shard_range(ga.size, r, world)
        sh = ga.shard(b, e)
        assert (sh.begin, sh.end, sh.size, sh.shape) == (b, e, e - b, (e - b, 4))
        assert np.array_equal(sh.points(), full[b:e])
        assert np.array_equal(sh.point(0), full[b]) and np.array_equal(sh.global_point(e - 1), full[e - 1])
        assert sh.full().size == ga.size
        parts.append(sh.points())
    assert np.array_equal(np.concatenate(parts), full)
    with pytest.raises(ValueError):
        ga.shard(0, ga.size + 1)


# ---- dpe_bcm_create_axes refusals: every check runs before the device is touched
def _create(pos, vel, size=None, offset=0, L=4, B=20, K=8, reference_pair=False, with_points=False):
    import ctypes as C
    import __graft_entry__ as ge
    ge.build()
    e = dpe.engine
    pts = np.zeros((4, 4))
    n = size if size is not None else int(np.prod(pos.dim))
    cfg = e._bcm_config(50000, L, B, 1, 1, K, 65536, 2.5e6, pts, pts, 0, 0, not with_points, True, False, reference_pair)
    cfg.posGridSize, cfg.velGridSize, cfg.posGridIndexOffset = n, int(np.prod(vel.dim)), offset
    h = C.c_void_p(None)
    pa, va = pos.c_struct(), vel.c_struct()
    rc = e.lib().dpe_bcm_create_axes(C.byref(cfg), C.byref(pa), C.byref(va), C.byref(h))
    assert rc != 0 and not h.value
    return e.lib().dpe_last_error().decode()


class _Raw:   # axes the Python class itself would refuse (dim 0)
    def __init__(self, *axes):
        self.axes = [np.ascontiguousarray(a, dtype=np.float64) for a in axes]
        self.dim = tuple(a.size for a in self.axes)

    def c_struct(self):
        return dpe.GridAxes.c_struct(self)


@pytest.mark.parametrize("what,kw,msg", [
    ("reference_pair", dict(reference_pair=True), "referencePair is not supported"),
    ("point lists too", dict(with_points=True), "posGrid / velGrid must be NULL"),
    ("compact banks", dict(K=37, L=174, B=20), "exceed the LDS"),
    ("slice beyond product", dict(size=25 ** 4, offset=1), "beyond the axis product"),
    # one entry past the widest banks admitted at K = 37 (max(L, B) = 113, run on the GPU by test_gpu_axes_scan.py):
    # 37 x (229 x 16 + 32) + 17408 = 154160 > 153600 bytes
    ("one lag entry past the LDS", dict(K=37, L=114, B=20), "score banks (135568 B) and the score stage (17408 B) exceed the LDS"),
    ("one bin entry past the LDS", dict(K=37, L=4, B=114), "score banks (135568 B) and the score stage (17408 B) exceed the LDS"),
])
def test_create_axes_refusals(what, kw, msg):
    g = dpe.GridAxes.uniform(25, 1.0)
    assert msg in _create(g, g, **kw), what


def test_create_axes_refuses_bad_axes():
    ok = dpe.GridAxes.uniform(5, 1.0)
    assert "is not finite" in _create(dpe.GridAxes([0.0, np.nan], [0.0], [0.0], [0.0]), ok)
    assert "is not finite" in _create(ok, dpe.GridAxes([0.0], [np.inf], [0.0], [0.0]))
    assert "dim 0 < 1" in _create(_Raw([0.0], [], [0.0], [0.0]), ok, size=1)
    assert "beyond 3 km" in _create(dpe.GridAxes.uniform(3, 2000.0), ok)
    big = _Raw(np.zeros(65536), np.zeros(65536), [0.0], [0.0, 1.0])
    assert "does not fit 32 bits" in _create(big, ok, size=1024, offset=1 << 32)
