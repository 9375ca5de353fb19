"""GPU (handles, not scans): every refusal of the manifold's create / Update / results entry points, for all six handle kinds --
dpe_bcm_create*, dpe_bcm_update*, dpe_bcm_results*, dpe_bcm_refine_scores, dpe_bcm_refine_keys -- that valid handles and small
arrays can reach, through engine.lib() directly.  The error's FULL text is compared with the literal strings below, and a refused
call leaves its handle usable: the same valid Update and results call gives the same bytes before and after the refusals.

Left out: refusals that need an allocation failure, a HIP error, a launch failure (hipGraph capture, "launch failed") or device
state that only a broken input produces -- fetch_device_frame's two ("DopplerSign on the device is not +/-1", "more candidate
points than the device list holds") and "arg-max index outside ...".  Nothing here provokes a fault.

Shapes: 7^4-point grids or 7-entry axes, two windows, maxChannels 8; the LDS-budget refusals use 37 channels x L 172 (L 176 for
the 12-byte entries), at create time only, where nothing has been allocated yet."""
import ctypes as C

import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from navlab_dpe_sdr_amd.grid_axes import GridAxesC
from tests import helpers

pytestmark = pytest.mark.gpu
E = dpe.engine
P = "[BatchCorrManifold] "
FS, S, K, W, L, B = 2.5e6, 12500, 8, 2, 8, 32
KW = dict(lag_half_width=L, bin_half_width=B, max_windows=W, max_channels=K)


def refused(rc, text):
    assert rc != 0
    assert E.lib().dpe_last_error().decode() == P + text


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def world():
    import torch
    case = helpers.make_case(seed=3, fs=FS, S=S, K=K, G=2401, W=W, grid="uniform")
    _iq, _cs, ce, bw = helpers.pack_gpu_inputs(case)
    g = torch.Generator().manual_seed(5)
    code = torch.rand(W * K * (2 * L + 1) * 2, generator=g).to("cuda:0")      # any banks will do: no score is looked at
    carr = torch.rand(W * K * (2 * B + 1) * 2, generator=g).to("cuda:0")
    ax = dpe.GridAxes.uniform(7, 1.0)
    return dict(pos=case["pos"], vel=case["vel"], C=case["C"], ce=ce, bw=bw, code=code, carr=carr, ax=ax,
                cp=C.c_void_p(code.data_ptr()), rp=C.c_void_p(carr.data_ptr()))


def config(world, axes=False, **over):
    f = dict(samplesPerWindow=S, lagHalfWidth=L, binHalfWidth=B, lPower=1, maxWindows=W, maxChannels=K, numFFTPoints=world["C"],
             samplingFrequency=FS, posGridSize=2401, velGridSize=2401, posGridIndexOffset=0, velGridIndexOffset=0, writeScores=1,
             weightedMean=0, referencePair=0, reserved=0)
    if not axes:
        dp = C.POINTER(C.c_double)
        f.update(posGrid=world["pos"].ctypes.data_as(dp), velGrid=world["vel"].ctypes.data_as(dp))
    f.update(over)
    return E.BcmConfig(**f)


BIG = dict(maxChannels=37, lagHalfWidth=172)      # 37 x (345 x 16 + 32) = 205424 B of banks


def test_create_refusals(world):
    lib, out = E.lib(), C.c_void_p()
    o = C.byref(out)
    c = lambda **kw: C.byref(config(world, **kw))
    far = world["pos"].copy()
    far[0, 0] = 4000.0
    dp = C.POINTER(C.c_double)
    plain = [
        (dict(samplesPerWindow=12501), "create: samplesPerWindow must be even and positive"),
        (dict(samplesPerWindow=0), "create: samplesPerWindow must be even and positive"),
        (dict(samplingFrequency=0.0), "create: bad fs / numFFTPoints"),
        (dict(numFFTPoints=0), "create: bad fs / numFFTPoints"),
        (dict(maxWindows=0), "create: maxWindows/maxChannels out of range"),
        (dict(maxChannels=38), "create: maxWindows/maxChannels out of range"),
        (dict(lagHalfWidth=0), "create: bad L/B/LPower"),
        (dict(lPower=0), "create: bad L/B/LPower"),
        (dict(posGrid=None), "create: grids missing"),
        (dict(velGridSize=0), "create: grids missing"),
        (dict(posGridIndexOffset=0xFFFFFFFF), "create: global grid index exceeds 32 bits"),
        (dict(maxChannels=37, lagHalfWidth=176), "create: score banks (156732 B even as 12-byte entries) exceed the 160 KB LDS"),
        (dict(posGrid=far.ctypes.data_as(dp)), "create: position grid extends beyond 3 km from its centre"),
        (dict(referencePair=1, writeScores=0), "create: referencePair needs writeScores (the arg-max is re-derived from the patched scores)"),
    ]
    refused(lib.dpe_bcm_create(None, o), "create: null argument")
    refused(lib.dpe_bcm_create(c(), None), "create: null argument")
    for over, text in plain:
        refused(lib.dpe_bcm_create(c(**over), o), text)
    # the family wrappers: their own checks under their own name, then the point-list create's under "create"
    for call, name in ((lambda cf: lib.dpe_bcm_create_joint(cf, 2, 12, o), "create_joint"), (lambda cf: lib.dpe_bcm_create_epochs(cf, 2, 0, o), "create_epochs"),
                       (lambda cf: lib.dpe_bcm_create_subsets(cf, 8, o), "create_subsets")):
        refused(call(None), name + ": null argument")
        refused(call(c(posGridIndexOffset=1)), name + ": grid shards are not supported (the index offsets must be 0)")
        refused(call(c(velGridIndexOffset=1)), name + ": grid shards are not supported (the index offsets must be 0)")
        refused(call(c(samplesPerWindow=12501)), "create: samplesPerWindow must be even and positive")
        refused(call(c(posGrid=None)), "create: grids missing")
    refused(lib.dpe_bcm_create_joint(c(), 2, 12, None), "create_joint: null argument")
    refused(lib.dpe_bcm_create_joint(c(), 9, 12, o), "create_joint: maxRx 9 out of range (1 .. 8 receivers)")
    refused(lib.dpe_bcm_create_joint(c(), 0, 12, o), "create_joint: maxRx 0 out of range (1 .. 8 receivers)")
    refused(lib.dpe_bcm_create_joint(c(), 2, 65, o), "create_joint: maxChannelsTotal 65 out of range (1 .. 64 (receiver, SV) pairs)")
    refused(lib.dpe_bcm_create_joint(c(), 2, 4, o), "create_joint: maxChannels 8 (the bound per receiver) exceeds maxChannelsTotal 4")
    refused(lib.dpe_bcm_create_joint(c(weightedMean=1), 2, 12, o),
            "create_joint: the weighted-mean estimator is not formed for several receivers (weightedMean must be 0)")
    refused(lib.dpe_bcm_create_joint(c(referencePair=1), 2, 12, o),
            "create_joint: referencePair is a single-receiver mode (it re-evaluates one receiver's first channel)")
    refused(lib.dpe_bcm_create_joint(c(**BIG), 2, 37, o),
            "create_joint: the score banks of 37 (receiver, SV) pairs x 345 entries (205424 B) exceed the 150 KB the joint scan keeps in LDS")
    refused(lib.dpe_bcm_create_epochs(c(), 2, 0, None), "create_epochs: null argument")
    refused(lib.dpe_bcm_create_epochs(c(maxChannels=0), 2, 0, o), "create_epochs: maxWindows/maxChannels out of range")
    refused(lib.dpe_bcm_create_epochs(c(), 3, 0, o), "create_epochs: maxEpochs 3 out of range (1 .. maxWindows = 2)")
    refused(lib.dpe_bcm_create_epochs(c(), 0, 0, o), "create_epochs: maxEpochs 0 out of range (1 .. maxWindows = 2)")
    refused(lib.dpe_bcm_create_epochs(c(binHalfWidth=0), 2, 0, o), "create_epochs: bad L/B")
    refused(lib.dpe_bcm_create_epochs(c(weightedMean=1), 2, 0, o),
            "create_epochs: the weighted-mean estimator is not formed for summed windows (weightedMean must be 0)")
    refused(lib.dpe_bcm_create_epochs(c(referencePair=1), 2, 0, o),
            "create_epochs: referencePair is a single-window mode (it re-evaluates one window's first channel)")
    refused(lib.dpe_bcm_create_epochs(c(**BIG), 2, 0, o), "create_epochs: the score banks of one window (37 channels x 345 entries, 205424 B) exceed "
            "the 150 KB the epochs scan keeps in LDS (no 12-byte bank entries here)")
    refused(lib.dpe_bcm_create_epochs(c(), 2, 4, o),
            "create_epochs: pairsPerPass 4 is below maxChannels 8 (a pass holds whole windows; 0 = as many as the LDS holds)")
    refused(lib.dpe_bcm_create_subsets(c(), 8, None), "create_subsets: null argument")
    refused(lib.dpe_bcm_create_subsets(c(), 17, o), "create_subsets: maxSubsets 17 out of range (1 .. 16 subsets per window)")
    refused(lib.dpe_bcm_create_subsets(c(), 0, o), "create_subsets: maxSubsets 0 out of range (1 .. 16 subsets per window)")
    refused(lib.dpe_bcm_create_subsets(c(maxWindows=0), 8, o), "create_subsets: maxWindows/maxChannels out of range")
    refused(lib.dpe_bcm_create_subsets(c(lagHalfWidth=0), 8, o), "create_subsets: bad L/B")
    refused(lib.dpe_bcm_create_subsets(c(weightedMean=1), 8, o),
            "create_subsets: the weighted-mean estimator is not formed per subset (weightedMean must be 0)")
    refused(lib.dpe_bcm_create_subsets(c(referencePair=1), 8, o), "create_subsets: referencePair re-evaluates the full set only (referencePair must be 0)")
    refused(lib.dpe_bcm_create_subsets(c(**BIG), 8, o), "create_subsets: the score banks of 37 channels x 345 entries (205424 B) exceed the 150 KB the "
            "subsets scan keeps in LDS (no 12-byte bank entries here)")
    assert out.value is None      # no refused create handed a handle out


def test_create_sharing_refusals(world):
    lib, out = E.lib(), C.c_void_p()
    donor = dpe.BatchCorrManifold(FS, S, world["C"], world["pos"], world["vel"], **KW)
    donor.Start()
    try:
        cfg = config(world, posGridSize=2400)
        refused(lib.dpe_bcm_create_sharing(C.byref(cfg), donor._h, C.byref(out)), "create: the grids to share are not these grids")
        ax = world["ax"]
        pa, va = ax.c_struct(), ax.c_struct()
        cfg = config(world, axes=True)
        refused(lib.dpe_bcm_create_axes_sharing(C.byref(cfg), C.byref(pa), C.byref(va), donor._h, C.byref(out)),
                "create: the grids to share are not these grids")
        assert out.value is None
        donor.Update(world["cp"].value, world["rp"].value, world["bw"], world["ce"])
        assert len(donor.results()) == W
    finally:
        donor.Stop()


def test_create_axes_and_refine_refusals(world):
    lib, out = E.lib(), C.c_void_p()
    o = C.byref(out)
    ax, ax3 = world["ax"], dpe.GridAxes.uniform(3, 10.0)
    c = lambda **kw: C.byref(config(world, axes=True, **kw))
    s = lambda a: C.byref(a.c_struct())
    dp = C.POINTER(C.c_double)
    axes = lambda cf, p=ax, v=ax: lib.dpe_bcm_create_axes(cf, s(p), s(v), o)

    def refine(cf, levels=((ax, ax), (ax3, ax3))):
        n = len(levels)
        pa, va = (GridAxesC * max(n, 1))(), (GridAxesC * max(n, 1))()
        for i, (p, v) in enumerate(levels):
            pa[i], va[i] = p.c_struct(), v.c_struct()
        return lib.dpe_bcm_create_refine(cf, n, pa, va, o)

    rc = lambda **kw: c(posGridSize=0, velGridSize=0, **kw)      # (a refine handle's sizes come from its levels)
    refused(lib.dpe_bcm_create_axes(c(), None, s(ax), o), "create_axes: null argument")
    refused(lib.dpe_bcm_create_axes(c(), s(ax), s(ax), None), "create_axes: null argument")
    refused(lib.dpe_bcm_create_refine(rc(), 1, None, s(ax), o), "create_refine: null argument")
    refused(axes(c(posGrid=world["pos"].ctypes.data_as(dp))), "create_axes: posGrid / velGrid must be NULL (the grids are the axes)")
    refused(axes(c(referencePair=1)), "create_axes: referencePair is not supported with grid axes")
    refused(refine(rc(), ()), "create_refine: nLevels 0 out of range (1 .. 4 levels)")
    refused(refine(rc(), ((ax, ax),) * 5), "create_refine: nLevels 5 out of range (1 .. 4 levels)")
    refused(refine(rc(velGrid=world["vel"].ctypes.data_as(dp))), "create_refine: posGrid / velGrid must be NULL (the grids are the levels' axes)")
    refused(refine(rc(weightedMean=1)), "create_refine: the weighted-mean estimator is not formed per level (weightedMean must be 0)")
    refused(refine(rc(referencePair=1)), "create_refine: referencePair is not supported with grid axes (referencePair must be 0)")
    refused(refine(rc(posGridIndexOffset=1)), "create_refine: grid shards are not supported (the index offsets must be 0)")
    for call, cf, name in ((axes, c, "create_axes"), (refine, rc, "create_refine")):
        refused(call(cf(samplesPerWindow=-2)), name + ": samplesPerWindow must be even and positive")
        refused(call(cf(samplingFrequency=-1.0)), name + ": bad fs / numFFTPoints")
        refused(call(cf(maxChannels=38)), name + ": maxWindows/maxChannels out of range")
        refused(call(cf(binHalfWidth=0)), name + ": bad L/B/LPower")
        refused(call(cf(**BIG)), name + ": score banks (204240 B) and the score stage (17408 B) exceed the LDS (no 12-byte bank entries with grid axes)")
    inf = dpe.GridAxes([0.0, np.inf], [0.0], [0.0], [0.0])
    nan = dpe.GridAxes([0.0], [np.nan], [0.0], [0.0])
    wide = dpe.GridAxes.uniform((70000, 70000, 1, 1), 1e-3)
    far = dpe.GridAxes.uniform(3, 900.0)
    empty = ax.c_struct()
    empty.dim[2] = 0
    noarr = ax.c_struct()
    noarr.axis[1] = None
    refused(lib.dpe_bcm_create_axes(c(), C.byref(empty), s(ax), o), "create_axes: position axis 2: dim 0 < 1 or no array")
    refused(lib.dpe_bcm_create_axes(c(), s(ax), C.byref(noarr), o), "create_axes: velocity axis 1: dim 7 < 1 or no array")
    refused(axes(c(posGridSize=2), inf, ax), "create_axes: position axis 0 entry 1 is not finite")
    refused(axes(c(velGridSize=1), ax, nan), "create_axes: velocity axis 1 entry 0 is not finite")
    refused(axes(c(), wide, ax), "create_axes: position grid index does not fit 32 bits")
    refused(axes(c(posGridSize=2402)), "create_axes: position slice [0, 2402) beyond the axis product 2401")
    refused(axes(c(velGridSize=2400, velGridIndexOffset=2)), "create_axes: velocity slice [2, 2402) beyond the axis product 2401")
    refused(axes(c(velGridSize=0)), "create_axes: velocity slice [0, 0) beyond the axis product 2401")
    refused(axes(c(posGridSize=81, velGridSize=81), dpe.GridAxes.uniform(3, 2000.0), ax3), "create_axes: position grid extends beyond 3 km from its centre")
    pa = (GridAxesC * 2)(ax.c_struct(), empty)
    va = (GridAxesC * 2)(ax.c_struct(), ax.c_struct())
    refused(lib.dpe_bcm_create_refine(rc(), 2, pa, va, o), "create_refine: level 1 position axis 2: dim 0 < 1 or no array")
    refused(refine(rc(), ((inf, ax3),)), "create_refine: level 0 position axis 0 entry 1 is not finite")
    refused(refine(rc(), ((ax, ax), (ax3, nan))), "create_refine: level 1 velocity axis 1 entry 0 is not finite")
    refused(refine(rc(), ((wide, ax3),)), "create_refine: level 0 position grid index does not fit 32 bits")
    refused(refine(rc(), ((far, ax3), (far, ax3))), "create_refine: the levels' position grids together extend beyond 3 km from the window centre "
            "(sum of the corner distances 3117.7 m)")
    assert out.value is None


class Handles:
    """One started handle of each kind, and per kind the valid Update + results call whose output bytes a refusal must not change."""

    def __init__(self, world):
        w = self.w = world
        a = (FS, S, w["C"])
        ax3 = dpe.GridAxes.uniform(3, 0.25)
        self.h = dict(plain=dpe.BatchCorrManifold(*a, w["pos"], w["vel"], **KW), axes=dpe.BatchCorrManifold(*a, w["ax"], w["ax"], **KW),
                      joint=dpe.JointManifold(*a, w["pos"], w["vel"], 2, 12, **KW), epochs=dpe.EpochManifold(*a, w["pos"], w["vel"], 2, **KW),
                      subsets=dpe.SubsetManifold(*a, w["pos"], w["vel"], 8, **KW), refine=dpe.RefineManifold(*a, [(w["ax"], w["ax"]), (ax3, ax3)], **KW))
        self.masks = E.leave_one_out_masks(K)
        for h in self.h.values():
            h.Start()

    def rx(self, k0=K, k1=4):
        w = self.w
        return [[dict(code=w["cp"].value + wi * K * (2 * L + 1) * 8, carr=w["rp"].value + wi * K * (2 * B + 1) * 8, win=w["bw"][wi], chan=w["ce"][wi][:k])
                 for k in (k0, k1)] for wi in range(W)]

    def snapshot(self, kind):
        w, h = self.w, self.h[kind]
        bank = (w["cp"].value, w["rp"].value)
        if kind == "joint":
            h.Update(self.rx())
            res = (E.BcmJointResult * W)(), (E.BcmJointRxResult * (2 * W))()
            E._check(E.lib().dpe_bcm_results_joint(h._h, res[0], res[1], None))
        elif kind == "epochs":
            h.Update(*bank, w["bw"], w["ce"], 2)
            res = ((E.BcmEpochsResult * 1)(),)
            E._check(E.lib().dpe_bcm_results_epochs(h._h, res[0], None))
        elif kind == "subsets":
            h.Update(*bank, w["bw"], w["ce"], self.masks)
            res = (E.BcmSubsetResult * W)(), (E.BcmSubsetResult * (W * K))(), (C.c_int64 * (W * 2 * K))()
            E._check(E.lib().dpe_bcm_results_subsets(h._h, res[0], res[1], res[2], None))
        elif kind == "refine":
            h.Update(*bank, w["bw"], w["ce"])
            res = ((E.BcmRefineResult * W)(),)
            E._check(E.lib().dpe_bcm_results_refine(h._h, res[0], None))
        else:
            h.Update(*bank, w["bw"], w["ce"])
            res = ((E.BcmResult * W)(),)
            E._check(E.lib().dpe_bcm_results(h._h, res[0], None))
        return b"".join(bytes(r) for r in res)

    def close(self):
        for h in self.h.values():
            h.Stop()


@pytest.fixture(scope="module")
def handles(world):
    hs = Handles(world)
    yield hs
    hs.close()


FAMILY = dict(joint=("scans several receivers", "joint"), epochs=("sums consecutive windows", "epochs"), subsets=("scans SV subsets", "subsets"),
              refine=("scans coarse-to-fine levels", "refine"))


def test_fresh_handles_have_no_results(world):
    """Before the first Update (own handles: the shared ones have been updated by then)."""
    hs = Handles(world)
    lib = E.lib()
    try:
        big = (C.c_char * 4096)()
        refused(lib.dpe_bcm_results(hs.h["plain"]._h, big, None), "results: no update yet")
        refused(lib.dpe_bcm_results(hs.h["axes"]._h, big, None), "results: no update yet")
        refused(lib.dpe_bcm_results(hs.h["joint"]._h, big, None), "results: no update yet")      # (before the cross-family refusal)
        refused(lib.dpe_bcm_results_joint(hs.h["joint"]._h, big, big, None), "results_joint: no joint update yet")
        refused(lib.dpe_bcm_results_epochs(hs.h["epochs"]._h, big, None), "results_epochs: no epochs update yet")
        refused(lib.dpe_bcm_results_subsets(hs.h["subsets"]._h, big, big, None, None), "results_subsets: no subsets update yet")
        refused(lib.dpe_bcm_results_refine(hs.h["refine"]._h, big, None), "results_refine: no refine update yet")
        for kind in hs.h:
            assert len(hs.snapshot(kind)) > 0
    finally:
        hs.close()


@pytest.mark.parametrize("kind", ["plain", "axes"])
def test_plain_update_and_results_refusals(world, handles, kind):
    lib, h = E.lib(), handles.h[kind]._h
    before = handles.snapshot(kind)
    cp, rp, bw, ce = world["cp"], world["rp"], world["bw"], world["ce"]
    bad = bw.copy()
    bad["dopplerSign"][1] = 0
    ports = E.BcmPortsDev(dimT=1, reserved=0)
    refused(lib.dpe_bcm_update(None, cp, rp, W, K, vp(bw), vp(ce), None), "Update: null argument")
    refused(lib.dpe_bcm_update(h, None, rp, W, K, vp(bw), vp(ce), None), "Update: null argument")
    refused(lib.dpe_bcm_update(h, cp, rp, W, K, None, vp(ce), None), "Update: null argument")
    refused(lib.dpe_bcm_update(h, cp, rp, W, K, vp(bw), None, None), "Update: null argument")
    refused(lib.dpe_bcm_update(h, cp, rp, 0, K, vp(bw), vp(ce), None), "Update: nWindows 0 out of range")
    refused(lib.dpe_bcm_update(h, cp, rp, 3, K, vp(bw), vp(ce), None), "Update: nWindows 3 out of range")
    refused(lib.dpe_bcm_update(h, cp, rp, W, 9, vp(bw), vp(ce), None), "Update: nChan 9 out of range")
    refused(lib.dpe_bcm_update(h, cp, rp, W, 0, vp(bw), vp(ce), None), "Update: nChan 0 out of range")
    refused(lib.dpe_bcm_update(h, cp, rp, W, K, vp(bad), vp(ce), None), "Update: dopplerSign must be +/-1")
    refused(lib.dpe_bcm_update_dev(h, cp, rp, K, None, C.c_double(0.0), None), "Update: null argument")
    refused(lib.dpe_bcm_update_dev(h, cp, rp, 9, C.byref(ports), C.c_double(0.0), None), "Update: nChan 9 out of range")
    refused(lib.dpe_bcm_update_dev(h, cp, rp, K, C.byref(ports), C.c_double(0.0), None), "Update: a device port pointer is null / dimT < 1")
    refused(lib.dpe_bcm_update_prepared(None, cp, rp, K, None), "Update: null argument")
    refused(lib.dpe_bcm_update_prepared(h, cp, rp, 99, None), "Update: nChan 99 out of range")
    refused(lib.dpe_bcm_results(h, None, None), "results: no update yet")
    big = (C.c_char * 4096)()
    p = C.c_void_p()
    refused(lib.dpe_bcm_update_joint(h, W, 2, big, None), "update_joint: the handle was not made by dpe_bcm_create_joint")
    refused(lib.dpe_bcm_update_epochs(h, cp, rp, 1, 2, K, vp(bw), vp(ce), None), "update_epochs: the handle was not made by dpe_bcm_create_epochs")
    refused(lib.dpe_bcm_update_subsets(h, cp, rp, W, K, vp(bw), vp(ce), 0, None, None), "update_subsets: the handle was not made by dpe_bcm_create_subsets")
    refused(lib.dpe_bcm_update_refine(h, cp, rp, W, K, vp(bw), vp(ce), None), "update_refine: the handle was not made by dpe_bcm_create_refine")
    refused(lib.dpe_bcm_results_joint(h, big, big, None), "results_joint: no joint update yet")
    refused(lib.dpe_bcm_results_epochs(h, big, None), "results_epochs: the handle was not made by dpe_bcm_create_epochs")
    refused(lib.dpe_bcm_results_subsets(h, big, big, None, None), "results_subsets: the handle was not made by dpe_bcm_create_subsets")
    refused(lib.dpe_bcm_results_refine(h, big, None), "results_refine: the handle was not made by dpe_bcm_create_refine")
    refused(lib.dpe_bcm_refine_scores(h, 0, C.byref(p), None, None, None), "refine_scores: the handle was not made by dpe_bcm_create_refine")
    refused(lib.dpe_bcm_refine_keys(h, 0, C.byref(p)), "refine_keys: the handle was not made by dpe_bcm_create_refine")
    assert handles.snapshot(kind) == before


@pytest.mark.parametrize("kind", sorted(FAMILY))
def test_cross_family_refusals(world, handles, kind):
    """The plain entry points on a family's handle: refused first, whatever else is wrong with the call."""
    lib, h = E.lib(), handles.h[kind]._h
    before = handles.snapshot(kind)
    what, name = FAMILY[kind]
    cp, rp, bw, ce = world["cp"], world["rp"], world["bw"], world["ce"]
    text = "Update: this handle %s (dpe_bcm_create_%s): use dpe_bcm_update_%s" % (what, name, name)
    ports = E.BcmPortsDev(dimT=1, reserved=0)
    refused(lib.dpe_bcm_update(h, cp, rp, W, K, vp(bw), vp(ce), None), text)
    refused(lib.dpe_bcm_update(h, cp, rp, 99, 99, vp(bw), vp(ce), None), text)      # (before the range checks)
    refused(lib.dpe_bcm_update_dev(h, cp, rp, 99, C.byref(ports), C.c_double(0.0), None), text)
    if kind in ("joint", "refine"):
        refused(lib.dpe_bcm_update_prepared(h, cp, rp, 99, None), text)
    else:
        refused(lib.dpe_bcm_update_prepared(h, cp, rp, 99, None), "Update: nChan 99 out of range")
    big = (C.c_char * 4096)()
    refused(lib.dpe_bcm_results(h, big, None), "results: this handle %s (dpe_bcm_create_%s): use dpe_bcm_results_%s" % (what, name, name))
    assert handles.snapshot(kind) == before


def test_joint_refusals(world, handles):
    lib, h = E.lib(), handles.h["joint"]._h
    before = handles.snapshot("joint")

    def update(rx, n_windows=W, n_rx=2):
        arr = (E.BcmJointRx * (len(rx) * len(rx[0])))()
        keep = []
        for i, x in enumerate(r for win in rx for r in win):
            chan = np.ascontiguousarray(x["chan"]) if x["chan"] is not None else None
            keep.append(chan)
            arr[i].codeBank_dev, arr[i].carrBank_dev = x["code"], x["carr"]
            arr[i].chan_host = chan.ctypes.data_as(C.POINTER(E.ChanEnd)) if chan is not None else None
            arr[i].win = E.BcmWindow.from_buffer_copy(np.ascontiguousarray(x["win"]).tobytes())
            arr[i].nChan = x.get("n", 0 if chan is None else chan.shape[0])
        return lib.dpe_bcm_update_joint(h, n_windows, n_rx, arr, None)

    def with_rx1(**kw):
        rx = handles.rx()
        rx[0][1] = dict(rx[0][1], **kw)
        return rx

    sign, rot = world["bw"][0].copy(), world["bw"][0].copy()
    sign["dopplerSign"] = 2
    rot["enu2ecef"][0] = np.nextafter(rot["enu2ecef"][0], 2.0)
    refused(lib.dpe_bcm_update_joint(h, W, 2, None, None), "update_joint: null argument")
    refused(lib.dpe_bcm_update_joint(None, W, 2, None, None), "update_joint: null argument")
    refused(update(handles.rx(), n_windows=3), "update_joint: nWindows 3 out of range")
    refused(update(handles.rx(), n_rx=3), "update_joint: nRx 3 out of range (the handle holds 2 receivers)")
    refused(update(handles.rx(), n_rx=0), "update_joint: nRx 0 out of range (the handle holds 2 receivers)")
    refused(update(with_rx1(code=None)), "update_joint: window 0 receiver 1: null pointer")
    refused(update(with_rx1(chan=None)), "update_joint: window 0 receiver 1: null pointer")
    refused(update(with_rx1(n=9)), "update_joint: window 0 receiver 1: nChan 9 out of range (1 .. 8)")
    refused(update(with_rx1(win=sign)), "update_joint: dopplerSign must be +/-1")
    refused(update(with_rx1(win=rot)), "update_joint: window 0: receiver 1's enu2ecef differs from receiver 0's (one grid offset must mean one "
            "ECEF displacement for every receiver: pass bit-equal matrices)")
    refused(update(handles.rx(K, K)), "update_joint: window 0 has 16 (receiver, SV) pairs, the handle holds 12")
    big = (C.c_char * 4096)()
    refused(lib.dpe_bcm_results_joint(h, None, big, None), "results_joint: null argument")
    refused(lib.dpe_bcm_results_joint(h, big, None, None), "results_joint: null argument")
    assert handles.snapshot("joint") == before


def test_epochs_refusals(world, handles):
    lib, h = E.lib(), handles.h["epochs"]._h
    before = handles.snapshot("epochs")
    cp, rp, bw, ce = world["cp"], world["rp"], world["bw"], world["ce"]
    bad = bw.copy()
    bad["dopplerSign"][1] = -2
    refused(lib.dpe_bcm_update_epochs(h, cp, rp, 1, 2, K, None, vp(ce), None), "update_epochs: null argument")
    refused(lib.dpe_bcm_update_epochs(h, None, rp, 1, 2, K, vp(bw), vp(ce), None), "update_epochs: null argument")
    refused(lib.dpe_bcm_update_epochs(h, cp, rp, 1, 3, K, vp(bw), vp(ce), None), "update_epochs: nEpochs 3 out of range (the handle holds 2 windows per group)")
    refused(lib.dpe_bcm_update_epochs(h, cp, rp, 1, 0, K, vp(bw), vp(ce), None), "update_epochs: nEpochs 0 out of range (the handle holds 2 windows per group)")
    refused(lib.dpe_bcm_update_epochs(h, cp, rp, 2, 2, K, vp(bw), vp(ce), None), "update_epochs: 2 groups of 2 windows out of range (maxWindows 2)")
    refused(lib.dpe_bcm_update_epochs(h, cp, rp, 0, 2, K, vp(bw), vp(ce), None), "update_epochs: 0 groups of 2 windows out of range (maxWindows 2)")
    refused(lib.dpe_bcm_update_epochs(h, cp, rp, 1, 2, 9, vp(bw), vp(ce), None), "update_epochs: nChan 9 out of range")
    refused(lib.dpe_bcm_update_epochs(h, cp, rp, 1, 2, K, vp(bad), vp(ce), None), "update_epochs: dopplerSign must be +/-1")
    refused(lib.dpe_bcm_results_epochs(h, None, None), "results_epochs: null argument")
    assert handles.snapshot("epochs") == before


def test_subsets_refusals(world, handles):
    lib, h = E.lib(), handles.h["subsets"]._h
    before = handles.snapshot("subsets")
    cp, rp, bw, ce = world["cp"], world["rp"], world["bw"], world["ce"]
    bad = bw.copy()
    bad["dopplerSign"][0] = 0
    m = np.ascontiguousarray(np.broadcast_to(handles.masks, (W, K)))
    empty, high = m.copy(), m.copy()
    empty[0, 1] = 0
    high[1, 0] = 0x100
    update = lambda n_win=W, n_chan=K, win=bw, n_sub=K, masks=m: lib.dpe_bcm_update_subsets(
        h, cp, rp, n_win, n_chan, vp(win), vp(ce), n_sub, None if masks is None else vp(masks), None)
    refused(lib.dpe_bcm_update_subsets(h, cp, None, W, K, vp(bw), vp(ce), K, vp(m), None), "update_subsets: null argument")
    refused(lib.dpe_bcm_update_subsets(h, cp, rp, W, K, vp(bw), None, K, vp(m), None), "update_subsets: null argument")
    refused(update(n_win=3), "update_subsets: nWindows 3 out of range")
    refused(update(n_chan=9), "update_subsets: nChan 9 out of range")
    refused(update(n_sub=9), "update_subsets: nSubsets 9 out of range (the handle holds 8 subsets per window)")
    refused(update(n_sub=-1), "update_subsets: nSubsets -1 out of range (the handle holds 8 subsets per window)")
    refused(update(masks=None), "update_subsets: null masks")
    refused(update(win=bad), "update_subsets: dopplerSign must be +/-1")
    refused(update(masks=empty), "update_subsets: window 0 subset 1: empty mask")
    refused(update(masks=high), "update_subsets: window 1 subset 0: mask 0x100 has a bit at or above nChan 8")
    big = (C.c_char * 4096)()
    refused(lib.dpe_bcm_results_subsets(h, None, big, None, None), "results_subsets: null argument")
    refused(lib.dpe_bcm_results_subsets(h, big, None, None, None), "results_subsets: null argument (the last Update ran 8 subsets)")
    assert handles.snapshot("subsets") == before


def test_refine_refusals(world, handles):
    lib, h = E.lib(), handles.h["refine"]._h
    before = handles.snapshot("refine")
    cp, rp, bw, ce = world["cp"], world["rp"], world["bw"], world["ce"]
    bad = bw.copy()
    bad["dopplerSign"][1] = 3
    p = C.c_void_p()
    refused(lib.dpe_bcm_update_refine(h, cp, rp, W, K, None, vp(ce), None), "update_refine: null argument")
    refused(lib.dpe_bcm_update_refine(h, cp, rp, 3, K, vp(bw), vp(ce), None), "update_refine: nWindows 3 out of range")
    refused(lib.dpe_bcm_update_refine(h, cp, rp, W, 9, vp(bw), vp(ce), None), "update_refine: nChan 9 out of range")
    refused(lib.dpe_bcm_update_refine(h, cp, rp, W, K, vp(bad), vp(ce), None), "update_refine: dopplerSign must be +/-1")
    refused(lib.dpe_bcm_results_refine(h, None, None), "results_refine: null argument")
    refused(lib.dpe_bcm_refine_scores(None, 0, C.byref(p), None, None, None), "refine_scores: null handle")
    refused(lib.dpe_bcm_refine_scores(h, 2, C.byref(p), None, None, None), "refine_scores: level 2 out of range (the handle holds 2 levels)")
    refused(lib.dpe_bcm_refine_scores(h, -1, C.byref(p), None, None, None), "refine_scores: level -1 out of range (the handle holds 2 levels)")
    refused(lib.dpe_bcm_refine_keys(h, 0, None), "refine_keys: null argument")
    refused(lib.dpe_bcm_refine_keys(h, 2, C.byref(p)), "refine_keys: level 2 out of range (the handle holds 2 levels)")
    noscores = dpe.RefineManifold(FS, S, world["C"], [(world["ax"], world["ax"])], write_scores=False, **KW)
    noscores.Start()
    try:
        refused(lib.dpe_bcm_refine_scores(noscores._h, 0, C.byref(p), None, None, None), "refine_scores: created with writeScores=0")
    finally:
        noscores.Stop()
    assert p.value is None
    assert handles.snapshot("refine") == before


def test_reference_pair_device_form_refusals(world):
    """referencePair is active only when S / 2 is a power of two: a handle of its own (16384 samples per window)."""
    lib = E.lib()
    h = dpe.BatchCorrManifold(FS, 16384, 16384, world["pos"], world["vel"], reference_pair=True, weighted_mean=True, **KW)
    h.Start()
    try:
        ports = E.BcmPortsDev(dimT=1, reserved=0)
        refused(lib.dpe_bcm_update_dev(h._h, world["cp"], world["rp"], K, C.byref(ports), C.c_double(0.0), None),
                "Update: referencePair with the device ports patches the scores on the device: it needs writeScores and no weightedMean "
                "(the weighted sums are corrected on the host in the host form only)")
        refused(lib.dpe_bcm_update_prepared(h._h, world["cp"], world["rp"], K, None),
                "Update: referencePair needs the port arrays: attach the device-resident channel "
                "manager (dpe_chm_dev_attach), or use dpe_bcm_update_dev / the host form of the inputs")
    finally:
        h.Stop()
