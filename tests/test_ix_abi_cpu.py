"""CPU: the dpe_ix_ family exists in the header, the library and the Python layer, each symbol has its INTEGRATION.md row, the three
structs have the header's layout, DPE_ABI_VERSION is unchanged (the change is additive), dpe_ix.hip is one of the sources build()
compiles, dpe_ix_plan.h holds nothing of HIP, the refusals that need no device refuse with "[Excisor] ...", and without a device
dpe_ix_create fails loudly."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests.test_moments_abi_cpu import _header_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dpe_ix_create", "dpe_ix_destroy", "dpe_ix_info", "dpe_ix_process", "dpe_ix_stats", "dpe_ix_analyse")
SIZES = {"double": 8, "int64_t": 8, "int32_t": 4}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return dpe.engine.lib()


def test_new_symbols_exported_and_documented(built):
    import __graft_entry__ as ge
    hdr = open(os.path.join(ROOT, "include", "dpe_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("## 1b."):]
    rows = dict(re.findall(r"^\| `(dpe_[a-z0-9_]+)` \| (.+) \|$", sec, flags=re.M))
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(built, n) and n in dpe.engine.EXPORTS, n
        assert len(rows.get(n, "")) > 20 and "no counterpart" in rows[n], n
    assert built.dpe_abi_version() == 4 and re.search(r"#define DPE_ABI_VERSION 4\b", hdr)
    assert "dpe_ix.hip" in ge.HIP_SOURCES
    assert "## 7i." in open(os.path.join(ROOT, "DESIGN.md")).read() and "dpe_ix.hip" in open(os.path.join(ROOT, "README.md")).read()
    plan = open(os.path.join(ROOT, "navlab-dpe-sdr_amd", "csrc", "dpe_ix_plan.h")).read()
    assert "hip/hip_runtime" not in plan and "dpe_common.h" not in plan and "__global__" not in plan      # plain C++: nothing of HIP
    assert re.search(r"#define DPE_IX_IN_I16 0\b", hdr) and re.search(r"#define DPE_IX_IN_F32 1\b", hdr)
    assert hdr.index("dpe_fe_clipped") < hdr.index("dpe_ix_create") < hdr.index("dpe_event_create")            # the section after the front end's
    assert "must be finite" in hdr[hdr.index("Interference excision"):hdr.index("dpe_ix_create")]
    ix = open(os.path.join(ROOT, "navlab-dpe-sdr_amd", "csrc", "dpe_ix.hip")).read()
    assert "rocfft" not in ix.lower() and ix.count("__global__") == 1                                          # one kernel, no FFT library


@pytest.mark.parametrize("cname,pytype,size", [("dpe_ix_config", "IxConfig", 40), ("dpe_ix_info_t", "IxInfo", 24), ("dpe_ix_stats_t", "IxStats", 32)])
def test_struct_layout_against_the_header(cname, pytype, size):
    hdr = open(os.path.join(ROOT, "include", "dpe_hip.h")).read()
    st = getattr(dpe.engine, pytype)
    fields = _header_fields(hdr, cname)
    assert [f for _, f, _ in fields] == [f[0] for f in st._fields_]
    off = 0
    for ctype, field, dims in fields:      # natural alignment: every member of these structs is 4 or 8 bytes
        sz = SIZES[ctype]
        n = int(np.prod(dims)) if dims else 1
        off = (off + sz - 1) // sz * sz
        assert getattr(st, field).offset == off and getattr(st, field).size == sz * n, (cname, field)
        off += sz * n
    assert C.sizeof(st) == (off + 7) // 8 * 8 == size


def test_python_face():
    assert dpe.Excisor is dpe.engine.Excisor and "Excisor" in dpe.__all__
    assert list(inspect.signature(dpe.Excisor.__init__).parameters) == ["self", "N", "threshold", "guard", "blank_power", "gain", "static_mask", "in_f32",
                                                                        "out_f32"]
    d = {k: v.default for k, v in inspect.signature(dpe.Excisor.__init__).parameters.items()}
    assert (d["guard"], d["blank_power"], d["gain"], d["static_mask"], d["in_f32"], d["out_f32"]) == (1, 0.0, 1.0, None, False, False)
    assert list(inspect.signature(dpe.Excisor.needed).parameters) == ["self", "out_first", "out_count", "record_length"]
    assert list(inspect.signature(dpe.Excisor.process).parameters) == ["self", "x", "x_first", "out_first", "out_count", "record_length", "x_count", "out",
                                                                       "stream"]
    assert list(inspect.signature(dpe.Excisor.analyse).parameters)[:6] == ["self", "x", "x_first", "frame_first", "frame_count", "record_length"]
    assert callable(dpe.Excisor.stats) and callable(dpe.Excisor.close)
    # the adapter convert_file takes in place of a front end: the members convert_file reads
    for name in ("needed", "convert"):
        assert list(inspect.signature(getattr(dpe.frontend.Excised, name)).parameters) == list(inspect.signature(getattr(dpe.FrontEnd, name)).parameters)
    assert os.path.exists(os.path.join(ROOT, "scripts", "excise_time.py"))


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except ImportError:
        return True


def _cfg(N=1024, kappa=10.0, guard=1, blank=0.0, gain=1.0, fin=0, fout=0):
    return dpe.engine.IxConfig(kappa, blank, gain, N, guard, fin, fout)


def test_refusals_that_need_no_device(built):
    def refused(rc, pattern):
        assert rc != 0
        msg = built.dpe_last_error().decode()
        assert msg.startswith("[Excisor] ") and re.search(pattern, msg), msg

    h = C.c_void_p(None)
    nan, inf = float("nan"), float("inf")
    refused(built.dpe_ix_create(None, None, C.byref(h)), "create: null argument")
    refused(built.dpe_ix_create(C.byref(_cfg()), None, None), "create: null argument")
    for cfg, pat in ((_cfg(N=1000), r"N = 1000 is no power of two in 64\.\.4096"), (_cfg(N=32), "N = 32 is no power of two"), (_cfg(N=8192), "N = 8192 is no power"),
                     (_cfg(kappa=0.0), "threshold not finite or not positive"), (_cfg(kappa=-2.0), "threshold not finite or not positive"),
                     (_cfg(kappa=nan), "threshold not finite"), (_cfg(kappa=inf), "threshold not finite"), (_cfg(guard=-1), r"guard -1 outside 0\.\.511"),
                     (_cfg(N=64, guard=32), r"guard 32 outside 0\.\.31"), (_cfg(blank=-1.0), "blanking power not finite or negative"),
                     (_cfg(blank=inf), "blanking power not finite"), (_cfg(gain=nan), "gain not finite"), (_cfg(gain=inf), "gain not finite"),
                     (_cfg(fin=2), "input format 2 is neither"), (_cfg(fout=2), "output format 2 is neither")):
        refused(built.dpe_ix_create(C.byref(cfg), None, C.byref(h)), pat)
        assert not h.value
    z = C.c_int64(0)
    refused(built.dpe_ix_process(None, None, z, z, C.c_int64(-1), None, z, C.c_int64(1), None), "process: null handle")
    refused(built.dpe_ix_analyse(None, None, z, z, C.c_int64(-1), z, C.c_int64(1), None, None, None, None), "analyse: null handle")
    refused(built.dpe_ix_info(None, None), "info: null argument")
    refused(built.dpe_ix_stats(None, None, None), "stats: null argument")
    assert built.dpe_ix_destroy(None) == 0
    with pytest.raises(dpe.DpeError, match=r"\[Excisor\] create: the static mask holds 5 bins, the frame 64"):
        dpe.Excisor(64, 10.0, static_mask=np.ones(5))


def test_create_fails_loudly_without_a_device(built):
    if _no_gpu():
        with pytest.raises(dpe.DpeError, match=r"\[Excisor\] create: no device memory"):
            dpe.Excisor(1024, 10.0)
    else:           # with a device the same call succeeds (tests/test_gpu_ix.py goes on from there)
        dpe.Excisor(1024, 10.0).close()
