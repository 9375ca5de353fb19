"""CPU: the dpe_arr_ family exists in the header, the library and the Python layer, each symbol has its INTEGRATION.md row, the three
structs have the header's layout, DPE_ABI_VERSION is unchanged (the change is additive), dpe_arr.hip is one of the sources build()
compiles, dpe_arr_plan.h holds nothing of HIP, the refusals that need no device refuse with "[ArrayCombiner] ...", and without a
device dpe_arr_create fails loudly."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests.test_moments_abi_cpu import _header_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dpe_arr_create", "dpe_arr_destroy", "dpe_arr_info", "dpe_arr_process", "dpe_arr_stats", "dpe_arr_analyse")
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
    assert "dpe_arr.hip" in ge.HIP_SOURCES
    assert "## 7j." in open(os.path.join(ROOT, "DESIGN.md")).read() and "dpe_arr.hip" in open(os.path.join(ROOT, "README.md")).read()
    plan = open(os.path.join(ROOT, "navlab-dpe-sdr_amd", "csrc", "dpe_arr_plan.h")).read()
    assert "hip/hip_runtime" not in plan and "dpe_common.h" not in plan and "__global__" not in plan      # plain C++: nothing of HIP
    assert hdr.index("dpe_ix_analyse") < hdr.index("dpe_arr_create") < hdr.index("dpe_event_create")         # the section after the excisor's
    arr = open(os.path.join(ROOT, "navlab-dpe-sdr_amd", "csrc", "dpe_arr.hip")).read()
    assert arr.count("__global__") == 1 and "arr_apply(" in arr                                              # one kernel; the header's FMA chain


@pytest.mark.parametrize("cname,pytype,size", [("dpe_arr_config", "ArrConfig", 40), ("dpe_arr_info_t", "ArrInfo", 16), ("dpe_arr_stats_t", "ArrStats", 24)])
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
    assert C.sizeof(st) == (off + 3) // 4 * 4 == size


def test_python_face():
    assert dpe.ArrayCombiner is dpe.engine.ArrayCombiner and "ArrayCombiner" in dpe.__all__
    assert list(inspect.signature(dpe.ArrayCombiner.__init__).parameters) == ["self", "n_elements", "block_length", "constraints", "reference", "loading",
                                                                              "gain", "output"]
    d = {k: v.default for k, v in inspect.signature(dpe.ArrayCombiner.__init__).parameters.items()}
    assert (d["constraints"], d["reference"], d["loading"], d["gain"], d["output"]) == (None, 0, 1e-3, 1.0, "i16")
    assert list(inspect.signature(dpe.ArrayCombiner.needed).parameters) == ["self", "first", "count", "record_length"]
    assert list(inspect.signature(dpe.ArrayCombiner.process).parameters) == ["self", "x", "x_first", "out_first", "out_count", "record_length", "x_count", "out",
                                                                             "stream"]
    assert list(inspect.signature(dpe.ArrayCombiner.analyse).parameters)[:6] == ["self", "x", "x_first", "block_first", "block_count", "record_length"]
    assert all(callable(getattr(dpe.ArrayCombiner, n)) for n in ("stats", "info", "close"))
    p = inspect.signature(dpe.engine.steering_vectors).parameters
    assert list(p) == ["element_pos_m", "los_unit", "wavelength"] and p["wavelength"].default == 299792458.0 / 1575.42e6
    assert os.path.exists(os.path.join(ROOT, "scripts", "array_time.py"))


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except ImportError:
        return True


def _cfg(M=4, L=1024, B=1, ref=0, lam=1e-3, gain=1.0, fout=0):
    return dpe.engine.ArrConfig(lam, gain, M, L, B, ref, fout, 0)


def test_refusals_that_need_no_device(built):
    def refused(rc, pattern):
        assert rc != 0
        msg = built.dpe_last_error().decode()
        assert msg.startswith("[ArrayCombiner] ") and re.search(pattern, msg), msg

    h = C.c_void_p(None)
    nan, inf = float("nan"), float("inf")
    refused(built.dpe_arr_create(None, None, C.byref(h)), "create: null argument")
    refused(built.dpe_arr_create(C.byref(_cfg()), None, None), "create: null argument")
    for cfg, pat in ((_cfg(M=1), r"1 elements outside 2\.\.8"), (_cfg(M=9), r"9 elements outside 2\.\.8"), (_cfg(L=1000), r"L = 1000 is no power of two in 256\.\.65536"),
                     (_cfg(L=128), "L = 128 is no power of two"), (_cfg(L=131072), "L = 131072 is no power"), (_cfg(B=2), "2 constraints without constraint vectors"),
                     (_cfg(B=0), r"0 constraints outside 1\.\.4"), (_cfg(ref=4), r"reference element 4 outside 0\.\.3"), (_cfg(ref=-1), "reference element -1"),
                     (_cfg(lam=-1.0), "loading not finite or negative"), (_cfg(lam=nan), "loading not finite"), (_cfg(lam=inf), "loading not finite"),
                     (_cfg(gain=nan), "gain not finite"), (_cfg(gain=inf), "gain not finite"), (_cfg(fout=2), "output format 2 is neither")):
        refused(built.dpe_arr_create(C.byref(cfg), None, C.byref(h)), pat)
        assert not h.value
    cons = np.ones((2, 4), dtype=np.complex128)
    cons[1] = 0.0
    refused(built.dpe_arr_create(C.byref(_cfg(B=2)), cons.ctypes.data_as(C.POINTER(C.c_double)), C.byref(h)), "constraint 1 is zero")
    cons[1, 2] = complex(1.0, inf)
    refused(built.dpe_arr_create(C.byref(_cfg(B=2)), cons.ctypes.data_as(C.POINTER(C.c_double)), C.byref(h)), "constraint 1 is not finite")
    z = C.c_int64(0)
    refused(built.dpe_arr_process(None, None, z, z, C.c_int64(-1), None, z, C.c_int64(1), None), "process: null handle")
    refused(built.dpe_arr_analyse(None, None, z, z, C.c_int64(-1), z, C.c_int64(1), None, None, None, None), "analyse: null handle")
    refused(built.dpe_arr_info(None, None), "info: null argument")
    refused(built.dpe_arr_stats(None, None), "stats: null argument")
    assert built.dpe_arr_destroy(None) == 0
    with pytest.raises(dpe.DpeError, match=r"\[ArrayCombiner\] create: constraints of shape \(2, 3\), not \[B, 4\]"):
        dpe.ArrayCombiner(4, 1024, constraints=np.ones((2, 3)))
    with pytest.raises(dpe.DpeError, match=r"\[ArrayCombiner\] create: output 'i8' is neither"):
        dpe.ArrayCombiner(4, 1024, output="i8")


def test_create_fails_loudly_without_a_device(built):
    if _no_gpu():
        with pytest.raises(dpe.DpeError, match=r"\[ArrayCombiner\] create: no device memory"):
            dpe.ArrayCombiner(4, 1024)
    else:           # with a device the same call succeeds (tests/test_gpu_arr.py goes on from there)
        dpe.ArrayCombiner(4, 1024).close()
