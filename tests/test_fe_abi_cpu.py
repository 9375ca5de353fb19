"""CPU: the dpe_fe_ family exists in the header, the library and the Python layer, each symbol has its INTEGRATION.md row, the two
structs have the header's layout, DPE_ABI_VERSION is unchanged (the change is additive), dpe_fe.hip is one of the sources build()
compiles, dpe_fe_plan.h holds nothing of HIP, the refusals that need no device refuse with "[FrontEnd] ...", and without a device
dpe_fe_create fails loudly.  From the gfx950 assembly of dpe_fe.hip: the three forms of the convert kernel use no scratch, and
their tap loops run on packed fp32 FMAs fed by LDS reads and scalar tap loads."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import navlab_dpe_sdr_amd as dpe
from tests.isa_asm import asm_of
from tests.test_moments_abi_cpu import _header_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dpe_fe_create", "dpe_fe_destroy", "dpe_fe_info", "dpe_fe_convert", "dpe_fe_clipped")
SIZES = {"double": 8, "int64_t": 8, "int32_t": 4}
KERNEL = "_ZN3dpe9fe_kernelILi%dEEE"


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
        assert len(rows.get(n, "")) > 20 and "no counterpart" in rows[n] and "rawfile.py:140-158" in rows[n], n
    assert built.dpe_abi_version() == 4 and re.search(r"#define DPE_ABI_VERSION 4\b", hdr)
    assert "dpe_fe.hip" in ge.HIP_SOURCES
    assert "## 7h." in open(os.path.join(ROOT, "DESIGN.md")).read() and "dpe_fe.hip" in open(os.path.join(ROOT, "README.md")).read()
    plan = open(os.path.join(ROOT, "navlab-dpe-sdr_amd", "csrc", "dpe_fe_plan.h")).read()
    assert "hip/hip_runtime" not in plan and "dpe_common.h" not in plan and "__global__" not in plan      # plain C++: nothing of HIP
    for name, value in dpe.engine.FE_FORMATS.items():
        assert re.search(r"#define DPE_FE_%s %d\b" % (name, value), hdr), name


@pytest.mark.parametrize("cname,pytype,size", [("dpe_fe_config", "FeConfig", 72), ("dpe_fe_info_t", "FeInfo", 48)])
def test_struct_layout_against_the_header(cname, pytype, size):
    hdr = open(os.path.join(ROOT, "include", "dpe_hip.h")).read()
    st = getattr(dpe.engine, pytype)
    fields = _header_fields(hdr, cname)
    assert [f for _, f, _ in fields] == [f[0] for f in st._fields_]
    off = 0
    for ctype, field, dims in fields:      # natural alignment: every member of these structs is 4 or 8 bytes, or an array of such
        sz = SIZES[ctype]
        n = int(np.prod(dims)) if dims else 1
        off = (off + sz - 1) // sz * sz
        assert getattr(st, field).offset == off and getattr(st, field).size == sz * n, (cname, field)
        off += sz * n
    assert C.sizeof(st) == (off + 7) // 8 * 8 == size


def test_python_face():
    assert dpe.FrontEnd is dpe.engine.FrontEnd and dpe.frontend.convert_file and inspect.isgeneratorfunction(dpe.frontend.convert_file)
    assert list(inspect.signature(dpe.FrontEnd.__init__).parameters)[:5] == ["self", "fs_in", "fmt", "D", "taps"]
    assert list(inspect.signature(dpe.FrontEnd.convert).parameters)[:5] == ["self", "raw", "raw_first", "out_first", "out_count"]
    assert list(inspect.signature(dpe.frontend.design_lowpass).parameters) == ["D", "taps_per_phase", "beta", "cutoff"]
    assert list(inspect.signature(dpe.frontend.convert_file).parameters) == ["path", "fe", "chunk_out", "record_length"]
    assert os.path.exists(os.path.join(ROOT, "scripts", "frontend_time.py"))


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except ImportError:
        return True


def _cfg(fmt=0, out=0, D=4, T=33, fs=1e7, f_if=0.0, gain=1.0):
    return dpe.engine.FeConfig(fs, f_if, gain, (C.c_double * 4)(-3, -1, 1, 3), fmt, out, D, T)


def test_refusals_that_need_no_device(built):
    def refused(rc, pattern):
        assert rc != 0
        msg = built.dpe_last_error().decode()
        assert msg.startswith("[FrontEnd] ") and re.search(pattern, msg), msg

    h = C.c_void_p(None)
    taps = (C.c_double * 1025)(*([1.0] * 1025))
    refused(built.dpe_fe_create(None, taps, C.byref(h)), "create: null argument")
    refused(built.dpe_fe_create(C.byref(_cfg()), None, C.byref(h)), "create: null argument")
    refused(built.dpe_fe_create(C.byref(_cfg()), taps, None), "create: null argument")
    for cfg, pat in ((_cfg(T=32), r"T = 32 taps is even"), (_cfg(D=0), r"D = 0 outside 1\.\.64"), (_cfg(D=65), r"D = 65 outside 1\.\.64"),
                     (_cfg(T=1025), r"T = 1025 taps outside 1\.\.1023"), (_cfg(T=0), "T = 0 taps outside"), (_cfg(fmt=7), "input format 7"),
                     (_cfg(out=2), "output format 2"), (_cfg(fs=0.0), "sampling frequency"), (_cfg(f_if=2e7), "intermediate frequency"),
                     (_cfg(gain=float("nan")), "gain not finite")):
        refused(built.dpe_fe_create(C.byref(cfg), taps, C.byref(h)), pat)
        assert not h.value
    bad = (C.c_double * 33)(*([1.0] * 32 + [float("inf")]))
    refused(built.dpe_fe_create(C.byref(_cfg()), bad, C.byref(h)), "tap 32 not finite")
    refused(built.dpe_fe_convert(None, None, C.c_int64(0), C.c_int64(0), C.c_int64(-1), None, C.c_int64(0), C.c_int64(1), None), "convert: null handle")
    refused(built.dpe_fe_info(None, None), "info: null argument")
    refused(built.dpe_fe_clipped(None, None), "clipped: null argument")
    assert built.dpe_fe_destroy(None) == 0
    with pytest.raises(dpe.DpeError, match=r"\[FrontEnd\] create: input format 'I4C'"):
        dpe.FrontEnd(1e7, "I4C", 4, np.ones(33))


def test_create_fails_loudly_without_a_device(built):
    if _no_gpu():
        with pytest.raises(dpe.DpeError, match=r"\[FrontEnd\] create: no device memory"):
            dpe.FrontEnd(1e7, "I16C", 4, dpe.frontend.design_lowpass(4))
    else:           # with a device the same call succeeds (tests/test_gpu_fe.py goes on from there)
        dpe.FrontEnd(1e7, "I16C", 4, dpe.frontend.design_lowpass(4)).close()


# ---- assembly
@pytest.fixture(scope="module")
def asm():
    return asm_of("dpe_fe.hip")


def _kernel(text, prefix):
    m = re.search(r"\.amdhsa_kernel (%s\S*)\n(.*?)\.end_amdhsa_kernel" % re.escape(prefix), text, flags=re.S)
    assert m, prefix
    body = re.search(r"^%s:[^\n]*\n(.*?)\n\s*s_endpgm" % re.escape(m.group(1)), text, flags=re.S | re.M)
    assert body, prefix
    return dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2))), body.group(1)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_no_scratch_and_packed_tap_loop(asm, mode):
    d, body = _kernel(asm, KERNEL % mode)
    assert int(d["private_segment_fixed_size"]) == 0 and int(d.get("uses_dynamic_stack", "0")) == 0, mode
    assert int(d["next_free_vgpr"]) <= 64, (mode, d["next_free_vgpr"])          # eight waves per SIMD
    assert int(d["group_segment_fixed_size"]) == 0                                # the tile is the launch's dynamic allocation
    assert "scratch_" not in body
    # the tap loop: an unguarded group of five taps and up to four guarded ones, five outputs each, one packed FMA per output and
    # tap (two where taps and input are both complex).  Unpacked fp32 multiply-adds may only be the rotation's: two multiplies and
    # four FMAs per output, none in the form without a mixer (a handful remain in the decoders).
    per_tap = 10 if mode == 2 else 5
    ops = [ln.split()[0] for ln in body.splitlines() if ln.strip() and not ln.strip().startswith((";", "."))]
    assert ops.count("v_pk_fma_f32") >= 9 * per_tap, (mode, ops.count("v_pk_fma_f32"))
    scalar = sum(1 for op in ops if op.startswith(("v_fma", "v_mul_f32", "v_mac_f32", "v_pk_mul_f32")))
    assert scalar <= (4 if mode == 1 else 5 * 6 + 5 * 4), (mode, scalar)        # (and what sincospif's polynomials take)


def test_three_forms_are_emitted(asm):
    names = set(re.findall(r"\.amdhsa_kernel (_ZN3dpe9fe_kernel\S+)", asm))
    assert len(names) == 3 and {n[:len(KERNEL % 0)] for n in names} == {KERNEL % m for m in range(3)}, sorted(names)
