"""CPU: the dpe_syn_ family exists in the header, the library and the Python layer, each symbol has its INTEGRATION.md row, the two
structs have the header's layout, DPE_ABI_VERSION is unchanged (the change is additive), dpe_syn.hip is one of the sources build()
compiles, and without a device dpe_syn_create fails loudly while the refusals that need none refuse."""
import ctypes as C
import inspect
import os
import re

import pytest

import navlab_dpe_sdr_amd as dpe
from tests.test_moments_abi_cpu import _header_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dpe_syn_create", "dpe_syn_destroy", "dpe_syn_set_nav_bits", "dpe_syn_windows", "dpe_syn_record")
SIZES = {"double": 8, "int64_t": 8, "uint64_t": 8, "int32_t": 4, "float": 4, "ptr": 8}


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
        assert "correlator.py:367-465" in rows[n] and "rawfile.py:140-158" in rows[n], n
    assert built.dpe_abi_version() == 4 and re.search(r"#define DPE_ABI_VERSION 4\b", hdr)
    assert "dpe_syn.hip" in ge.HIP_SOURCES
    assert "## 7f." in open(os.path.join(ROOT, "DESIGN.md")).read() and "dpe_syn.hip" in open(os.path.join(ROOT, "README.md")).read()
    plan = open(os.path.join(ROOT, "navlab-dpe-sdr_amd", "csrc", "dpe_syn_plan.h")).read()
    assert "hip/hip_runtime" not in plan and "dpe_common.h" not in plan            # plain C++: nothing of HIP


@pytest.mark.parametrize("cname,pytype,size", [("dpe_syn_config", "SynConfig", 24), ("dpe_syn_signal", "SynSignal", 32)])
def test_struct_layout_against_the_header(cname, pytype, size):
    hdr = open(os.path.join(ROOT, "include", "dpe_hip.h")).read()
    st = getattr(dpe.engine, pytype)
    fields = _header_fields(hdr, cname)
    assert [f for _, f, _ in fields] == [f[0] for f in st._fields_]
    off = 0
    for ctype, field, dims in fields:      # natural alignment: every member of these structs is 4 or 8 bytes
        sz = SIZES[ctype]
        off = (off + sz - 1) // sz * sz
        assert getattr(st, field).offset == off and getattr(st, field).size == sz and not dims, (cname, field)
        off += sz
    assert C.sizeof(st) == (off + 7) // 8 * 8 == size


def test_python_face():
    assert dpe.Synthesizer is dpe.engine.Synthesizer
    assert list(inspect.signature(dpe.Synthesizer.windows).parameters)[:3] == ["self", "S", "chan"]
    assert list(inspect.signature(dpe.Synthesizer.record).parameters)[:4] == ["self", "first_sample", "n_samples", "chan"]
    sig = inspect.signature(dpe.pipeline.run_monte_carlo)
    assert list(sig.parameters)[:9] == ["ho", "fs", "S", "K", "pos_grid", "vel_grid", "cn0_dbhz", "n_real", "seed"]
    assert {"init_delta", "lpower", "weighted_mean"} <= set(sig.parameters)
    assert callable(dpe.synth.cn0_to_amp) and callable(dpe.synth.amp_to_cn0)
    for script in ("monte_carlo_cn0.py", "synth_time.py"):
        assert os.path.exists(os.path.join(ROOT, "scripts", script))
    assert "monte_carlo_cn0.py" in open(os.path.join(ROOT, "scripts", "monte_carlo.py")).read()


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except ImportError:
        return True


def test_refusals_that_need_no_device(built):
    def refused(rc, pattern):
        assert rc != 0
        msg = built.dpe_last_error().decode()
        assert msg.startswith("[Synthesizer]") and re.search(pattern, msg), msg

    h = C.c_void_p(None)
    refused(built.dpe_syn_create(None, C.byref(h)), "null argument")
    for cfg, pat in ((dpe.engine.SynConfig(0.0, 1, 1, 0, 0), "sampling frequency"), (dpe.engine.SynConfig(2.5e6, 0, 1, 0, 0), "maxSegments 0"),
                     (dpe.engine.SynConfig(2.5e6, 1, 38, 0, 0), r"maxChannels 38 outside 1\.\.37"), (dpe.engine.SynConfig(2.5e6, 1, 8, -1, 0), "maxNavBits")):
        refused(built.dpe_syn_create(C.byref(cfg), C.byref(h)), pat)
        assert not h.value
    refused(built.dpe_syn_windows(None, None, C.c_int64(0), 1, 1, 1, None, None, None, None, C.c_uint64(0), None), "windows: null handle")
    refused(built.dpe_syn_record(None, None, C.c_int64(0), C.c_int64(1), 1, None, None, None, C.c_uint64(0), None), "record: null handle")
    refused(built.dpe_syn_set_nav_bits(None, 0, None, 0, None), "set_nav_bits: null argument")
    assert built.dpe_syn_destroy(None) == 0


def test_create_fails_loudly_without_a_device(built):
    if _no_gpu():
        with pytest.raises(dpe.DpeError, match=r"\[Synthesizer\] create: no device memory"):
            dpe.Synthesizer(2.5e6, max_segments=4, max_channels=8, max_nav_bits=64)
    else:           # with a device the same call succeeds (tests/test_gpu_syn.py goes on from there)
        dpe.Synthesizer(2.5e6, max_segments=4, max_channels=8, max_nav_bits=64).close()
