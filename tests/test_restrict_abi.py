"""CPU-side checks of the MPS-valued restriction (qil_mps_restrict): declared with its signature, exported and bound; null
arguments come back before any device is touched, and that check sits ahead of the context activation in the source; the Python
front-ends (restrict, zt_row, zt_column, copy_marginal) are exported and reject a wrong-length spec, a spec value above 3 and an
index outside the register before the native entry is called; the Julia shim binds the entry and INTEGRATION.md names it."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QIL_EINVAL_ARG = 7

NAME = "qil_mps_restrict"
SIGNATURE = r"const qil_mps\* psi,\s*const uint8_t\* spec,\s*qil_mps\*\* out"
FRONT_ENDS = ("restrict", "zt_row", "zt_column", "copy_marginal")


def _lib():
    import importlib
    return importlib.import_module("qilaplace_jl_amd._lib")


def _source():
    return open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "qil_restrict.hip")).read()


def test_entry_is_declared_exported_and_prototyped():
    import qilaplace_jl_amd as qil
    L = _lib()
    decl = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qilaplace_hip.h")).read(), flags=re.S)
    so = ctypes.CDLL(qil.LIB_PATH)
    assert re.search(r"QIL_API\s+int\s+" + NAME + r"\s*\(\s*" + SIGNATURE + r"\s*\)\s*;", decl)
    assert hasattr(so, NAME)
    assert len(L.PROTOTYPES[NAME]) == 3
    for name in FRONT_ENDS:
        assert name in qil.__all__ and callable(getattr(qil, name)), name
    assert "qil_restrict.hip" in open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "Makefile")).read()


def test_null_arguments_precede_the_context_activation():
    """QIL_EINVAL_ARG with the documented message for a null psi, spec or out.  This runs on a machine without a GPU: an
    activation would fail with QIL_EHIP instead.  The non-null stand-ins are never dereferenced: a null comes first in every
    call."""
    L = _lib()
    out = ctypes.c_void_p()
    dummy = ctypes.create_string_buffer(4096)
    spec = (ctypes.c_uint8 * 4)(3, 3, 3, 3)
    handle = ctypes.c_void_p(ctypes.addressof(dummy))
    for args in ((None, spec, ctypes.byref(out)), (handle, None, ctypes.byref(out)), (handle, spec, None),
                 (None, None, None)):
        assert L.lib.qil_mps_restrict(*args) == QIL_EINVAL_ARG
        assert "mps_restrict: null argument" in L.last_error()
    assert out.value is None


def test_the_null_check_sits_first_in_the_body():
    src = _source()
    m = re.search(r'extern "C" int ' + NAME + r"\(.*?\n}\n", src, flags=re.S)
    assert m
    body = m.group(0)
    first = body[body.index("{") + 1:].lstrip()
    assert first.startswith('QIL_REQUIRE(psi && spec && out, QIL_EINVAL_ARG, "mps_restrict: null argument");')
    act = body.find("qil_ctx_activate")
    assert 0 <= body.find("QIL_EINVAL_ARG") < act
    # the spec is read after the activation, as qil_mps_block does
    assert act < body.find("QIL_EINVAL_CONFIG")
    assert "coefficient" in body[body.find("keeps no site"):][:120]


def test_the_restriction_has_kernels_of_its_own():
    code = re.sub(r"//[^\n]*", "", _source())
    assert re.search(r"__global__ __launch_bounds__\(kThreads\) void restrict_absorb_grouped\(", code)
    assert re.search(r"__global__ __launch_bounds__\(kThreads\) void restrict_runs_lds\(", code)
    assert "mfma_step(" in code                                         # the f64 MFMA tile step: one definition, in the shared header
    utils = open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "qil_device_utils.h")).read()
    assert utils.count("void mfma_step(") == 1 and utils.count("__builtin_amdgcn_mfma_f64_16x16x4f64(") == 4
    assert code.count("hipLaunchKernelGGL(restrict_absorb_grouped<") == 2       # one launch site per dtype: all sites in one grid
    assert "asm" not in code


class _Boom:
    def __init__(self):
        self.calls = 0

    def __call__(self, *a):
        self.calls += 1
        raise AssertionError("native call made before the argument checks")


def _fake(cls):
    """a container object that never touched the device: enough for the front-ends' checks"""
    x = object.__new__(cls)
    x.handle = None
    x.ctx = None
    return x


def test_python_checks_precede_the_native_entry(monkeypatch):
    """The chain length is the one thing the checks need from the handle; it is served here by a stand-in (6 tensors), and
    every other native entry the front-ends could reach raises."""
    import qilaplace_jl_amd as qil
    L = _lib()
    boom = _Boom()

    def nsites(handle, ref):
        ref._obj.value = 6
        return 0

    monkeypatch.setattr(L.lib, "qil_mps_nsites", nsites)
    for name in (NAME, "qil_mps_is_paired", "qil_mps_block", "qil_mps_clone"):
        monkeypatch.setattr(L.lib, name, boom)
    psi, zt = _fake(qil.SignalMPS), _fake(qil.ZTMPS)
    for state in (psi, zt):
        for bad in ([3] * 5, [3] * 7, [], np.full((2, 3), 3)):
            with pytest.raises(ValueError, match="expected 6 entries"):
                qil.restrict(state, bad)
        for bad in ([3, 3, 4, 3, 3, 3], [0, 1, 2, 3, 200, 0]):
            with pytest.raises(ValueError, match=r"outside \[0,3\]"):
                qil.restrict(state, bad)
    for bad in (None, np.zeros((1, 2, 1)), _fake(qil.SingleSiteMPO)):
        with pytest.raises(TypeError, match="restrict: unsupported operand types"):
            qil.restrict(bad, [3] * 6)
    for fn in (qil.zt_row, qil.zt_column):
        with pytest.raises(TypeError, match="needs a ZTMPS"):
            fn(psi, 0)
        for bad in (-1, 8, 1 << 40):                     # three sites per register: indices 0 .. 7
            with pytest.raises(ValueError, match="outside"):
                fn(zt, bad)
        for bad in (1.0, "1", None, True):
            with pytest.raises(TypeError, match="must be an integer"):
                fn(zt, bad)
    with pytest.raises(TypeError, match="needs a ZTMPS"):
        qil.copy_marginal(psi)
    assert boom.calls == 0


def test_julia_shim_and_documents_name_the_entry():
    src = open(os.path.join(ROOT, "julia", "QILaplaceHIP.jl")).read()
    assert re.search(r"function restrict\(psi::DeviceMPS, spec::AbstractVector\{<:Integer\}\)", src)
    assert f"(:{NAME}, LIB)" in src
    assert re.search(r"export .*\brestrict\b", src, flags=re.S)
    assert f"`{NAME}`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`restrict`" in open(os.path.join(ROOT, "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "examples", "zplane_row.py"))
    header = open(os.path.join(ROOT, "include", "qilaplace_hip.h")).read()
    for phrase in ("lazy form", "batch of specs", "Born marginals"):        # what is deliberately left out is said
        assert phrase in header, phrase
