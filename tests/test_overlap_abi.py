"""CPU-side checks of the overlap entries (qil_inner, qil_apply_inner, qil_apply_norm): declared, exported, bound;
argument errors come back before any device is touched; the Python front-ends reject wrong operand kinds before any
native call."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("qil_inner", "qil_apply_inner", "qil_apply_norm")
QIL_EINVAL_ARG = 7


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qilaplace_hip.h")).read(), flags=re.S)


def test_overlap_entries_are_declared_exported_and_prototyped():
    import qilaplace_jl_amd as qil
    import importlib
    L = importlib.import_module("qilaplace_jl_amd._lib")
    decl = _header()
    lib = ctypes.CDLL(qil.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"QIL_API\s+int\s+" + name + r"\s*\(", decl), name
        assert hasattr(lib, name), name
        assert name in L.PROTOTYPES, name
    assert len(L.PROTOTYPES["qil_inner"]) == 3 and len(L.PROTOTYPES["qil_apply_inner"]) == 4
    assert len(L.PROTOTYPES["qil_apply_norm"]) == 3


def test_null_handles_fail_without_a_device():
    """QIL_EINVAL_ARG for every null operand, returned before the context is activated (this runs on a machine
    without a GPU: an activation would fail with QIL_EHIP instead)."""
    import importlib
    L = importlib.import_module("qilaplace_jl_amd._lib")
    v = (ctypes.c_double * 2)()
    assert L.lib.qil_inner(None, None, v) == QIL_EINVAL_ARG
    assert "inner: null argument" in L.last_error()
    assert L.lib.qil_apply_inner(None, None, None, v) == QIL_EINVAL_ARG
    assert "null argument" in L.last_error()
    assert L.lib.qil_apply_norm(None, None, v) == QIL_EINVAL_ARG
    assert "null argument" in L.last_error()
    # a non-null output but null operands, and the other way round
    fake = ctypes.c_void_p(0)
    assert L.lib.qil_inner(fake, fake, None) == QIL_EINVAL_ARG
    assert L.lib.qil_apply_norm(fake, fake, None) == QIL_EINVAL_ARG


def test_null_checks_precede_the_context_activation():
    """As in qil_norm: each entry validates its arguments before qil_ctx_activate (and so before any HIP call)."""
    src = open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "qil_inner.hip")).read()
    for name in ENTRIES:
        m = re.search(r'extern "C" int ' + name + r"\(.*?\n}\n", src, flags=re.S)
        assert m, name
        body = m.group(0)
        null_at = body.find("null argument")
        act_at = body.find("qil_ctx_activate")
        assert 0 <= null_at < act_at, name
        # the operand checks of apply are reused, not restated
        if name != "qil_inner":
            assert 0 <= body.find("qil_check_apply_operands") < act_at, name


class _Boom:
    def __init__(self):
        self.calls = 0

    def __call__(self, *a):
        self.calls += 1
        raise AssertionError("native call made before the type check")


@pytest.fixture
def no_native(monkeypatch):
    import importlib
    L = importlib.import_module("qilaplace_jl_amd._lib")
    boom = _Boom()
    for name in ENTRIES + ("qil_norm", "qil_mps_is_paired", "qil_mpo_is_paired", "qil_mps_dtype", "qil_mpo_dtype"):
        monkeypatch.setattr(L.lib, name, boom)
    return boom


def _bare(cls):
    """A container object without a device handle (only its class matters to the type checks)."""
    obj = object.__new__(cls)
    obj.handle = None
    obj.ctx = None
    return obj


def test_python_type_errors_precede_native_calls(no_native):
    import qilaplace_jl_amd as qil
    psi, zt = _bare(qil.SignalMPS), _bare(qil.ZTMPS)
    W, Wp = _bare(qil.SingleSiteMPO), _bare(qil.PairedSiteMPO)
    cases = [
        (lambda: qil.inner(W, psi), "unsupported operand types"),          # an MPO where an MPS goes
        (lambda: qil.inner(psi, W), "unsupported operand types"),
        (lambda: qil.inner(psi, psi, psi), "unsupported operand types"),
        (lambda: qil.inner(W, W, psi), "unsupported operand types"),
        (lambda: qil.inner(psi, W, W), "unsupported operand types"),
        (lambda: qil.inner(zt, W, zt), "PairedSiteMPO acts on ZTMPS"),      # SingleSiteMPO with ZTMPS
        (lambda: qil.inner(psi, Wp, psi), "PairedSiteMPO acts on ZTMPS"),
        (lambda: qil.apply_norm(W, zt), "PairedSiteMPO acts on ZTMPS"),
        (lambda: qil.apply_norm(psi, psi), "unsupported operand types"),
        (lambda: qil.apply_norm(W, W), "unsupported operand types"),
        (lambda: qil.distance(W, psi), "unsupported operand types"),
        (lambda: qil.apply_distance(psi, W, zt), "PairedSiteMPO acts on ZTMPS"),
        (lambda: qil.apply_distance(W, W, psi), "unsupported operand types"),
    ]
    for fn, msg in cases:
        with pytest.raises(TypeError, match=msg):
            fn()
    with pytest.raises(TypeError):
        qil.inner(psi)
    assert no_native.calls == 0


def test_overlap_names_are_exported_from_the_package():
    import qilaplace_jl_amd as qil
    for name in ("inner", "apply_norm", "distance", "apply_distance"):
        assert name in qil.__all__ and callable(getattr(qil, name))


def test_julia_shim_binds_the_overlaps_as_methods_of_inner():
    src = open(os.path.join(ROOT, "julia", "QILaplaceHIP.jl")).read()
    assert re.search(r"import ITensors:.*\binner\b", src)
    assert re.search(r"function inner\(phi::DeviceMPS, psi::DeviceMPS\)", src)
    assert re.search(r"function inner\(phi::DeviceMPS, W::DeviceMPO, psi::DeviceMPS\)", src)
    assert re.search(r"function apply_norm\(W::DeviceMPO, psi::DeviceMPS\)", src)
    for name in ENTRIES:
        assert f"(:{name}, LIB)" in src, name
