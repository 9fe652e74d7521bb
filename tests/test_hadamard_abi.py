"""CPU-side checks of the element-wise products and adjoints (qil_hadamard, qil_mpo_diagonal, qil_mpo_adjoint,
qil_hadamard_compress): declared with their signatures, exported and bound; null arguments come back before any device is
touched; every operand check sits ahead of the context activation; the Python front-ends reject wrong operand types before any
native call; the Julia shim binds all four and INTEGRATION.md names them."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QIL_EINVAL_ARG = 7

SIGNATURES = {
    "qil_hadamard": r"const qil_mps\* phi,\s*int conj_phi,\s*const qil_mps\* psi,\s*qil_mps\*\* out",
    "qil_mpo_diagonal": r"const qil_mps\* phi,\s*int conj_phi,\s*qil_mpo\*\* out",
    "qil_mpo_adjoint": r"const qil_mpo\* W,\s*qil_mpo\*\* out",
    "qil_hadamard_compress": r"const qil_mps\* phi,\s*int conj_phi,\s*const qil_mps\* psi,\s*int64_t maxdim,\s*double tol,\s*"
                             r"int sweeps,\s*int64_t zip_maxdim,\s*qil_mps\*\* out",
}
ARITY = {"qil_hadamard": 4, "qil_mpo_diagonal": 3, "qil_mpo_adjoint": 2, "qil_hadamard_compress": 8}
VERBS = {"qil_hadamard": "hadamard", "qil_mpo_diagonal": "mpo_diagonal", "qil_mpo_adjoint": "mpo_adjoint",
         "qil_hadamard_compress": "hadamard_compress"}


def _lib():
    import importlib
    return importlib.import_module("qilaplace_jl_amd._lib")


def _source():
    return open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "qil_hadamard.hip")).read()


def test_entries_are_declared_exported_and_prototyped():
    import qilaplace_jl_amd as qil
    L = _lib()
    decl = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qilaplace_hip.h")).read(), flags=re.S)
    so = ctypes.CDLL(qil.LIB_PATH)
    for name, args in SIGNATURES.items():
        assert re.search(r"QIL_API\s+int\s+" + name + r"\s*\(\s*" + args + r"\s*\)\s*;", decl), name
        assert hasattr(so, name), name
        assert len(L.PROTOTYPES[name]) == ARITY[name], name
    for name in ("hadamard", "hadamard_compress", "diagonal_mpo", "adjoint", "convolve", "correlate", "power_spectrum"):
        assert name in qil.__all__ and callable(getattr(qil, name)), name
    assert "qil_hadamard.hip" in open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "Makefile")).read()


def test_null_arguments_precede_the_context_activation():
    """QIL_EINVAL_ARG with "<verb>: null argument", returned before the context is activated (this runs on a machine without
    a GPU: an activation would fail with QIL_EHIP instead)."""
    L = _lib()
    out = ctypes.c_void_p()
    assert L.lib.qil_hadamard(None, 0, None, ctypes.byref(out)) == QIL_EINVAL_ARG
    assert "hadamard: null argument" in L.last_error()
    assert L.lib.qil_mpo_diagonal(None, 1, ctypes.byref(out)) == QIL_EINVAL_ARG
    assert "mpo_diagonal: null argument" in L.last_error()
    assert L.lib.qil_mpo_adjoint(None, ctypes.byref(out)) == QIL_EINVAL_ARG
    assert "mpo_adjoint: null argument" in L.last_error()
    assert L.lib.qil_hadamard_compress(None, 0, None, 8, 1e-10, 1, 0, ctypes.byref(out)) == QIL_EINVAL_ARG
    assert "hadamard_compress: null argument" in L.last_error()
    # a null `out` with null handles: still the argument error
    assert L.lib.qil_hadamard(None, 0, None, None) == QIL_EINVAL_ARG
    assert L.lib.qil_mpo_diagonal(None, 0, None) == QIL_EINVAL_ARG
    assert L.lib.qil_mpo_adjoint(None, None) == QIL_EINVAL_ARG
    assert L.lib.qil_hadamard_compress(None, 0, None, 0, 0.0, 1, 0, None) == QIL_EINVAL_ARG
    assert out.value is None


def _body(src, name):
    m = re.search(r'extern "C" int ' + name + r"\(.*?\n}\n", src, flags=re.S)
    assert m, name
    return m.group(0)


def test_checks_precede_the_activation_in_the_source():
    src = _source()
    for name, verb in VERBS.items():
        body = _body(src, name)
        act = body.find("qil_ctx_activate")
        assert act > 0, name
        assert 0 <= body.find(f'"{verb}: null argument"') < act, name
        assert re.search(r"QIL_REQUIRE\([^;]*\bout\b[^;]*null argument", body[:act]), name      # `out` is part of the null check
    for name in ("qil_hadamard", "qil_hadamard_compress"):
        body = _body(src, name)
        assert 0 <= body.find("check_pair(") < body.find("qil_ctx_activate"), name
    pair = re.search(r"int check_pair\(.*?\n}\n", src, flags=re.S).group(0)
    order = [pair.find(s) for s in ("phi->ctx == psi->ctx, QIL_EINVAL_ARG", "phi->paired == psi->paired, QIL_EINVAL_ARG",
                                    "phi->n() == psi->n(), QIL_EINVAL_LENGTH", "phi->site_ids == psi->site_ids, QIL_EINVAL_SITES")]
    assert all(o >= 0 for o in order) and order == sorted(order), order
    assert "qil_ctx_activate" not in pair


def test_the_product_has_a_kernel_of_its_own_and_the_fused_route_composes():
    src = _source()
    assert re.search(r"__global__ __launch_bounds__\(kRows\) void site_hadamard_grouped\(", src)
    assert "site_hadamard_grouped" in _body(src, "qil_hadamard") or "launch_hadamard" in _body(src, "qil_hadamard")
    fused = _body(src, "qil_hadamard_compress")
    assert "make_diagonal(" in fused and "qil_apply_compress(" in fused and "qil_mpo_destroy(D)" in fused
    assert "site_apply_grouped" not in re.sub(r"//[^\n]*", "", src)


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


def test_python_checks_precede_native_calls(monkeypatch):
    import qilaplace_jl_amd as qil
    L = _lib()
    boom = _Boom()
    for name in list(SIGNATURES) + ["qil_apply_compress", "qil_build_qft_mpo", "qil_mps_nsites", "qil_mpo_nsites"]:
        monkeypatch.setattr(L.lib, name, boom)
    psi, zt = _fake(qil.SignalMPS), _fake(qil.ZTMPS)
    W, Wp = _fake(qil.SingleSiteMPO), _fake(qil.PairedSiteMPO)
    bad = (None, np.zeros((4, 2, 4)), [np.zeros((1, 2, 1))], W, Wp)
    for x in bad:
        for fn in (qil.hadamard, qil.hadamard_compress):
            with pytest.raises(TypeError, match="hadamard: unsupported operand types"):
                fn(x, psi)
            with pytest.raises(TypeError, match="hadamard: unsupported operand types"):
                fn(psi, x)
        with pytest.raises(TypeError, match="diagonal_mpo: unsupported operand types"):
            qil.diagonal_mpo(x)
        with pytest.raises(TypeError, match="hadamard: unsupported operand types"):
            qil.power_spectrum(x)
        with pytest.raises(TypeError, match="convolve: unsupported operand types"):
            qil.convolve(x, psi)
        with pytest.raises(TypeError, match="correlate: unsupported operand types"):
            qil.correlate(psi, x)
    for x in (None, np.zeros((2, 2, 2, 2)), psi, zt):
        with pytest.raises(TypeError, match="adjoint: unsupported operand types"):
            qil.adjoint(x)
    with pytest.raises(TypeError, match="convolve: unsupported operand types"):
        qil.convolve(zt, zt)
    with pytest.raises(TypeError, match="convolve: unsupported operand types"):
        qil.convolve(psi, psi, F=Wp)
    with pytest.raises(TypeError, match="correlate: unsupported operand types"):
        qil.correlate(psi, psi, F=psi)
    assert boom.calls == 0


def test_states_do_not_overload_multiplication():
    """`*` stays the operator application W * psi: a product of two states is spelled out (hadamard)."""
    import qilaplace_jl_amd as qil
    assert "__mul__" not in qil.SignalMPS.__dict__ and "__mul__" not in qil.ZTMPS.__dict__
    assert "__rmul__" not in qil.SignalMPS.__dict__


def test_convolve_documents_the_unitarity_of_the_default_qft():
    import qilaplace_jl_amd as qil
    doc = " ".join(qil.convolve.__doc__.split())
    assert "unitary only to" in doc and "1e-7" in doc and "cutoff" in doc and "build_qft_mpo" in doc
    assert "marginal_batch" in qil.power_spectrum.__doc__


def test_julia_shim_binds_all_four():
    src = open(os.path.join(ROOT, "julia", "QILaplaceHIP.jl")).read()
    assert re.search(r"function hadamard\(phi::DeviceMPS, psi::DeviceMPS; conj::Bool=false\)", src)
    assert re.search(r"function hadamard_compress\(phi::DeviceMPS, psi::DeviceMPS; conj::Bool=false,", src)
    assert re.search(r"function diagonal_mpo\(phi::DeviceMPS; conj::Bool=false\)", src)
    assert re.search(r"function adjoint\(W::DeviceMPO\)", src)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in SIGNATURES:
        assert f"(:{name}, LIB)" in src, name
        assert f"`{name}`" in doc, name
    for name in ("hadamard", "hadamard_compress", "diagonal_mpo"):
        assert re.search(r"export .*\b" + name + r"\b", src, flags=re.S), name
