"""CPU-side checks of the top-k coefficient search (qil_top_k): declared, exported and bound; argument errors come back before
any device is touched; the Python front-end rejects non-MPS operands and bad k or beam before any native call."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QIL_EINVAL_ARG = 7


def _lib():
    import importlib
    return importlib.import_module("qilaplace_jl_amd._lib")


def test_top_k_is_declared_exported_and_prototyped():
    import qilaplace_jl_amd as qil
    L = _lib()
    decl = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qilaplace_hip.h")).read(), flags=re.S)
    assert re.search(r"QIL_API\s+int\s+qil_top_k\s*\(\s*const qil_mps\* psi,\s*int64_t k,\s*int64_t beam,\s*"
                     r"uint8_t\* bits_out,\s*double\* val_out,\s*double\* bound_out\s*\)\s*;", decl)
    assert hasattr(ctypes.CDLL(qil.LIB_PATH), "qil_top_k")
    assert len(L.PROTOTYPES["qil_top_k"]) == 6
    assert "top_k" in qil.__all__ and callable(qil.top_k)
    assert "qil_topk.hip" in open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "Makefile")).read()


def test_argument_errors_precede_the_context_activation():
    """QIL_EINVAL_ARG for a null handle, returned before the context is activated (this runs on a machine without a GPU:
    an activation would fail with QIL_EHIP instead)."""
    L = _lib()
    bits = (ctypes.c_uint8 * 64)()
    vals = (ctypes.c_double * 16)()
    bound = ctypes.c_double()
    assert L.lib.qil_top_k(None, 4, 16, bits, vals, ctypes.byref(bound)) == QIL_EINVAL_ARG
    assert "top_k: null argument" in L.last_error()
    assert L.lib.qil_top_k(None, 0, 0, None, None, None) == QIL_EINVAL_ARG


def test_checks_precede_the_activation_in_the_source():
    src = open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "qil_topk.hip")).read()
    m = re.search(r'extern "C" int qil_top_k\(.*?\n}\n', src, flags=re.S)
    assert m
    body = m.group(0)
    act = body.find("qil_ctx_activate")
    for needle in ("null argument", "k >= 0", "beam >= k", "beam <= beam_cap(psi)", "k <= (1LL << psi->n())",
                   "if (k == 0) return QIL_OK", "bits_out && val_out && bound_out"):
        assert 0 <= body.find(needle) < act, needle
    assert body.count("QIL_EINVAL_ARG") >= 6


class _Boom:
    def __init__(self):
        self.calls = 0

    def __call__(self, *a):
        self.calls += 1
        raise AssertionError("native call made before the argument checks")


def _fake(cls, ntensors):
    """a container object that never touched the device: enough for the front-end's checks"""
    x = object.__new__(cls)
    x.handle = None
    x.ctx = None
    x.__dict__["_n"] = ntensors
    return x


def test_python_checks_precede_native_calls(monkeypatch):
    import qilaplace_jl_amd as qil
    L = _lib()
    boom = _Boom()
    monkeypatch.setattr(L.lib, "qil_top_k", boom)
    for cls in (qil.SingleSiteMPO, qil.PairedSiteMPO):
        W = object.__new__(cls)
        W.handle = None
        W.ctx = None
        with pytest.raises(TypeError, match="top_k: unsupported operand types"):
            qil.top_k(W, 1)
    for x in (None, np.zeros((4, 2, 4)), [np.zeros((1, 2, 1))]):
        with pytest.raises(TypeError, match="top_k: unsupported operand types"):
            qil.top_k(x, 1)
    psi = object.__new__(qil.SignalMPS)
    psi.handle = None
    psi.ctx = None
    for k, beam in ((1.5, 4), (1, 4.0), (True, 4), (1, None)):
        with pytest.raises(TypeError, match="top_k: k and beam must be integers"):
            qil.top_k(psi, k, beam=beam)
    with pytest.raises(ValueError, match="non-negative"):
        qil.top_k(psi, -1, beam=4)
    with pytest.raises(ValueError, match="at least k"):
        qil.top_k(psi, 5, beam=4)
    assert boom.calls == 0


def test_k_above_the_configuration_count_is_rejected_before_native_calls(monkeypatch):
    import qilaplace_jl_amd as qil
    from qilaplace_jl_amd import ops
    L = _lib()
    boom = _Boom()
    monkeypatch.setattr(L.lib, "qil_top_k", boom)
    monkeypatch.setattr(ops, "_ntensors", lambda psi: 3)
    psi = object.__new__(qil.SignalMPS)
    psi.handle = None
    psi.ctx = None
    with pytest.raises(ValueError, match="2\\^3 configurations"):
        qil.top_k(psi, 9, beam=16)
    assert boom.calls == 0


def test_julia_shim_binds_top_k():
    src = open(os.path.join(ROOT, "julia", "QILaplaceHIP.jl")).read()
    assert re.search(r"function top_k\(psi::DeviceMPS, k::Integer; beam::Integer=4096\)", src)
    assert "(:qil_top_k, LIB)" in src
    assert re.search(r"export .*\btop_k\b", src, flags=re.S)
    assert "`qil_top_k`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
