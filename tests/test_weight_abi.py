"""CPU-side checks of the Born weights (qil_weight_batch): declared with its signature, exported and bound; null arguments come
back before any device is touched, and that check sits first in the body, ahead of the context activation; the file has the LDS
kernel with launch bounds on the f64 MFMA and no inline assembly; the Python front-ends (weight_batch, weight, bit_probabilities,
range_weight, weight_quantiles, zt_row_weights, zt_column_weights) are exported and reject a wrong-length spec, a spec value
above 2, a wrong operand, lo > hi, a q outside [0, 1] and a SignalMPS where a ZTMPS is needed before the native entry is called;
the Julia shim binds the entry and the documents name it."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QIL_EINVAL_ARG = 7

NAME = "qil_weight_batch"
SIGNATURE = r"const qil_mps\* psi,\s*int64_t nb,\s*const uint8_t\* spec,\s*double\* out"
FRONT_ENDS = ("weight_batch", "weight", "bit_probabilities", "range_weight", "weight_quantiles", "zt_row_weights",
              "zt_column_weights")


def _lib():
    import importlib
    return importlib.import_module("qilaplace_jl_amd._lib")


def _source():
    return open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "qil_weight.hip")).read()


def test_entry_is_declared_exported_and_prototyped():
    import qilaplace_jl_amd as qil
    L = _lib()
    decl = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qilaplace_hip.h")).read(), flags=re.S)
    so = ctypes.CDLL(qil.LIB_PATH)
    assert re.search(r"QIL_API\s+int\s+" + NAME + r"\s*\(\s*" + SIGNATURE + r"\s*\)\s*;", decl)
    assert hasattr(so, NAME)
    assert len(L.PROTOTYPES[NAME]) == 4
    for name in FRONT_ENDS:
        assert name in qil.__all__ and callable(getattr(qil, name)), name
    ops = __import__("importlib").import_module("qilaplace_jl_amd.ops")
    assert (ops.FIX0, ops.FIX1, ops.TRACE) == (0, 1, 2)
    assert "qil_weight.hip" in open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "Makefile")).read()


def test_null_arguments_precede_the_context_activation():
    """QIL_EINVAL_ARG with the documented message for a null psi and, with nb > 0, a null spec or out.  This runs on a machine
    without a GPU: an activation would fail with QIL_EHIP instead.  The non-null stand-ins are never dereferenced: a null comes
    first in every call."""
    L = _lib()
    dummy = ctypes.create_string_buffer(4096)
    spec = (ctypes.c_uint8 * 4)(2, 2, 2, 2)
    out = (ctypes.c_double * 1)(-7.0)
    handle = ctypes.c_void_p(ctypes.addressof(dummy))
    for args in ((None, 1, spec, out), (handle, 1, None, out), (handle, 1, spec, None), (None, 0, None, None),
                 (None, 1, None, None)):
        assert L.lib.qil_weight_batch(*args) == QIL_EINVAL_ARG
        assert "weight_batch: null argument" in L.last_error()
    assert out[0] == -7.0


def test_the_null_check_sits_first_in_the_body():
    src = _source()
    m = re.search(r'extern "C" int ' + NAME + r"\(.*?\n}\n", src, flags=re.S)
    assert m
    body = m.group(0)
    first = body[body.index("{") + 1:].lstrip()
    assert first.startswith('QIL_REQUIRE(psi && (nb <= 0 || (spec && out)), QIL_EINVAL_ARG, "weight_batch: null argument");')
    act = body.find("qil_ctx_activate")
    assert 0 <= body.find("QIL_EINVAL_ARG") < act
    # every error is raised before the activation: the negative count and the spec values too
    assert 0 <= body.find("nb >= 0") < act
    assert 0 <= body.find("QIL_EINVAL_CONFIG") < act


def test_the_weights_have_a_kernel_of_their_own():
    code = re.sub(r"//[^\n]*", "", _source())
    assert re.search(r"__global__ __launch_bounds__\(kThreads\) void weight_walk_lds\(", code)
    assert "mfma_step(" in code                                         # the f64 MFMA tile step: one definition, in the shared header
    utils = open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "qil_device_utils.h")).read()
    assert utils.count("void mfma_step(") == 1 and utils.count("__builtin_amdgcn_mfma_f64_16x16x4f64(") == 4
    assert code.count("hipLaunchKernelGGL(weight_walk_lds<") == 1       # one launch site: the whole batch in one grid
    assert "qil_dev_table" in code and "qil_dev_gemm_batched" in code
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
    for name in (NAME, "qil_mps_restrict", "qil_norm", "qil_coefficient_marginal_batch", "qil_mps_block"):
        monkeypatch.setattr(L.lib, name, boom)
    psi, zt = _fake(qil.SignalMPS), _fake(qil.ZTMPS)
    for state in (psi, zt):
        for bad in ([[2] * 5], [[2] * 7], [2] * 6, [], np.full((2, 3), 2)):
            with pytest.raises(ValueError, match="expected 6 entries"):
                qil.weight_batch(state, bad)
        for bad in ([2] * 5, [2] * 7, [], [[2] * 6]):
            with pytest.raises(ValueError, match="expected 6 entries"):
                qil.weight(state, bad)
        for bad in ([2, 2, 3, 2, 2, 2], [0, 1, 2, 1, 200, 0], [0, 1, 2, -1, 0, 0]):
            with pytest.raises(ValueError, match=r"outside \[0,2\]"):
                qil.weight_batch(state, [bad])
            with pytest.raises(ValueError, match=r"outside \[0,2\]"):
                qil.weight(state, bad)
        for lo, hi in ((3, 2), (-1, 4), (0, 65), (64, 63)):                     # six tensors: 0 <= lo <= hi <= 64
            with pytest.raises(ValueError, match="range_weight"):
                qil.range_weight(state, lo, hi)
        for bad in (1.0, "1", None, True):
            with pytest.raises(TypeError, match="must be integers"):
                qil.range_weight(state, 0, bad)
        assert qil.range_weight(state, 5, 5) == 0.0 and qil.range_weight(state, 64, 64) == 0.0   # no native call
        for bad in ([0.5, 1.5], [-0.1], 2.0, [float("nan")]):
            with pytest.raises(ValueError, match=r"\[0, 1\]"):
                qil.weight_quantiles(state, bad)
    for bad in (None, np.zeros((1, 2, 1)), _fake(qil.SingleSiteMPO)):
        for call in (lambda x: qil.weight_batch(x, [[2] * 6]), lambda x: qil.weight(x, [2] * 6), qil.bit_probabilities,
                     lambda x: qil.range_weight(x, 0, 1), lambda x: qil.weight_quantiles(x, [0.5])):
            with pytest.raises(TypeError, match="weight: unsupported operand types"):
                call(bad)
    for fn in (qil.zt_row_weights, qil.zt_column_weights):
        with pytest.raises(TypeError, match="needs a ZTMPS"):
            fn(psi, [0])
        for bad in (-1, 8, 1 << 40):                     # three sites per register: indices 0 .. 7
            with pytest.raises(ValueError, match="outside"):
                fn(zt, [0, bad])
        for bad in (1.0, "1", None, True):
            with pytest.raises(TypeError, match="must be an integer"):
                fn(zt, [bad])
    assert boom.calls == 0


def test_dyadic_blocks_tile_the_range():
    """[lo, hi) in at most 2n aligned blocks, ascending, disjoint and complete -- what range_weight sums."""
    import importlib
    ops = importlib.import_module("qilaplace_jl_amd.ops")
    rng = np.random.default_rng(5)
    n = 11
    cases = [(0, 2 ** n), (1, 2 ** n - 1), (0, 1), (2 ** n - 1, 2 ** n), (2 ** (n - 1) - 3, 2 ** (n - 1) + 5)]
    cases += [tuple(sorted(int(v) for v in rng.integers(0, 2 ** n + 1, size=2))) for _ in range(200)]
    for lo, hi in cases:
        blocks = ops._dyadic_blocks(lo, hi, n)
        assert len(blocks) <= 2 * n
        at = lo
        for start, k in blocks:
            assert start == at and start % (1 << k) == 0 and 0 <= k <= n
            at += 1 << k
        assert at == max(lo, hi)
    assert ops._dyadic_blocks(0, 2 ** 70, 70) == [(0, 70)]                      # python integers: no 64-bit limit


def test_julia_shim_and_documents_name_the_entry():
    src = open(os.path.join(ROOT, "julia", "QILaplaceHIP.jl")).read()
    assert re.search(r"function weight_batch\(psi::DeviceMPS, specs::AbstractMatrix\{<:Integer\}\)", src)
    assert f"(:{NAME}, LIB)" in src
    assert re.search(r"export .*\bweight_batch\b", src, flags=re.S)
    assert f"`{NAME}`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`weight_batch`" in open(os.path.join(ROOT, "README.md")).read()
    assert "weight_walk_lds" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert os.path.exists(os.path.join(ROOT, "examples", "band_power.py"))
    header = open(os.path.join(ROOT, "include", "qilaplace_hip.h")).read()
    decl = header[header.index("Born weights (no reference counterpart)"):header.index("QIL_API int " + NAME)]
    for phrase in ("lazy form on W psi", "weights of operators"):                # what is deliberately left out is said
        assert phrase in decl, phrase
