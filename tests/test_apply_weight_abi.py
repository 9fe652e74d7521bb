"""CPU-side checks of the lazy Born weights (qil_apply_weight_batch): declared with its signature, exported and bound; null
arguments come back before any device is touched, and that check sits first in the body, ahead of the context activation, as
does every other error; the file has the seed, mask and finish kernels, goes through the strided-batch GEMM and has no inline
assembly; the Python front-ends (apply_weight_batch, apply_weight, apply_bit_probabilities, apply_range_weight,
apply_weight_quantiles, apply_zt_row_weights, apply_zt_column_weights) are exported and reject a wrong-length spec, a spec value
above 2, a wrong operand, lo > hi, a q outside [0, 1] and a SignalMPS where a ZTMPS is needed before any native entry is
called; the Julia shim binds the entry and the documents name it."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QIL_EINVAL_ARG = 7

NAME = "qil_apply_weight_batch"
SIGNATURE = r"const qil_mpo\* W,\s*const qil_mps\* psi,\s*int64_t nb,\s*const uint8_t\* spec,\s*double\* out"
FRONT_ENDS = ("apply_weight_batch", "apply_weight", "apply_bit_probabilities", "apply_range_weight", "apply_weight_quantiles",
              "apply_zt_row_weights", "apply_zt_column_weights")


def _lib():
    import importlib
    return importlib.import_module("qilaplace_jl_amd._lib")


def _source():
    return open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "qil_apply_weight.hip")).read()


def test_entry_is_declared_exported_and_prototyped():
    import qilaplace_jl_amd as qil
    L = _lib()
    decl = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qilaplace_hip.h")).read(), flags=re.S)
    so = ctypes.CDLL(qil.LIB_PATH)
    assert re.search(r"QIL_API\s+int\s+" + NAME + r"\s*\(\s*" + SIGNATURE + r"\s*\)\s*;", decl)
    assert hasattr(so, NAME)
    assert len(L.PROTOTYPES[NAME]) == 5
    for name in FRONT_ENDS:
        assert name in qil.__all__ and callable(getattr(qil, name)), name
    assert "qil_apply_weight.hip" in open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "Makefile")).read()


def test_null_arguments_precede_the_context_activation():
    """QIL_EINVAL_ARG with the documented message for a null W or psi and, with nb > 0, a null spec or out.  This runs on a
    machine without a GPU: an activation would fail with QIL_EHIP instead.  The non-null stand-ins are never dereferenced: a null
    comes first in every call."""
    L = _lib()
    dummy = ctypes.create_string_buffer(4096)
    spec = (ctypes.c_uint8 * 4)(2, 2, 2, 2)
    out = (ctypes.c_double * 1)(-7.0)
    h = ctypes.c_void_p(ctypes.addressof(dummy))
    for args in ((None, h, 1, spec, out), (h, None, 1, spec, out), (h, h, 1, None, out), (h, h, 1, spec, None),
                 (None, None, 0, None, None), (None, h, 0, None, None), (h, None, 0, spec, out), (None, None, 1, None, None)):
        assert L.lib.qil_apply_weight_batch(*args) == QIL_EINVAL_ARG
        assert "apply_weight_batch: null argument" in L.last_error()
    assert out[0] == -7.0


def test_the_null_check_sits_first_and_every_error_precedes_the_activation():
    src = _source()
    m = re.search(r'extern "C" int ' + NAME + r"\(.*?\n}\n", src, flags=re.S)
    assert m
    body = m.group(0)
    first = body[body.index("{") + 1:].lstrip()
    assert first.startswith('QIL_REQUIRE(W && psi && (nb <= 0 || (spec && out)), QIL_EINVAL_ARG, "apply_weight_batch: null argument");')
    act = body.find("qil_ctx_activate")
    assert 0 <= body.find("QIL_EINVAL_ARG") < act
    assert 0 <= body.find("nb >= 0") < act
    assert 0 <= body.find("qil_check_apply_operands(W, psi)") < act
    assert 0 <= body.find("QIL_EINVAL_CONFIG") < act
    assert body.count("QIL_REQUIRE") == 3 and body.rfind("QIL_REQUIRE") < act      # no check is left for after it
    assert 0 <= body.find("if (nb == 0) return QIL_OK;") < act
    assert act < body.find("qil_call_scope")                                       # the temporaries' owner, as in every entry


def test_the_lazy_weights_have_kernels_of_their_own():
    code = re.sub(r"//[^\n]*", "", _source())
    for kernel in ("apply_weight_seed", "apply_weight_mask", "apply_weight_finish"):
        assert re.search(r"__global__ (__launch_bounds__\(\w+\) )?void " + kernel + r"\(", code), kernel
        assert "hipLaunchKernelGGL(" + kernel + "<" in code, kernel
    assert "qil_scratch" in code
    # the middle's four products are the shared environment step, strided-batch GEMMs, in two halves around the mask
    assert code.index("qil_norm_env_ket(") < code.index("hipLaunchKernelGGL(apply_weight_mask<") < code.index("qil_norm_env_bra(")
    contract = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "qil_contract.hip")).read())
    for half in ("ket", "bra"):
        m = re.search(r"\nint qil_norm_env_" + half + r"\(.*?\n}\n", contract, flags=re.S)
        assert m and "qil_dev_gemm_batched(" in m.group(0), half
    assert "qil_lazy_row_step" in code                                             # the lead step is the read-out's, not a copy
    readout = open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "qil_readout.hip")).read()
    assert readout.count("int qil_lazy_row_step(") == 1 and "QIL_TRY(qil_lazy_row_step(" in readout
    assert "atomic" not in code and "asm" not in code
    assert 'getenv("QIL_APPLY_WEIGHT_RENV_BYTES")' in code and "kRightEnvBudget" in code and "kChunkBudget = 64LL << 20" in code


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
    every native entry the front-ends could reach raises."""
    import qilaplace_jl_amd as qil
    L = _lib()
    boom = _Boom()

    def nsites(handle, ref):
        ref._obj.value = 6
        return 0

    monkeypatch.setattr(L.lib, "qil_mps_nsites", nsites)
    for name in (NAME, "qil_weight_batch", "qil_apply", "qil_apply_norm", "qil_apply_coefficient_batch", "qil_mps_restrict"):
        monkeypatch.setattr(L.lib, name, boom)
    pairs = ((_fake(qil.SingleSiteMPO), _fake(qil.SignalMPS)), (_fake(qil.PairedSiteMPO), _fake(qil.ZTMPS)))
    for W, state in pairs:
        for bad in ([[2] * 5], [[2] * 7], [2] * 6, [], np.full((2, 3), 2)):
            with pytest.raises(ValueError, match="expected 6 entries"):
                qil.apply_weight_batch(W, state, bad)
        for bad in ([2] * 5, [2] * 7, [], [[2] * 6]):
            with pytest.raises(ValueError, match="expected 6 entries"):
                qil.apply_weight(W, state, bad)
        for bad in ([2, 2, 3, 2, 2, 2], [0, 1, 2, 1, 200, 0], [0, 1, 2, -1, 0, 0]):
            with pytest.raises(ValueError, match=r"outside \[0,2\]"):
                qil.apply_weight_batch(W, state, [bad])
            with pytest.raises(ValueError, match=r"outside \[0,2\]"):
                qil.apply_weight(W, state, bad)
        for lo, hi in ((3, 2), (-1, 4), (0, 65), (64, 63)):                     # six tensors: 0 <= lo <= hi <= 64
            with pytest.raises(ValueError, match="range_weight"):
                qil.apply_range_weight(W, state, lo, hi)
        for bad in (1.0, "1", None, True):
            with pytest.raises(TypeError, match="must be integers"):
                qil.apply_range_weight(W, state, 0, bad)
        assert qil.apply_range_weight(W, state, 5, 5) == 0.0                    # no native call
        for bad in ([0.5, 1.5], [-0.1], 2.0, [float("nan")]):
            with pytest.raises(ValueError, match=r"\[0, 1\]"):
                qil.apply_weight_quantiles(W, state, bad)
    (W, psi), (Wp, zt) = pairs
    calls = (lambda w, x: qil.apply_weight_batch(w, x, [[2] * 6]), lambda w, x: qil.apply_weight(w, x, [2] * 6),
             qil.apply_bit_probabilities, lambda w, x: qil.apply_range_weight(w, x, 0, 1),
             lambda w, x: qil.apply_weight_quantiles(w, x, [0.5]), lambda w, x: qil.apply_zt_row_weights(w, x, [0]),
             lambda w, x: qil.apply_zt_column_weights(w, x, [0]))
    for call in calls:
        for w, x in ((None, psi), (np.zeros((1, 2, 2, 1)), psi), (psi, psi), (zt, zt), (W, None), (W, W)):   # no operator / no state
            with pytest.raises(TypeError, match="apply: unsupported operand types"):
                call(w, x)
        for w, x in ((Wp, psi), (W, zt)):                                       # the register kinds must agree
            with pytest.raises(TypeError, match="PairedSiteMPO acts on ZTMPS"):
                call(w, x)
    for fn in (qil.apply_zt_row_weights, qil.apply_zt_column_weights):
        with pytest.raises(TypeError, match="needs a ZTMPS"):
            fn(W, psi, [0])
        for bad in (-1, 8, 1 << 40):                     # three sites per register: indices 0 .. 7
            with pytest.raises(ValueError, match="outside"):
                fn(Wp, zt, [0, bad])
        for bad in (1.0, "1", None, True):
            with pytest.raises(TypeError, match="must be an integer"):
                fn(Wp, zt, [bad])
    assert boom.calls == 0


def test_the_existing_front_ends_still_end_in_their_own_entry(monkeypatch):
    """weight_batch and the front-ends on it call qil_weight_batch and never the lazy entry; the apply_ ones the reverse."""
    import qilaplace_jl_amd as qil
    L = _lib()
    seen = []

    def nsites(handle, ref):
        ref._obj.value = 6
        return 0

    def entry(name):
        def call(*args):
            seen.append((name, len(args)))
            return 0
        return call

    monkeypatch.setattr(L.lib, "qil_mps_nsites", nsites)
    monkeypatch.setattr(L.lib, "qil_weight_batch", entry("plain"))
    monkeypatch.setattr(L.lib, NAME, entry("lazy"))
    W, psi = _fake(qil.SingleSiteMPO), _fake(qil.SignalMPS)
    qil.weight_batch(psi, [[2] * 6])
    qil.weight(psi, [0] * 6)
    qil.range_weight(psi, 3, 9)
    assert seen and all(s == ("plain", 4) for s in seen)
    del seen[:]
    qil.apply_weight_batch(W, psi, [[2] * 6])
    qil.apply_weight(W, psi, [0] * 6)
    qil.apply_range_weight(W, psi, 3, 9)
    assert seen and all(s == ("lazy", 5) for s in seen)


def test_julia_shim_and_documents_name_the_entry():
    src = open(os.path.join(ROOT, "julia", "QILaplaceHIP.jl")).read()
    assert re.search(r"function apply_weight_batch\(W::DeviceMPO, psi::DeviceMPS, specs::AbstractMatrix\{<:Integer\}\)", src)
    assert f"(:{NAME}, LIB)" in src
    assert re.search(r"export .*\bapply_weight_batch\b", src, flags=re.S)
    assert f"`{NAME}`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "`apply_weight_batch`" in readme and "derived" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "qil_apply_weight_batch" in design and "apply_weight_finish" in design
    assert os.path.exists(os.path.join(ROOT, "examples", "lazy_band_power.py"))
    assert os.path.exists(os.path.join(ROOT, "tools", "_apply_weight_time.py"))
    header = open(os.path.join(ROOT, "include", "qilaplace_hip.h")).read()
    decl = header[header.index("QIL_API int qil_weight_batch"):header.index("QIL_API int " + NAME)]
    for phrase in ("lead", "middle", "tail", "chunk = max(1, min(nb, 32768,", "QIL_APPLY_WEIGHT_RENV_BYTES",
                   "weights of operators", "device-resident out"):
        assert phrase in decl, phrase
