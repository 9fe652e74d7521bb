"""CPU-side checks of lazy perfect sampling (qil_apply_sample): declared with its signature, exported and bound; null arguments
come back before any device is touched, and that check sits first in the body, ahead of the context activation, as does every
other error but the zero norm; the file has the scoring, choosing and environment-scaling kernels, takes the lazy row step and
the environment step of the shared contraction code instead of copies, reads its two environment variables and has neither
atomics nor inline assembly; the Python front-end rejects wrong operands, a wrong `uniforms` shape and a uniform outside [0, 1)
before any native entry is called; `sample` stays on its own entry; the Julia shim binds the entry and the documents name it."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QIL_EINVAL_ARG = 7

NAME = "qil_apply_sample"
SIGNATURE = (r"const qil_mpo\* W,\s*const qil_mps\* psi,\s*int64_t nb,\s*uint64_t seed,\s*const double\* uniforms,\s*"
             r"uint8_t\* bits_out,\s*double\* prob_out")
KERNELS = ("apply_sample_score", "apply_sample_choose", "apply_sample_env_scale")


def _lib():
    import importlib
    return importlib.import_module("qilaplace_jl_amd._lib")


def _source():
    return open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "qil_apply_sample.hip")).read()


def test_entry_is_declared_exported_and_prototyped():
    import qilaplace_jl_amd as qil
    L = _lib()
    decl = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qilaplace_hip.h")).read(), flags=re.S)
    so = ctypes.CDLL(qil.LIB_PATH)
    assert re.search(r"QIL_API\s+int\s+" + NAME + r"\s*\(\s*" + SIGNATURE + r"\s*\)\s*;", decl)
    assert hasattr(so, NAME)
    assert len(L.PROTOTYPES[NAME]) == 7
    assert "apply_sample" in qil.__all__ and callable(qil.apply_sample)
    assert "qil_apply_sample.hip" in open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "Makefile")).read()


def test_null_arguments_precede_the_context_activation():
    """QIL_EINVAL_ARG with the documented message for a null W or psi and, with nb > 0, a null bits_out.  This runs on a machine
    without a GPU: an activation would fail with QIL_EHIP instead.  The non-null stand-ins are never dereferenced: a null comes
    first in every call."""
    L = _lib()
    dummy = ctypes.create_string_buffer(4096)
    bits = (ctypes.c_uint8 * 8)(*([9] * 8))
    prob = (ctypes.c_double * 1)(-7.0)
    h = ctypes.c_void_p(ctypes.addressof(dummy))
    for args in ((None, h, 1, 0, None, bits, prob), (h, None, 1, 0, None, bits, prob), (h, h, 1, 0, None, None, prob),
                 (None, None, 0, 0, None, None, None), (None, h, 0, 0, None, None, None), (h, None, 0, 5, None, bits, prob),
                 (None, None, 1, 0, None, None, None), (None, None, -1, 0, None, bits, None)):
        assert L.lib.qil_apply_sample(*args) == QIL_EINVAL_ARG
        assert "apply_sample: null argument" in L.last_error()
    assert list(bits) == [9] * 8 and prob[0] == -7.0


def test_the_null_check_sits_first_and_every_error_precedes_the_activation():
    src = _source()
    m = re.search(r'extern "C" int ' + NAME + r"\(.*?\n}\n", src, flags=re.S)
    assert m
    body = m.group(0)
    first = body[body.index("{") + 1:].lstrip()
    assert first.startswith('QIL_REQUIRE(W && psi && (nb <= 0 || bits_out), QIL_EINVAL_ARG, "apply_sample: null argument");')
    act = body.find("qil_ctx_activate")
    assert 0 <= body.find("QIL_EINVAL_ARG") < act
    assert 0 <= body.find("nb >= 0") < act
    assert 0 <= body.find("qil_check_apply_operands(W, psi)") < act
    assert 0 <= body.find("QIL_EINVAL_CONFIG") < act                               # the uniforms
    assert 0 <= body.find("QIL_ENOMEM") < act                                      # the environment cap
    assert body.count("QIL_REQUIRE") == 4 and body.rfind("QIL_REQUIRE") < act      # no check is left for after it
    assert 0 <= body.find("if (nb == 0) return QIL_OK;") < act
    assert act < body.find("qil_call_scope")                                       # the temporaries' owner, as in every entry
    # the one error after the activation, in the implementation
    assert 'QIL_EDOMAIN, "apply_sample: the transformed state has zero norm"' in src and "QIL_EDOMAIN" not in body


def test_the_lazy_sampler_has_kernels_of_its_own_and_shares_the_contraction_steps():
    code = re.sub(r"//[^\n]*", "", _source())
    for kernel in KERNELS:
        assert re.search(r"__global__ (__launch_bounds__\([\w *]+\) )?void " + kernel + r"\(", code), kernel
        assert "hipLaunchKernelGGL(" + kernel + "<" in code, kernel
    assert "qil_scratch" in code and "qil_call_scope" in code
    assert "mfma_step(" in code and "row16_sum(" in code                           # the scoring kernel is on the matrix cores
    assert "QIL_TRY(qil_lazy_row_step(" in code and "QIL_TRY(qil_norm_env_step(" in code
    assert "qil_dev_gemm(" in code                                                 # the other route
    readout = open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "qil_readout.hip")).read()
    assert readout.count("int qil_lazy_row_step(") == 1
    tree = os.path.join(ROOT, "qilaplace.jl_amd", "csrc")
    for name in ("int qil_norm_env_ket(", "int qil_norm_env_bra("):                # defined once, in qil_contract.hip
        hits = [f for f in os.listdir(tree) if f.endswith(".hip") and name in open(os.path.join(tree, f)).read()]
        assert hits == ["qil_contract.hip"], (name, hits)
    assert 'getenv("QIL_APPLY_SAMPLE_ROUTE")' in code and 'getenv("QIL_APPLY_SAMPLE_RENV_BYTES")' in code
    assert "kChunkBudget = 64LL << 20" in code and "kRightEnvBudget = 16LL << 30" in code and "kMaxChunk = 32768" in code
    assert "atomic" not in code and "asm" not in code


class _Boom:
    def __init__(self):
        self.calls = 0

    def __call__(self, *a):
        self.calls += 1
        raise AssertionError("native call made before the argument checks")


def _fake(cls):
    """a container object that never touched the device: enough for the front-end's checks"""
    x = object.__new__(cls)
    x.handle = None
    x.ctx = None
    return x


def _six_tensors(monkeypatch, L):
    def nsites(handle, ref):
        ref._obj.value = 6
        return 0

    monkeypatch.setattr(L.lib, "qil_mps_nsites", nsites)


def test_python_checks_precede_the_native_entry(monkeypatch):
    """The chain length is the one thing the checks need from the handle; it is served here by a stand-in (6 tensors), and
    every native entry the front-end could reach raises."""
    import qilaplace_jl_amd as qil
    L = _lib()
    boom = _Boom()
    _six_tensors(monkeypatch, L)
    for name in (NAME, "qil_sample", "qil_apply", "qil_apply_norm", "qil_apply_coefficient_batch"):
        monkeypatch.setattr(L.lib, name, boom)
    (W, psi), (Wp, zt) = ((_fake(qil.SingleSiteMPO), _fake(qil.SignalMPS)), (_fake(qil.PairedSiteMPO), _fake(qil.ZTMPS)))
    for w, x in ((None, psi), (np.zeros((1, 2, 2, 1)), psi), (psi, psi), (zt, zt), (W, None), (W, W)):   # no operator / no state
        with pytest.raises(TypeError, match="apply: unsupported operand types"):
            qil.apply_sample(w, x, 4)
    for w, x in ((Wp, psi), (W, zt)):                                           # the register kinds must agree
        with pytest.raises(TypeError, match="PairedSiteMPO acts on ZTMPS"):
            qil.apply_sample(w, x, 4)
    rng = np.random.default_rng(3)
    for w, x in ((W, psi), (Wp, zt)):
        with pytest.raises(ValueError, match="non-negative"):
            qil.apply_sample(w, x, -1)
        for shape in ((4, 5), (4, 7), (3, 6), (5, 6), (24,), (4, 6, 1)):
            with pytest.raises(ValueError, match="shape"):
                qil.apply_sample(w, x, 4, uniforms=rng.random(shape))
        for bad in (1.0, -1e-300, np.nan, np.inf):
            U = rng.random((4, 6))
            U[2, 5] = bad
            with pytest.raises(ValueError, match=r"outside \[0, 1\)"):
                qil.apply_sample(w, x, 4, uniforms=U)
    assert boom.calls == 0


def test_sample_and_apply_sample_end_in_their_own_entries(monkeypatch):
    import qilaplace_jl_amd as qil
    L = _lib()
    seen = []
    _six_tensors(monkeypatch, L)

    def entry(name):
        def call(*args):
            seen.append((name, len(args)))
            return 0
        return call

    monkeypatch.setattr(L.lib, "qil_sample", entry("plain"))
    monkeypatch.setattr(L.lib, NAME, entry("lazy"))
    W, psi = _fake(qil.SingleSiteMPO), _fake(qil.SignalMPS)
    qil.sample(psi, 3)
    qil.sample(psi, 3, uniforms=np.full((3, 6), 0.5), bits=True)
    assert seen == [("plain", 6)] * 2
    del seen[:]
    idx, p = qil.apply_sample(W, psi, 3)
    rows, _ = qil.apply_sample(W, psi, 3, seed=2 ** 64 - 1, uniforms=np.full((3, 6), 0.5), bits=True)
    (k, l), _ = qil.apply_sample(_fake(qil.PairedSiteMPO), _fake(qil.ZTMPS), 3)
    assert seen == [("lazy", 7)] * 3
    assert idx.shape == (3,) and p.shape == (3,) and rows.shape == (3, 6) and rows.dtype == np.uint8 and k.shape == l.shape == (3,)


def test_julia_shim_and_documents_name_the_entry():
    src = open(os.path.join(ROOT, "julia", "QILaplaceHIP.jl")).read()
    assert re.search(r"function apply_sample\(W::DeviceMPO, psi::DeviceMPS, nsamples::Integer; seed::Integer=1234, uniforms=nothing\)", src)
    assert f"(:{NAME}, LIB)" in src
    assert re.search(r"export .*\bapply_sample\b", src, flags=re.S)
    assert f"`{NAME}`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "`apply_sample`" in readme and "QIL_APPLY_SAMPLE_ROUTE" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 3.15" in design and NAME in design and all(k in design for k in KERNELS)
    measurements = open(os.path.join(ROOT, "MEASUREMENTS.md")).read()
    assert re.search(r"^## 18\. .*apply_sample", measurements, flags=re.M)
    assert os.path.exists(os.path.join(ROOT, "examples", "lazy_sample.py"))
    assert os.path.exists(os.path.join(ROOT, "tools", "_apply_sample_time.py"))
    header = open(os.path.join(ROOT, "include", "qilaplace_hip.h")).read()
    decl = header[header.index("QIL_API int qil_apply_weight_batch"):header.index("QIL_API int " + NAME)]
    for phrase in ("environments", "sweep", "uniforms", "chunk = max(1, min(nb, 32768,", "QIL_APPLY_SAMPLE_RENV_BYTES",
                   "QIL_APPLY_SAMPLE_ROUTE", "16 GiB", "zero norm", "apply_top_k", "device-resident output"):
        assert phrase in decl, phrase
