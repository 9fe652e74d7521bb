"""CPU-side checks of perfect sampling (qil_sample): declared, exported and bound; argument errors come back before any
device is touched; the Python front-end rejects non-MPS operands before any native call; the documented counter-based
uniforms lie in [0, 1)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QIL_EINVAL_CONFIG, QIL_EINVAL_ARG = 3, 7


def _lib():
    import importlib
    return importlib.import_module("qilaplace_jl_amd._lib")


def test_sample_is_declared_exported_and_prototyped():
    import qilaplace_jl_amd as qil
    L = _lib()
    decl = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qilaplace_hip.h")).read(), flags=re.S)
    assert re.search(r"QIL_API\s+int\s+qil_sample\s*\(\s*const qil_mps\* psi,\s*int64_t nb,\s*uint64_t seed,\s*"
                     r"const double\* uniforms,\s*uint8_t\* bits_out,\s*double\* prob_out\s*\)\s*;", decl)
    assert hasattr(ctypes.CDLL(qil.LIB_PATH), "qil_sample")
    assert len(L.PROTOTYPES["qil_sample"]) == 6
    assert "sample" in qil.__all__ and callable(qil.sample)


def test_argument_errors_precede_the_context_activation():
    """QIL_EINVAL_* for null handles, null outputs, nb < 0 and bad uniforms, returned before the context is activated
    (this runs on a machine without a GPU: an activation would fail with QIL_EHIP instead)."""
    L = _lib()
    bits = (ctypes.c_uint8 * 64)()
    prob = (ctypes.c_double * 8)()
    assert L.lib.qil_sample(None, 4, 1, None, bits, prob) == QIL_EINVAL_ARG
    assert "sample: null argument" in L.last_error()
    assert L.lib.qil_sample(None, 0, 1, None, None, None) == QIL_EINVAL_ARG


def test_checks_precede_the_activation_in_the_source():
    src = open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", "qil_sample.hip")).read()
    m = re.search(r'extern "C" int qil_sample\(.*?\n}\n', src, flags=re.S)
    assert m
    body = m.group(0)
    act = body.find("qil_ctx_activate")
    for needle in ("null argument", "nb >= 0", "bits_out", "outside [0, 1)", "if (nb == 0) return QIL_OK"):
        assert 0 <= body.find(needle) < act, needle


class _Boom:
    def __init__(self):
        self.calls = 0

    def __call__(self, *a):
        self.calls += 1
        raise AssertionError("native call made before the type check")


def test_python_type_errors_precede_native_calls(monkeypatch):
    import qilaplace_jl_amd as qil
    L = _lib()
    boom = _Boom()
    monkeypatch.setattr(L.lib, "qil_sample", boom)
    for cls in (qil.SingleSiteMPO, qil.PairedSiteMPO):
        W = object.__new__(cls)
        W.handle = None
        W.ctx = None
        with pytest.raises(TypeError, match="sample: unsupported operand types"):
            qil.sample(W, 8)
    for x in (None, np.zeros((4, 2, 4)), [np.zeros((1, 2, 1))]):
        with pytest.raises(TypeError, match="sample: unsupported operand types"):
            qil.sample(x, 8)
    assert boom.calls == 0


def test_uniform_formula_lies_in_the_unit_interval():
    """numpy restatement of u[r, i] = (splitmix64(seed ^ splitmix64(r n + i)) >> 11) 2^-53"""
    def splitmix64(x):
        x = np.asarray(x, dtype=np.uint64)
        with np.errstate(over="ignore"):
            x = x + np.uint64(0x9E3779B97F4A7C15)
            x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))

    n = 48
    for seed in (0, 1234, 2 ** 64 - 1):
        idx = np.arange(4096, dtype=np.uint64)[:, None] * np.uint64(n) + np.arange(n, dtype=np.uint64)[None, :]
        u = (splitmix64(np.uint64(seed) ^ splitmix64(idx)) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
        assert u.min() >= 0.0 and u.max() < 1.0
        assert abs(u.mean() - 0.5) < 0.01 and len(np.unique(u)) == u.size
    # the largest value the formula can produce is the largest double below 1
    top = float(np.uint64(2 ** 53 - 1)) * 2.0 ** -53
    assert top < 1.0 and top == np.nextafter(1.0, 0.0)
    # the hash is the one qil_dev_fill_normal uses: the shared device header holds its only definition
    csrc = os.path.join(ROOT, "qilaplace.jl_amd", "csrc")
    hits = [f for f in os.listdir(csrc) if "splitmix64(uint64_t" in open(os.path.join(csrc, f), errors="replace").read()]
    assert hits == ["qil_device_utils.h"]


def test_the_sampling_rule_has_one_home_and_the_temporaries_one_owner():
    """`sample` and `apply_sample` promise the same arithmetic: the uniforms and the choice are defined once, in the shared device
    header.  The direct verbs hold every pool block through a qil_scratch: no hand-kept free list is left in their files, and
    the environment pass they share takes the caller's scratch."""
    csrc = os.path.join(ROOT, "qilaplace.jl_amd", "csrc")
    text = {f: open(os.path.join(csrc, f), errors="replace").read() for f in os.listdir(csrc)}
    for definition in ("seeded_uniform(uint64_t", "int choose("):
        assert [f for f in sorted(text) if definition in text[f]] == ["qil_device_utils.h"], definition
        assert text["qil_device_utils.h"].count(definition) == 1, definition
    for f in ("qil_sample.hip", "qil_topk.hip"):
        assert "qil_ctx_free(" not in text[f] and "qil_scratch tmp(ctx);" in text[f], f
    for f in ("qil_internal.h", "qil_sample.hip"):
        assert re.search(r"int qil_dev_right_envs\(const (struct )?qil_mps\* psi, qil_scratch& tmp,", text[f]), f
        assert text[f].count("int qil_dev_right_envs(") == 1, f


def test_julia_shim_binds_sample():
    src = open(os.path.join(ROOT, "julia", "QILaplaceHIP.jl")).read()
    assert re.search(r"import ITensors:.*\bsample\b", src)
    assert re.search(r"function sample\(psi::DeviceMPS, nsamples::Integer; seed::Integer=1234\)", src)
    assert "(:qil_sample, LIB)" in src
    assert "`qil_sample`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
