"""CPU-side checks of the lazy top-k search (qil_apply_top_k): declared with its signature, exported and bound; null and argument
errors come back before any device is touched, and in the source every check, the k = 0 return and the operand checks sit ahead
of the context activation, the temporaries' owner behind it; the Python front-end rejects wrong operands and a bad k or beam
before any native entry is called; `top_k` and `apply_top_k` end in their own entries; the selection kernels exist once in the
tree, shared by both verbs; the Julia shim binds the entry and the documents name it."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qilaplace.jl_amd", "csrc")
QIL_EINVAL_ARG = 7

NAME = "qil_apply_top_k"
SIGNATURE = (r"const qil_mpo\* W,\s*const qil_mps\* psi,\s*int64_t k,\s*int64_t beam,\s*uint8_t\* bits_out,\s*double\* val_out,\s*"
             r"double\* bound_out")
KERNELS = ("apply_top_k_keys", "apply_top_k_gather", "apply_top_k_finish")
SELECTION = ("select_init", "select_pass", "compact_count", "compact_scan", "compact_write")


def _lib():
    import importlib
    return importlib.import_module("qilaplace_jl_amd._lib")


def _source(name="qil_apply_topk.hip"):
    return open(os.path.join(CSRC, name)).read()


def test_entry_is_declared_exported_and_prototyped():
    import qilaplace_jl_amd as qil
    L = _lib()
    decl = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qilaplace_hip.h")).read(), flags=re.S)
    so = ctypes.CDLL(qil.LIB_PATH)
    assert re.search(r"QIL_API\s+int\s+" + NAME + r"\s*\(\s*" + SIGNATURE + r"\s*\)\s*;", decl)
    assert decl.index("QIL_API int qil_apply_sample") < decl.index("QIL_API int " + NAME)
    assert hasattr(so, NAME)
    assert len(L.PROTOTYPES[NAME]) == 7
    assert "apply_top_k" in qil.__all__ and callable(qil.apply_top_k)
    assert "qil_apply_topk.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_null_and_argument_errors_precede_the_context_activation():
    """QIL_EINVAL_ARG with the documented message.  This runs on a machine without a GPU: an activation would fail with QIL_EHIP
    instead.  The non-null stand-ins are never dereferenced: the failing check comes first in every call."""
    L = _lib()
    dummy = ctypes.create_string_buffer(4096)
    bits = (ctypes.c_uint8 * 8)(*([9] * 8))
    vals = (ctypes.c_double * 4)(*([-7.0] * 4))
    bound = ctypes.c_double(-3.0)
    h = ctypes.c_void_p(ctypes.addressof(dummy))
    out = (bits, vals, ctypes.byref(bound))
    for args in ((None, h, 1, 4) + out, (h, None, 1, 4) + out, (None, None, 0, 0, None, None, None), (None, h, -1, 4) + out,
                 (h, None, 5, 4, None, None, None)):
        assert L.lib.qil_apply_top_k(*args) == QIL_EINVAL_ARG
        assert "apply_top_k: null argument" in L.last_error()
    assert L.lib.qil_apply_top_k(h, h, -1, 4, *out) == QIL_EINVAL_ARG
    assert "apply_top_k: negative k -1" in L.last_error()
    assert L.lib.qil_apply_top_k(h, h, 5, 4, *out) == QIL_EINVAL_ARG
    assert "apply_top_k: beam 4 below k 5" in L.last_error()
    assert list(bits) == [9] * 8 and list(vals) == [-7.0] * 4 and bound.value == -3.0


def test_every_check_precedes_the_activation_in_the_source():
    src = _source()
    m = re.search(r'extern "C" int ' + NAME + r"\(.*?\n}\n", src, flags=re.S)
    assert m
    body = m.group(0)
    first = body[body.index("{") + 1:].lstrip()
    assert first.startswith('QIL_REQUIRE(W && psi, QIL_EINVAL_ARG, "apply_top_k: null argument");')
    act = body.find("qil_ctx_activate")
    order = ["W && psi", "k >= 0", "beam >= k", "qil_check_apply_operands(W, psi)", "beam <= beam_cap(W, psi)",
             "k <= (1LL << psi->n())", "if (k == 0) return QIL_OK;", "bits_out && val_out && bound_out", "QIL_ENOMEM",
             "qil_ctx_activate", "qil_call_scope"]
    at = [body.find(x) for x in order]
    assert all(a >= 0 for a in at) and at == sorted(at), list(zip(order, at))
    assert body.count("QIL_REQUIRE") == 7 and body.rfind("QIL_REQUIRE") < act      # no check is left for after it
    assert body.count("QIL_EINVAL_ARG") == 6
    assert "the right environments need %.0f bytes" in body and "QIL_APPLY_SAMPLE_RENV_BYTES raises it" in body
    # the one error after the activation, in the implementation
    assert 'QIL_EDOMAIN, "apply_top_k: the transformed state has zero norm"' in src and "QIL_EDOMAIN" not in body


def _code(name):
    return re.sub(r"//[^\n]*", "", _source(name))


def test_the_verb_has_kernels_of_its_own_and_shares_the_rest():
    code = _code("qil_apply_topk.hip")
    for kernel in KERNELS:
        assert re.search(r"__global__ __launch_bounds__\([\w *]+\) void " + kernel + r"\(", code), kernel
        assert re.search(r"hipLaunchKernelGGL\(" + kernel + r"[<,]", code), kernel
    assert "qil_scratch" in code and "qil_call_scope" in code and "asm" not in code
    for shared in ("qil_apply_right_envs(", "qil_apply_score_children(", "qil_apply_score_fused(", "qil_apply_env_budget(",
                   "qil_lazy_row_step(", "qil_beam_search("):
        assert shared in code, shared
    assert "getenv" not in code                                                    # budget and route are read in one place
    # the search itself, with the selection and the delivery, is the driver's: declared once, defined once, and each of the two
    # calls occurs once in the tree outside its definition
    sources = {f: _code(f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))}
    assert sources["qil_internal.h"].count("int qil_beam_search(") == 1 and sources["qil_topk.hip"].count("int qil_beam_search(") == 1
    assert sorted(f for f, text in sources.items() if "int qil_beam_search(" in text) == ["qil_internal.h", "qil_topk.hip"]
    for call, definition in (("qil_dev_select_largest(", "int qil_dev_select_largest("), ("qil_top_k_deliver(", "void qil_top_k_deliver(")):
        uses = {f: text.count(call) - text.count(definition) for f, text in sources.items()}
        assert {f: u for f, u in uses.items() if u} == {"qil_topk.hip": 1}, (call, uses)
    internal = open(os.path.join(CSRC, "qil_internal.h")).read()
    for decl in ("int qil_apply_right_envs(", "int qil_apply_score_children(", "int qil_dev_select_largest("):
        assert internal.count(decl) == 1, decl
    sampler = _code("qil_apply_sample.hip")
    assert sampler.count("int qil_apply_right_envs(") == 1 and sampler.count("int qil_apply_score_children(") == 1
    assert "log_trace" in sampler and "nullptr));" in sampler                      # apply_sample passes no log-trace output
    topk = _code("qil_topk.hip")
    assert topk.count("int qil_dev_select_largest(") == 1 and "qil_dev_select_largest(ctx," in topk


def test_selection_kernels_are_defined_once_in_the_tree():
    sources = {f: _code(f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))}
    for kernel in SELECTION:
        hits = [f for f, code in sources.items() if re.search(r"__global__[^;{]*\bvoid " + kernel + r"\(", code)]
        assert hits == ["qil_topk.hip"], (kernel, hits)
        users = sorted(f for f, code in sources.items() if kernel + "," in code or kernel + "<" in code)
        assert users == ["qil_topk.hip"], (kernel, users)


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


def _three_tensors(monkeypatch):
    from qilaplace_jl_amd import ops
    monkeypatch.setattr(ops, "_ntensors", lambda psi: 3)


def test_python_checks_precede_the_native_entry(monkeypatch):
    import qilaplace_jl_amd as qil
    L = _lib()
    boom = _Boom()
    _three_tensors(monkeypatch)
    for name in (NAME, "qil_top_k", "qil_apply", "qil_apply_norm", "qil_apply_sample", "qil_apply_coefficient_batch"):
        monkeypatch.setattr(L.lib, name, boom)
    (W, psi), (Wp, zt) = ((_fake(qil.SingleSiteMPO), _fake(qil.SignalMPS)), (_fake(qil.PairedSiteMPO), _fake(qil.ZTMPS)))
    for w, x in ((None, psi), (np.zeros((1, 2, 2, 1)), psi), (psi, psi), (zt, zt), (W, None), (W, W)):   # no operator / no state
        with pytest.raises(TypeError, match="apply: unsupported operand types"):
            qil.apply_top_k(w, x, 1)
    for w, x in ((Wp, psi), (W, zt)):                                           # the register kinds must agree
        with pytest.raises(TypeError, match="PairedSiteMPO acts on ZTMPS"):
            qil.apply_top_k(w, x, 1)
    for w, x in ((W, psi), (Wp, zt)):
        for k, beam in ((1.5, 4), (1, 4.0), (True, 4), (1, None)):
            with pytest.raises(TypeError, match="apply_top_k: k and beam must be integers"):
                qil.apply_top_k(w, x, k, beam=beam)
        with pytest.raises(ValueError, match="apply_top_k: k must be non-negative"):
            qil.apply_top_k(w, x, -1, beam=4)
        with pytest.raises(ValueError, match=r"apply_top_k: beam \(4\) must be at least k \(5\)"):
            qil.apply_top_k(w, x, 5, beam=4)
        with pytest.raises(ValueError, match=r"apply_top_k: k \(9\) exceeds the 2\^3 configurations"):
            qil.apply_top_k(w, x, 9, beam=16)
    assert boom.calls == 0


def test_top_k_and_apply_top_k_end_in_their_own_entries(monkeypatch):
    import qilaplace_jl_amd as qil
    L = _lib()
    seen = []
    _three_tensors(monkeypatch)

    def entry(name):
        def call(*args):
            seen.append((name, len(args)))
            return 0
        return call

    monkeypatch.setattr(L.lib, "qil_top_k", entry("plain"))
    monkeypatch.setattr(L.lib, NAME, entry("lazy"))
    codes = {"qil_mps_dtype": 0, "qil_mpo_dtype": 0}                            # QIL_F64; served by stand-ins, as the length is

    def dtype_of(name):
        def call(handle, ref):
            ref._obj.value = codes[name]
            return 0
        return call

    for name in codes:
        monkeypatch.setattr(L.lib, name, dtype_of(name))
    W, psi = _fake(qil.SingleSiteMPO), _fake(qil.SignalMPS)
    qil.top_k(psi, 2)
    qil.top_k(psi, 2, beam=8, bits=True)
    assert seen == [("plain", 6)] * 2
    del seen[:]
    idx, vals, bound, certified = qil.apply_top_k(W, psi, 2)
    rows, _, _, _ = qil.apply_top_k(W, psi, 2, beam=8, bits=True)
    assert seen == [("lazy", 7)] * 2
    assert idx.shape == (2,) and vals.shape == (2,) and vals.dtype == np.float64 and bound == 0.0 and certified is False
    assert rows.shape == (2, 3) and rows.dtype == np.uint8
    codes["qil_mpo_dtype"] = 1                                                  # a complex operator makes the values complex
    assert qil.apply_top_k(W, psi, 2)[1].dtype == np.complex128
    assert qil.apply_top_k(W, psi, 0)[3] is True


def test_julia_shim_and_documents_name_the_entry():
    src = open(os.path.join(ROOT, "julia", "QILaplaceHIP.jl")).read()
    assert re.search(r"function apply_top_k\(W::DeviceMPO, psi::DeviceMPS, k::Integer; beam::Integer=4096\)", src)
    assert f"(:{NAME}, LIB)" in src
    assert re.search(r"export .*\bapply_top_k\b", src, flags=re.S)
    assert f"`{NAME}`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`apply_top_k`" in open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 3.16" in design and NAME in design and all(k in design for k in KERNELS)
    for text in (design, open(os.path.join(ROOT, "include", "qilaplace_hip.h")).read(), _source(), _source("qil_apply_sample.hip")):
        assert "Left out: apply_top_k" not in text and "Left out: `apply_top_k`" not in text
    assert os.path.exists(os.path.join(ROOT, "examples", "lazy_top_k.py"))
    assert os.path.exists(os.path.join(ROOT, "tools", "_apply_top_k_time.py"))
    header = open(os.path.join(ROOT, "include", "qilaplace_hip.h")).read()
    decl = header[header.index("QIL_API int qil_apply_sample"):header.index("QIL_API int " + NAME)]
    for phrase in ("environments", "search", "beam <= min(2^29, 2^30 / (3 maxM e + 4 n + 64))",
                   "chunk = max(1, min(largest frontier, 32768, 64 MiB / ((2 maxM + maxX) e + 16 ceil(maxM / 64))))",
                   "QIL_APPLY_SAMPLE_RENV_BYTES", "QIL_APPLY_SAMPLE_ROUTE", "zero norm", "bit-identical", "device-resident output"):
        assert phrase in decl, phrase
