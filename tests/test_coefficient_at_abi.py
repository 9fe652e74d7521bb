"""CPU-side checks of the read-out by index and of the element-wise maps (qil_coefficient_at, qil_mps_map): declared with their
signatures, exported, prototyped, bound in the Julia shim and listed in INTEGRATION.md; every argument error comes back as
QIL_EINVAL_ARG with its message before a context is activated or a state is read; the Python front-ends refuse wrong operands
before any native call.  The errors that need live states are in tests/test_gpu_coefficient_at.py and tests/test_gpu_map.py."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qilaplace.jl_amd", "csrc")
QIL_EINVAL_ARG = 7

ENTRIES = {
    "qil_coefficient_at": (r"const qil_mps\* psi,\s*int64_t count,\s*const int64_t\* idx_dev,\s*void\* out_dev", 4),
    "qil_mps_map": (r"const qil_mps\* const\* states,\s*int64_t nstates,\s*int op,\s*const double\* params,\s*int64_t maxdim,\s*"
                    r"double tol,\s*int max_sweeps,\s*const int64_t\* seeds,\s*int64_t nseeds,\s*qil_mps\*\* out,\s*double\* est,\s*"
                    r"int64_t\* nevals,\s*int\* sweeps,\s*int\* converged", 14),
}
FRONT_ENDS = ("coefficient_at", "coefficient_at_route", "map_states", "cross_map", "magnitude", "log_power", "shrink", "divide",
              "deconvolve")


def _lib():
    import importlib
    return importlib.import_module("qilaplace_jl_amd._lib")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qilaplace_hip.h")).read(), flags=re.S)


def test_entries_are_declared_exported_prototyped_and_bound():
    import qilaplace_jl_amd as qil
    L = _lib()
    decl = _header()
    so = ctypes.CDLL(qil.LIB_PATH)
    for name, (signature, arity) in ENTRIES.items():
        assert re.search(r"QIL_API\s+int\s+" + name + r"\s*\(\s*" + signature + r"\s*\)\s*;", decl), name
        assert hasattr(so, name)
        assert len(L.PROTOTYPES[name]) == arity
    assert re.search(r"enum\s*\{\s*QIL_MAP_ABS = 0,\s*QIL_MAP_POWER = 1,\s*QIL_MAP_LOG = 2,\s*QIL_MAP_DIVIDE = 3,\s*QIL_MAP_SHRINK = 4\s*\}\s*;", decl)
    assert (L.QIL_MAP_ABS, L.QIL_MAP_POWER, L.QIL_MAP_LOG, L.QIL_MAP_DIVIDE, L.QIL_MAP_SHRINK) == (0, 1, 2, 3, 4)
    m = re.search(r"#define\s+QIL_COEFFICIENT_AT_WAVE_MAX_BOND\s+(\d+)", decl)
    assert m and int(m.group(1)) == L.QIL_COEFFICIENT_AT_WAVE_MAX_BOND
    testing = open(os.path.join(ROOT, "include", "qilaplace_hip_testing.h")).read()
    assert "coefficient_at" not in testing and "mps_map" not in testing and "QIL_MAP_" not in testing
    for py in FRONT_ENDS:
        assert py in qil.__all__ and callable(getattr(qil, py)), py
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "qil_index.hip" in make and "qil_map.hip" in make
    shim = open(os.path.join(ROOT, "julia", "QILaplaceHIP.jl")).read()
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert f"(:{name}, LIB)" in shim, name
        assert f"`{name}`" in table, name


def test_header_documents_the_contract():
    raw = open(os.path.join(ROOT, "include", "qilaplace_hip.h")).read()
    at = raw[raw.find("Read-out by index"):raw.find("qil_coefficient_at(")]
    for word in ("most significant bit", "NaN", "QIL_COEFFICIENT_AT_ROUTE", "synchronises", "MEASUREMENTS section 29", "doubles"):
        assert word in at, word
    mp = raw[raw.find("An element-wise function of up to four states"):raw.find("qil_mps_map(")]
    for word in ("QIL_MAP_SHRINK", "site ids of states[0]", "blind spot", "QIL_EDOMAIN", "paired states are not supported", "seeds"):
        assert word in mp, word


def _stub():
    """Non-null memory that must never be read as a handle: every check below fails before a state or a context is touched."""
    return ctypes.create_string_buffer(256)


def test_coefficient_at_refuses_bad_arguments_before_the_context_is_touched():
    L = _lib()
    call = L.lib.qil_coefficient_at
    idx, out = (ctypes.c_int64 * 4)(), (ctypes.c_double * 8)()
    assert call(None, 4, idx, out) == QIL_EINVAL_ARG and "coefficient_at: null argument" in L.last_error()
    assert call(None, 0, None, None) == QIL_EINVAL_ARG and "coefficient_at: null argument" in L.last_error()
    assert call(_stub(), 4, None, out) == QIL_EINVAL_ARG and "coefficient_at: null argument" in L.last_error()
    assert call(_stub(), 4, idx, None) == QIL_EINVAL_ARG and "coefficient_at: null argument" in L.last_error()
    assert call(_stub(), -1, idx, out) == QIL_EINVAL_ARG and "coefficient_at: count = -1 must be >= 0" in L.last_error()
    assert call(_stub(), -1, None, None) == QIL_EINVAL_ARG and "count = -1" in L.last_error()


def _map_call(L, states=True, nstates=1, op=0, params=None, maxdim=8, tol=1e-9, max_sweeps=4, seeds=(0,), nseeds=None, out=True):
    handles = (ctypes.c_void_p * 2)(ctypes.addressof(_STUBS[0]), ctypes.addressof(_STUBS[1])) if states else None
    par = (ctypes.c_double * 1)(params) if params is not None else None
    sd = (ctypes.c_int64 * max(1, len(seeds)))(*seeds) if seeds is not None else None
    h = ctypes.c_void_p()
    st = L.lib.qil_mps_map(handles, nstates, op, par, maxdim, tol, max_sweeps, sd, len(seeds or ()) if nseeds is None else nseeds,
                           ctypes.byref(h) if out else None, None, None, None, None)
    assert h.value is None
    return st, L.last_error()


_STUBS = [ctypes.create_string_buffer(256), ctypes.create_string_buffer(256)]

BAD_MAP = [
    (dict(states=False), "map: null argument"),
    (dict(out=False), "map: null argument"),
    (dict(op=5), "map: unknown op 5"),
    (dict(op=-1), "map: unknown op -1"),
    (dict(op=0, nstates=2), "map: abs takes 1 state, got nstates = 2"),
    (dict(op=3, nstates=1, params=0.0), "map: divide takes 2 states, got nstates = 1"),
    (dict(op=3, nstates=0, params=0.0), "map: divide takes 2 states, got nstates = 0"),
    (dict(op=4, nstates=4, params=0.0), "map: shrink takes 1 state"),
    (dict(op=1), "params: power takes a parameter"),
    (dict(op=1, params=0.0), "of power must be finite and > 0"),
    (dict(op=1, params=-2.0), "of power must be finite and > 0"),
    (dict(op=1, params=float("inf")), "of power must be finite and > 0"),
    (dict(op=2, params=0.0), "of log must be finite and > 0"),
    (dict(op=2, params=float("nan")), "of log must be finite and > 0"),
    (dict(op=3, nstates=2, params=-0.1), "of divide must be finite and >= 0"),
    (dict(op=3, nstates=2, params=float("nan")), "of divide must be finite and >= 0"),
    (dict(op=4, params=-1.0), "of shrink must be finite and >= 0"),
    (dict(maxdim=0), "map: maxdim must be finite, 1 .. 256"),
    (dict(maxdim=257), "map: maxdim must be finite, 1 .. 256"),
    (dict(maxdim=2 ** 63 - 1), "map: maxdim must be finite, 1 .. 256"),
    (dict(tol=-1e-9), "map: tol must be >= 0"),
    (dict(tol=float("nan")), "map: tol must be >= 0"),
    (dict(max_sweeps=0), "map: max_sweeps must be >= 1"),
    (dict(seeds=None, nseeds=1), "map: between 1 and 1024 seeds"),
    (dict(seeds=(0,), nseeds=0), "map: between 1 and 1024 seeds"),
    (dict(seeds=(0,), nseeds=1025), "map: between 1 and 1024 seeds"),
    (dict(seeds=(5, -1)), "map: seed -1 outside"),
    (dict(seeds=(2 ** 62,)), "outside"),
]


@pytest.mark.parametrize("kwargs, message", BAD_MAP, ids=[m for _, m in BAD_MAP])
def test_map_refuses_bad_arguments_before_a_state_is_read(kwargs, message):
    st, err = _map_call(_lib(), **kwargs)
    assert st == QIL_EINVAL_ARG and message in err, err


def test_a_null_state_is_named():
    L = _lib()
    handles = (ctypes.c_void_p * 2)(ctypes.addressof(_STUBS[0]), None)
    par, sd, h = (ctypes.c_double * 1)(0.0), (ctypes.c_int64 * 1)(0), ctypes.c_void_p()
    assert L.lib.qil_mps_map(handles, 2, 3, par, 8, 1e-9, 4, sd, 1, ctypes.byref(h), None, None, None, None) == QIL_EINVAL_ARG
    assert "map: null argument (states[1])" in L.last_error()


def test_every_check_precedes_the_activation_in_the_source():
    for fname, name in (("qil_index.hip", "qil_coefficient_at"), ("qil_map.hip", "qil_mps_map")):
        src = open(os.path.join(CSRC, fname)).read()
        m = re.search(r'extern "C" int ' + name + r"\(.*?\n}\n", src, flags=re.S)
        assert m, name
        body = m.group(0)
        act = body.index("qil_ctx_activate")
        assert body.index("QIL_REQUIRE") < act < body.index("qil_call_scope call_scope"), name
        assert "QIL_REQUIRE" not in body[act:] and "qil_cross_check_args(" not in body[act:], name
    mp = open(os.path.join(CSRC, "qil_map.hip")).read()
    assert '"map: paired states are not supported; map the SignalMPS and call ztmps_from_mps"' in mp
    assert "QIL_EINVAL_LENGTH" in mp and "QIL_EINVAL_SITES" in mp
    # the session itself is shared with the encoder: one loop behind both verbs
    cr = open(os.path.join(CSRC, "qil_cross.hip")).read()
    assert cr.count("qil_cross_run(ctx,") == 1 and cr.count("cross_consume(s, s->vals)") == 2
    assert "qil_cross_run(ctx," in mp
    ix = open(os.path.join(CSRC, "qil_index.hip")).read()
    body = ix[ix.index("void index_wave_body"):ix.index("struct index_wave_k")]
    assert "__syncthreads" not in body and "extern __shared__" in body


def test_front_ends_reject_wrong_operands_before_any_native_call(monkeypatch):
    import qilaplace_jl_amd as qil
    L = _lib()

    class _Refuse:
        def __getattr__(self, name):
            raise AssertionError(f"native entry {name} was reached")

    monkeypatch.setattr(L, "lib", _Refuse())
    psi = qil.SignalMPS.__new__(qil.SignalMPS)             # a state object without a handle: any use of it reaches _Refuse
    for bad in (None, 3, np.ones(4), [np.ones(2)]):
        with pytest.raises(TypeError, match="coefficient_at: unsupported operand types"):
            qil.coefficient_at(bad, np.arange(4))
        for fn, args in ((qil.magnitude, ()), (qil.log_power, (1e-12,)), (qil.shrink, (0.1,))):
            with pytest.raises(TypeError, match="map_states: unsupported operand types"):
                fn(bad, *args)
        with pytest.raises(TypeError, match="map_states: unsupported operand types"):
            qil.divide(psi, bad)
        with pytest.raises(TypeError, match="map_states: unsupported operand types"):
            qil.map_states("abs", bad)
        with pytest.raises(TypeError, match="cross_map: unsupported operand types"):
            qil.cross_map(abs, bad)
        with pytest.raises(TypeError, match="deconvolve: unsupported operand types"):
            qil.deconvolve(bad, psi)
        with pytest.raises(TypeError, match="deconvolve: unsupported operand types"):
            qil.deconvolve(psi, psi, F=bad if bad is not None else 3)
    for host in (np.arange(4), [0, 1, 2], 5):
        with pytest.raises(TypeError, match="coefficient_batch"):
            qil.coefficient_at(psi, host)
    import torch
    with pytest.raises(TypeError, match="coefficient_batch"):
        qil.coefficient_at(psi, torch.arange(4))
    with pytest.raises(TypeError, match="map_states: unsupported operand types"):
        qil.map_states("divide", psi)                       # one state short
    with pytest.raises(TypeError, match="map_states: unsupported operand types"):
        qil.map_states("abs", psi, psi)
    with pytest.raises(ValueError, match="unknown op"):
        qil.map_states("sqrt", psi)
    with pytest.raises(TypeError, match="cross_map: f must be callable"):
        qil.cross_map(3, psi)
    z = qil.ZTMPS.__new__(qil.ZTMPS)
    with pytest.raises(ValueError, match="paired states are not supported; map the SignalMPS and call ztmps_from_mps"):
        qil.magnitude(z)
    with pytest.raises(TypeError, match="deconvolve: unsupported operand types"):
        qil.deconvolve(z, psi)
    for fn in (qil.map_states, qil.cross_map):
        assert "blind spot" in fn.__doc__
    assert "min |F h|" in qil.deconvolve.__doc__ and "unitary" in qil.deconvolve.__doc__


def test_route_helper_mirrors_the_header():
    import qilaplace_jl_amd as qil
    cap = _lib().QIL_COEFFICIENT_AT_WAVE_MAX_BOND
    assert qil.coefficient_at_route([1, 2, cap, 2, 1]) == "wave" and qil.coefficient_at_route([1, 2, cap + 1, 2, 1]) == "bits"
    assert qil.coefficient_at_route([1, 2, cap + 1, 1], "wave") == "wave" and qil.coefficient_at_route([1, 1025, 1], "wave") == "bits"
    assert qil.coefficient_at_route([1, 2, 1], "bits") == "bits" and qil.coefficient_at_route([1, 1]) == "wave"
    src = open(os.path.join(CSRC, "qil_index.hip")).read()
    assert "kWaveFitBond = 1024" in src and 'getenv("QIL_COEFFICIENT_AT_ROUTE")' in src
