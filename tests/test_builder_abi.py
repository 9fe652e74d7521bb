"""CPU-side checks of the builders' argument validation (qil_build_dt_mpo_batch, qil_build_zt_mpo_batch): a damping value that
is NaN or infinite, or negative where a gate entry exp(-w 2^(n-2)) overflows, is refused with QIL_EINVAL_ARG naming its index
before the context is activated -- this runs on a machine without a GPU, where an activation would fail with QIL_EHIP
instead -- and therefore before any allocation or launch.  tests/test_gpu_builders.py sends the same values through the Python
front-ends on the device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QIL_EINVAL_ARG = 7
ENTRIES = ("qil_build_dt_mpo_batch", "qil_build_zt_mpo_batch")


def _lib():
    import importlib
    return importlib.import_module("qilaplace_jl_amd._lib")


def _call(entry, n, values):
    """The entry with a context that is never looked at: zeroed host memory stands in for it (the refusal comes first)."""
    L = _lib()
    fake = ctypes.create_string_buffer(1 << 16)
    w = (ctypes.c_double * len(values))(*values)
    outs = (ctypes.c_void_p * len(values))()
    st = getattr(L.lib, entry)(ctypes.cast(fake, ctypes.c_void_p), n, len(values), w, 1e-14, 1000, None, outs)
    assert all(h is None for h in outs)
    return st, L.last_error()


def test_checks_precede_the_activation_in_the_source():
    for entry, name in zip(ENTRIES, ("qil_build.hip", "qil_build_zt.hip")):
        src = open(os.path.join(ROOT, "qilaplace.jl_amd", "csrc", name)).read()
        body = re.search(r'extern "C" int ' + entry + r"\(.*?\n}\n", src, flags=re.S).group(0)
        assert 0 < body.find("qil_check_damping_values") < body.find("qil_ctx_activate")
        assert body.find("qil_check_damping_values") < body.find("qil_call_scope")


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("n,values,index,what", [
    (8, [0.5, float("nan")], 1, "not finite"),
    (8, [float("inf"), 1.0], 0, "not finite"),
    (1, [1.0, 2.0, float("-inf")], 2, "not finite"),
    (24, [0.25, 1.0, -0.5], 2, "overflows"),             # exp(0.5 2^22) = inf
    (12, [-1.0], 0, "overflows"),                        # exp(2^10) = inf
    (2, [-710.0], 0, "overflows"),                       # exp(710) = inf: the gate exp(-w) of the shortest chains
])
def test_bad_damping_values_are_refused_by_index(entry, n, values, index, what):
    st, msg = _call(entry, n, values)
    assert st == QIL_EINVAL_ARG
    assert re.search(rf"damping value {index} .*{what}", msg), msg
    assert msg.startswith("build_dt_mpo" if "dt" in entry else "build_zt_mpo")
