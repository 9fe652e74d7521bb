"""The host side of the gauge sweeps, the signal encoders (qilaplace.jl_amd/csrc/qil_truncate.hip) and the launch-per-step DT
builder (qil_build.hip), read as text with the comments stripped: every pool temporary belongs to a qil_scratch, so no path
frees a block by hand -- least of all twice -- and the LDS grant of the builder's Jacobi kernel is per device.  Needs no GPU.

tests/test_gpu_fused_failures.py makes every allocation of these calls fail in turn on the device; a worker context of a batch
has no call scope behind it, so there the scratch is all that returns a block an early `return` leaves, and this file is what
keeps a bare free or a bare clean-up loop from coming back."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qilaplace.jl_amd", "csrc")


def _code(name):
    text = open(os.path.join(CSRC, name), errors="replace").read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


SOURCES = {f: _code(f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))}
FILES = ("qil_truncate.hip", "qil_build.hip")
# functions that open a call scope and allocate nothing themselves: all their blocks are those of the functions they call
FORWARDERS = ("qil_canonicalize", "compress_impl", "qil_mpo_compress", "qil_signal_ztmps", "qil_ztmps_from_mps")


def _functions(code):
    """(first line, text) of every definition: the pieces between closing braces in column 0, named by their last line in
    column 0 (a signature's continuation lines are indented)."""
    out = []
    for piece in code.split("\n}\n"):
        heads = [ln for ln in piece.split("\n") if ln and not ln[0].isspace() and not ln.startswith(("}", "#"))]
        if heads:
            out.append((heads[-1], piece))
    return out


@pytest.mark.parametrize("name", FILES)
def test_no_block_is_freed_by_hand(name):
    code = SOURCES[name]
    for banned in ("qil_ctx_free(", "bfree(", "static bool", "hipFuncSetAttribute(", "unknown block"):
        assert banned not in code, banned
    assert "qil_scratch" in code and "qil_call_scope" in code


def test_the_lds_grant_has_one_home():
    assert [f for f, code in SOURCES.items() if "hipFuncSetAttribute(" in code] == ["qil_internal.h"]
    assert SOURCES["qil_internal.h"].count("hipFuncSetAttribute(") == 1
    build = SOURCES["qil_build.hip"]
    assert build.count("static qil_lds_grant grant;") == 1
    assert "grant.ensure(ctx->device, reinterpret_cast<const void*>(&bjacobi<true, 1024>)" in build


@pytest.mark.parametrize("name", FILES)
def test_every_call_scope_is_followed_by_a_scratch(name):
    code = SOURCES[name]
    seen = 0
    for head, text in _functions(code):
        at = text.find("qil_call_scope call_scope(")
        if at < 0:
            continue
        seen += 1
        assert text.count("qil_call_scope call_scope(") == 1, head
        if any(f + "(" in head for f in FORWARDERS):
            assert "qil_ctx_alloc(" not in text and ".alloc(" not in text, head
        else:
            assert re.search(r"\bqil_scratch \w+\((ctx|\w+->ctx)\);", text[at:]), head
    assert seen == code.count("qil_call_scope call_scope(") and seen >= 1, (name, seen)


def test_blocks_that_change_hands_are_owned_on_arrival():
    by_head = dict(_functions(SOURCES["qil_truncate.hip"]))
    # the consumers take their operand into their scratch before anything can fail
    for name in ("int compress_tt(", "int svd_sweep("):
        text = next(t for h, t in by_head.items() if h.startswith(name))
        body = text[text.index(") {\n") + 4:]
        assert re.match(r"\s*qil_scratch tmp\(ctx\);\s*tmp\.own\(X\);", body), name
    # a block moves to another context only outside every scratch: the root gives a task away before it is placed, a node
    # gives what it made before the level brings it home, and the root lists what comes home
    root = next(t for h, t in by_head.items() if h.startswith("static int compress_tt_root("))
    assert root.index("keep.give(t.X)") < root.index("qil_run_batch_on(")
    assert "qil_scratch made(work);" in root and "made.give(" in root
    assert root.index("made.give(") < root.index("keep.own(")
