"""The host side of the read-out (qilaplace.jl_amd/csrc/qil_readout.hip), read as text with the comments stripped: every pool
temporary belongs to a qil_scratch, the fill, the finish, the slice selection and the row gather are each written once, the route
is decided once per read-out, and the download has one home.  Needs no GPU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qilaplace.jl_amd", "csrc")


def _code(name):
    text = open(os.path.join(CSRC, name), errors="replace").read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


SOURCES = {f: _code(f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))}
READOUT = SOURCES["qil_readout.hip"]


def _function(code, head):
    """The text of the function whose definition starts with `head`, up to the closing brace in column 0."""
    start = code.index(head)
    return code[start:code.index("\n}\n", start) + 3]


def test_the_temporaries_belong_to_a_scratch():
    assert "qil_ctx_free(" not in READOUT
    assert "#define" not in READOUT
    assert "qil_scratch" in READOUT and "qil_call_scope" in READOUT
    # every entry point that opens a call scope declares its scratch right behind it
    scopes = [m.end() for m in re.finditer(r"qil_call_scope call_scope\(ctx\);\n", READOUT)]
    assert len(scopes) == 4
    for at in scopes:
        assert READOUT[at:].lstrip().startswith("qil_scratch tmp(ctx);")
    assert "qil_scratch tmp(psi->ctx);" in _function(READOUT, "static int coefficient_enqueue(")
    assert "const int* dmap" in _function(READOUT, "struct SortPlan {")          # the plan points into its builder's scratch
    assert "static int build_sort_plan(qil_scratch& tmp," in READOUT


def test_each_kernel_body_has_one_home():
    homes = {"fill_ones": "qil_contract.hip", "finish_coeff": "qil_readout.hip", "select_slice": "qil_readout.hip",
             "gather_rows": "qil_readout.hip"}
    for body, home in homes.items():
        hits = [f for f, code in SOURCES.items() if re.search(r"\bvoid " + body + r"_body\(", code)]
        assert hits == [home], (body, hits)
        assert len(re.findall(r"\bvoid " + body + r"_body\(", SOURCES[home])) == 1, body
        assert [f for f, code in SOURCES.items() if re.search(r"\bstruct " + body + r"_k\b", code)] == [home], body
    for f, code in SOURCES.items():                                                # no plain kernel beside the table form
        assert not re.search(r"__global__[^;{]*\bvoid (finish_coeff|fill_ones)\(", code), f
    # the only fill-with-one and the only last step are the shared functions
    for name, home in (("int qil_dev_fill_ones(", "qil_contract.hip"), ("int qil_dev_finish_coeff(", "qil_readout.hip")):
        assert sorted(f for f, code in SOURCES.items() if name in code) == sorted(["qil_internal.h", home]), name
    assert READOUT.count("finish_coeff_k<") == 1 and READOUT.count("qil_dev_fill_ones(") >= 4
    assert "qil_apply_sizes_of(" in _function(READOUT, "static int readout_route(")
    assert "qil_apply_sizes_of(W, psi)" in _function(READOUT, "int lazy_gemm_path(")
    assert READOUT.count("ChainSite{") == 1                                        # one builder of the site table


def test_the_route_is_decided_once_per_readout():
    assert READOUT.count("static int readout_route(") == 1
    for head in ("static int coefficient_enqueue(", "static bool wants_sort_plan(", "int qil_apply_coefficient_sweep_dev(",
                 'extern "C" int qil_apply_coefficient_sweep(', 'extern "C" int qil_apply_coefficient_batch('):
        assert _function(READOUT, head).count("readout_route(") <= 1, head
    enqueue = _function(READOUT, "static int coefficient_enqueue(")
    assert enqueue.count("readout_route(") == 1
    for route in ("readout_chain(", "readout_gemm_select(", "readout_gemm_sorted("):
        assert enqueue.count(route) == 1 and READOUT.count("static int " + route) == 1, route


def test_the_download_has_one_home():
    hits = sorted(f for f, code in SOURCES.items() if "int qil_download(" in code)
    assert hits == ["qil_contract.hip", "qil_internal.h"]
    for f in hits:
        assert SOURCES[f].count("int qil_download(") == 1, f
    body = _function(SOURCES["qil_contract.hip"], "int qil_download(")
    assert "QIL_HIP(hipMemcpyAsync(" in body and "hipMemcpyDeviceToHost" in body and "QIL_HIP(qil_stream_sync(ctx))" in body
    assert READOUT.count("return qil_download(") == 4 and "hipMemcpyDeviceToHost" not in READOUT
    assert "qil_fail(" not in READOUT and "hipStreamSynchronize" not in READOUT     # QIL_HIP / QIL_TRY / QIL_REQUIRE throughout
