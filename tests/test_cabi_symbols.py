"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol
include/qilaplace_hip.h declares; host-side argument parsing mirrors the reference."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


TESTING_HOOKS = {"qil_context_fail_alloc_after", "qil_context_unowned_bytes", "qil_timer_start", "qil_timer_stop",
                 "qil_profile_enable", "qil_profile_read", "qil_gemm_device_time", "qil_hbm_store_peak",
                 "qil_gemm_plan", "qil_gemm_batched_host", "qil_readout_route", "qil_qr_plan", "qil_qr_host"}


def _symbols_of(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(qil_[a-z0-9_]+)\s*\(", src))


def _declared_symbols():
    """Boundary (include/qilaplace_hip.h) + test / measurement hooks (include/qilaplace_hip_testing.h)."""
    return sorted(_symbols_of("qilaplace_hip.h") | _symbols_of("qilaplace_hip_testing.h"))


def test_testing_hooks_live_in_their_own_header():
    """fault injection, pool accounting, timers and the kernel profile are not part of SURVEY 8(b)'s interface."""
    assert _symbols_of("qilaplace_hip_testing.h") == TESTING_HOOKS
    assert not (_symbols_of("qilaplace_hip.h") & TESTING_HOOKS)


def test_header_declares_the_boundary():
    syms = _declared_symbols()
    for must in ("qil_apply", "qil_apply_into", "qil_apply_mpo_mpo", "qil_coefficient_batch",
                 "qil_compress", "qil_canonicalize", "qil_signal_mps", "qil_signal_ztmps", "qil_rsvd",
                 "qil_mps_to_vector", "qil_norm", "qil_mps_create", "qil_mpo_create", "qil_last_error"):
        assert must in syms


def test_library_exports_every_declared_symbol():
    import qilaplace_jl_amd as qil
    lib = ctypes.CDLL(qil.LIB_PATH)
    missing = [s for s in _declared_symbols() if not hasattr(lib, s)]
    assert not missing, f"declared in the header but not exported: {missing}"


def test_library_exports_nothing_but_the_declared_symbols():
    """built with -fvisibility=hidden + a linker version script, the dynamic symbol table of the drop-in
    library is the C ABI and nothing else -- no mangled C++ internals, no weak STL instantiations, no HIP unit ids."""
    import subprocess
    import qilaplace_jl_amd as qil
    out = subprocess.run(["nm", "-D", "--defined-only", qil.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {l.split()[-1].split("@")[0] for l in out.splitlines() if l.strip()}
    assert not [s for s in exported if s.startswith("_Z")], "mangled C++ symbols exported"
    assert exported == set(_declared_symbols()), exported ^ set(_declared_symbols())


def test_library_build_is_reproducible(tmp_path):
    """r06: -ffile-prefix-map and a fixed -cuid per source make libqilhip.so bit-reproducible whatever directory it is built in, so the
    sha256 the evidence under profiles/ is keyed to (bench.py: `config.lib_sha16`, `roofline.traffic_source`) can be re-derived from
    the sources: `git archive HEAD` into a scratch directory, `make`, compare.  Two and a half minutes of hipcc: opt-in
    (QIL_TEST_REBUILD=1)."""
    import hashlib
    import shutil
    import subprocess
    if os.environ.get("QIL_TEST_REBUILD") != "1":
        pytest.skip("set QIL_TEST_REBUILD=1 (rebuilds the whole library, ~2.5 min)")
    import qilaplace_jl_amd as qil
    src = os.path.join(str(tmp_path), "src")
    os.makedirs(src)
    for d in ("include", os.path.join("qilaplace.jl_amd", "csrc")):
        shutil.copytree(os.path.join(ROOT, d), os.path.join(src, d))
    subprocess.run(["make", "-C", os.path.join(src, "qilaplace.jl_amd", "csrc"), "-j", "8"], check=True, capture_output=True)
    sha = lambda p: hashlib.sha256(open(p, "rb").read()).hexdigest()
    assert sha(os.path.join(src, "qilaplace.jl_amd", "lib", "libqilhip.so")) == sha(qil.LIB_PATH)


def test_python_prototypes_cover_the_header():
    import importlib
    L = importlib.import_module("qilaplace_jl_amd._lib")
    declared = set(_declared_symbols())
    bound = set(L.PROTOTYPES) | {"qil_last_error", "qil_version"}
    assert declared == bound, (declared ^ bound)


def test_config_parsing_matches_reference_front_ends():
    import importlib
    ops = importlib.import_module("qilaplace_jl_amd.ops")
    for cfg in ([1, 0, 1], (1, 0, 1), "101", "[1,0,1]", "1 0 1", 0b101):
        assert ops._parse_config(cfg, 3) == [1, 0, 1]
    with pytest.raises(ValueError, match="more than 3 bits"):
        ops._parse_config(8, 3)
    with pytest.raises(ValueError, match="non-negative"):
        ops._parse_config(-1, 3)
    with pytest.raises(ValueError, match="only '0' or '1'"):
        ops._parse_config("1a1", 3)
    with pytest.raises(ValueError, match="empty"):
        ops._parse_config("[]", 3)


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "qilaplace.jl_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(import|from)\s+oracle\b", txt, flags=re.M), f
    bench = open(os.path.join(ROOT, "qilaplace_jl_amd.py")).read()
    assert "oracle" not in bench


def _build_c_client(tmp_path):
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "qilaplace.jl_amd", "lib")
    exe = os.path.join(str(tmp_path), "cabi_client")
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(root, "include"),
                        os.path.join(root, "tests", "cabi_client.c"), "-L", lib, "-lqilhip", f"-Wl,-rpath,{lib}", "-lm",
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_host_only_c99_client_runs_without_a_gpu(tmp_path):
    """The host-only entries of the boundary from plain C, RUN here: the layout rule of the multi-GPU gather,
    the CPU budget, the version string and the error convention (tests/cabi_host_client.c)."""
    import shutil
    import subprocess
    lib = os.path.join(ROOT, "qilaplace.jl_amd", "lib")
    exe = os.path.join(str(tmp_path), "cabi_host_client")
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cabi_host_client.c"), "-L", lib, "-lqilhip", f"-Wl,-rpath,{lib}",
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.returncode, r.stdout, r.stderr)


def test_plain_c99_client_compiles_and_links(tmp_path):
    """The header is C (not C++): a C99 translation unit using the boundary compiles warning-free and links against
    libqilhip.so.  (It is RUN by the GPU suite.)"""
    _build_c_client(tmp_path)


def test_host_cpu_budget_follows_quota_ranks_and_override():
    """qil_host_cpu_budget (no GPU needed): min(cgroup quota, affinity) / LOCAL_WORLD_SIZE, QIL_CPU_BUDGET overrides -- what caps the
    polling launcher threads of the lock-step batches when 8 ranks share a node's CPU quota."""
    import subprocess
    import sys
    code = "import qilaplace_jl_amd as q; print(q.host_cpu_budget())"

    def run(**env):
        e = dict(os.environ, **env)
        for k in ("QIL_CPU_BUDGET", "LOCAL_WORLD_SIZE"):
            if k not in env:
                e.pop(k, None)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=e, timeout=300)
        assert r.returncode == 0, r.stderr
        return int(r.stdout.strip().splitlines()[-1])

    base = run()
    avail = len(os.sched_getaffinity(0))
    assert 1 <= base <= avail
    assert run(QIL_CPU_BUDGET="3") == 3
    assert run(LOCAL_WORLD_SIZE="2") == max(1, base // 2)
    assert run(LOCAL_WORLD_SIZE="1000") == 1
