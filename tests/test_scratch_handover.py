"""qil_scratch (qilaplace.jl_amd/csrc/qil_internal.h), the owner of a call's pool temporaries, under AddressSanitizer and
UndefinedBehaviorSanitizer on the CPU: tests/scratch_handover.cpp binds it to a stub pool that counts a second free of an address and
drives the alloc / own / give / free patterns of the overlaps, the lazy read-out and the Born weights, with every allocation and every
later step failing in turn.  No return path may free a block twice or strand one.  Host code only: nothing here opens a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_return_path_frees_twice_or_strands_a_block(tmp_path):
    cxx = shutil.which("g++")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if not cxx or not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime.h")):
        pytest.skip("needs g++ and the HIP headers")
    exe = str(tmp_path / "scratch_handover")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-static-libasan", "-static-libubsan",      # the runtimes inside the program: no library load order to get right
                        "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "qilaplace.jl_amd", "csrc"), os.path.join(ROOT, "tests", "scratch_handover.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr[-3000:]
    assert " 0 double frees" in r.stdout and "186 calls" in r.stdout, r.stdout
