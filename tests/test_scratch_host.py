"""CPU: the policy of the library's device-memory pool (abr_iod_amd/csrc/scratch.h, DESIGN.md "Library-owned scratch") against a fake backend
that records every call and fails on demand -- what no GPU test can show without a real out-of-memory condition.  tests/host/scratch_main.cpp
is a stand-alone program; it is built with the address and undefined-behaviour sanitizers and run as a child process (nothing is preloaded)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to build the host program with")
def test_scratch_policy_under_sanitizers(tmp_path):
    exe = str(tmp_path / "scratch_main")
    # (the sanitizer runtimes are linked statically where the compiler has them: the program then does not care in which order the
    # environment loads shared libraries)
    cmd = ["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
           "-I", os.path.join(ROOT, "abr_iod_amd", "csrc"), os.path.join(ROOT, "tests", "host", "scratch_main.cpp"), "-o", exe]
    static = ["-static-libasan", "-static-libubsan"]
    if subprocess.run(cmd + static, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode != 0:
        subprocess.check_call(cmd)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0 and "scratch ok" in run.stdout, run.stdout
