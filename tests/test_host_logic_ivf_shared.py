"""
The host arithmetic of the list-major IVF-Flat scan, without a GPU: tests/host/ivf_shared_plan_main.cpp over
smqtk_indexing_amd/csrc/sq_ivf_plan.hpp (plain C++), compiled with ROCm's clang++ under AddressSanitizer and
UndefinedBehaviorSanitizer and linked statically against the sanitizer runtime -- nothing is preloaded and nothing is
loaded into Python.  It cuts lists of 0 .. 1025 rows probed by 1 .. 3 G + 1 pairs into groups and work items, walks them
as the kernel does and checks that every row of every pair is covered once, that the launch bound holds, and the route.
"""
import os
import subprocess

import pytest

from tests.test_host_logic_buffers import HOST, _clangxx


@pytest.mark.skipif(_clangxx() is None, reason="ROCm's clang++ is not installed: nothing to compile the program with")
def test_shared_scan_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "ivf_shared_plan_main")
    cmd = [_clangxx(), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libsan",
           os.path.join(HOST, "ivf_shared_plan_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, "compiling tests/host/ivf_shared_plan_main.cpp failed:\n" + r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0, "status %d:\n%s" % (r.returncode, r.stdout[-4000:])
    assert "ivf shared plan ok: group=8 chunk=256" in r.stdout, r.stdout[-4000:]
    for word in ("Sanitizer", "runtime error"):
        assert word not in r.stdout, r.stdout[-4000:]
