"""
The asynchronous call pipeline and the host-memory call (smqtk_indexing_amd/csrc/sq_pipeline.hpp: SlotSync, CallRing,
staged_call) on the CPU, under AddressSanitizer (with its leak check) and UndefinedBehaviorSanitizer.

tests/host/pipeline_main.cpp includes the real header; tests/host/hip_stub/hip/hip_runtime.h stands in for the runtime:
streams and events are counted heap objects, and what is recorded on them and waited for goes into a log, so the program
asserts the rotation of the call slots, what is resolved when, the order of the events of a call and -- with the N-th
allocation failing -- what a host-memory call leaves behind.  Built and run as tests/test_host_logic_buffers.py does it:
linked statically against the sanitizer runtime, nothing preloaded, status 0 and no report.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")


def _clangxx():
    hipcc = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for sub in (("llvm", "bin"), ("lib", "llvm", "bin")):
        p = os.path.join(rocm, *sub, "clang++")
        if os.path.isfile(p) and os.access(p, os.X_OK):
            return p
    return None


pytestmark = pytest.mark.skipif(_clangxx() is None, reason="ROCm's clang++ is not installed: nothing to compile the program with")


def test_call_pipeline_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pipeline_main")
    cmd = [_clangxx(), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libsan",
           "-I", os.path.join(HOST, "hip_stub"), os.path.join(HOST, "pipeline_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, "compiling tests/host/pipeline_main.cpp failed:\n" + r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0, "status %d:\n%s" % (r.returncode, r.stdout[-4000:])
    assert "pipeline ok" in r.stdout, r.stdout[-4000:]
    for word in ("Sanitizer", "runtime error"):
        assert word not in r.stdout, r.stdout[-4000:]
