"""
The owning buffer types (smqtk_indexing_amd/csrc/sq_buffers.hpp: DevBuf, HostPinned, PinnedStage, grow_keep) on the CPU,
under AddressSanitizer (with its leak check) and UndefinedBehaviorSanitizer.

tests/host/buffers_main.cpp includes the real header; tests/host/hip_stub/hip/hip_runtime.h stands in for the runtime
(malloc / free / memcpy, and it can fail the N-th allocation).  The program is linked statically against the sanitizer
runtime -- nothing is preloaded -- and must end with status 0 and without a report: a free the types forget is a
leak, one they do twice or a block used after a move an address error.
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


def test_owning_buffers_under_sanitizers(tmp_path):
    exe = str(tmp_path / "buffers_main")
    cmd = [_clangxx(), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libsan",
           "-I", os.path.join(HOST, "hip_stub"), os.path.join(HOST, "buffers_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, "compiling tests/host/buffers_main.cpp failed:\n" + r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0, "status %d:\n%s" % (r.returncode, r.stdout[-4000:])
    assert "buffers ok" in r.stdout, r.stdout[-4000:]
    for word in ("Sanitizer", "runtime error"):
        assert word not in r.stdout, r.stdout[-4000:]
