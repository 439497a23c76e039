"""
The host side of the list-major IVF-SQ scan, without a GPU: tests/host/isq_shared_plan_main.cpp over
smqtk_indexing_amd/csrc/sq_isq_plan.hpp (plain C++), compiled with ROCm's clang++ under AddressSanitizer and
UndefinedBehaviorSanitizer and linked statically against the sanitizer runtime (nothing is preloaded, nothing is loaded
into Python), checks the LDS sizes and the route per kind.  Here: "isq_scan" is an option the library knows, an unknown
name is still refused, and the scan added no entry point.
"""
import os
import subprocess

import pytest

from smqtk_indexing_amd import _lib
from tests.test_host_logic_buffers import HOST, _clangxx


@pytest.mark.skipif(_clangxx() is None, reason="ROCm's clang++ is not installed: nothing to compile the program with")
def test_isq_shared_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "isq_shared_plan_main")
    cmd = [_clangxx(), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libsan",
           os.path.join(HOST, "isq_shared_plan_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, "compiling tests/host/isq_shared_plan_main.cpp failed:\n" + r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0 and "isq shared plan ok: group=8 lds=163584" in r.stdout, "status %d:\n%s" % (r.returncode, r.stdout[-4000:])
    assert "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]


def test_the_option_is_known_and_no_entry_point_was_added():
    for value in (0, 1, -1):                          # -1 last: the shipped default
        _lib.set_option("isq_scan", value)
    with pytest.raises(Exception, match="unknown option"):
        _lib.set_option("isq_scan_", 1)
    assert (len(_lib.ISQ_EXPORTS), len(_lib.IVF_EXPORTS), len(_lib.EXPORTS)) == (7, 7, 44)
