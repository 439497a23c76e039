"""
The host arithmetic of the dense index's int8 copy (smqtk_indexing_amd/csrc/sq_dense_i8_policy.hpp) on the CPU, under
AddressSanitizer and UndefinedBehaviorSanitizer: the choice among the clamp candidates (first cut inside the budget per
clamp, smallest bound across clamps, none; the budget's floor; counts of every 8th row, saturating) and the truth table
of what an index does about its copy when its row count changes.

tests/host/i8_policy_main.cpp includes the real header (plain C++: no runtime, no stand-in) and checks those itself; it
prints the candidates for one (rms, d), which are recomputed here from their formulas in the same number formats.  The
program is linked statically against the sanitizer runtime -- nothing is preloaded -- and must end with status 0 and
without a report.
"""
import math
import os
import subprocess

import numpy as np
import pytest

from tests.test_host_logic_buffers import HOST, _clangxx

pytestmark = pytest.mark.skipif(_clangxx() is None, reason="ROCm's clang++ is not installed: nothing to compile the program with")

CLAMPS = (1.75, 2.5, 3.25, 4.0, 4.75, 5.5, 6.5, 7.5, 9.0, 11.0, 14.0, 18.0)   # multiples of the element rms
CUTS = (0.6, 0.8, 1.0, 1.10, 1.15, 1.20, 1.30, 1.50, 2.0, 3.0)                # R in units of Dx sqrt(d / 12)


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("i8_policy") / "i8_policy_main")
    cmd = [_clangxx(), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libsan",
           os.path.join(HOST, "i8_policy_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, "compiling tests/host/i8_policy_main.cpp failed:\n" + r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0, "status %d:\n%s" % (r.returncode, r.stdout[-4000:])
    return r.stdout


def test_choice_and_append_action_under_sanitizers(output):
    assert "i8 policy ok" in output, output[-4000:]
    for word in ("Sanitizer", "runtime error"):
        assert word not in output, output[-4000:]


def test_clip_candidates_match_their_formulas(output):
    lines = output.splitlines()
    head = next(ln for ln in lines if ln.startswith("candidates "))
    fields = dict(w.split("=") for w in head.split()[1:])
    rms, d = float.fromhex(fields["rms"]), int(fields["d"])
    assert (int(fields["nclip"]), int(fields["ncut"])) == (len(CLAMPS), len(CUTS))
    assert tuple(float.fromhex(w) for w in next(ln for ln in lines if ln.startswith("cuts")).split()[1:]) == CUTS
    rows = [ln.split() for ln in lines if ln.startswith("clamp ")]
    assert len(rows) == len(CLAMPS)
    unit = math.sqrt(d / 12.0)
    for clamp, row in zip(CLAMPS, rows):
        assert float.fromhex(row[1]) == clamp
        dx = np.float32(clamp * rms / 127.0)            # the step: float64 arithmetic, rounded once
        inv_dx = np.float32(1.0) / dx                   # its reciprocal: a float32 division
        assert np.float32(float.fromhex(row[3])) == dx and float.fromhex(row[3]) == float(dx)
        assert float.fromhex(row[5]) == float(inv_dx) and type(inv_dx) is np.float32
        cuts = [float.fromhex(w) for w in row[7:]]
        assert len(cuts) == len(CUTS)
        for cut, got in zip(CUTS, cuts):
            r = cut * float(dx) * unit                  # R of this pair, float64
            assert got == float(np.float32(r * r))
