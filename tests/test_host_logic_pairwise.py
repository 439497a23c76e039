"""
The tree walks that every exact distance rests on (smqtk_indexing_amd/csrc/sq_pairwise.hpp: pw_tree / pw_tree_buffer,
pw_tree_multi, pw_tree_depth) on the CPU, at EVERY row width 1 .. 8192 and at widths beyond numpy's 8192-element
buffers, under AddressSanitizer and UndefinedBehaviorSanitizer.

tests/host/pairwise_main.cpp includes the real header (tests/host/hip_stub/hip/hip_runtime.h stands in for the runtime),
supplies a plainly written leaf (numpy's rule for 128 elements or fewer) and prints the bits of every sum; they are
compared here with np.sum of the same elements -- numpy itself, not the oracle's restatement -- byte for byte, float32
and float64, and the group walk (three sums per pass, the exact path's depth) at every width that depth takes.
pw_tree_depth is checked against a three-line recursion.  The program is linked statically against the sanitizer
runtime -- nothing is preloaded -- and must end with status 0 and without a report.

Before the program's output is looked at the inputs have to show that they can tell a wrong walk from a right one:
a left-to-right sum and an even split (n // 2 without the rounding to a multiple of 8) must differ from np.sum nearly
everywhere.
"""
import os
import subprocess

import numpy as np
import pytest

from tests.test_host_logic_buffers import HOST, _clangxx

pytestmark = pytest.mark.skipif(_clangxx() is None, reason="ROCm's clang++ is not installed: nothing to compile the program with")

# One vector tells an even split from numpy's at about a third of the widths where the two differ (measured: an input
# property, not the code's); R independent vectors miss a width with probability (2/3)^R, below 1 % from R = 12 on.
R, L, SEED = 16, 20000, 5
BUF = 8192
BEYOND = (8193, 8199, 8200, 8300, 12288, 16384, 16385, 20000)
WIDTHS = tuple(range(1, BUF + 1)) + BEYOND
GROUP_DEPTH = 6          # EXACT_GROUP_DEPTH (sq_pairwise.hpp): the program prints its own and a `multi` line per width that takes


def _split(n):
    return n // 2 - (n // 2) % 8


def _depth(n):
    return 0 if n <= 128 else 1 + max(_depth(_split(n)), _depth(n - _split(n)))


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(SEED)
    a32 = np.square(rng.standard_normal((R, L)).astype(np.float32) * 7)
    a64 = np.square(rng.standard_normal((R, L)) * 7)
    assert a32.dtype == np.float32 and a64.dtype == np.float64
    return a32, a64


@pytest.fixture(scope="module")
def numpy_sums(data):
    """np.sum(a[:n]) of every vector at every width: {n: [R] array}, float32 and float64."""
    a32, a64 = data
    ref32 = {n: np.array([np.sum(a32[r, :n]) for r in range(R)], dtype=np.float32) for n in WIDTHS}
    ref64 = {n: np.array([np.sum(a64[r, :n]) for r in range(R)], dtype=np.float64) for n in WIDTHS}
    return ref32, ref64


@pytest.fixture(scope="module")
def output(tmp_path_factory, data):
    tmp = tmp_path_factory.mktemp("pairwise")
    exe, path = str(tmp / "pairwise_main"), str(tmp / "vectors.bin")
    with open(path, "wb") as f:
        f.write(data[0].tobytes())
        f.write(data[1].tobytes())
    cmd = [_clangxx(), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libsan",
           "-I", os.path.join(HOST, "hip_stub"), os.path.join(HOST, "pairwise_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, "compiling tests/host/pairwise_main.cpp failed:\n" + r.stdout[-4000:]
    r = subprocess.run([exe, path, str(R), str(L)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True,
                       timeout=600)
    assert r.returncode == 0, "status %d:\n%s" % (r.returncode, r.stdout[-4000:])
    return r.stdout


def _even_split_sums(a):
    """The walk with the split at n // 2, NOT rounded down to a multiple of 8, for all rows of `a` at once: {n: [R]}.
    (Leaves are np.sum over 128 elements or fewer of each row; left parts start at 0 and are shared between widths.)"""
    memo = {}

    def tree(off, m):
        if m <= 128:
            return np.sum(a[:, off:off + m], axis=1)
        if (off, m) not in memo:
            memo[(off, m)] = tree(off, m // 2) + tree(off + m // 2, m - m // 2)
        return memo[(off, m)]

    return {n: tree(0, n) for n in range(129, BUF + 1) if (n // 2) % 8}


def test_inputs_tell_a_wrong_walk_from_a_right_one(data, numpy_sums):
    a32, _ = data
    ref32, _ = numpy_sums
    # (the leaves of _even_split_sums: a row-wise sum of a slice is numpy's sum of that row's elements)
    for n in (1, 7, 8, 100, 128):
        assert np.sum(a32[:, 40:40 + n], axis=1).tobytes() == np.array([np.sum(a32[r, 40:40 + n]) for r in range(R)]).tobytes()
    # a left-to-right float32 sum of one vector differs from np.sum at nearly every width
    serial = np.cumsum(a32[0], dtype=np.float32)
    assert serial[:7].tobytes() == np.array([ref32[n][0] for n in range(1, 8)], dtype=np.float32).tobytes()   # (below 8 numpy is serial)
    ns = range(16, BUF + 1)
    differ = sum(serial[n - 1] != ref32[n][0] for n in ns)
    print("left-to-right differs at %d of %d widths (%.1f %%)" % (differ, len(ns), 100.0 * differ / len(ns)))
    assert differ >= 0.95 * len(ns)
    # an even split differs, for at least one of the R vectors, at nearly every width where it is another split
    even = _even_split_sums(a32)
    assert len(even) == sum(1 for n in range(129, BUF + 1) if (n // 2) % 8) > 7000
    differ = sum(bool((even[n] != ref32[n]).any()) for n in even)
    one = sum(bool(even[n][0] != ref32[n][0]) for n in even)
    print("even split differs at %d of %d widths (%.1f %%); one vector alone: %.1f %%"
          % (differ, len(even), 100.0 * differ / len(even), 100.0 * one / len(even)))
    assert differ >= 0.99 * len(even)


def _lines(output, word):
    out = {}
    for ln in output.splitlines():
        if ln.startswith(word + " "):
            f = ln.split()
            assert int(f[1]) not in out, ln
            out[int(f[1])] = f[2:]
    return out


def test_program_ends_clean(output):
    assert output.rstrip().endswith("pairwise ok"), output[-4000:]
    for word in ("Sanitizer", "runtime error", "CHECK("):
        assert word not in output, output[-4000:]


def test_tree_depth_at_every_width(output):
    got = _lines(output, "depth")
    assert sorted(got) == list(range(1, BUF + 1))
    want = {n: _depth(n) for n in range(1, BUF + 1)}
    assert {n: int(v[0]) for n, v in got.items()} == want
    # the right spine goes deeper than ceil(log2(n / 128)): 441 widths need 7 levels, all of them in 7689 .. 8191
    deep = [n for n, v in want.items() if v > GROUP_DEPTH]
    assert (len(deep), min(deep), max(deep), max(want.values())) == (441, 7689, 8191, 7)
    assert want[8192] == 6 and want[255] == 2 and want[256] == 1     # (255 = a leaf of 120 + a subtree of 135)


def test_walk_matches_numpy_at_every_width(output, numpy_sums):
    ref32, ref64 = numpy_sums
    for word, ref, view in (("f32", ref32, np.uint32), ("f64", ref64, np.uint64)):
        got = _lines(output, word)
        assert sorted(got) == sorted(WIDTHS), word
        bad = [n for n in WIDTHS if [int(h, 16) for h in got[n]] != ref[n].view(view).tolist()]
        assert not bad, "%s: %d widths differ from np.sum, the first %s" % (word, len(bad), bad[:20])


def test_group_walk_matches_numpy_at_every_width_its_depth_takes(output, numpy_sums):
    ref32, _ = numpy_sums
    assert "group_depth %d\n" % GROUP_DEPTH in output       # the constant the library is compiled with
    got = _lines(output, "multi")
    takes = [n for n in range(1, BUF + 1) if _depth(n) <= GROUP_DEPTH]
    assert sorted(got) == takes and len(takes) == BUF - 441
    bad = [n for n in takes if [int(h, 16) for h in got[n]] != ref32[n].view(np.uint32).tolist()]
    assert not bad, "%d widths differ from np.sum, the first %s" % (len(bad), bad[:20])
