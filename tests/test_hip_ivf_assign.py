"""
Tests of the MFMA nearest-centroid assignment behind every inverted-list build (`ivf_assign_kernel`, option "ivf_assign").

The assignment must be the exact path's for every input: lists are compared exactly with the numpy restatement of
tests/ivf_cases.py (`assign`, `lists_of`) or with option 0 of the same run, and the handle's stats after an add say how
many rows the kernel decided (`candidates`) and how many went to the exact path (`fallback_queries`).
"""
import functools

import numpy as np
import pytest
import torch

from smqtk_indexing_amd import _lib
from tests import ivf_cases as C

gpu = pytest.mark.gpu

# (n, nlist, d): partial and several row tiles, padded and several centroid tiles, unaligned strides, one and many k slabs,
# both sides of the resident / re-staged boundary (kAsgResidentMaxD = 240), the route's last width and the first beyond it
ROUTE_MAX_D = 1024
EDGES = [(1, 1, 1), (300, 31, 1), (127, 2, 3), (129, 31, 4), (300, 33, 33), (300, 65, 35), (300, 257, 36), (300, 257, 128),
         (129, 33, 130), (300, 65, 240), (300, 33, 241), (129, 2, 244), (127, 2, 1024), (300, 2, 1028)]


@functools.lru_cache(maxsize=None)
def edge_case(n, nlist, d):
    rng = np.random.default_rng([11, n, nlist, d])
    x = rng.standard_normal((n, d)).astype(np.float32)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    want = C.lists_of(C.assign(cent, x), nlist)
    for a in (x, cent, *want):
        a.setflags(write=False)
    return x, cent, want


def slack64(d, x, cent):
    """T_i of sq_ivf_assign_plan.hpp (ivf_assign_slack) in float64, X = |x_i| and C = max |c_l|."""
    u = 2.0 ** -24
    X, Cm = np.linalg.norm(x.astype(np.float64), axis=1), np.linalg.norm(cent.astype(np.float64), axis=1).max()
    rel = (8 * d + 64) * X * Cm + 5 * (X * Cm + Cm * Cm) + (2 * d + 14) * (X + Cm) ** 2
    return 1.001 * u * rel + 2.0 ** -60 * (1 + X + Cm) ** 2


class process_option:
    """The process-wide option for a block, put back behind it.  The library has no getter, so "back" is the shipped
    default, 1 (Options::ivf_assign in sq_common.hpp): change the two together.  The same holds for test_option_is_known."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        _lib.set_option("ivf_assign", self.value)

    def __exit__(self, *exc):
        _lib.set_option("ivf_assign", 1)


def test_option_is_known():
    try:
        _lib.set_option("ivf_assign", 0)
        _lib.set_option("ivf_assign", 1)
    finally:
        _lib.set_option("ivf_assign", 1)


@pytest.mark.parametrize("n,nlist,d", [e for e in EDGES if e[2] <= ROUTE_MAX_D])
def test_the_edge_cases_leave_room_to_decide(n, nlist, d):
    """In float64 at least 95 % of a case's rows have a best-to-second gap of |c|^2 - 2 x.c above twice the documented slack,
    so the GPU test may ask that at most 10 % of them reach the exact path."""
    x, cent, _ = edge_case(n, nlist, d)
    c64 = cent.astype(np.float64)
    s = np.sort((c64 * c64).sum(axis=1)[None, :] - 2.0 * x.astype(np.float64) @ c64.T, axis=1)
    gap = s[:, 1] - s[:, 0] if nlist > 1 else np.full(n, np.inf)
    assert (gap > 2 * slack64(d, x, cent)).mean() >= 0.95


@gpu
@pytest.mark.parametrize("n,nlist,d,device", [(*e, False) for e in EDGES] + [(300, 65, 35, True)])
def test_tile_edges(n, nlist, d, device):
    x, cent, want = edge_case(n, nlist, d)
    with _lib.IvfIndex(cent) as idx:
        idx.set_option("ivf_assign", 1)
        if device:
            xd = torch.from_numpy(x.copy()).cuda()
            idx.add(xd.data_ptr(), n=n, device_ptr=True)
        else:
            idx.add(x)
        st = idx.stats()
        got = idx.lists()
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    assert st["candidates"] + st["fallback_queries"] == n
    if d > ROUTE_MAX_D:
        assert st["scan_launches"] == 0 and st["candidates"] == 0
    else:
        assert st["scan_launches"] >= 1 and st["fallback_queries"] <= 0.10 * n


@functools.lru_cache(maxsize=None)
def adversarial_case(d):
    """Integer coordinates, so the planted ties are exact in float32.  Returns rows, centroids, the number of exact ties
    and the rows the restatement does not speak for (one NaN, one inf)."""
    rng = np.random.default_rng([13, d])
    n, nlist = 200, 40
    x = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    cent = rng.integers(-8, 9, size=(nlist, d)).astype(np.float32)
    cent[7] = cent[3]                                  # bit-equal centroids, and rows equal to them
    x[0:5] = cent[3]
    cent[11] = cent[10]
    cent[11, :2] += 2                                  # rows at the exact midpoint of lists 10 and 11
    x[5:10] = cent[10]
    x[5:10, :2] += 1
    cent[21] = cent[20]                                # one ulp apart in one coordinate
    cent[21, 0] = np.nextafter(cent[20, 0], np.float32(np.inf))
    x[10:15] = cent[20]
    x[10:15, 1:6] += rng.integers(-1, 2, size=(5, 5)).astype(np.float32)
    cent[30:35] += 1000                                # a block far from the origin: cancellation inflates the slack
    x[100:120] = cent[30 + np.arange(20) % 5] + rng.integers(-2, 3, size=(20, d)).astype(np.float32)
    x[150, 3], x[151, 5] = np.nan, np.inf
    special = np.array([150, 151])
    a = C.assign(cent, x)
    assert (a[0:5] == 3).all() and (a[5:10] == 10).all() and np.isin(a[10:15], (20, 21)).all() and np.isin(a[100:120], range(30, 35)).all()
    return x, cent, a, 10, special


@gpu
@pytest.mark.parametrize("d", [36, 128])
def test_ties_and_bad_rows_go_to_the_exact_path(d):
    x, cent, want, ties, special = adversarial_case(d)
    lists, stats = {}, {}
    for mode in (0, 1):
        with _lib.IvfIndex(cent) as idx:
            idx.set_option("ivf_assign", mode)
            idx.add(x)
            lists[mode], stats[mode] = idx.lists(), idx.stats()
    for g, w in zip(lists[1], lists[0]):
        np.testing.assert_array_equal(g, w)
    off, ids = lists[1]
    got = np.empty(len(x), dtype=np.int64)
    got[ids] = np.repeat(np.arange(len(cent)), np.diff(off))
    keep = np.setdiff1d(np.arange(len(x)), special)
    np.testing.assert_array_equal(got[keep], want[keep])
    assert stats[1]["scan_launches"] == 1 and stats[1]["fallback_queries"] >= ties + len(special)
    assert stats[0]["scan_launches"] == 0 and stats[0]["fallback_queries"] == len(x)


@gpu
def test_kmeans_and_pq_train_are_the_same_bits():
    rng = np.random.default_rng(17)
    x = rng.standard_normal((3000, 100)).astype(np.float32)
    y = rng.standard_normal((2000, 32)).astype(np.float32)
    out = {}
    for mode in (0, 1):
        with process_option(mode):
            out[mode] = [_lib.ivf_kmeans(x, x[:40], 5)] + [
                _lib.pq_train(y, np.ascontiguousarray(y[:ksub].reshape(ksub, 8, 4).transpose(1, 0, 2)), 3) for ksub in (256, 16)]
    for a, b in zip(out[0], out[1]):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


@gpu
@pytest.mark.parametrize("kind", ["pq", "pq_residual", "pq_packed", "isq"])
def test_coded_indexes_are_the_same_bits(kind):
    rng = np.random.default_rng(19)
    x = rng.standard_normal((5000, 32)).astype(np.float32)
    cent = x[:50]
    ksub = 16 if kind == "pq_packed" else 256
    books = np.ascontiguousarray(x[100:100 + ksub].reshape(ksub, 8, 4).transpose(1, 0, 2))
    out = {}
    for mode in (0, 1):
        if kind == "isq":
            idx = _lib.IsqIndex(cent, _lib.SQ_ISQ_SQ8, *_lib.isq_train(x))
        else:
            idx = _lib.PqIndex(cent, books, residual=kind == "pq_residual", packed=kind == "pq_packed")
        with idx:
            idx.set_option("ivf_assign", mode)
            idx.add(x)
            out[mode], st = idx.lists(), idx.stats()
        assert (st["scan_launches"] >= 1) == (mode == 1) and st["candidates"] + st["fallback_queries"] == (1 if kind == "isq" else 9) * len(x)
    for a, b in zip(out[0], out[1]):
        np.testing.assert_array_equal(a, b)
