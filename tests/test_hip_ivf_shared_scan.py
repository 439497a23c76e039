"""
The list-major scan of the IVF-Flat index (handle option "ivf_scan" = 1: ivf_scan_shared_kernel behind the pair grouping
of sq_ivf_group.hpp) against the numpy restatement of tests/ivf_cases.py and against the per-query scan ("ivf_scan" = 0)
on the same handle: ids equal, float32 distance bits equal.  stats()["mid_tier_queries"] is the number of (query, list)
pairs the list-major scan served -- every probed pair of a non-empty list -- and 0 when the per-query scan ran.
"""
import numpy as np
import pytest

from smqtk_indexing_amd import _lib
from tests import ivf_cases as C
from tests import width_cases as W

pytestmark = pytest.mark.gpu

_indexes = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _index(key, case):
    if key not in _indexes:
        idx = _lib.IvfIndex(case.centroids)
        idx.add(case.x)
        _indexes[key] = idx
    return _indexes[key]


def _same(got, want_idx, want_dist, what):
    np.testing.assert_array_equal(got[1], want_idx, err_msg=what)
    np.testing.assert_array_equal(_bits(got[0]), _bits(want_dist), err_msg=what)


def _live_pairs(case, queries, nprobe):
    """(query, list) pairs whose list holds rows."""
    sizes = np.diff(case.off)
    return sum(int((sizes[C.probe(case.centroids, q, nprobe)] > 0).sum()) for q in queries)


def _both_scans(idx, case, queries, k, nprobe, want, what, routed=True):
    """Option 1 and option 0 on one handle: the same answer; the stats say which scan ran."""
    idx.set_option("ivf_scan", 1)
    got = idx.search(queries, k, nprobe)
    served = idx.stats()["mid_tier_queries"]
    idx.set_option("ivf_scan", 0)
    old = idx.search(queries, k, nprobe)
    assert idx.stats()["mid_tier_queries"] == 0
    _same(got, *want, what + " (list-major)")
    _same(old, *want, what + " (per query)")
    assert served == (_live_pairs(case, queries, nprobe) if routed else 0), what


@pytest.mark.parametrize("nq", [1, 9, 33])
@pytest.mark.parametrize("nprobe", [1, 5, 64, 100])
@pytest.mark.parametrize("d", C.DIMS)
def test_search_equals_the_restatement(d, nprobe, nq):
    """33 queries at nprobe 64 share every list in groups of 8, 8, 8, 8, 1; nq = 9 is one full group and one of one;
    nprobe 5 shares lists among one to several queries; the far query's first list is empty."""
    case = C.make_case(d)
    idx = _index(d, case)
    for k in (1, 10, 200, 30_000):
        _both_scans(idx, case, case.pool[:nq], k, nprobe, case.expected(nq, nprobe, k), f"d={d} nprobe={nprobe} nq={nq} k={k}")
    cands = sum(case.answer(qi, nprobe)[0].shape[0] for qi in range(nq))
    idx.set_option("ivf_scan", 1)
    idx.search(case.pool[:nq], 10, nprobe)
    st = idx.stats()
    assert (st["candidates"], st["scan_launches"]) == (cands, 1 if cands else 0)


@pytest.mark.parametrize("nq", [1, 33])
@pytest.mark.parametrize("nprobe", [1, 63, 64, 65, 257, 700])
def test_many_lists(nprobe, nq):
    """700 lists of fewer than 256 rows: one chunk per group, many groups, empty lists at probe ranks 63 / 255 / 257 of
    the planted query."""
    case = C.make_many_lists_case()
    idx = _index("many", case)
    for k in (10, 7000):
        _both_scans(idx, case, case.pool[:nq], k, nprobe, case.expected(nq, nprobe, k), f"many lists nprobe={nprobe} nq={nq} k={k}")


WIDTHS = sorted(set(W.WIDTHS) | {35}) + [W.BEYOND[0]]      # 35: rows padded to a stride of 36 floats


@pytest.mark.parametrize("d", WIDTHS)
def test_widths(d):
    """Every width at which the summation branches.  The route takes the widths whose eight staged queries fit the LDS
    (every one of those has a tree the fixed-depth walk covers); beyond them option 1 answers through the per-query scan."""
    case = C.make_width_case(d)
    with _lib.IvfIndex(case.centroids) as idx:
        idx.add(case.x)
        for nprobe in (3, 8):
            _both_scans(idx, case, case.pool, C.W_K, nprobe, case.expected(C.W_POOL, nprobe, C.W_K), f"d={d} nprobe={nprobe}",
                        routed=d <= W.GROUP_LDS_EDGE)


def test_slices():
    """A key budget of 1 MB: 33 queries run a few to a slice (ivf_slice_queries); each slice is grouped and scanned."""
    case = C.make_case(128)
    with _lib.IvfIndex(case.centroids) as idx:
        idx.add(case.x)
        idx.set_option("ivf_key_budget_mb", 1)
        idx.set_option("ivf_scan", 1)
        for nprobe, k in ((C.NLIST, 10), (5, 200)):
            got = idx.search(case.pool, k, nprobe)
            st = idx.stats()
            _same(got, *case.expected(C.POOL, nprobe, k), f"nprobe={nprobe} in slices")
            maxc = max(case.answer(qi, nprobe)[0].shape[0] for qi in range(C.POOL))
            per_slice = (1 << 20) // ((maxc + min(k, maxc)) * 8)
            assert st["scan_launches"] == -(-C.POOL // per_slice) > 1
            assert st["mid_tier_queries"] == _live_pairs(case, case.pool, nprobe)


def test_repeated_query():
    """One query 17 times in a batch: every list it probes is shared by 17 pairs (8 + 8 + 1)."""
    case = C.make_case(36)
    idx = _index(36, case)
    idx.set_option("ivf_scan", 1)
    for qi in (C.Q_ROW7, 4):
        want_idx, want_dist = case.expected(qi + 1, 5, 200)
        one = idx.search(case.pool[qi:qi + 1], 200, 5)
        _same(one, want_idx[qi:], want_dist[qi:], "one query")
        got = idx.search(np.repeat(case.pool[qi:qi + 1], 17, axis=0), 200, 5)
        assert idx.stats()["mid_tier_queries"] == 17 * _live_pairs(case, case.pool[qi:qi + 1], 5)
        _same(got, np.repeat(one[1], 17, axis=0), np.repeat(one[0], 17, axis=0), "17 copies")
