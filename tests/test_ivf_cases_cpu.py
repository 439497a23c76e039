"""
CPU tests of tests/ivf_cases.py, the case builder and numpy restatement behind tests/test_hip_ivf.py: every case the GPU
tests run is built here, so the conditions they lean on (two empty lists, a list longer than a scan chunk, a list
shorter than k = 200, the 41-way tie at distance 0, the far query's empty first list) are proven without a GPU; and the
restatement with every list probed is the oracle's `dense_topk` over all rows, ids and float32 bits.
"""
import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import ivf_cases as C


# the cases are cut for the library's own constants: chunk of the scan, lists the coarse index answers exactly
assert C.SCAN_CHUNK == C.plan_constant("kIvfChunk") and C.NLIST <= C.plan_constant("kIvfMaxLists")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("d", C.DIMS)
def test_builder_conditions_hold(d):
    case = C.make_case(d)                                                # asserts the conditions itself
    sizes = np.diff(case.off)
    assert case.x.shape == (C.N, d) and case.centroids.shape == (C.NLIST, d) and case.pool.shape == (C.POOL, d)
    assert case.off[0] == 0 and case.off[-1] == C.N and np.array_equal(np.sort(case.order), np.arange(C.N))
    # rows ascend inside every list
    assert all((np.diff(case.order[case.off[l]:case.off[l + 1]]) > 0).all() for l in range(C.NLIST))
    # exactly two empty lists, and why: the twin centroid loses every tie, nothing lies near the far one
    assert np.flatnonzero(sizes == 0).tolist() == [C.LIST_TWIN, C.LIST_FAR]
    assert np.array_equal(case.centroids[C.LIST_TWIN], case.centroids[C.LIST_TWIN_OF]) and sizes[C.LIST_TWIN_OF] > 0
    assert (case.centroids[C.LIST_FAR] == 1000).all()
    # a list longer than a scan chunk (and than four), a list shorter than k = 200
    assert sizes.max() > 4 * C.SCAN_CHUNK and sizes[sizes > 0].min() < 200
    # the copies of row 7 and the three special queries
    assert all(np.array_equal(case.x[r], case.x[7]) for r in range(100, 140))
    assert np.array_equal(case.pool[C.Q_ROW7], case.x[7]) and not case.pool[C.Q_ZERO].any()
    ids, dist = case.answer(C.Q_ROW7, 1)
    assert ids[:41].tolist() == [7] + list(range(100, 140)) and not dist[:41].any() and dist[41] > 0
    ids, dist = case.answer(C.Q_FAR, 1)
    assert ids.shape == (0,) and dist.shape == (0,)                      # its first list is the empty far one
    oi, od = case.expected(3, 1, 5)
    assert (oi[C.Q_FAR] == -1).all() and np.isposinf(od[C.Q_FAR]).all() and oi[C.Q_ROW7].tolist() == [7, 100, 101, 102, 103]
    # nprobe = 5 of the far query: the empty list first, then real ones
    assert C.probe(case.centroids, case.pool[C.Q_FAR], 5)[0] == C.LIST_FAR and case.answer(C.Q_FAR, 5)[0].shape[0] > 0


@pytest.mark.parametrize("d", C.DIMS)
def test_every_list_probed_is_the_dense_oracle(d):
    case = C.make_case(d)
    for qi in (C.Q_ROW7, C.Q_FAR, C.Q_ZERO, 5, 32):
        rd, ri = O.dense_topk(case.x, case.pool[qi], C.N)
        for nprobe in (C.NLIST, 100):                                    # 100 clamps to nlist
            ids, dist = case.answer(qi, nprobe)
            np.testing.assert_array_equal(ids, ri)
            np.testing.assert_array_equal(_bits(dist), _bits(rd))
        # the candidate sets are nested in nprobe, and a list's rows are exactly the rows assigned to it
        few = set(case.answer(qi, 5)[0].tolist())
        assert set(case.answer(qi, 1)[0].tolist()) <= few <= set(ri.tolist())
        lists = C.probe(case.centroids, case.pool[qi], 5)
        assert few == set(np.flatnonzero(np.isin(case.assignment, lists)).tolist())


def test_restatement_without_the_cache_and_padding():
    case = C.make_case(36)
    for qi, nprobe in ((4, 1), (C.Q_ROW7, 5)):
        ids, dist = C.search(case.x, case.centroids, case.off, case.order, case.pool[qi], nprobe)
        ci, cd = case.answer(qi, nprobe)
        np.testing.assert_array_equal(ids, ci)
        np.testing.assert_array_equal(_bits(dist), _bits(cd))
        # (distance, id) order, and every distance is the oracle's for its row
        assert ((dist[1:] > dist[:-1]) | ((dist[1:] == dist[:-1]) & (ids[1:] > ids[:-1]))).all()
        for j in (0, len(ids) // 2, len(ids) - 1):
            assert _bits(O.euclidean_distance(case.x[ids[j]], case.pool[qi]))[0] == _bits(dist)[j]
    oi, od = C.pad(np.array([4, 9], np.int64), np.array([0.5, 2.0], np.float32), 4, id_base=1000)
    assert oi.tolist() == [1004, 1009, -1, -1] and od[:2].tolist() == [0.5, 2.0] and np.isposinf(od[2:]).all()
