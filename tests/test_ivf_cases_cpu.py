"""
CPU tests of tests/ivf_cases.py, the case builder and numpy restatement behind tests/test_hip_ivf.py: every case the GPU
tests run is built here, so the conditions they lean on (two empty lists, a list longer than a scan chunk, a list
shorter than k = 200, the 41-way tie at distance 0, the far query's empty first list) are proven without a GPU; and the
restatement with every list probed is the oracle's `dense_topk` over all rows, ids and float32 bits.

The same for the two later builders: the many-lists case (700 lists of fewer than 256 rows, four of them empty, three of
those planted at probe positions 63, 255 and 257 of one query) and the width case, whose point -- a sum in another order
than numpy's changes at least one compared distance -- is checked at every width of tests/width_cases.py.
"""
import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import ivf_cases as C
from tests import width_cases as W


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


# ------------------------------------------------------------------------------------ many short lists
def test_many_lists_builder_conditions_hold():
    case = C.make_many_lists_case()                                      # asserts the conditions itself
    sizes = np.diff(case.off)
    assert (case.n, case.d, case.nlist) == (6007, 20, 700) and case.nlist <= C.plan_constant("kIvfMaxLists")
    assert case.x.shape == (case.n, case.d) and case.centroids.shape == (case.nlist, case.d) and case.pool.shape == (33, case.d)
    assert case.off[0] == 0 and case.off[-1] == case.n and np.array_equal(np.sort(case.order), np.arange(case.n))
    assert all((np.diff(case.order[case.off[l]:case.off[l + 1]]) > 0).all() for l in range(case.nlist))
    # every full scan chunk crosses list boundaries; a list of one row; the four empty lists and why
    assert sizes.max() < C.SCAN_CHUNK and (sizes == 1).any()
    assert np.flatnonzero(sizes == 0).tolist() == [C.M_LIST_FAR, *C.M_TWINS]
    assert (case.centroids[C.M_LIST_FAR] == 1000).all()
    # the planted query: each twin equals a lower-numbered centroid, probes directly behind it, and holds no row; the
    # three sit in the first wave of the prefix kernel, in the rest of its first block of 256, and in its second block
    ranked = C.probe(case.centroids, case.pool[C.Q_PLANT], case.nlist)
    assert np.array_equal(np.sort(ranked), np.arange(case.nlist))
    assert [int(np.flatnonzero(ranked == t)[0]) for t in C.M_TWINS] == list(C.M_TWIN_AT) == [63, 255, 257]
    for twin, orig, at in zip(C.M_TWINS, case.twin_of, C.M_TWIN_AT):
        assert np.array_equal(case.centroids[twin], case.centroids[orig]) and orig < twin and ranked[at - 1] == orig
        assert sizes[twin] == 0 and sizes[orig] > 0
        # one more list probed (the twin): the same candidates
        assert np.array_equal(case.answer(C.Q_PLANT, at)[0], case.answer(C.Q_PLANT, at + 1)[0])
    # the copies of row 7, the far query, and candidate counts that grow with every block of the prefix kernel
    assert all(np.array_equal(case.x[r], case.x[7]) for r in range(100, 140))
    ids, dist = case.answer(C.Q_ROW7, 1)
    assert ids[:41].tolist() == [7] + list(range(100, 140)) and not dist[:41].any() and dist[41] > 0
    assert case.answer(C.Q_FAR, 1)[0].shape == (0,) and C.probe(case.centroids, case.pool[C.Q_FAR], 1)[0] == C.M_LIST_FAR
    counts = [case.answer(5, nprobe)[0].shape[0] for nprobe in (1, 64, 65, 256, 257, 513, 700, 1000)]
    assert counts == sorted(counts) and counts[1] < counts[3] < counts[5] < counts[6] == counts[7] == case.n
    assert case.answer(5, 700)[0].shape[0] < 7000                        # k = 7000 pads at every nprobe


def test_many_lists_every_list_probed_is_the_dense_oracle():
    case = C.make_many_lists_case()
    for qi in (C.Q_ROW7, C.Q_FAR, C.Q_ZERO, C.Q_PLANT, 32):
        rd, ri = O.dense_topk(case.x, case.pool[qi], case.n)
        for nprobe in (case.nlist, 1000):                                # 1000 clamps to nlist
            ids, dist = case.answer(qi, nprobe)
            np.testing.assert_array_equal(ids, ri)
            np.testing.assert_array_equal(_bits(dist), _bits(rd))
        # nested candidate sets, and a list's rows are exactly the rows assigned to it
        sets = [set(case.answer(qi, nprobe)[0].tolist()) for nprobe in (1, 63, 64, 65, 255, 256, 257, 511, 513, 700)]
        assert all(a <= b for a, b in zip(sets, sets[1:])) and sets[-1] == set(range(case.n))
        lists = C.probe(case.centroids, case.pool[qi], 257)
        assert sets[6] == set(np.flatnonzero(np.isin(case.assignment, lists)).tolist())


# ------------------------------------------------------------------------------------ every row width
@pytest.mark.parametrize("d", [7, 129, 8191])
def test_width_builder_conditions_hold(d):
    case = C.make_width_case(d)                                          # asserts the conditions itself
    sizes = np.diff(case.off)
    assert (case.n, case.nlist) == (W.N_INDEX, 8) == (1049, 8)
    assert case.x.shape == (1049, d) and case.centroids.shape == (8, d) and case.pool.shape == (5, d) and case.x.dtype == np.float32
    assert case.off[0] == 0 and case.off[-1] == case.n and np.array_equal(np.sort(case.order), np.arange(case.n))
    assert np.flatnonzero(sizes == 0).tolist() == [C.W_TWIN] and np.array_equal(case.centroids[C.W_TWIN], case.centroids[C.W_TWIN_OF])
    assert np.array_equal(case.x[C.W_ROW_COPY], case.x[C.W_ROW]) and np.array_equal(case.pool[0], case.x[C.W_ROW])
    for nprobe in (1, 3, 8):                                             # query 0 always probes the list of its own row
        ids, dist = case.answer(0, nprobe)
        assert ids[:2].tolist() == [C.W_ROW, C.W_ROW_COPY] and not dist[:2].any() and dist[2] > 0
    for qi in range(5):
        rd, ri = O.dense_topk(case.x, case.pool[qi], case.n)
        ids, dist = case.answer(qi, 8)
        np.testing.assert_array_equal(ids, ri)
        np.testing.assert_array_equal(_bits(dist), _bits(rd))
        few, some = (set(case.answer(qi, nprobe)[0].tolist()) for nprobe in (1, 3))
        assert few <= some <= set(ri.tolist())


def test_another_summation_order_is_seen_at_every_width():
    """What the width tests of the scan rest on: at every width of the list a left-to-right sum (from 8 elements on) and
    a sum of one eight-accumulator leaf (from 129 on) change at least one of the 50 distances compared; below those
    widths they are numpy's own arithmetic and change none."""
    for d in list(W.WIDTHS) + list(W.BEYOND) + list(C.DEVICE_ROW_DIMS):
        case = C.make_width_case(d)
        seq, leaf = C.orders_that_differ(case)
        assert (seq > 0) == (d >= 8) and (leaf > 0) == (d >= 129), (d, seq, leaf)


def test_the_large_batch_fits_one_slice_of_the_raised_budget():
    """tests/test_hip_ivf.py runs 70 000 queries over the d = 8 width case with a key budget of 1 GiB so that the budget
    alone would put them all into one scan launch: more work items along the grid's second axis than 65 535."""
    case = C.make_width_case(C.BATCH_D)
    q = C.batch_queries(case)
    assert q.shape == (C.BATCH_DISTINCT, case.d) and np.unique(q, axis=0).shape[0] == C.BATCH_DISTINCT
    maxc = max(C.search(case.x, case.centroids, case.off, case.order, qq, C.BATCH_NPROBE)[0].shape[0] for qq in q)
    per = (maxc + min(C.BATCH_K, maxc)) * 8                              # ivf_query_scratch_bytes below the sort
    assert maxc > 0 and C.BATCH_K <= C.plan_constant("kIvfSelectLdsKeys")
    assert (C.BATCH_BUDGET_MB << 20) // per > C.BATCH_NQ > 65_536 and C.BATCH_NQ % C.BATCH_DISTINCT == 0


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
