"""
CPU tests of tests/pq_cases.py, the case builder and numpy restatement behind tests/test_hip_pq.py: every case the GPU
tests run is built here, so the conditions they lean on (the sum order that shows in the bits, the 41-way tie, the
duplicated codebook entry, two empty lists, a list longer than 1024 rows, a list shorter than k = 10) are proven without
a GPU, and the restatement is checked against its own definition on single rows.
"""
import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import pq_cases as C
from tests.ivf_cases import plan_constant, probe

ALL = [(d, m, C.KSUB) for d, m in C.SHAPES] + [(*C.KSUB_SHAPE, ksub) for ksub in C.KSUBS]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("d,m,ksub", ALL)
def test_builder_conditions_hold(d, m, ksub):
    case = C.make_case(d, m, ksub)                                      # asserts the conditions itself
    sizes = np.diff(case.off)
    assert case.x.shape == (C.N, d) and case.codebooks.shape == (m, ksub, d // m) and case.codes.shape == (C.N, m)
    assert case.codes.dtype == np.uint8 and int(case.codes.max()) < ksub and case.nlist <= plan_constant("kIvfMaxLists")
    assert case.off[0] == 0 and case.off[-1] == C.N and np.array_equal(np.sort(case.order), np.arange(C.N))
    assert np.flatnonzero(sizes == 0).tolist() == [C.LIST_TWIN, C.LIST_FAR]
    assert sizes[C.LIST_BIG] > 1024 and sizes[C.LIST_SMALL] == C.SMALL_ROWS < 10
    # the far query alone probes an empty list, the small list alone pads at k = 10
    assert case.answer(C.Q_FAR, 1)[0].shape == (0,)
    oi, od = case.expected([C.Q_SMALL], 1, 10)
    assert sorted(oi[0, :C.SMALL_ROWS].tolist()) == list(range(C.SMALL_AT, C.SMALL_AT + C.SMALL_ROWS))
    assert (oi[0, C.SMALL_ROWS:] == -1).all() and np.isposinf(od[0, C.SMALL_ROWS:]).all()
    # sum order: seen in the bits exactly when the pairwise order is another arithmetic
    assert (case.differ > 0) == (m >= 8)
    print("%s: a pairwise sum changes %d of 50 distances" % (case.what, case.differ))


def test_sum_orders_coincide_below_eight_entries_only():
    assert C.make_case(516, 4).differ == 0 and C.make_case(516, 4).dsub == 129
    for d, m in C.SHAPES[:4]:
        assert C.make_case(d, m).differ > 0, (d, m)


@pytest.mark.parametrize("d,m", [(32, 8), (12, 12)])
def test_restatement_is_its_definition_on_single_rows(d, m):
    case = C.make_case(d, m)
    dsub = d // m
    for qi in (C.Q_ROW7, 5):
        q = case.pool[qi]
        t = C.tables(case.codebooks, q)
        assert t.dtype == np.float32 and t.shape == (m, case.ksub)
        for j, c in ((0, 0), (m - 1, case.ksub - 1), (1, 7)):
            want = np.square(case.codebooks[j][c] - q[j * dsub:(j + 1) * dsub]).sum()
            assert _bits(t[j, c]) == _bits(want)
            assert _bits(np.sqrt(t[j, c])) == _bits(O.euclidean_distance(case.codebooks[j][c], q[j * dsub:(j + 1) * dsub]))
        for r in (7, 999, C.N - 1):
            acc = t[0, case.codes[r, 0]]
            for j in range(1, m):
                acc = np.float32(acc + t[j, case.codes[r, j]])
            assert _bits(np.sqrt(acc)) == _bits(case.dist_all(qi)[r])
        # (distance, id) order over exactly the rows of the probed lists
        ids, dist = case.answer(qi, 3)
        assert ((dist[1:] > dist[:-1]) | ((dist[1:] == dist[:-1]) & (ids[1:] > ids[:-1]))).all()
        lists = probe(case.centroids, q, 3)
        assert set(ids.tolist()) == set(np.flatnonzero(np.isin(case.assignment, lists)).tolist())
    assert case.answer(5, case.nlist)[0].shape[0] == C.N == case.answer(5, 100)[0].shape[0]


def test_the_duplicated_entry_goes_to_the_lower_one():
    case = C.make_case(*C.KSUB_SHAPE)
    assert np.array_equal(case.codebooks[C.DUP_J, C.DUP_HI], case.codebooks[C.DUP_J, C.DUP_LO]) and C.DUP_LO < C.DUP_HI
    col = case.codes[:, C.DUP_J]
    assert (col == C.DUP_LO).any() and not (col == C.DUP_HI).any()


def test_the_sliced_batch_takes_more_than_one_slice():
    """tests/test_hip_pq.py runs 70 queries with every list probed under a key budget of 1 MiB: pq_slice_queries'
    arithmetic (keys, selected keys and the tables per query) puts them into more than one slice."""
    d, m = C.KSUB_SHAPE
    per = (C.N + C.SLICE_K) * 8 + m * C.KSUB * 4
    assert 1 < (C.SLICE_BUDGET_MB << 20) // per < C.SLICE_NQ and C.SLICE_K <= plan_constant("kIvfSelectLdsKeys")
