"""
CPU tests of tests/pq_cases.py, the case builder and numpy restatement behind tests/test_hip_pq.py: every case the GPU
tests run is built here, so the conditions they lean on (the sum order that shows in the bits, the 41-way tie, the
duplicated codebook entry, two empty lists, a list longer than 1024 rows, a list shorter than k = 10) are proven without
a GPU, and the restatement is checked against its own definition on single rows.  The same for the strided-scan, every-m,
sub-vector-width, LDS-limit and 700-list cases and the small ones beside them.
"""
import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import pq_cases as C
from tests.ivf_cases import M_TWIN_AT, Q_PLANT, plan_constant, probe
from tests.width_cases import WIDTHS

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


# ------------------------------------------------------------------------------------ the scan's stride loop
def test_scan_groups_restated():
    """The Python pq_scan_groups on the values tests/host/pq_plan_main.cpp CHECKs of the real one (the full comparison is
    tests/test_host_logic_pq.py's), and the two regimes by hand for 256 compute units."""
    assert (C.pq_scan_groups(0, 1, 256), C.pq_scan_groups(611, 1, 256), C.pq_scan_groups(611, 32, 256)) == (1, 512, 39)
    assert C.pq_scan_groups(4096, 70000, 256) == 256 and C.pq_scan_groups(12, 33, 256) == 12 and C.pq_scan_groups(12, 70, 256) == 8
    assert C.pq_scan_groups(47, 600, 256) == 3 and C.pq_scan_groups(47, 64, 256) == 8 and C.pq_scan_groups(47, 50, 256) == 11
    assert C.SCAN_CHUNK == plan_constant("kIvfChunk")


@pytest.mark.parametrize("d,m", C.S_SHAPES)
def test_strided_case_conditions_hold(d, m):
    case = C.make_strided_case(d, m)                                    # asserts the conditions itself
    assert case.x.shape == (C.S_N, d) and case.codebooks.shape == (m, C.S_KSUB, d // m) and case.pool.shape == (C.S_POOL, d)
    assert (-(-m // 4)) % 4 == (0 if (d, m) == C.S_SHAPES[0] else 2)     # 16-byte loads / dword loads
    for nprobe in C.S_NPROBES:
        assert C.chunks_without_a_result(case, nprobe, C.S_K) == []
        for nq in C.S_NQS:
            plan = C.strided_plan(case, nprobe, nq, C.S_CUS)
            C.assert_regime(plan, nq, case.what)
            print("%s nprobe=%d nq=%d: %d chunks, %d workgroups per query, candidates %d .. %d, return at entry: %s"
                  % (case.what, nprobe, nq, plan["chunks"], plan["groups"], min(plan["counts"]), max(plan["counts"]), plan["early"]))
    # every list probed: the partial last chunk is some workgroup's LATER trip in both regimes
    for nq in C.S_NQS:
        groups = C.strided_plan(case, 8, nq, C.S_CUS)["groups"]
        assert (C.S_N // C.SCAN_CHUNK) // groups >= 1 and C.S_N % C.SCAN_CHUNK
    # three lists probed, 64 queries: the planted query's last workgroups return at entry, the longest query's stride
    spread = C.strided_plan(case, 3, C.S_NQS[1], C.S_CUS)
    assert spread["early"][C.S_Q_SHORT] and case.shortest <= (spread["groups"] - 1) * C.SCAN_CHUNK < case.longest
    # the tiled batch: row i is pool query i % 50
    queries, qis = C.strided_queries(case, 64)
    assert queries.shape == (64, d) and qis[50] == 0 and np.array_equal(queries[63], case.pool[13])


# ------------------------------------------------------------------------------------ every m
@pytest.mark.parametrize("ksub", C.M_KSUBS)
@pytest.mark.parametrize("m", range(1, 65))
def test_m_case_conditions_hold(m, ksub):
    case = C.make_m_case(m, ksub)                                       # asserts the conditions itself
    assert case.x.shape == (C.M_N, 2 * m) and case.codes.shape == (C.M_N, m) and (case.differ > 0) == (m >= 8)
    off, ids, codes = C.lists_after(case, C.M_SPLIT)
    assert off[-1] == C.M_SPLIT == ids.shape[0] == codes.shape[0] and C.M_SPLIT % 2 == 1 and 0 < C.M_SPLIT < C.M_N


def test_m_cases_meet_both_staging_branches_at_padded_and_unpadded_strides():
    """Over m = 1 .. 64 at ksub 13 and 16: the tables are staged 16 bytes at a time (m * ksub % 4 == 0) and one float at
    a time, by the dword and by the 16-byte code loads; the 16-byte staging meets strides with and without padding bytes
    (an unpadded stride, m % 4 == 0, never leaves a table count that is no multiple of 4)."""
    seen = {((m * ksub) % 4 == 0, m % 4 == 0, (-(-m // 4)) % 4 == 0) for m in range(1, 65) for ksub in C.M_KSUBS}
    assert len(seen) == 6 and not any(not vec and unpadded for vec, unpadded, _ in seen)
    assert {-(-m // 4) for m in range(1, 65)} >= {5, 8, 9, 12}            # code strides in dwords the issue names


@pytest.mark.parametrize("m,ksub,dsub", [(*mk, 2) for mk in C.M_EXTRA] + [C.M_DEVICE])
def test_further_m_case_conditions_hold(m, ksub, dsub):
    case = C.make_m_case(m, ksub, dsub)
    if ksub == 1:
        ids, dist = case.answer(1, 3)
        assert not case.codes.any() and (dist == dist[0]).all() and (np.diff(ids) > 0).all()
    if (m, ksub) == (5, 255):
        assert (m * ksub) % 4 and m * ksub > 4 * 256                     # scalar staging, five passes of 256 lanes
    if dsub == 35:
        assert case.d == 35 and m == 1                                    # pq_add_part hands the rows to the codebook index as they are


# ------------------------------------------------------------------------------------ every sub-vector width
@pytest.mark.parametrize("dsub", list(WIDTHS) + list(C.D_BEYOND))
def test_dsub_case_conditions_hold(dsub):
    case = C.make_dsub_case(dsub)                                       # asserts the conditions itself
    assert case.m == 3 and case.d == 3 * dsub and case.codes.shape == (C.D_N, 3)
    assert case.seq > 0 or dsub < 8
    assert case.leaf > 0 or dsub < 129
    assert case.answer(0, C.D_NLIST)[0].shape[0] == C.D_N


def test_dsub_widths():
    assert len(WIDTHS) == 58 and C.D_BEYOND == (8193, 8199, 8200, 16384) and len(set(WIDTHS) | set(C.D_BEYOND)) == 62


# ------------------------------------------------------------------------------------ the LDS limit, 700 lists, small things
def test_lds_limit_case_conditions_hold():
    d, m, ksub = C.LDS_SHAPE
    case = C.make_case(d, m, ksub)                                      # the module's conditions hold at this shape too
    assert m * ksub * 4 == 65536 and case.differ > 0 and int(case.codes.max()) == 255


def test_many_lists_case_conditions_hold():
    case = C.make_many_lists_case()
    assert (case.nlist, case.d, case.m, case.ksub, case.dsub) == (700, 20, C.ML_M, C.ML_KSUB, 4)
    assert C.ML_ADDS[0][0] == 0 and all(a[1] == b[0] for a, b in zip(C.ML_ADDS, C.ML_ADDS[1:])) and C.ML_ADDS[-1][1] == case.n
    for _, hi in C.ML_ADDS:
        off, ids, codes = C.lists_after(case, hi)
        assert off[-1] == hi and np.array_equal(np.sort(ids), np.arange(hi)) and codes.shape == (hi, C.ML_M)
    assert np.array_equal(C.lists_after(case, case.n)[1], case.order)
    # the planted query's empty lists at probe positions 63, 255, 257
    ranked = probe(case.centroids, case.pool[Q_PLANT], 700)
    assert [int(np.diff(case.off)[ranked[at]]) for at in M_TWIN_AT] == [0, 0, 0]
    assert case.answer(Q_PLANT, 64)[0].shape == case.answer(Q_PLANT, 63)[0].shape


def test_the_overflowing_query_ties_every_candidate_at_infinity():
    case = C.make_m_case(5, 13)
    q = C.huge_query(case.d)
    with np.errstate(over="ignore"):
        assert np.isposinf(C.tables(case.codebooks, q)).all()
        for nprobe in (3, 8):
            ids, dist = C.answer_of(case, q, nprobe)
            assert np.isposinf(dist).all() and (np.diff(ids) > 0).all() and ids.shape[0] > 10
    oi, od = C.pad(ids, dist, case.n + 3)
    assert oi[:case.n].tolist() == list(range(case.n)) and (oi[case.n:] == -1).all() and np.isposinf(od).all()


def test_answer_of_is_the_cached_answer():
    case = C.make_m_case(5, 13)
    for nprobe in (1, 8):
        ids, dist = C.answer_of(case, case.pool[1], nprobe)
        want_ids, want_dist = case.answer(1, nprobe)
        assert np.array_equal(ids, want_ids) and np.array_equal(_bits(dist), _bits(want_dist))
    assert C.ID_BASE == 2 ** 40 + 5


def test_the_plugin_plan_for_40_descriptors():
    from smqtk_indexing_amd.impls.nn_index.hip_ivf_pq import HipIvfPqNearestNeighborsIndex
    sample, init, entries = HipIvfPqNearestNeighborsIndex(nlist=8, nprobe=8, m=4).training_plan(40)
    assert len(sample) == 40 and entries.shape == (40,) and np.unique(entries).shape == (40,) and init.shape == (8,)


def test_the_sliced_batch_takes_more_than_one_slice():
    """tests/test_hip_pq.py runs 70 queries with every list probed under a key budget of 1 MiB: pq_slice_queries'
    arithmetic (keys, selected keys and the tables per query) puts them into more than one slice."""
    d, m = C.KSUB_SHAPE
    per = (C.N + C.SLICE_K) * 8 + m * C.KSUB * 4
    assert 1 < (C.SLICE_BUDGET_MB << 20) // per < C.SLICE_NQ and C.SLICE_K <= plan_constant("kIvfSelectLdsKeys")
