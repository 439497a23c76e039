"""
CPU tests of tests/pq_residual_cases.py, the case builders and numpy restatement behind tests/test_hip_pq_residual.py:
every case the GPU tests run is built here, so the conditions they lean on -- residual codes that differ from plain
codes outside the zero-centroid list, the wrong pair's tables changing an answer, the regrouped subtraction and the
pairwise sum showing in the bits, the 41-way tie, a result in every chunk of the long list, both scan regimes, ranges
that end inside a query, residual recall above plain recall -- are proven without a GPU, and the restatement is checked
against its own definition on single rows.
"""
import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import pq_cases as C
from tests import pq_residual_cases as R
from tests.ivf_cases import plan_constant, probe

M_LIST = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 33, 64)
DSUBS = (1, 4, 129, 8193, 16384)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("d,m", R.SHAPES)
def test_main_case_conditions_hold(d, m):
    case = R.make_case(d, m)                                            # asserts (a) .. (e) itself
    plain = C.make_case(d, m)
    assert all(np.array_equal(getattr(case, name), getattr(plain, name)) for name in ("x", "centroids", "pool", "off", "order"))
    assert case.codes.shape == (C.N, m) and case.codes.dtype == np.uint8 and int(case.codes.max()) < case.ksub
    assert case.wrong_pair is not None and case.wrong_pair[1] >= 2 and case.regrouped > 0 and (case.differ > 0) == (m >= 8)
    print("%s: wrong pair %s, regrouped subtraction changes %d of 50, pairwise sum %d of 50" % (case.what, case.wrong_pair, case.regrouped, case.differ))
    # the far query alone probes an empty list; the small list alone pads at k = 10
    assert case.answer(C.Q_FAR, 1)[0].shape == (0,)
    oi, od = case.expected([C.Q_SMALL], 1, 10)
    assert sorted(oi[0, :5].tolist()) == list(range(C.SMALL_AT, C.SMALL_AT + 5)) and (oi[0, 5:] == -1).all() and np.isposinf(od[0, 5:]).all()
    assert case.answer(5, 100)[0].shape[0] == C.N


@pytest.mark.parametrize("d,m", [(32, 8), (12, 12)])
def test_restatement_is_its_definition_on_single_rows(d, m):
    case = R.make_case(d, m)
    dsub = d // m
    for r in (0, 7, C.SMALL_AT, 1500, C.N - 1):
        l = int(O.dense_topk(case.centroids, case.x[r], 1)[1][0])
        assert l == case.assignment[r]
        res = case.x[r] - case.centroids[l]
        assert np.array_equal(_bits(res), _bits(case.res[r]))
        literal = [O.dense_topk(case.codebooks[j], res[j * dsub:(j + 1) * dsub], 1)[1][0] for j in range(m)]
        assert case.codes[r].tolist() == literal
    for qi in (C.Q_SMALL, 5):
        q = case.pool[qi]
        lists = probe(case.centroids, q, 3)
        cand, dist = case.candidates_of(q, 3)
        assert set(cand.tolist()) == set(np.flatnonzero(np.isin(case.assignment, lists)).tolist())
        for p in (0, cand.shape[0] // 2, cand.shape[0] - 1):
            r = int(cand[p])
            rq = q - case.centroids[case.assignment[r]]
            acc = None
            for j in range(m):
                t = np.square(case.codebooks[j][case.codes[r, j]] - rq[j * dsub:(j + 1) * dsub]).sum()
                acc = t if acc is None else np.float32(acc + t)
            assert _bits(np.sqrt(acc)) == _bits(dist[p])
        ids, dd = case.answer(qi, 3)
        assert ((dd[1:] > dd[:-1]) | ((dd[1:] == dd[:-1]) & (ids[1:] > ids[:-1]))).all()


def test_lds_shape_case_and_its_ranges():
    d, m, ksub = C.LDS_SHAPE
    case = R.make_case(d, m, ksub)
    assert m * ksub * 4 == 65536 and case.differ > 0
    # 3 queries x 8 lists under 1 MiB: two ranges, the second beginning inside query 1; 5 queries: three ranges
    maxc = max(case.count(qi, 8) for qi in range(R.RANGE_Q0, R.RANGE_Q0 + 5))
    assert R.RANGE_OTHER + 5 <= C.POOL and R.RANGE_Q0 + 5 <= R.RANGE_OTHER
    assert maxc == C.N
    for k in (10, 5000):
        slice_, ppl, launches = R.res_plan(3, 8, maxc, k, m, ksub, 1 << 20)
        assert slice_ == 3 and 8 < ppl < 24 and ppl % 8 and launches == 2
        assert R.range_starts(3, 8, ppl)[1][1] != 0                      # a range boundary inside a query
    for nq, k in ((3, 10), (3, 5000), (5, 10), (5, 5000)):              # ... at a list with rows, for a query that differs from the
        for ql, pos in R.range_starts(nq, 8, R.res_plan(nq, 8, maxc, k, m, ksub, 1 << 20)[1])[1:]:     # one the GPU test runs before
            assert case.rows_of(probe(case.centroids, case.pool[R.RANGE_Q0 + ql], 8)[pos]).shape[0] > 0
            assert not np.array_equal(case.pool[R.RANGE_Q0 + ql], case.pool[R.RANGE_OTHER + ql])
    slice_, ppl, launches = R.res_plan(5, 8, maxc, 10, m, ksub, 1 << 20)
    assert slice_ == 5 and launches == 3 and all(pos for _, pos in R.range_starts(5, 8, ppl)[1:])
    assert R.res_plan(3, 8, maxc, 10, m, ksub)[2] == 1


def test_plan_restated_by_hand():
    assert R.query_scratch_bytes(3001, 10) == 3011 * 8 and R.query_scratch_bytes(0, 10) == 16 and R.query_scratch_bytes(5, 10) == 80
    assert R.query_scratch_bytes(20000, 20000) == 40000 * 8 + 2 * 32768 * 8
    assert R.res_plan(3, 8, 3001, 10, 64, 256, 1 << 20) == (3, 14, 2)
    assert R.res_plan(70000, 1, 10, 1, 1, 1)[1:] == (65535, 2) and R.res_plan(5, 3, 0, 10, 8, 64)[2] == 0
    assert R.SELECT_LDS_KEYS == plan_constant("kIvfSelectLdsKeys") and R.SORT_CHUNK == plan_constant("kIvfSortChunk")
    assert C.SCAN_CHUNK == plan_constant("kIvfChunk")


@pytest.mark.parametrize("d,m", R.S_SHAPES)
def test_strided_case_conditions_hold(d, m):
    case = R.make_strided_case(d, m)                                    # asserts the conditions itself
    sizes = np.diff(case.off)
    assert sizes.tolist() == [R.S_LONG_ROWS, R.S_SMALL_ROWS, 0, R.S_N - R.S_LONG_ROWS - R.S_SMALL_ROWS]
    assert (-(-m // 4)) % 4 == (0 if (d, m) == R.S_SHAPES[0] else 2)     # 16-byte loads / dword loads
    for nq in R.S_NQS:
        plan = R.strided_plan(case, nq, R.S_CUS)
        R.assert_regime(plan, nq, case.what)
        print("%s nq=%d: %s" % (case.what, nq, plan))
    assert R.strided_plan(case, 600, R.S_CUS)["groups"] == 2 and R.strided_plan(case, 64, R.S_CUS)["groups"] == 3
    assert R.S_LONG_ROWS % C.SCAN_CHUNK                                  # the long list's last chunk is partial
    # the planted queries: an empty list and the 5-row list at the first probe position
    assert case.count(R.S_Q_EMPTY, 1) == 0 and case.count(R.S_Q_SMALL, 1) == R.S_SMALL_ROWS and case.count(R.S_Q_EMPTY, 3) > 0
    # residual codes are no plain codes here: the middle list lies at -20
    assert (case.codes[case.rows_of(R.S_MID)] != C.encode(case.codebooks, case.x[case.rows_of(R.S_MID)])).any()


@pytest.mark.parametrize("ksub", C.M_KSUBS)
@pytest.mark.parametrize("m", M_LIST)
def test_m_cases_recoded(m, ksub):
    case = R.from_plain(C.make_m_case(m, ksub))                          # asserts that some code differs from the plain one
    assert case.codes.shape == (C.M_N, m) and case.lists_after(C.M_SPLIT)[0][-1] == C.M_SPLIT


@pytest.mark.parametrize("dsub", DSUBS)
def test_dsub_cases_recoded(dsub):
    case = R.from_plain(C.make_dsub_case(dsub))
    assert case.m == 3 and case.d == 3 * dsub and case.count(0, C.D_NLIST) == C.D_N


def test_recall_case():
    case, plain, r_res, r_plain = R.make_recall_case()                  # asserts r_res >= 1.5 r_plain itself
    print("recall@10 against the exact answer: residual codes %.3f, plain codes %.3f" % (r_res, r_plain))
    assert (case.n, case.d, case.m, case.ksub, case.nlist) == (3000, 32, 8, 16, 8) and case.pool.shape == (32, 32)
    assert r_res >= 1.5 * r_plain and np.array_equal(case.off, plain.off)


def test_the_overflowing_query_ties_every_candidate_at_infinity():
    case = R.from_plain(C.make_m_case(5, 13))
    with np.errstate(over="ignore"):
        ids, dist = case.answer_of(R.huge_query(case.d), 3)
    assert np.isposinf(dist).all() and (np.diff(ids) > 0).all() and ids.shape[0] > 10
