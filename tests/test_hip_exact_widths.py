"""
Every kernel that sums in numpy's order, at the row widths where its code takes another branch.

Float32 L2 distances are promised bit-identical to numpy's; that rests on the tree walk of
smqtk_indexing_amd/csrc/sq_pairwise.hpp (walked at every width on the CPU by tests/test_host_logic_pairwise.py) and
on the leaf code that five kernels put on top of it: dense_distances_kernel, rows_rerank_keys_kernel, SqLeafLane (the
one-query exact path), dense_exact_group_kernel (the group exact path, pw_tree_multi) and SqLeafPair (the survivor
re-rank behind every filter and in the tail of the fused int8 pass).  What those branch on is the width alone: the tail
n % 8, leaves shorter than 8, trees whose right spine is deeper than their left, ldq <= 156 (the re-rank's query tile in
LDS or not), the 64-float staging stride of the cosine re-rank, the 160 KiB of LDS that hold the group kernel's eight
queries (round_up(d, 4) <= 5112), the depth its walk is compiled for, and numpy's 8192-element buffers.

WIDTHS is derived from those rules in tests/width_cases.py, not typed in.  The reference everywhere is numpy and scipy on
the same inputs (oracle/cpu_ref.py: euclidean_distance, cosine_distance, dense_distances, dense_topk).  L2: distances
equal to the last bit, ids equal.  Cosine: rtol 1e-12, atol 1e-15, and where an id differs
O.assert_topk_equivalent(rtol=1e-12) decides.
"""
import numpy as np
import pytest

from oracle import cpu_ref as O
from smqtk_indexing_amd import _lib
from tests.width_cases import BEYOND, BUF, EXTREMES, GROUP_LDS_EDGE, N_INDEX, WIDTHS, _depth, _split

pytestmark = pytest.mark.gpu

METRICS = {"euclidean": _lib.SQ_METRIC_L2, "cosine": _lib.SQ_METRIC_COSINE}
K = 10
NOISE = np.float32(1e-3)


def test_width_list():
    assert EXTREMES == {1: (129, 256), 2: (249, 512), 3: (489, 1024), 4: (969, 2048), 5: (1929, 4096), 6: (3849, 8192), 7: (7689, 8191)}
    assert GROUP_LDS_EDGE == 5112 and {5109, 5112, 5113, 5116, 5117}.issubset(WIDTHS)
    assert _depth(255) == 2 and _split(255) == 120
    assert BEYOND == (8193, 8199, 8200, 16389) and max(WIDTHS) == BUF


def _assert_cosine_topk(dist, ids, rd, ri, what):
    np.testing.assert_allclose(dist, rd, rtol=1e-12, atol=1e-15, err_msg=what)
    if not np.array_equal(ids, ri):
        O.assert_topk_equivalent(rd, ri, dist, ids, rtol=1e-12)


def _assert_topk(metric, dist, ids, rd, ri, what):
    if metric == "euclidean":
        assert dist.dtype == np.float32
        np.testing.assert_array_equal(ids, ri, err_msg=what)
        np.testing.assert_array_equal(dist.view(np.uint32), rd.view(np.uint32), err_msg=what)
    else:
        assert dist.dtype == np.float64
        _assert_cosine_topk(dist, ids, rd, ri, what)


# ---------------------------------------------------------------------------------------------- 1. sq_dense_distances
@pytest.mark.parametrize("d", WIDTHS + list(BEYOND))
def test_dense_distances_at_width(d):
    rng = np.random.default_rng([1, d])
    for dt, n, view in ((np.float32, 257, np.uint32), (np.float64, 65, np.uint64)):
        rows = (rng.standard_normal((n, d)) * 3).astype(dt)
        queries = (rng.standard_normal(d).astype(dt), rows[n // 3] + (rng.standard_normal(d) * 1e-3).astype(dt))
        for qi, q in enumerate(queries):
            what = "%s query %d" % (np.dtype(dt).name, qi)
            got = _lib.dense_distances(q, rows, _lib.SQ_METRIC_L2)
            ref = O.euclidean_distance(rows, q)
            assert got.dtype == ref.dtype == dt
            np.testing.assert_array_equal(got.view(view), ref.view(view), err_msg=what)
            got = _lib.dense_distances(q, rows, _lib.SQ_METRIC_COSINE)
            assert got.dtype == np.float64
            np.testing.assert_allclose(got, O.dense_distances(rows, q, "cosine"), rtol=1e-12, atol=1e-15, err_msg=what)


# -------------------------------------------------------------------------------------------------- 2. sq_rows_rerank
@pytest.mark.parametrize("d", WIDTHS + list(BEYOND))
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_rows_rerank_at_width(dt, d):
    n = 300
    rng = np.random.default_rng([2, d])
    rows = (rng.standard_normal((n, d)) * 3).astype(dt)
    qs = rng.standard_normal((3, d)).astype(dt)
    qs[1] = rows[17] + (rng.standard_normal(d) * 1e-3).astype(dt)
    # candidate lists: all rows, a short one with a repeated row, an empty one
    lists = [rng.permutation(n).astype(np.int64), np.array([5, 17, 299, 5, 0], dtype=np.int64), np.zeros(0, dtype=np.int64)]
    cand = np.concatenate(lists)
    off = np.concatenate([[0], np.cumsum([len(c) for c in lists])]).astype(np.int64)
    m = _lib.RowMatrix(rows)
    try:
        for metric, code in METRICS.items():
            dist, pos = m.rerank(qs, code, cand, off, K)
            l2_f32 = metric == "euclidean" and dt == np.float32
            assert dist.dtype == (np.float32 if l2_f32 else np.float64) and dist.shape == pos.shape == (3, K)
            for qi, c in enumerate(lists):
                what = "%s, list %d" % (metric, qi)
                kk = min(K, len(c))
                assert (pos[qi, kk:] == -1).all() and np.isinf(dist[qi, kk:]).all(), what
                if kk == 0:
                    continue
                full = O.dense_distances(rows[c], qs[qi], metric)
                order = np.argsort(full, kind="stable")[:kk]          # the order of (distance, position in the list)
                gd, gp = dist[qi, :kk], pos[qi, :kk]
                if metric == "euclidean":
                    assert full.dtype == dist.dtype
                    np.testing.assert_array_equal(gp, order, err_msg=what)
                    np.testing.assert_array_equal(gd.view(np.uint8), full[order].view(np.uint8), err_msg=what)
                else:
                    _assert_cosine_topk(gd, gp, full[order], order, what)
                later = (gd[1:] > gd[:-1]) | ((gd[1:] == gd[:-1]) & (gp[1:] > gp[:-1]))
                assert later.all(), "%s: not in (distance, position) order: %s %s" % (what, gd, gp)
            # the repeated row: two positions of one distance, the earlier position first
            p = pos[1, :5].tolist()
            assert p.index(0) < p.index(3) and dist[1, p.index(0)] == dist[1, p.index(3)], metric
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ the dense index
_index_data = {}


def _index_case(case, d, nq):
    """(db, queries, {metric: oracle answers per query}) of one width, computed once for both metrics of a case.
    Rows N(0, 1) * 3 with a tie pair (rows 20 and 700); query 0 is that row, odd queries are random, the other even ones
    stored rows plus noise (`case` 4: every query but 0 a stored row plus noise, as the scan tests have them)."""
    key = (case, d)
    if key not in _index_data:
        _index_data.clear()                                  # (one width at a time: 69 MB at 16389 dimensions)
        rng = np.random.default_rng([case, d])
        db = (rng.standard_normal((N_INDEX, d)) * 3).astype(np.float32)
        db[700] = db[20]
        qs = (rng.standard_normal((nq, d)) * 3).astype(np.float32)
        for qi in range(nq):
            if case == 4 or qi % 2 == 0:
                qs[qi] = db[(qi * 131 + 7) % N_INDEX] + NOISE * rng.standard_normal(d).astype(np.float32)
        qs[0] = db[20]
        _index_data[key] = (db, qs, {})
    db, qs, refs = _index_data[key]
    assert len(qs) == nq
    return db, qs, refs


def _refs(db, qs, refs, metric):
    if metric not in refs:
        refs[metric] = [O.dense_topk(db, q, K, metric) for q in qs]
    return refs[metric]


# ---- 3. the exact path, forced: dense_exact_group_kernel for groups of up to eight queries where it takes the width,
# dense_exact_l2_kernel (SqLeafLane) / dense_exact_cos_kernel one query per pass where it does not
@pytest.mark.parametrize("d", WIDTHS + [BUF + 8, 2 * BUF + 5])
@pytest.mark.parametrize("metric", list(METRICS))
def test_exact_path_at_width(metric, d):
    db, qs, refs = _index_case(3, d, 9)
    ref = _refs(db, qs, refs, metric)
    idx = _lib.DenseIndex(db, metric=METRICS[metric], options={"candidate_cap": N_INDEX - 1, "dense_int8": 0})
    try:
        idx.set_option("force_fallback", 1)
        idx.set_option("dense_mid_tier", 0)
        for nq in (1, 3, 9):                  # nine: a full group of eight and a group of one
            idx.set_option("dense_debug", 0)
            dist, ids = idx.search(qs[:nq], K)
            st = idx.stats()
            assert st["fallback_queries"] == nq, (nq, st)
            for qi in range(nq):
                _assert_topk(metric, dist[qi], ids[qi], ref[qi][0], ref[qi][1], "%d queries, query %d" % (nq, qi))
            idx.set_option("dense_debug", 256)            # one query per pass
            dist1, ids1 = idx.search(qs[:nq], K)
            assert idx.stats()["fallback_queries"] == nq
            np.testing.assert_array_equal(ids1, ids, err_msg="%d queries, one per pass" % nq)
            np.testing.assert_array_equal(dist1.view(np.uint8), dist.view(np.uint8), err_msg="%d queries, one per pass" % nq)
        # the tie pair comes back in row order (one-dimensional rows under cosine: two distances, all ties)
        if d > 1 or metric == "euclidean":
            assert ref[0][1][:2].tolist() == [20, 700]
            assert ids[0, :2].tolist() == [20, 700] and dist[0, 0] == dist[0, 1]
    finally:
        idx.close()


# ---- 4. the survivor re-rank behind the bfloat16 filters (SqLeafPair / cosine_dot_pair_f64): one query tile (queries in
# LDS up to ldq = 156) and two tiles (never in LDS)
_RERANK_WIDTHS = [w for w in WIDTHS if w <= 160] + sorted({w for pair in EXTREMES.values() for w in pair if w > 160})


@pytest.mark.parametrize("d", _RERANK_WIDTHS)
@pytest.mark.parametrize("metric", list(METRICS))
def test_bf16_filter_rerank_at_width(metric, d):
    db, qs, refs = _index_case(4, d, 33)
    ref = _refs(db, qs, refs, metric)
    idx = _lib.DenseIndex(db, metric=METRICS[metric], options={"candidate_cap": N_INDEX - 1, "dense_int8": 0})
    try:
        for nq in (5, 33):
            dist, ids = idx.search(qs[:nq], K)
            st = idx.stats()
            print(metric, d, nq, st)
            # the answer checked is the re-rank kernel's: no query went on to a later tier
            assert st["fallback_queries"] == 0 and st["mid_tier_queries"] == 0, (nq, st)
            assert st["scan_launches"] >= 1, st
            for qi in range(nq):
                _assert_topk(metric, dist[qi], ids[qi], ref[qi][0], ref[qi][1], "%d queries, query %d" % (nq, qi))
    finally:
        idx.close()


# ---- 5. the survivor re-rank in the tail of the fused int8 pass (the int8 copy needs 65536 rows or more)
@pytest.mark.parametrize("d", [7, 100, 127, 129, 153, 156, 157, 160, 255, 257, 500, 511, 512])
@pytest.mark.parametrize("metric", list(METRICS))
def test_int8_fused_tail_rerank_at_width(metric, d):
    n, nq = 65536 + 17, 17
    rng = np.random.default_rng([5, d, METRICS[metric]])
    db = (rng.standard_normal((n, d)) * 3).astype(np.float32)
    db[40000] = db[20]
    qs = (rng.standard_normal((nq, d)) * 3).astype(np.float32)
    for qi in range(0, nq, 2):
        qs[qi] = db[(qi * 4099 + 31) % n] + NOISE * rng.standard_normal(d).astype(np.float32)
    qs[0] = db[20]
    idx = _lib.DenseIndex(db, metric=METRICS[metric])
    try:
        assert idx.info()["int8_in_use"], "no int8 copy: the fused int8 pass is not reached"
        dist, ids = idx.search(qs, K)
        st = idx.stats()
        print(metric, d, st)
        assert st["fallback_queries"] == 0 and st["mid_tier_queries"] == 0, st
        for qi in range(nq):
            rd, ri = O.dense_topk(db, qs[qi], K, metric)
            _assert_topk(metric, dist[qi], ids[qi], rd, ri, "query %d" % qi)
    finally:
        idx.close()


# ---- 6. L2 rows wider than a workgroup's LDS holds (160 KiB: 40 960 floats): dense_exact_l2_pieces_kernel stages the
# query two of numpy's 8192-element buffers at a time; 40 960 is the widest row still staged whole
@pytest.mark.parametrize("d", [40960, 40961, 3 * 16384, 3 * 16384 + 5])
def test_l2_rows_wider_than_the_lds(d):
    n, nq = 300, 3
    rng = np.random.default_rng([6, d])
    db = rng.standard_normal((n, d), dtype=np.float32) * np.float32(3)
    db[200] = db[20]
    qs = rng.standard_normal((nq, d), dtype=np.float32) * np.float32(3)
    qs[0] = db[20]
    qs[2] = db[131] + NOISE * rng.standard_normal(d, dtype=np.float32)
    ref = [O.dense_topk(db, q, K) for q in qs]
    assert ref[0][1][:2].tolist() == [20, 200]
    # every row a candidate: exact keys for all rows of all queries in one launch
    idx = _lib.DenseIndex(db)
    try:
        dist, ids = idx.search(qs, K)
        for qi in range(nq):
            _assert_topk("euclidean", dist[qi], ids[qi], ref[qi][0], ref[qi][1], "all rows, query %d" % qi)
    finally:
        idx.close()
    # the exact path, forced: one query per pass
    idx = _lib.DenseIndex(db, options={"candidate_cap": n - 1, "dense_int8": 0})
    try:
        idx.set_option("force_fallback", 1)
        idx.set_option("dense_mid_tier", 0)
        dist, ids = idx.search(qs, K)
        assert idx.stats()["fallback_queries"] == nq
        for qi in range(nq):
            _assert_topk("euclidean", dist[qi], ids[qi], ref[qi][0], ref[qi][1], "exact path, query %d" % qi)
    finally:
        idx.close()
