"""
Option "dense_bf16" (DESIGN.md section 4.8): a dense index that builds its bfloat16 scan copy when a search first
streams it (-1), or never (0), next to the default that builds it at create (1).

Shapes: 70 001 rows -- just over the 65 536-row floor of the int8 copy and over the candidate cap, the last 32-row tile
partial -- of 128 and of 100 dimensions (a partial 64-column unit), k = 10.  A call of 4 queries is the int8 stage's, one
of 65 queries the bfloat16 chain's (128-byte int8 rows take up to 64 queries; 256-byte rows up to 32, hence 33 queries
at d = 256).  Every result is compared bit for bit -- ids and distances -- with an index created with default options
from the same rows and given the same appends / removals, and eight of its queries with `oracle.cpu_ref.dense_topk` over
all rows (float32 bits for L2; float64 within the suite's rtol 1e-12 for cosine, ids equal wherever the reference
distances are distinguishable).
"""
import functools

import numpy as np
import pytest

from oracle import cpu_ref as O
from smqtk_indexing_amd import _lib

pytestmark = pytest.mark.gpu

L2, COS = _lib.SQ_METRIC_L2, _lib.SQ_METRIC_COSINE
N, K = 70001, 10
SMALL, BIG = 4, 65
ORACLE_Q = (0, 1, 2, 3, 20, 33, 50, 64)    # queries the oracle is asked about (the first four are the 4-query call)
ON_DEMAND, NEVER = {"dense_bf16": -1}, {"dense_bf16": 0}


def _nbig(d):
    return 33 if d == 256 else BIG      # the smallest batch the int8 stage does not take


def _name(metric):
    return "euclidean" if metric == L2 else "cosine"


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@functools.lru_cache(maxsize=None)
def _base():
    return np.random.default_rng(20261019).standard_normal((N, 516), dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _db(d):
    x = np.ascontiguousarray(_base()[:, :d])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _queries(d, nq=BIG, seed=1):
    db = _db(d)
    rng = np.random.default_rng(1000 * d + seed)
    rows = rng.integers(0, len(db), nq)
    q = (db[rows] + np.float32(0.05) * rng.standard_normal((nq, d), dtype=np.float32)).astype(np.float32)
    q.setflags(write=False)
    return q


def _against_oracle(db, q, metric, dist, ids, rows=None):
    """dist / ids of one query against the oracle over `db` (ids mapped through `rows` when db is a subset)."""
    rd, ri = O.dense_topk(db, q, K, _name(metric))
    want = ri if rows is None else rows[ri]
    if metric == L2:
        np.testing.assert_array_equal(ids, want)
        np.testing.assert_array_equal(_bits(dist), _bits(rd))
        return
    np.testing.assert_allclose(dist, rd, rtol=1e-12, atol=1e-15, equal_nan=True)
    mism = ids != want
    if mism.any():   # rows the reference itself cannot tell apart
        full = O.dense_distances(db, q, "cosine")
        back = ids[mism] if rows is None else np.searchsorted(rows, ids[mism])
        a, b = full[back], full[ri[mism]]
        assert (np.isnan(a) == np.isnan(b)).all() and np.nanmax(np.abs(a - b), initial=0.0) < 1e-14


def _same_bits(a, b, rows=None):
    """Results a == results b, ids and distance bits (`rows`: b is of an index over that subset of a's rows)."""
    np.testing.assert_array_equal(a[1], b[1] if rows is None else rows[b[1]])
    np.testing.assert_array_equal(_bits(a[0]), _bits(b[0]))


def _check(got, ref, db, qs, metric, rows=None):
    """`got` (of the index under test) against `ref` (the default index's, over db) and against the oracle."""
    _same_bits(got, ref, rows)
    for qi in ORACLE_Q:
        if qi < len(qs):
            _against_oracle(db, qs[qi], metric, got[0][qi], got[1][qi], rows)


@functools.lru_cache(maxsize=None)
def _reference(d, metric):
    """What an index with default options answers, and what it keeps: shared by the tests, left unchanged."""
    nbig = _nbig(d)
    idx = _lib.DenseIndex(_db(d), metric=metric)
    info = idx.info()
    qs = _queries(d)
    small = idx.search(qs[:SMALL], K)
    big = idx.search(qs[:nbig], K)
    st = idx.stats()
    idx.close()
    return {"info": info, "small": small, "big": big, "stats_big": st}


def _bf16(idx):
    return idx.info()["bf16_copy_bytes"]


# ------------------------------------------------------------------------------------------- 1: on demand
@pytest.mark.parametrize("metric,d", [(L2, 128), (COS, 128), (L2, 100), (COS, 100), (L2, 256)])
def test_on_demand(metric, d):
    nbig = _nbig(d)
    db, qs, ref = _db(d), _queries(d), _reference(d, metric)
    idx = _lib.DenseIndex(db, metric=metric, options=ON_DEMAND)
    info = idx.info()
    assert info["bf16_copy_bytes"] == 0 and info["int8_copy_bytes"] > 0 and info["int8_in_use"], info
    assert info["int8_copy_bytes"] == ref["info"]["int8_copy_bytes"] and info["row_stats_bytes"] == ref["info"]["row_stats_bytes"]
    small = idx.search(qs[:SMALL], K)
    _check(small, ref["small"], db, qs[:SMALL], metric)
    assert _bf16(idx) == 0, "a call of the int8 stage built the bfloat16 copy"
    big = idx.search(qs[:nbig], K)
    st = idx.stats()
    print("on demand, metric %d d %d: candidates %d (default index %d), fallback %d, mid tier %d" %
          (metric, d, st["candidates"], ref["stats_big"]["candidates"], st["fallback_queries"], st["mid_tier_queries"]))
    _check(big, ref["big"], db, qs[:nbig], metric)
    assert _bf16(idx) == ref["info"]["bf16_copy_bytes"] > 0
    assert st["fallback_queries"] == 0, st
    assert st["candidates"] == ref["stats_big"]["candidates"], (st, ref["stats_big"])
    assert st["bytes_scanned"] == ref["stats_big"]["bytes_scanned"] and st["scan_launches"] == ref["stats_big"]["scan_launches"]
    _same_bits(idx.search(qs[:SMALL], K), small)
    assert idx.info()["int8_in_use"]
    idx.close()


# ------------------------------------------------------------------------------------------- 2: removal
@pytest.mark.parametrize("metric", [COS, L2])
def test_removal_before_the_copy_exists(metric):
    d = 128
    db, qs, ref = _db(d), _queries(d), _reference(d, metric)
    idx = _lib.DenseIndex(db, metric=metric, options=ON_DEMAND)
    live = np.ones(N, dtype=bool)
    rng = np.random.default_rng(2)

    def remove(neighbours, seed_rows):
        gone = np.unique(np.concatenate([neighbours, seed_rows]))
        gone = gone[live[gone]]
        keep = np.isin(gone, neighbours)
        gone = np.concatenate([gone[keep], gone[~keep]])[:300]   # 300 rows, every listed neighbour among them
        assert len(gone) == 300 and np.isin(neighbours, gone).all()
        idx.remove(gone)
        live[gone] = False

    def compare():
        rows = np.flatnonzero(live)
        dbl = np.ascontiguousarray(db[rows])
        fresh = _lib.DenseIndex(dbl, metric=metric)
        got = idx.search(qs, K)
        assert live[got[1]].all(), "a removed row was returned"
        _check(got, fresh.search(qs, K), dbl, qs, metric, rows)
        fresh.close()
        return got

    # the nearest three rows of every query the oracle is asked about, and of ten more
    remove(ref["big"][1][list(ORACLE_Q) + list(range(40, 50)), :3].reshape(-1), rng.choice(N, 400, replace=False))
    assert _bf16(idx) == 0
    first = compare()
    assert _bf16(idx) == ref["info"]["bf16_copy_bytes"]
    assert not np.array_equal(first[1], ref["big"][1])
    # ... and once more with the copy in place: the new first neighbours leave
    remove(first[1][:, :2].reshape(-1), rng.choice(N, 400, replace=False))
    compare()
    idx.close()


# ------------------------------------------------------------------------------------------- 3: append
@pytest.mark.parametrize("metric", [L2, COS])
def test_append_before_and_after_the_copy_exists(metric):
    d = 100
    db0, qs0 = _db(d), _queries(d)
    rng = np.random.default_rng(3)
    extra1 = rng.standard_normal((1003, d), dtype=np.float32)    # neither count is a multiple of 32, nor is 70 001:
    extra2 = rng.standard_normal((517, d), dtype=np.float32)     # each append rebuilds the tile the old rows ended in
    qs = np.array(qs0)
    qs[:3] = extra1[[0, 500, 1002]] + np.float32(0.01)           # neighbours among the appended rows
    qs[60:63] = extra2[[0, 100, 516]] + np.float32(0.01)
    idx = _lib.DenseIndex(db0, metric=metric, options=ON_DEMAND)
    default = _lib.DenseIndex(db0, metric=metric)
    for a in (idx, default):
        a.append(extra1)
    db1 = np.concatenate([db0, extra1])
    assert _bf16(idx) == 0 and idx.info()["int8_in_use"]
    got = idx.search(qs, K)
    _check(got, default.search(qs, K), db1, qs, metric)
    assert list(got[1][:3, 0]) == [N, N + 500, N + 1002]
    assert _bf16(idx) >= len(db1) * 128 * 2
    for a in (idx, default):
        a.append(extra2)
    db2 = np.concatenate([db1, extra2])
    assert _bf16(idx) >= len(db2) * 128 * 2
    got = idx.search(qs, K)
    _check(got, default.search(qs, K), db2, qs, metric)
    assert list(got[1][60:63, 0]) == [len(db1), len(db1) + 100, len(db1) + 516]
    _same_bits(idx.search(qs[:SMALL], K), (got[0][:SMALL], got[1][:SMALL]))
    for a in (idx, default):
        a.close()


# ------------------------------------------------------------------------------------------- 4: compact
def test_compact_sheds_the_copy():
    d, metric = 128, L2
    db, qs, ref = _db(d), _queries(d), _reference(d, metric)
    idx = _lib.DenseIndex(db, metric=metric, options=ON_DEMAND)
    _same_bits(idx.search(qs, K), ref["big"])
    assert _bf16(idx) == ref["info"]["bf16_copy_bytes"]
    gone = np.unique(np.concatenate([ref["big"][1][:, 0], np.random.default_rng(4).choice(N, 3000, replace=False)]))
    idx.remove(gone)
    old_to_new = idx.compact()
    assert (old_to_new[gone] == -1).all()
    assert _bf16(idx) == 0, "sq_dense_compact kept the copy of an on-demand index"
    rows = np.flatnonzero(old_to_new >= 0)
    dbl = np.ascontiguousarray(db[rows])
    fresh = _lib.DenseIndex(dbl, metric=metric)
    small = idx.search(qs[:SMALL], K)
    _same_bits(small, fresh.search(qs[:SMALL], K))
    assert _bf16(idx) == 0
    got = idx.search(qs, K)
    _check(got, fresh.search(qs, K), dbl, qs, metric)
    assert _bf16(idx) == fresh.info()["bf16_copy_bytes"] > 0
    fresh.close()
    idx.close()


# ------------------------------------------------------------------------------------------- 5: never
@pytest.mark.parametrize("metric", [L2, COS])
def test_never(metric):
    d = 128
    db, qs, ref = _db(d), _queries(d), _reference(d, metric)
    idx = _lib.DenseIndex(db, metric=metric, options=NEVER)
    assert _bf16(idx) == 0
    got = idx.search(qs, K)
    st = idx.stats()
    _check(got, ref["big"], db, qs, metric)
    assert _bf16(idx) == 0
    assert st["mid_tier_queries"] + st["fallback_queries"] == BIG, st
    small = idx.search(qs[:SMALL], K)
    st = idx.stats()
    _check(small, ref["small"], db, qs[:SMALL], metric)
    assert idx.info()["int8_in_use"] and st["fallback_queries"] == 0 and st["bytes_scanned"] == (-(-N // 64) * 64) * 132, st
    assert _bf16(idx) == 0
    idx.close()


def test_zero_on_a_handle_leaves_the_copy_alone():
    d, metric = 128, L2
    db, qs, ref = _db(d), _queries(d), _reference(d, metric)
    idx = _lib.DenseIndex(db, metric=metric)
    idx.set_option("dense_bf16", 0)
    got = idx.search(qs, K)
    st = idx.stats()
    assert st["mid_tier_queries"] + st["fallback_queries"] == BIG, st
    _same_bits(got, ref["big"])
    assert _bf16(idx) == ref["info"]["bf16_copy_bytes"]     # not used, not freed
    idx.set_option("dense_bf16", 1)
    _same_bits(idx.search(qs, K), ref["big"])
    assert idx.stats()["bytes_scanned"] == ref["stats_big"]["bytes_scanned"]
    idx.close()


# ------------------------------------------------------------------------------------------- 6: pipelined
def test_pipelined_call_builds_the_copy():
    import torch
    d, metric = 128, L2
    db, qs, ref = _db(d), _queries(d), _reference(d, metric)
    idx = _lib.DenseIndex(db, metric=metric, options=ON_DEMAND)
    idx.set_option("dense_async_depth", 2)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    other = _queries(d, SMALL, seed=6)
    want_other = idx.search(other, K)
    for qi in range(SMALL):
        _against_oracle(db, other[qi], metric, want_other[0][qi], want_other[1][qi])
    calls = [(torch.from_numpy(np.array(qs[:SMALL])).to(dev), SMALL), (torch.from_numpy(np.array(other)).to(dev), SMALL),
             (torch.from_numpy(np.array(qs)).to(dev), BIG)]
    od = [torch.empty((nq, K), dtype=torch.float32, device=dev) for _, nq in calls]
    oi = [torch.empty((nq, K), dtype=torch.int64, device=dev) for _, nq in calls]
    torch.cuda.synchronize()
    assert _bf16(idx) == 0
    for j, (q, nq) in enumerate(calls):   # two int8 calls in flight, then the call that builds the copy
        idx.search_device_async(q.data_ptr(), nq, K, od[j].data_ptr(), oi[j].data_ptr(), stream)
    assert _bf16(idx) == ref["info"]["bf16_copy_bytes"]
    idx.sync()
    out = [(od[j].cpu().numpy(), oi[j].cpu().numpy()) for j in range(3)]
    _check(out[0], ref["small"], db, qs[:SMALL], metric)
    _same_bits(out[1], want_other)
    _check(out[2], ref["big"], db, qs, metric)
    idx.close()


# ------------------------------------------------------------------------------------------- 7: no int8 copy
@pytest.mark.parametrize("metric", [L2, COS])
def test_without_an_int8_copy(metric):
    n, d = 12000, 128
    db = np.ascontiguousarray(_db(d)[:n])
    rng = np.random.default_rng(7)
    qs = (db[rng.integers(0, n, 8)] + np.float32(0.05) * rng.standard_normal((8, d), dtype=np.float32)).astype(np.float32)
    cap = {"candidate_cap": 2048}     # (12 000 rows are beyond it: the filter path, and below the int8 copy's floor)
    default = _lib.DenseIndex(db, metric=metric, options=cap)
    want = default.search(qs, K)
    assert default.info()["int8_copy_bytes"] == 0 and default.info()["bf16_copy_bytes"] > 0
    assert default.stats()["scan_launches"] >= 2 and default.stats()["bytes_scanned"] >= n * d * 2
    idx = _lib.DenseIndex(db, metric=metric, options=dict(cap, **ON_DEMAND))
    assert _bf16(idx) == 0 and idx.info()["int8_copy_bytes"] == 0
    got = idx.search(qs[:SMALL], K)
    assert _bf16(idx) == default.info()["bf16_copy_bytes"], "the first filtered search of an index without an int8 copy builds it"
    _same_bits(got, (want[0][:SMALL], want[1][:SMALL]))
    got = idx.search(qs, K)
    assert idx.stats()["candidates"] == default.stats()["candidates"]
    for qi in range(len(qs)):
        _against_oracle(db, qs[qi], metric, got[0][qi], got[1][qi])
    _same_bits(got, want)
    idx.close()
    idx = _lib.DenseIndex(db, metric=metric, options=dict(cap, **NEVER))
    got = idx.search(qs, K)
    st = idx.stats()
    assert st["mid_tier_queries"] + st["fallback_queries"] == len(qs) and _bf16(idx) == 0, st
    _same_bits(got, want)
    idx.close()
    default.close()


def test_an_index_under_the_candidate_cap_never_builds_it():
    d = 128
    db = np.ascontiguousarray(_db(d)[:12000])
    qs = _queries(d)
    idx = _lib.DenseIndex(db, options=ON_DEMAND)
    got = idx.search(qs, K)
    assert _bf16(idx) == 0
    for qi in (0, 64):
        _against_oracle(db, qs[qi], L2, got[0][qi], got[1][qi])
    idx.close()


# ------------------------------------------------------------------------------------------- 8: wide rows
def test_wide_rows():
    d, metric = 516, L2
    db, qs = _db(d), _queries(d, 33)
    default = _lib.DenseIndex(db, metric=metric)
    want = default.search(qs, K)
    idx = _lib.DenseIndex(db, metric=metric, options=dict(ON_DEMAND, dense_int8_wide=1))
    info = idx.info()
    assert info["bf16_copy_bytes"] == 0 and info["int8_in_use"], info
    small = idx.search(qs[:SMALL], K)
    assert idx.stats()["bytes_scanned"] >= (-(-N // 32) * 32) * (640 + 4)
    assert _bf16(idx) == 0
    _same_bits(small, (want[0][:SMALL], want[1][:SMALL]))
    got = idx.search(qs, K)
    assert _bf16(idx) == default.info()["bf16_copy_bytes"] > 0
    assert idx.stats()["bytes_scanned"] == default.stats()["bytes_scanned"]
    _check(got, want, db, qs, metric)
    idx.close()
    default.close()


# ------------------------------------------------------------------------------------------- 9: default
def test_default_builds_the_copy_at_create():
    idx = _lib.DenseIndex(_db(128))
    info = idx.info()
    assert info["bf16_copy_bytes"] >= (-(-N // 32) * 32) * 128 * 2 and info["int8_copy_bytes"] > 0
    idx.close()
