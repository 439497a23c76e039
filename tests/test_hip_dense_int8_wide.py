"""
The int8 first-stage filter for rows of 513 to 8192 dimensions (option "dense_int8_wide", sq_dense_i8_wide.hpp;
DESIGN.md section 4.1d).

Every case creates its index with the option set, and compares ids and distance bits with `oracle.cpu_ref.dense_topk`
over all rows (float32 bits for L2; float64 within the suite's rtol 1e-12 for cosine, ids equal wherever the reference
distances are distinguishable).  All cases use n = 65536 + 37 rows -- the row floor of the copy is just met and the last
32-row tile is partial -- and k = 100.  The oracle costs ~0.2 s of numpy per query and 1000 dimensions here, so a batch
is compared with it on a spread of its queries and, every query of it, bit for bit with the bfloat16 chain of the same
index ("dense_int8" = 0 on the handle), which tests/test_hip_parity.py holds against the oracle.
"""
import functools

import numpy as np
import pytest

from oracle import cpu_ref as O
from smqtk_indexing_amd import _lib

pytestmark = pytest.mark.gpu

L2, COS = _lib.SQ_METRIC_L2, _lib.SQ_METRIC_COSINE
N, K = 65536 + 37, 100
N_PAD = -(-N // 32) * 32
OPTS = {"dense_int8_wide": 1}
SPREAD = (0, 3, 6, 17, 31)     # queries of a 32-query batch the oracle is asked about


def _name(metric):
    return "euclidean" if metric == L2 else "cosine"


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _row8(d):
    return -(-d // 128) * 128


def _first_stage_bytes(d):
    return N_PAD * (_row8(d) + 4)


def _bf16_bytes(d, metric, n_pad=N_PAD):
    return n_pad * (2 * _row8(d) + (0 if metric == COS else 4))


@functools.lru_cache(maxsize=None)
def _base():
    return np.random.default_rng(20261017).standard_normal((N, 2048), dtype=np.float32)


def _data(kind, d):
    x = np.ascontiguousarray(_base()[:, :d])
    if kind == "relu":
        np.maximum(x, np.float32(0), out=x)       # non-negative, ReLU-like
    elif kind == "offset":
        x += np.float32(8.0)                       # rows sharing an offset of 8 sigma
    return x


def _queries(db, nq, seed):
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, len(db), nq)
    return (db[rows] + np.float32(0.05) * rng.standard_normal((nq, db.shape[1]), dtype=np.float32)).astype(np.float32)


def _against_oracle(db, q, metric, dist, ids, k=K, rows=None):
    """dist / ids of one query against the oracle over `db` (ids mapped through `rows` when db is a subset)."""
    rd, ri = O.dense_topk(db, q, k, _name(metric))
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


def _same_bits(a, b):
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(_bits(a[0]), _bits(b[0]))


def _stage_accounting(st, d, n=N):
    """The int8 pass took the call: its bytes, plus one pass over the float32 rows per exact-path launch."""
    n_pad = -(-n // 32) * 32
    assert st["scan_launches"] >= 2
    assert st["bytes_scanned"] == n_pad * (_row8(d) + 4) + (st["scan_launches"] - 2) * n * d * 4, st


def _create(db, metric):
    idx = _lib.DenseIndex(db, metric=metric, options=OPTS)
    info = idx.info()
    assert info["int8_in_use"], "no int8 copy for rows of %d dimensions" % db.shape[1]
    assert info["int8_copy_bytes"] >= len(db) * _row8(db.shape[1])
    idx.set_option("dense_int8", 1)   # (never suspended: every call below is the int8 stage's)
    return idx


# ------------------------------------------------------------------------------------------- parity over widths
@pytest.mark.parametrize("kind,metric", [("gauss", L2), ("relu", L2), ("gauss", COS), ("relu", COS), ("offset", COS)])
@pytest.mark.parametrize("d", [520, 1000, 2048])
def test_parity_over_widths(d, metric, kind):
    db = _data(kind, d)
    qs = _queries(db, 32, 7 * d + metric)
    idx = _create(db, metric)
    got = {}
    for nq in (1, 7, 32):
        got[nq] = idx.search(qs[:nq], K)
        st = idx.stats()
        _stage_accounting(st, d)
        if kind == "gauss":
            assert st["fallback_queries"] == 0 and st["mid_tier_queries"] == 0, st
            assert st["bytes_scanned"] == _first_stage_bytes(d), st
        assert idx.info()["int8_in_use"]
    for qi in SPREAD:
        for nq in (1, 7, 32):
            if qi < nq:
                _against_oracle(db, qs[qi], metric, got[nq][0][qi], got[nq][1][qi])
    # every query of the batch: the same bits as the bfloat16 chain's, and as the smaller batches'
    idx.set_option("dense_int8", 0)
    ref = idx.search(qs, K)
    assert idx.stats()["bytes_scanned"] >= _bf16_bytes(d, metric)
    _same_bits(got[32], ref)
    for nq in (1, 7):
        _same_bits(got[nq], (ref[0][:nq], ref[1][:nq]))
    idx.close()


# ------------------------------------------------------------------------------------------- accumulator range
def test_accumulator_range_8192():
    """d = 8192, L2: rows and queries whose every element sits at the clamp with equal signs, and a second batch with
    alternating signs -- the largest sums the planes' accumulators can see (127 * 127 * 8192 per plane; the narrow
    kernel's joined 256 * sum + sum' is 64 times beyond an i32 there).

    The clamp is chosen from the data as a multiple of the element rms (1.75 rms is the narrowest candidate), so a matrix
    of +-A elements alone is quantised to +-73.  Here 21500 of the 65573 rows hold +-A and the rest are zero rows: the rms
    is 0.5726 A, the narrowest clamp 1.0021 A, and every element of the +-A rows becomes +-127 without being cut off
    (the column means are exactly zero: as many +A as -A rows of each kind).  Every query element is +-B: Q8 = -+127.
    The matrix (2.1 GB) is built on the device; it has five distinct rows, so the oracle's distance of every row is the
    oracle's distance of its kind's representative, evaluated once per kind and expanded -- the oracle over all rows."""
    import torch
    d, A = 8192, np.float32(0.75)
    dev = torch.device("cuda", 0)
    alt = np.where(np.arange(d) % 2 == 0, 1.0, -1.0).astype(np.float32)
    kinds = np.stack([np.zeros(d, np.float32), np.full(d, A), np.full(d, -A), A * alt, -A * alt])
    kind_of = np.zeros(N, dtype=np.int64)
    per = 21500 // 4
    marked = np.random.default_rng(8192).permutation(N)[:4 * per]
    for j in range(4):
        kind_of[marked[j * per:(j + 1) * per]] = 1 + j
    x = torch.from_numpy(kinds).to(dev)[torch.from_numpy(kind_of).to(dev)].contiguous()
    idx = _lib.DenseIndex(x.data_ptr(), n=N, d=d, metric=L2, device_ptr=True, keepalive=x, options=OPTS)
    assert idx.info()["int8_in_use"]
    idx.set_option("dense_int8", 1)
    same = np.stack([np.full(d, b, np.float32) for b in (0.5, 1.25, -0.5, -2.0)])
    for qs in (same, same * alt):
        dist, ids = idx.search(qs, K)
        st = idx.stats()
        assert st["fallback_queries"] == 0 and st["mid_tier_queries"] == 0, st    # zero uncertified queries
        assert st["bytes_scanned"] == _first_stage_bytes(d), st
        for qi, q in enumerate(qs):
            per_kind = O.dense_distances(kinds, q, "euclidean")
            full = per_kind[kind_of]
            order = np.argsort(full, kind="stable")[:K]
            np.testing.assert_array_equal(ids[qi], order)
            np.testing.assert_array_equal(_bits(dist[qi]), _bits(full[order]))
    idx.close()


# ------------------------------------------------------------------------------------------- always-candidate rows
@pytest.mark.parametrize("metric", [L2, COS])
def test_always_candidate_rows(metric):
    d = 520
    db = _data("gauss", d)
    wild = np.array([100, 101, 102, 40000, N - 1])
    db[wild, np.arange(5) * 97] = np.float32(1e4)       # one element 1e4 times the rms: far beyond any clamp
    db[200, 3] = np.inf
    db[201, 5] = np.nan
    if metric == COS:
        db[202] = 0.0
    qs = _queries(db, 7, 99)
    qs[0] = db[100] + np.float32(0.01)                   # its nearest neighbour is an always-candidate row
    qs[1] = db[N - 1]
    idx = _create(db, metric)
    dist, ids = idx.search(qs, K)
    _stage_accounting(idx.stats(), d)
    for qi in range(len(qs)):
        _against_oracle(db, qs[qi], metric, dist[qi], ids[qi])
    assert ids[0, 0] == 100 and ids[1, 0] == N - 1
    idx.close()


# ------------------------------------------------------------------------------------------- certificate hand-on
def test_certificate_hand_on():
    d = 1000
    db = _data("gauss", d)
    rng = np.random.default_rng(5)
    qs = (300.0 * rng.standard_normal((6, d))).astype(np.float32)   # 300 times longer than the rows
    qs[5] = db[4242]                                                 # a stored row
    idx = _create(db, L2)
    got = idx.search(qs, K)
    st = idx.stats()
    handed = st["mid_tier_queries"] + st["fallback_queries"]
    assert 0 <= handed <= len(qs)
    assert (st["scan_launches"] > 2) == (handed > 0)
    _stage_accounting(st, d)
    idx.set_option("force_fallback", 1)      # every query handed on to the exact path
    forced = idx.search(qs, K)
    st = idx.stats()
    assert st["mid_tier_queries"] + st["fallback_queries"] == len(qs)
    _stage_accounting(st, d)
    _same_bits(got, forced)
    for qi in (0, 5):
        _against_oracle(db, qs[qi], L2, got[0][qi], got[1][qi])
    assert got[1][5, 0] == 4242 and got[0][5, 0] == 0.0
    idx.close()


# ------------------------------------------------------------------------------------------- mutation
def test_mutation_append_remove_compact():
    d = 520
    db0 = _data("gauss", d)
    extra = np.random.default_rng(11).standard_normal((5000, d), dtype=np.float32)
    qs = _queries(db0, 7, 12)
    idx = _create(db0, L2)
    b0 = idx.info()["int8_copy_bytes"]
    idx.append(extra)
    db = np.concatenate([db0, extra])
    n1 = len(db)
    b1 = idx.info()["int8_copy_bytes"]
    assert b1 > b0 and idx.info()["int8_in_use"]
    got = idx.search(qs, K)
    _stage_accounting(idx.stats(), d, n1)
    for qi in (0, 6):
        _against_oracle(db, qs[qi], L2, got[0][qi], got[1][qi])
    gone = np.unique(np.concatenate([[got[1][0, 0]], np.random.default_rng(13).choice(n1, 3100, replace=False)]))[:3000]
    if got[1][0, 0] not in gone:
        gone[0] = got[1][0, 0]
    idx.remove(gone)
    live = np.ones(n1, dtype=bool)
    live[gone] = False
    rows = np.flatnonzero(live)
    dbl = np.ascontiguousarray(db[rows])
    got = idx.search(qs, K)
    _stage_accounting(idx.stats(), d, n1)
    assert live[got[1]].all(), "a removed row was returned"
    for qi in (0, 6):
        _against_oracle(dbl, qs[qi], L2, got[0][qi], got[1][qi], rows=rows)
    old_to_new = idx.compact()
    assert (old_to_new[gone] == -1).all()
    b2 = idx.info()["int8_copy_bytes"]
    assert 0 < b2 < b1 and idx.info()["int8_in_use"]
    idx.set_option("dense_int8", 1)
    after = idx.search(qs, K)
    _stage_accounting(idx.stats(), d, len(rows))
    fresh = _create(dbl, L2)
    assert fresh.info()["int8_copy_bytes"] == b2
    _same_bits(after, fresh.search(qs, K))
    np.testing.assert_array_equal(rows[after[1]], got[1])
    np.testing.assert_array_equal(_bits(after[0]), _bits(got[0]))
    for qi in (0, 6):
        _against_oracle(dbl, qs[qi], L2, after[0][qi], after[1][qi])
    fresh.close()
    idx.close()


# ------------------------------------------------------------------------------------------- switch
@pytest.mark.parametrize("metric", [L2, COS])
def test_switch(metric):
    d = 1000
    db = _data("gauss", d)
    qs = _queries(db, 96, 21)
    off = _lib.DenseIndex(db, metric=metric, options={"dense_int8_wide": 0})
    info = off.info()
    assert info["int8_copy_bytes"] == 0 and not info["int8_in_use"]
    def bf16_took_the_call(st):   # its pass, plus one pass over the float32 rows per exact-path launch
        assert st["bytes_scanned"] == _bf16_bytes(d, metric) + (st["scan_launches"] - 2) * N * d * 4, st

    ref32 = off.search(qs[:32], K)
    bf16_took_the_call(off.stats())
    ref96 = off.search(qs, K)
    st96 = off.stats()
    bf16_took_the_call(st96)
    off.close()
    idx = _create(db, metric)
    _same_bits(idx.search(qs[:32], K), ref32)
    _stage_accounting(idx.stats(), d)
    # beyond one query tile: the bfloat16 chain takes the call (four query tiles per wave: one pass over the copy),
    # exactly as on the index without the copy
    got96 = idx.search(qs, K)
    assert idx.stats()["bytes_scanned"] == st96["bytes_scanned"] and idx.stats()["scan_launches"] == st96["scan_launches"]
    _same_bits(got96, ref96)
    for qi in (0, 50, 95):
        _against_oracle(db, qs[qi], metric, got96[0][qi], got96[1][qi])
    idx.close()


# ------------------------------------------------------------------------------------------- pipelined calls
def test_pipelined_calls_equal_blocking_calls():
    import torch
    d = 520
    db = _data("gauss", d)
    idx = _create(db, L2)
    idx.set_option("dense_async_depth", 2)
    batches = [_queries(db, 32, 30 + j) for j in range(4)]
    want = [idx.search(q, K) for q in batches]
    _against_oracle(db, batches[0][0], L2, want[0][0][0], want[0][1][0])
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    qd = [torch.from_numpy(q).to(dev) for q in batches]
    od = [torch.empty((32, K), dtype=torch.float32, device=dev) for _ in range(2)]
    oi = [torch.empty((32, K), dtype=torch.int64, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    for j in range(4):
        idx.search_device_async(qd[j].data_ptr(), 32, K, od[j % 2].data_ptr(), oi[j % 2].data_ptr(), stream)
        if j >= 1:   # depth 2: the previous call is final now, and it was the int8 stage's
            assert idx.stats()["bytes_scanned"] == _first_stage_bytes(d)
            _same_bits((od[(j - 1) % 2].cpu().numpy(), oi[(j - 1) % 2].cpu().numpy()), want[j - 1])
    idx.sync()
    _same_bits((od[1].cpu().numpy(), oi[1].cpu().numpy()), want[3])
    idx.close()
