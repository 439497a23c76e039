"""
sq_dense_remove / sq_dense_compact / sq_dense_count on the device.

The contract: a search over an index with removed rows returns what a search over an index created from the
remaining rows returns, with the original ids.  Every case is compared with the oracle
(`oracle.cpu_ref.dense_topk` over the remaining rows, ids mapped back):

* L2: ids equal, float32 distance bits equal.
* cosine: ids equal wherever the reference distances are distinguishable and float64 distances within rtol 1e-12 --
  the comparison the existing suite makes for this metric (`tests/test_hip_parity.py::_dense_check`: the device's and
  libm's `acos` are each within an ulp of the true value, not of each other) -- AND bits equal to a fresh
  `DenseIndex` over the remaining rows, which is the bit-for-bit statement of the contract itself.

Batches beyond 64 queries are compared with the oracle on a spread of 48 queries and, all of them, bit for bit with
a fresh index over the remaining rows (the oracle costs ~30 ms of numpy per query at these sizes).
"""
import numpy as np
import pytest

from oracle import cpu_ref as O
from smqtk_indexing_amd import _lib

pytestmark = pytest.mark.gpu

L2, COS = _lib.SQ_METRIC_L2, _lib.SQ_METRIC_COSINE


def _name(metric):
    return "euclidean" if metric == L2 else "cosine"


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _check(idx, db, live, qs, k, metric=L2, id_base=0, which=None, fresh=None):
    """Search `qs` on `idx` and compare with the oracle over db[live]; returns (dist, ids)."""
    rows = np.flatnonzero(live)
    dbl = np.ascontiguousarray(db[rows])
    d, i = idx.search(qs, k)
    assert idx.count() == (len(db), len(rows))
    for qi in (range(len(qs)) if which is None else which):
        rd, ri = O.dense_topk(dbl, qs[qi], k, _name(metric))
        kk = len(rd)
        want = rows[ri] + id_base
        if metric == L2:
            np.testing.assert_array_equal(i[qi, :kk], want, err_msg="query %d" % qi)
            np.testing.assert_array_equal(_bits(d[qi, :kk]), _bits(rd), err_msg="query %d" % qi)
        else:
            np.testing.assert_allclose(d[qi, :kk], rd, rtol=1e-12, atol=1e-15, equal_nan=True)
            mism = i[qi, :kk] != want
            if mism.any():
                full = O.dense_distances(dbl, qs[qi], "cosine")
                got_rows = np.searchsorted(rows, i[qi, :kk][mism] - id_base)
                assert (rows[got_rows] == i[qi, :kk][mism] - id_base).all(), "a removed row was returned"
                a, b = full[got_rows], full[ri[mism]]
                assert (np.isnan(a) == np.isnan(b)).all() and np.nanmax(np.abs(a - b), initial=0.0) < 1e-14
        # k beyond the rows that are left: padding, as for k beyond the rows of an index
        assert (i[qi, kk:] == -1).all() and np.isposinf(d[qi, kk:]).all()
    got = i[i >= 0] - id_base
    assert live[got].all(), "a removed row was returned"
    if fresh is not None:
        fd, fi = fresh.search(qs, k)
        back = np.where(fi >= 0, rows[np.clip(fi, 0, None)] + id_base, -1)
        np.testing.assert_array_equal(i, back)
        np.testing.assert_array_equal(_bits(d), _bits(fd))
    return d, i


def _top_rows(db, qs, k, metric=L2):
    out = set()
    for q in qs:
        out.update(int(r) for r in O.dense_topk(db, q, k, _name(metric))[1])
    return np.array(sorted(out), dtype=np.int64)


def _stages(n, db, qs, k, metric):
    """Removed sets chosen to hurt, cumulative: each query's true top-k; the trailing partial tile, a whole 64-row
    block and a whole 128-row scan unit; every second row."""
    yield "top-k of every query", _top_rows(db, qs[:32], k, metric)
    blocks = np.concatenate([np.arange(n - n % 32 if n % 32 else n - 32, n), np.arange(640, 704), np.arange(2560, 2688)])
    yield "partial tile + 64-row block + 128-row unit", blocks
    yield "every second row", np.arange(1, n, 2)


def _run_stages(idx, db, qs, k, metric, which=None, with_fresh=False, options=None, expect=None):
    n = len(db)
    live = np.ones(n, dtype=bool)
    for what, rows in _stages(n, db, qs, k, metric):
        rows = rows[live[rows]]
        idx.remove(rows)
        live[rows] = False
        fresh = _lib.DenseIndex(np.ascontiguousarray(db[live]), metric=metric, options=options) if with_fresh else None
        _check(idx, db, live, qs, k, metric, which=which, fresh=fresh)
        if expect is not None:
            expect(idx.stats(), what)
        if fresh is not None:
            fresh.close()
    return live


# ------------------------------------------------------------------------------------------------ every tier
@pytest.mark.parametrize("d,metric", [(100, L2), (128, L2), (512, L2), (128, COS), (512, COS)])
def test_fused_int8_filter(d, metric):
    rng = np.random.default_rng(d + metric)
    n, k = 70_001, 50
    db = rng.standard_normal((n, d)).astype(np.float32)
    qs = (db[rng.integers(0, n, 20)] + 0.05 * rng.standard_normal((20, d))).astype(np.float32)
    idx = _lib.DenseIndex(db, metric=metric)
    idx.set_option("dense_int8", 1)
    assert idx.info()["int8_in_use"]
    row8 = 128 if d <= 128 else 512

    def expect(st, what):
        assert st["bytes_scanned"] == (-(-n // 64) * 64) * (row8 + 4), (what, st)   # the int8 pass took the call

    _run_stages(idx, db, qs, k, metric, with_fresh=(metric == COS), expect=expect)
    idx.close()


@pytest.mark.parametrize("nq,qt", [(33, 2), (64, 4)])
def test_int8_two_and_four_query_tiles(nq, qt):
    rng = np.random.default_rng(nq)
    n, d, k = 70_001, 128, 30
    db = rng.standard_normal((n, d)).astype(np.float32)
    qs = rng.standard_normal((nq, d)).astype(np.float32)
    idx = _lib.DenseIndex(db)
    idx.set_option("dense_int8", 1)
    idx.set_option("dense_int8_batch", 256)
    idx.set_option("dense_qt", qt)
    groups = -(-nq // (32 * qt))

    def expect(st, what):
        assert st["bytes_scanned"] == (-(-n // 64) * 64) * 132 * groups, (what, st)

    _run_stages(idx, db, qs, k, L2, expect=expect)
    idx.close()


@pytest.mark.parametrize("nq,metric", [(20, L2), (128, L2), (1024, L2), (20, COS), (128, COS)])
def test_bf16_filter_one_and_many_tiles(nq, metric):
    rng = np.random.default_rng(1000 + nq + metric)
    n, d, k = 70_001, 128, 30
    db = rng.standard_normal((n, d)).astype(np.float32)
    qs = rng.standard_normal((nq, d)).astype(np.float32)
    opts = {"dense_int8": 0}
    idx = _lib.DenseIndex(db, metric=metric, options=opts)
    assert idx.info()["int8_copy_bytes"] == 0
    which = None if nq <= 64 else list(range(0, nq, max(1, nq // 48)))[:48]

    def expect(st, what):
        assert st["scan_launches"] >= 2 and st["fallback_queries"] < nq, (what, st)

    _run_stages(idx, db, qs, k, metric, which=which, with_fresh=(nq > 64 or metric == COS), options=opts, expect=expect)
    idx.close()


@pytest.mark.parametrize("d,metric", [(1024, L2), (4100, L2), (1024, COS)])
def test_wide_rows(d, metric):
    rng = np.random.default_rng(d)
    n, k = 66_000, 20
    db = rng.standard_normal((n, d), dtype=np.float32)
    qs = (db[rng.integers(0, n, 6)] + np.float32(0.05) * rng.standard_normal((6, d), dtype=np.float32)).astype(np.float32)
    idx = _lib.DenseIndex(db, metric=metric)
    d_pad = -(-d // 128) * 128

    def expect(st, what):
        assert st["scan_launches"] >= 2 and st["bytes_scanned"] >= (-(-n // 32) * 32) * 2 * d_pad, (what, st)   # the wide-row filter ran

    _run_stages(idx, db, qs, k, metric, with_fresh=(metric == COS), expect=expect)
    idx.close()


@pytest.mark.parametrize("d,family", [(128, "long_query"), (64, "two_clusters"), (100, "two_clusters")])
def test_middle_tier(d, family):
    """The families of tests/test_hip_parity.py::test_dense_middle_tier_certifies_what_the_bf16_filter_cannot."""
    rng = np.random.default_rng(500 + d)
    n, k = 200_000, 25
    db = rng.standard_normal((n, d)).astype(np.float32)
    qs = rng.standard_normal((12, d)).astype(np.float32)
    if family == "long_query":
        qs[:6] *= np.float32(300.0)
    else:
        off = np.zeros(d, dtype=np.float32)
        off[0] = 100.0
        db = (0.5 * db + np.where(np.arange(n)[:, None] % 2 == 0, off, -off)).astype(np.float32)
        qs[6:] = (0.5 * qs[6:] + off).astype(np.float32)
    idx = _lib.DenseIndex(db, options={"dense_int8": 0})

    def expect(st, what):
        assert st["mid_tier_queries"] > 0, (what, st)

    live = _run_stages(idx, db, qs, k, L2, expect=expect)
    # ... and the exact path behind it gives the same bits
    d1, i1 = idx.search(qs, k)
    idx.set_option("dense_mid_tier", 0)
    d0, i0 = _check(idx, db, live, qs, k)
    assert idx.stats()["mid_tier_queries"] == 0 and idx.stats()["fallback_queries"] > 0
    np.testing.assert_array_equal(i0, i1)
    np.testing.assert_array_equal(_bits(d0), _bits(d1))
    idx.close()


def test_middle_tier_cosine_offset_descriptors():
    """Descriptors sharing a large offset: the first cosine filter cannot tell them apart, the middle tier's per-row
    terms (built at first use, after the removal here, and again after an append) must leave the removed rows out."""
    rng = np.random.default_rng(77)
    n, d, k = 150_000, 128, 20
    db = (rng.standard_normal((n, d)) * 0.5 + 20.0).astype(np.float32)
    qs = (rng.standard_normal((8, d)) * 0.5 + 20.0).astype(np.float32)
    opts = {"dense_int8": 0}
    idx = _lib.DenseIndex(db, metric=COS, options=opts)
    live = np.ones(n, dtype=bool)
    rows = _top_rows(db, qs, k, COS)
    idx.remove(rows)
    live[rows] = False
    fresh = _lib.DenseIndex(np.ascontiguousarray(db[live]), metric=COS, options=opts)
    _check(idx, db, live, qs, k, COS, fresh=fresh)
    assert idx.stats()["mid_tier_queries"] == fresh.stats()["mid_tier_queries"]
    rows = _top_rows(np.where(live[:, None], db, np.float32(-1.0)), qs, k, COS)   # the next best, with the terms resident
    rows = rows[live[rows]]
    idx.remove(rows)
    live[rows] = False
    fresh.close()
    fresh = _lib.DenseIndex(np.ascontiguousarray(db[live]), metric=COS, options=opts)
    _check(idx, db, live, qs, k, COS, fresh=fresh)
    fresh.close()
    idx.close()


@pytest.mark.parametrize("metric", [L2, COS])
@pytest.mark.parametrize("n,d", [(70_001, 128), (5_000, 36), (66_000, 700)])
def test_exact_path(n, d, metric):
    """dense_mid_tier = 0 and every query forced down the exact all-rows path (the group kernel; n = 5 000: every row is
    a candidate, the one-query kernels)."""
    rng = np.random.default_rng(n + d + metric)
    k = 40
    db = rng.standard_normal((n, d)).astype(np.float32)
    qs = rng.standard_normal((11, d)).astype(np.float32)
    idx = _lib.DenseIndex(db, metric=metric)
    idx.set_option("dense_mid_tier", 0)
    idx.set_option("force_fallback", 1)

    def expect(st, what):
        if n > 65536:
            assert st["fallback_queries"] == len(qs), (what, st)

    _run_stages(idx, db, qs, k, metric, with_fresh=(metric == COS), expect=expect)
    idx.close()


# ------------------------------------------------------------------------------------- k beyond the rows left
@pytest.mark.parametrize("metric", [L2, COS])
@pytest.mark.parametrize("int8", [1, 0])
def test_all_but_k_minus_one_rows_removed(metric, int8):
    rng = np.random.default_rng(31 + metric + int8)
    n, d, k = 70_001, 128, 50
    db = rng.standard_normal((n, d)).astype(np.float32)
    qs = rng.standard_normal((5, d)).astype(np.float32)
    idx = _lib.DenseIndex(db, metric=metric)
    idx.set_option("dense_int8", int8)
    keep = np.sort(rng.choice(n, k - 1, replace=False))
    live = np.zeros(n, dtype=bool)
    live[keep] = True
    idx.remove(np.flatnonzero(~live))
    d_, i_ = _check(idx, db, live, qs, k, metric)
    assert (i_[:, k - 1] == -1).all() and (np.sort(i_[:, :k - 1], axis=1) == keep).all()
    # one row cannot leave: an index holds at least one
    with pytest.raises(_lib.HipError):
        idx.remove(keep)
    idx.remove(keep[1:])
    live[keep[1:]] = False
    _check(idx, db, live, qs, k, metric)
    idx.close()


@pytest.mark.parametrize("n", [3_000, 70_001])
@pytest.mark.parametrize("metric", [L2, COS])
def test_removed_rows_next_to_nan_inf_and_zero_rows(n, metric):
    """Live rows holding NaN / inf (and, under cosine, zero rows: NaN distance) rank last, in row order; removed rows
    next to them -- and removed NaN rows -- never appear.  k reaches into that tail."""
    rng = np.random.default_rng(n + metric)
    d = 64
    db = rng.standard_normal((n, d)).astype(np.float32)
    db[100, 3] = np.nan
    db[101, :] = 0.0
    db[102, 5] = np.inf
    db[103, :] = np.nan
    db[104, 7] = -np.inf
    db[n - 2, 0] = np.nan
    qs = rng.standard_normal((4, d)).astype(np.float32)
    idx = _lib.DenseIndex(db, metric=metric)
    live = np.ones(n, dtype=bool)
    gone = np.array([99, 103, 105, n - 1, n - 3] + list(range(200, 264)), dtype=np.int64)
    idx.remove(gone)
    live[gone] = False
    n_live = int(live.sum())
    for k in (10, n_live, n_live + 5) if n <= 10_000 else (10, 3000):
        d_, i_ = idx.search(qs, k)
        rows = np.flatnonzero(live)
        for qi in range(len(qs)):
            rd, ri = O.dense_topk(np.ascontiguousarray(db[rows]), qs[qi], k, _name(metric))
            kk = len(rd)
            np.testing.assert_array_equal(np.isnan(d_[qi, :kk]), np.isnan(rd))
            fin = ~np.isnan(rd)
            if metric == L2:
                np.testing.assert_array_equal(i_[qi, :kk], rows[ri])
                np.testing.assert_array_equal(_bits(d_[qi, :kk][fin]), _bits(rd[fin]))
            else:
                np.testing.assert_allclose(d_[qi, :kk][fin], rd[fin], rtol=1e-12, atol=1e-15)
                np.testing.assert_array_equal(i_[qi, :kk][~fin], rows[ri][~fin])
            assert (i_[qi, kk:] == -1).all() and np.isposinf(d_[qi, kk:]).all()
            assert live[i_[qi, :kk]].all()
    idx.close()


# ------------------------------------------------------------------------------------------------ lifecycle
@pytest.mark.parametrize("metric", [L2, COS])
def test_remove_search_append_search_remove_appended(metric):
    rng = np.random.default_rng(5 + metric)
    n, d, k, base = 70_001, 128, 30, 1_000_000
    db = rng.standard_normal((n, d)).astype(np.float32)
    qs = rng.standard_normal((9, d)).astype(np.float32)
    idx = _lib.DenseIndex(db, metric=metric, id_base=base)
    live = np.ones(n, dtype=bool)
    rows = np.concatenate([_top_rows(db, qs, k, metric), np.arange(n - 40, n)])   # ... and the tile / unit an append redoes
    rows = np.unique(rows)
    idx.remove(rows + base)
    live[rows] = False
    _check(idx, db, live, qs, k, metric, id_base=base)
    add = (qs[:5] + 0.01 * rng.standard_normal((5, d))).astype(np.float32)   # new nearest neighbours
    add = np.concatenate([add, rng.standard_normal((300, d)).astype(np.float32)])
    idx.append(add)
    db = np.concatenate([db, add])
    live = np.concatenate([live, np.ones(len(add), dtype=bool)])
    assert idx.count() == (n + len(add), int(live.sum()))
    _, i_ = _check(idx, db, live, qs, k, metric, id_base=base)
    assert (i_[:5, 0] == base + n + np.arange(5)).all()          # new ids follow the old ones: holes are not reused
    idx.remove(base + n + np.arange(0, 5, 2))
    live[n + np.arange(0, 5, 2)] = False
    _check(idx, db, live, qs, k, metric, id_base=base)
    # an index that doubles rebuilds its int8 copy from all rows: the removed ones stay out
    more = rng.standard_normal((len(db) + 10, d)).astype(np.float32)
    idx.append(more)
    db = np.concatenate([db, more])
    live = np.concatenate([live, np.ones(len(more), dtype=bool)])
    _check(idx, db, live, qs, k, metric, id_base=base)
    idx.close()


def test_borrowed_device_matrix_is_never_written():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(8)
    n, d, k = 70_016, 128, 30
    dbh = rng.standard_normal((n, d)).astype(np.float32)
    qs = rng.standard_normal((7, d)).astype(np.float32)
    for metric in (L2, COS):
        t = torch.from_numpy(dbh).to("cuda:0")
        before = t.clone()
        idx = _lib.DenseIndex(t.data_ptr(), n=n, d=d, metric=metric, device_ptr=True, id_base=17, keepalive=t)
        live = np.ones(n, dtype=bool)
        rows = np.concatenate([_top_rows(dbh, qs, k, metric), np.arange(1, n, 2)])
        rows = np.unique(rows)
        idx.remove(rows + 17)
        live[rows] = False
        _check(idx, dbh, live, qs, k, metric, id_base=17)
        idx.set_option("force_fallback", 1)
        _check(idx, dbh, live, qs, k, metric, id_base=17)
        with pytest.raises(_lib.HipError, match="borrows"):
            idx.compact()
        assert idx.count() == (n, int(live.sum()))
        torch.cuda.synchronize()
        assert torch.equal(t.view(torch.int32), before.view(torch.int32)), "the caller's matrix was written"
        idx.close()


@pytest.mark.parametrize("depth", [2, 3])
def test_removal_between_pipelined_calls(depth):
    """SQ_MEM_DEVICE_ASYNC with captured call graphs: a removal finishes the calls in flight, and the calls after it
    (replayed graphs included: same shapes, same buffers) see it."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(depth)
    dev = torch.device("cuda", 0)
    n, d, k, nq = 100_000, 128, 20, 16
    db = rng.standard_normal((n, d)).astype(np.float32)
    idx = _lib.DenseIndex(db)
    idx.set_option("dense_graph", 1)
    idx.set_option("dense_async_depth", depth)
    qs = [rng.standard_normal((nq, d)).astype(np.float32) for _ in range(12)]
    qd = [torch.from_numpy(q).to(dev) for q in qs]
    od = [torch.empty((nq, k), dtype=torch.float32, device=dev) for _ in qs]
    oi = [torch.empty((nq, k), dtype=torch.int64, device=dev) for _ in qs]
    live = np.ones(n, dtype=bool)
    live_at = []
    st = torch.cuda.current_stream().cuda_stream
    for j in range(len(qs)):
        if j in (5, 9):   # (calls 0 .. 4 have run eagerly, captured and replayed by now)
            rows = _top_rows(db, np.concatenate(qs[j:j + 3]), k)
            rows = rows[live[rows]]
            idx.remove(rows)
            live[rows] = False
            # the removal finished everything in flight
            for f in range(j):
                got = oi[f].cpu().numpy()
                assert live_at[f][got].all()
        live_at.append(live.copy())
        idx.search_device_async(qd[j].data_ptr(), nq, k, od[j].data_ptr(), oi[j].data_ptr(), st)
    idx.sync()
    for j in range(len(qs)):
        rows = np.flatnonzero(live_at[j])
        dbl = np.ascontiguousarray(db[rows])
        gi, gd = oi[j].cpu().numpy(), od[j].cpu().numpy()
        for r in range(0, nq, 3):
            rd, ri = O.dense_topk(dbl, qs[j][r], k)
            np.testing.assert_array_equal(gi[r], rows[ri], err_msg="call %d" % j)
            np.testing.assert_array_equal(_bits(gd[r]), _bits(rd))
    idx.close()


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("first", [True, False])
def test_refused_removals_change_nothing(first):
    rng = np.random.default_rng(12)
    n, d, k = 70_001, 128, 30
    db = rng.standard_normal((n, d)).astype(np.float32)
    qs = rng.standard_normal((6, d)).astype(np.float32)
    idx = _lib.DenseIndex(db, id_base=5)
    live = np.ones(n, dtype=bool)
    if not first:
        idx.remove(np.array([5 + 10, 5 + 11, 5 + 4000]))
        live[[10, 11, 4000]] = False
    top = _top_rows(db, qs, k) + 5
    before = idx.search(qs, k)
    cnt = idx.count()
    bad = [np.concatenate([top, top[:1]]),                 # listed twice
           np.concatenate([top, [5 + n]]),                 # out of range (above)
           np.concatenate([top, [4]]),                     # out of range (below id_base)
           np.concatenate([[5 + n, top[0]], top])]         # both
    if not first:
        bad.append(np.concatenate([top, [5 + 11]]))        # already removed
    for ids in bad:
        with pytest.raises(_lib.HipError, match="nothing was removed"):
            idx.remove(ids)
        assert idx.count() == cnt
        after = idx.search(qs, k)
        np.testing.assert_array_equal(after[1], before[1])
        np.testing.assert_array_equal(_bits(after[0]), _bits(before[0]))
        idx.set_option("force_fallback", 1)                # (the exact path reads the bitmap itself)
        after = idx.search(qs, k)
        idx.set_option("force_fallback", 0)
        np.testing.assert_array_equal(after[1], before[1])
    _check(idx, db, live, qs, k, id_base=5)
    idx.remove(top)                                        # the same ids without the offender go through
    live[top - 5] = False
    _check(idx, db, live, qs, k, id_base=5)
    idx.close()


# ---------------------------------------------------------------------------------------------- compaction
@pytest.mark.parametrize("n,d,metric", [(140_003, 128, L2), (140_003, 100, COS), (70_001, 600, L2), (9_000, 30, L2)])
def test_compact_equals_a_fresh_index(n, d, metric):
    rng = np.random.default_rng(n + d)
    k, base = 30, 40
    db = rng.standard_normal((n, d)).astype(np.float32)
    qs = rng.standard_normal((10, d)).astype(np.float32)
    idx = _lib.DenseIndex(db, metric=metric, id_base=base)
    o2n = idx.compact()                                     # nothing removed: nothing changes
    np.testing.assert_array_equal(o2n, base + np.arange(n))
    live = np.ones(n, dtype=bool)
    rows = np.unique(np.concatenate([_top_rows(db, qs, k, metric), rng.choice(n, n // 3, replace=False), np.arange(n - 70, n), [0]]))
    idx.remove(rows + base)
    live[rows] = False
    _check(idx, db, live, qs, k, metric, id_base=base)
    o2n = idx.compact()
    n_live = int(live.sum())
    assert idx.count() == (n_live, n_live) and idx.n == n_live
    assert (o2n[~live] == -1).all()
    np.testing.assert_array_equal(o2n[live], base + np.arange(n_live))
    dbl = np.ascontiguousarray(db[live])
    fresh = _lib.DenseIndex(dbl, metric=metric, id_base=base)
    fi, ci = fresh.info(), idx.info()
    for key in ("rows", "d", "f32_rows_bytes", "f32_rows_owned", "bf16_copy_bytes", "int8_copy_bytes", "row_stats_bytes", "int8_in_use"):
        assert ci[key] == fi[key], (key, ci, fi)
    _check(idx, dbl, np.ones(n_live, dtype=bool), qs, k, metric, id_base=base, fresh=None)
    fd, fidx = fresh.search(qs, k)
    cd, cidx = idx.search(qs, k)
    np.testing.assert_array_equal(cidx, fidx)
    np.testing.assert_array_equal(_bits(cd), _bits(fd))
    assert idx.stats()["fallback_queries"] == fresh.stats()["fallback_queries"]
    # the compacted index is an ordinary index: it appends, removes and compacts again
    add = rng.standard_normal((50, d)).astype(np.float32)
    idx.append(add)
    dbl = np.concatenate([dbl, add])
    live2 = np.ones(len(dbl), dtype=bool)
    idx.remove(base + np.array([0, n_live - 1, n_live + 3]))
    live2[[0, n_live - 1, n_live + 3]] = False
    _check(idx, dbl, live2, qs, k, metric, id_base=base)
    o2n = idx.compact()
    assert (o2n[~live2] == -1).all() and idx.count() == (len(dbl) - 3, len(dbl) - 3)
    _check(idx, np.ascontiguousarray(dbl[live2]), np.ones(len(dbl) - 3, dtype=bool), qs, k, metric, id_base=base)
    fresh.close()
    idx.close()


# ------------------------------------------------------------------------- removal does not push queries down a tier
@pytest.mark.parametrize("int8", [1, 0])
def test_one_per_cent_removed_keeps_the_tier(int8):
    rng = np.random.default_rng(90 + int8)
    n, d, k = 400_000, 128, 100
    db = rng.standard_normal((n, d)).astype(np.float32)
    qs = rng.standard_normal((32, d)).astype(np.float32)
    opts = {"dense_int8": 0} if not int8 else None
    idx = _lib.DenseIndex(db, options=opts)
    live = np.ones(n, dtype=bool)
    rows = np.sort(rng.choice(n, n // 100, replace=False))
    idx.remove(rows)
    live[rows] = False
    fresh = _lib.DenseIndex(np.ascontiguousarray(db[live]), options=opts)
    _check(idx, db, live, qs, k, which=range(0, 32, 4), fresh=fresh)
    a, b = idx.stats(), fresh.stats()
    assert a["fallback_queries"] == b["fallback_queries"] and a["mid_tier_queries"] == b["mid_tier_queries"], (a, b)
    assert a["scan_launches"] == b["scan_launches"]
    assert idx.info()["int8_in_use"] == bool(int8)
    fresh.close()
    idx.close()


# ------------------------------------------------------------------------------------------------ full size
def test_dense_l2_10m_x_128_removed_oracle_literal():
    """Beside tests/test_hip_full_size.py::test_dense_l2_10m_x_128_oracle_literal: 10 M x 128, 100 k random rows and the
    top 100 of 6 queries removed; those 6 queries literally against the oracle over the remaining rows."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    n, d, k = 10_000_000, 128, 100
    g = torch.Generator(device=dev)
    g.manual_seed(202)
    db = torch.empty((n, d), dtype=torch.float32, device=dev)
    for s in range(0, n, 1 << 21):
        db[s:s + (1 << 21)].normal_(generator=g)
    q = torch.empty((6, d), dtype=torch.float32, device=dev).normal_(generator=g)
    dbh, qh = db.cpu().numpy(), q.cpu().numpy()
    idx = _lib.DenseIndex(db.data_ptr(), n=n, d=d, device_ptr=True, keepalive=db)
    rng = np.random.default_rng(3)
    d0, i0 = idx.search(qh, k)
    rows = np.unique(np.concatenate([rng.choice(n, 100_000, replace=False), i0.reshape(-1)]))
    idx.remove(rows)
    live = np.ones(n, dtype=bool)
    live[rows] = False
    assert idx.count() == (n, n - len(rows))
    keep = np.flatnonzero(live)
    dbl = dbh[keep]
    d1, i1 = idx.search(qh, k)
    assert idx.stats()["fallback_queries"] == 0
    for qi in range(6):
        rd, ri = O.dense_topk(dbl, qh[qi], k)
        np.testing.assert_array_equal(i1[qi], keep[ri])
        np.testing.assert_array_equal(_bits(d1[qi]), _bits(rd))
    idx.close()
