"""
GPU tests of the IVF-Flat index (`sq_ivf_*`, `_lib.IvfIndex`, `HipIvfFlatNearestNeighborsIndex`).

Every answer is compared with the numpy restatement of tests/ivf_cases.py (assignment, probe and result over
`oracle.cpu_ref`), ids exactly and distances in float32 bits; the cases' preconditions -- two empty lists, a list of
several scan chunks, a list shorter than k = 200, the 41-way tie at distance 0 -- are proven on the CPU by
tests/test_ivf_cases_cpu.py.  The restatement of a case is computed once and shared by all tests here.

Beside that 64-list case: 700 lists of fewer than 256 rows probed 1 to 700 at a time (the prefix of the probed lists'
sizes across waves and across blocks of 256, scan chunks that span many lists, empty lists planted at probe positions 63,
255 and 257); the scan at every row width of tests/width_cases.py, padded rows included, on a case in which another
summation order changes a compared distance; device rows with a padded stride and from an unaligned base; 70 000 queries
in one call; and the k-means update over two dimension blocks with lists of one, two and three rows.
"""
import warnings

import numpy as np
import pytest

from oracle import cpu_ref as O
from smqtk_indexing_amd import _lib
from smqtk_indexing_amd._compat import DescriptorMemoryElement
from smqtk_indexing_amd.impls.nn_index.hip_bruteforce import HipBruteForceNearestNeighborsIndex
from smqtk_indexing_amd.impls.nn_index.hip_ivf import HipIvfFlatNearestNeighborsIndex
from tests import ivf_cases as C
from tests import width_cases as W

pytestmark = pytest.mark.gpu

NPROBES = (1, 5, 64, 100)        # 100 clamps to nlist = 64
KS = (1, 10, 200, 30_000)        # 30 000 is beyond every candidate count: padding
_indexes = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _index(d):
    """The case's index, built once: one add of all rows."""
    if d not in _indexes:
        case = C.make_case(d)
        idx = _lib.IvfIndex(case.centroids)
        idx.add(case.x)
        _indexes[d] = idx
    return _indexes[d]


def _same(got_dist, got_idx, want_idx, want_dist, what):
    np.testing.assert_array_equal(got_idx, want_idx, err_msg=what)
    np.testing.assert_array_equal(_bits(got_dist), _bits(want_dist), err_msg=what)


# ------------------------------------------------------------------------------------ search
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("nq", [1, 33])
@pytest.mark.parametrize("nprobe", NPROBES)
@pytest.mark.parametrize("d", C.DIMS)
def test_search_equals_the_restatement(d, nprobe, nq, mem):
    """The first nq pool queries -- x[7] (41 ties at distance 0), the query at the far centroid (its first list is
    empty), the zero vector, then random ones -- for every k, from host and from device memory."""
    case, idx = C.make_case(d), _index(d)
    if mem == "device":
        torch = pytest.importorskip("torch")
        dev = torch.device("cuda:0")
        q_t = torch.from_numpy(np.array(case.pool[:nq])).to(dev)
        stream = torch.cuda.Stream(device=dev)
    for k in KS:
        want_idx, want_dist = case.expected(nq, nprobe, k)
        if mem == "host":
            dist, ids = idx.search(case.pool[:nq], k, nprobe)
        else:
            od = torch.full((nq, k), -3.0, dtype=torch.float32, device=dev)
            oi = torch.full((nq, k), -77, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            idx.search_device(q_t.data_ptr(), nq, k, nprobe, od.data_ptr(), oi.data_ptr(), stream.cuda_stream)
            dist, ids = od.cpu().numpy(), oi.cpu().numpy()           # (the call is blocking: the results are final)
            assert not (ids == -77).any() and not (dist == -3.0).any(), "a sentinel survived"
        _same(dist, ids, want_idx, want_dist, f"d={d} nprobe={nprobe} nq={nq} k={k} {mem}")
        if k == 30_000:
            assert (ids[:, -1] == -1).all() and np.isposinf(dist[:, -1]).all()
    st = idx.stats()
    cands = sum(case.answer(qi, nprobe)[0].shape[0] for qi in range(nq))
    assert st["candidates"] == cands and st["bytes_scanned"] == cands * (-(-d // 4) * 4) * 4
    assert st["scan_launches"] == (1 if cands else 0)
    if nprobe == 1 and nq == 1:
        assert ids[0, :41].tolist() == [7] + list(range(100, 140)) and not dist[0, :41].any()


@pytest.mark.parametrize("d", C.DIMS)
def test_every_list_probed_equals_the_dense_search(d):
    case, idx = C.make_case(d), _index(d)
    dense = _lib.DenseIndex(case.x)
    try:
        for k in (1, 10, 200):
            dd, di = dense.search(case.pool, k)
            for nprobe in (C.NLIST, 100):
                dist, ids = idx.search(case.pool, k, nprobe)
                _same(dist, ids, di, dd, f"d={d} k={k} nprobe={nprobe}")
    finally:
        dense.close()


def test_modes_other_than_blocking_are_refused():
    case, idx = C.make_case(36), _index(36)
    lib = _lib.load_ivf()
    q = np.ascontiguousarray(case.pool[:1])
    dist, ids = np.empty((1, 4), np.float32), np.empty((1, 4), np.int64)
    for mem in (_lib.SQ_MEM_DEVICE_ASYNC, _lib.SQ_MEM_PLAN, 9):
        assert lib.sq_ivf_search(idx.handle, q.ctypes.data, 1, 4, 1, dist.ctypes.data, ids.ctypes.data, mem, None) == -4
    assert lib.sq_ivf_search(idx.handle, q.ctypes.data, 1, 4, 0, dist.ctypes.data, ids.ctypes.data, 0, None) == -1   # nprobe < 1


# ------------------------------------------------------------------------------------ many short lists
M_NPROBES = (1, 63, 64, 65, 255, 256, 257, 511, 513, 700, 1000)       # 1000 clamps to nlist = 700
M_KS = (1, 10, 300, 7000)                                             # 7000 is beyond the 6007 rows: padding


def _many():
    """The many-lists case and its index, built once: one add of all rows."""
    case = C.make_many_lists_case()
    if "many" not in _indexes:
        idx = _lib.IvfIndex(case.centroids)
        idx.add(case.x)
        _indexes["many"] = idx
    return case, _indexes["many"]


@pytest.mark.parametrize("nq", [1, 33])
@pytest.mark.parametrize("nprobe", M_NPROBES)
def test_many_lists_search_equals_the_restatement(nprobe, nq):
    """700 lists of fewer than 256 rows: beyond 64 probed lists the prefix of a query's list sizes crosses waves, beyond
    256 it carries from one block of the prefix kernel to the next, and every full scan chunk spans several lists."""
    case, idx = _many()
    for k in M_KS:
        dist, ids = idx.search(case.pool[:nq], k, nprobe)
        _same(dist, ids, *case.expected(nq, nprobe, k), f"many lists nprobe={nprobe} nq={nq} k={k}")
        if k == 7000:
            assert (ids[:, -1] == -1).all() and np.isposinf(dist[:, -1]).all()
    st = idx.stats()
    cands = sum(case.answer(qi, nprobe)[0].shape[0] for qi in range(nq))
    assert st["candidates"] == cands and st["bytes_scanned"] == cands * case.d * 4       # d = 20: no padding
    assert st["scan_launches"] == (1 if cands else 0)


def test_many_lists_planted_query_with_its_empty_lists_probed():
    """The planted query alone: the empty twins at probe positions 63, 255 and 257 are the last list probed, or lie
    inside the probed range."""
    case, idx = _many()
    q = case.pool[C.Q_PLANT:C.Q_PLANT + 1]
    for nprobe in (63, 64, 255, 256, 257, 258, 700):
        for k in (10, 7000):
            dist, ids = idx.search(q, k, nprobe)
            oi, od = C.pad(*case.answer(C.Q_PLANT, nprobe), k)
            _same(dist[0], ids[0], oi, od, f"planted query nprobe={nprobe} k={k}")
        assert idx.stats()["candidates"] == case.answer(C.Q_PLANT, nprobe)[0].shape[0]


def test_many_lists_search_from_device_memory():
    torch = pytest.importorskip("torch")
    case, idx = _many()
    dev = torch.device("cuda:0")
    nq, nprobe = 33, 257
    q_t = torch.from_numpy(np.array(case.pool[:nq])).to(dev)
    stream = torch.cuda.Stream(device=dev)
    for k in M_KS:
        od = torch.full((nq, k), -3.0, dtype=torch.float32, device=dev)
        oi = torch.full((nq, k), -77, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        idx.search_device(q_t.data_ptr(), nq, k, nprobe, od.data_ptr(), oi.data_ptr(), stream.cuda_stream)
        dist, ids = od.cpu().numpy(), oi.cpu().numpy()
        assert not (ids == -77).any() and not (dist == -3.0).any(), "a sentinel survived"
        _same(dist, ids, *case.expected(nq, nprobe, k), f"many lists from device memory k={k}")


def test_many_lists_three_adds_are_one_add():
    case, one = _many()
    sizes = np.diff(case.off)
    with _lib.IvfIndex(case.centroids, id_base=1000) as idx:
        for lo, hi in ((0, 1), (1, 2500), (2500, case.n)):
            idx.add(case.x[lo:hi])
        off, ids_by_list = idx.lists()
        np.testing.assert_array_equal(off, case.off)
        np.testing.assert_array_equal(ids_by_list, case.order + 1000)
        one_off, one_ids = one.lists()
        np.testing.assert_array_equal(off, one_off)
        np.testing.assert_array_equal(ids_by_list, one_ids + 1000)
        info = idx.info()
        assert (info["rows"], info["d"], info["nlist"], info["longest_list"], info["empty_lists"]) == (case.n, case.d, case.nlist, sizes.max(), 4)
        assert info["rows_bytes"] == case.n * case.d * 4
        for nprobe, k in ((1, 10), (65, 300), (257, 10), (700, 7000)):
            dist, ids = idx.search(case.pool, k, nprobe)
            _same(dist, ids, *case.expected(C.POOL, nprobe, k, id_base=1000), f"many lists nprobe={nprobe} k={k} after three adds")
            d1, i1 = one.search(case.pool, k, nprobe)
            _same(dist, ids, np.where(i1 < 0, i1, i1 + 1000), d1, f"many lists nprobe={nprobe} k={k}: three adds against one")


def test_many_lists_every_list_probed_equals_the_dense_search():
    case, idx = _many()
    dense = _lib.DenseIndex(case.x)
    try:
        for k in (1, 10, 300):
            dd, di = dense.search(case.pool, k)
            for nprobe in (case.nlist, 1000):
                dist, ids = idx.search(case.pool, k, nprobe)
                _same(dist, ids, di, dd, f"many lists k={k} nprobe={nprobe}")
    finally:
        dense.close()


# ------------------------------------------------------------------------------------ every row width
def _ld(d):
    return -(-d // 4) * 4


def _width_checks(case, idx, nprobes):
    for nprobe in nprobes:
        dist, ids = idx.search(case.pool, C.W_K, nprobe)
        _same(dist, ids, *case.expected(C.W_POOL, nprobe, C.W_K), f"d={case.d} nprobe={nprobe}")
        cands = sum(case.answer(qi, nprobe)[0].shape[0] for qi in range(C.W_POOL))
        st = idx.stats()
        assert st["candidates"] == cands and st["bytes_scanned"] == cands * _ld(case.d) * 4
        # the tie pair in row order: query 0 is row 20 itself; any other query that returns one returns both
        assert ids[0, :2].tolist() == [C.W_ROW, C.W_ROW_COPY] and dist[0, 0] == dist[0, 1] == 0
        for qi in range(1, C.W_POOL):
            at = np.flatnonzero(ids[qi] == C.W_ROW)
            if at.size and at[0] + 1 < C.W_K:
                assert ids[qi, at[0] + 1] == C.W_ROW_COPY and dist[qi, at[0]] == dist[qi, at[0] + 1]
    assert idx.info()["rows_bytes"] == case.n * _ld(case.d) * 4


@pytest.mark.parametrize("d", W.WIDTHS)
def test_scan_at_width(d):
    """ivf_scan_kernel sums in numpy's order (SqLeafLane over rows padded to a multiple of four floats) at every width
    where that code branches; a sum in another order fails here (tests/test_ivf_cases_cpu.py).  Two adds, so that the
    second moves the first one's rows at this row stride."""
    case = C.make_width_case(d)
    with _lib.IvfIndex(case.centroids) as idx:
        idx.add(case.x[:500])
        idx.add(case.x[500:])
        off, ids_by_list = idx.lists()
        np.testing.assert_array_equal(off, case.off)
        np.testing.assert_array_equal(ids_by_list, case.order)
        _width_checks(case, idx, (1, 3, 8))


@pytest.mark.parametrize("d", W.BEYOND)
def test_scan_at_width_beyond_numpys_buffer(d):
    """Rows longer than numpy's 8192-element buffer, every list probed: the dense search's bits, as the header says."""
    case = C.make_width_case(d)
    with _lib.IvfIndex(case.centroids) as idx:
        idx.add(case.x)
        _width_checks(case, idx, (8,))


# ------------------------------------------------------------------------------------ add
@pytest.mark.parametrize("d", [36, 128])
def test_three_adds_are_one_add(d):
    case = C.make_case(d)
    with _lib.IvfIndex(case.centroids, id_base=1000) as idx:
        # nothing added yet: padding only
        dist, ids = idx.search(case.pool[:3], 5, 4)
        assert (ids == -1).all() and np.isposinf(dist).all()
        assert idx.info()["rows"] == 0 and idx.info()["empty_lists"] == C.NLIST
        for lo, hi in ((0, 1), (1, 7001), (7001, C.N)):
            idx.add(case.x[lo:hi])
        off, ids_by_list = idx.lists()
        np.testing.assert_array_equal(off, case.off)
        np.testing.assert_array_equal(ids_by_list, case.order + 1000)          # list-major, ascending inside a list
        one_off, one_ids = _index(d).lists()
        np.testing.assert_array_equal(off, one_off)
        np.testing.assert_array_equal(ids_by_list, one_ids + 1000)
        info = idx.info()
        sizes = np.diff(case.off)
        assert (info["rows"], info["d"], info["nlist"], info["longest_list"], info["empty_lists"]) == (C.N, d, C.NLIST, sizes.max(), 2)
        assert info["rows_bytes"] == C.N * (-(-d // 4) * 4) * 4 and info["add_us"] > 0 and info["key_budget_bytes"] == 256 << 20
        for nprobe, k in ((1, 200), (5, 10), (64, 10)):
            dist, ids = idx.search(case.pool, k, nprobe)
            want_idx, want_dist = case.expected(C.POOL, nprobe, k, id_base=1000)
            _same(dist, ids, want_idx, want_dist, f"d={d} nprobe={nprobe} k={k} after three adds")


def test_rows_added_from_device_memory():
    torch = pytest.importorskip("torch")
    case = C.make_case(36)
    x_t = torch.from_numpy(np.array(case.x)).to(torch.device("cuda:0"))
    torch.cuda.synchronize()
    with _lib.IvfIndex(case.centroids) as idx:
        idx.add(x_t.data_ptr(), n=C.N, device_ptr=True)
        off, ids_by_list = idx.lists()
        np.testing.assert_array_equal(off, case.off)
        np.testing.assert_array_equal(ids_by_list, case.order)
        dist, ids = idx.search(case.pool, 10, 5)
        _same(dist, ids, *case.expected(C.POOL, 5, 10), "rows added from device memory")


@pytest.mark.parametrize("d", C.DEVICE_ROW_DIMS)
def test_device_rows_padded_and_unaligned(d):
    """Device rows that the 16-byte copy cannot take: d = 35 is stored with a stride of 36 floats (the copy pads with a
    zero), d = 36 needs no padding but starts 4 bytes into an allocation.  Lists and answers are the host-added index's."""
    torch = pytest.importorskip("torch")
    case = C.make_width_case(d)
    shift = 1 if d % 4 == 0 else 0
    flat = torch.zeros(case.n * d + shift, dtype=torch.float32, device=torch.device("cuda:0"))
    flat[shift:].copy_(torch.from_numpy(np.array(case.x)).reshape(-1))
    ptr = flat.data_ptr() + 4 * shift
    torch.cuda.synchronize()
    assert flat.data_ptr() % 16 == 0 and ptr % 16 == 4 * shift and (_ld(d) != d or shift)
    with _lib.IvfIndex(case.centroids) as idx, _lib.IvfIndex(case.centroids) as host:
        idx.add(ptr, n=500, device_ptr=True)
        idx.add(ptr + 500 * d * 4, n=case.n - 500, device_ptr=True)      # (18 000 or 17 500 floats on: the same remainder)
        host.add(case.x)
        off, ids_by_list = idx.lists()
        h_off, h_ids = host.lists()
        np.testing.assert_array_equal(off, case.off)
        np.testing.assert_array_equal(ids_by_list, case.order)
        np.testing.assert_array_equal(off, h_off)
        np.testing.assert_array_equal(ids_by_list, h_ids)
        assert idx.info()["rows_bytes"] == case.n * _ld(d) * 4
        for nprobe in (1, 3, 8):
            dist, ids = idx.search(case.pool, C.W_K, nprobe)
            _same(dist, ids, *case.expected(C.W_POOL, nprobe, C.W_K), f"d={d} device rows nprobe={nprobe}")
            hd, hi = host.search(case.pool, C.W_K, nprobe)
            _same(dist, ids, hi, hd, f"d={d} device rows against host rows nprobe={nprobe}")


# ------------------------------------------------------------------------------------ the slice budget
def test_a_small_key_budget_runs_the_batch_in_slices():
    case = C.make_case(128)
    with _lib.IvfIndex(case.centroids) as idx:
        idx.add(case.x)
        idx.set_option("ivf_key_budget_mb", 1)
        assert idx.info()["key_budget_bytes"] == 1 << 20
        # every list probed: 20 011 candidates per query.  k = 10: (20 011 + 10) * 8 bytes per query, 6 queries per
        # slice, 6 slices for 33 queries; k = 30 000 sorts (2 * 32 768 more keys per query): one query per slice
        for k, slices in ((10, 6), (30_000, 33)):
            dist, ids = idx.search(case.pool, k, C.NLIST)
            assert idx.stats()["scan_launches"] == slices
            _same(dist, ids, *case.expected(C.POOL, C.NLIST, k), f"k={k} in {slices} slices")
        dist, ids = idx.search(case.pool, 200, 5)                      # uneven candidate counts across the slices
        assert idx.stats()["scan_launches"] > 1
        _same(dist, ids, *case.expected(C.POOL, 5, 200), "nprobe=5 in slices")
        idx.reset_options()
        dist, ids = idx.search(case.pool, 10, C.NLIST)
        assert idx.stats()["scan_launches"] == 1


def test_a_batch_beyond_65536_queries():
    """The queries of a slice are the second axis of the scan's grid.  70 000 queries (50 distinct ones, tiled) with the
    default key budget, and with a budget of 1 GiB that puts them all into one slice; the number of scan launches is
    ivf_slice_queries' arithmetic."""
    case = C.make_width_case(C.BATCH_D)
    q50 = C.batch_queries(case)
    answers = [C.search(case.x, case.centroids, case.off, case.order, q, C.BATCH_NPROBE) for q in q50]
    want = [C.pad(ids, dist, C.BATCH_K) for ids, dist in answers]
    reps = C.BATCH_NQ // C.BATCH_DISTINCT
    want_idx, want_dist = np.tile(np.stack([w[0] for w in want]), (reps, 1)), np.tile(np.stack([w[1] for w in want]), (reps, 1))
    queries = np.tile(q50, (reps, 1))
    maxc = max(a[0].shape[0] for a in answers)
    per = (maxc + min(C.BATCH_K, maxc)) * 8
    with _lib.IvfIndex(case.centroids) as idx:
        idx.add(case.x)
        for budget_mb in (256, C.BATCH_BUDGET_MB):
            idx.set_option("ivf_key_budget_mb", budget_mb)
            assert idx.info()["key_budget_bytes"] == budget_mb << 20
            dist, ids = idx.search(queries, C.BATCH_K, C.BATCH_NPROBE)
            slice_q = min(C.BATCH_NQ, (budget_mb << 20) // per)
            st = idx.stats()
            print("70 000 queries, budget %d MiB: %d per slice, %d scan launches" % (budget_mb, slice_q, st["scan_launches"]))
            assert st["scan_launches"] == -(-C.BATCH_NQ // slice_q) and st["candidates"] == reps * sum(a[0].shape[0] for a in answers)
            _same(dist, ids, want_idx, want_dist, f"70 000 queries, budget {budget_mb} MiB")
        assert slice_q == C.BATCH_NQ                                     # the raised budget: one slice holds the batch


# ------------------------------------------------------------------------------------ k-means
KM_N, KM_D, KM_LISTS = 6000, 32, 16


def _blobs():
    rng = np.random.default_rng(77)
    centres = (rng.standard_normal((KM_LISTS, KM_D)) * 4).astype(np.float32)
    x = (centres[rng.integers(0, KM_LISTS, KM_N)] + rng.standard_normal((KM_N, KM_D))).astype(np.float32)
    init = x[rng.choice(KM_N, KM_LISTS, replace=False)].copy()
    return x, init


def _lloyd_step(x, c):
    """One iteration in numpy: the oracle's assignment, float64 mean in list order, rounded to float32 once."""
    a = C.assign(c, x)
    out = c.copy()
    for l in range(c.shape[0]):
        rows = x[a == l]
        if rows.shape[0]:
            out[l] = (rows.astype(np.float64).sum(axis=0) / rows.shape[0]).astype(np.float32)
    return out, a


def _objective(x, c):
    d2 = ((x.astype(np.float64)[:, None, :] - c.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    return d2.min(axis=1).sum()


def _ulps(a, b):
    ia, ib = (v.view(np.int32).astype(np.int64) for v in (np.ascontiguousarray(a), np.ascontiguousarray(b)))
    ia, ib = (np.where(v < 0, np.int64(-2 ** 31) - v, v) for v in (ia, ib))
    return np.abs(ia - ib)


def test_kmeans_one_iteration_equals_numpy():
    """The float64 sums differ from numpy's only in order -- far below half a float32 ulp of the mean -- so the rounded
    centroids differ by at most one float32 step per element."""
    x, init = _blobs()
    got = _lib.ivf_kmeans(x, init, 1)
    want, a = _lloyd_step(x, init)
    assert got.dtype == np.float32 and got.shape == init.shape and np.bincount(a, minlength=KM_LISTS).min() > 0
    worst = _ulps(got, want).max()
    print("k-means, one iteration: largest difference %d ulp" % worst)
    assert worst <= 1
    np.testing.assert_array_equal(_lib.ivf_kmeans(x, init, 0), init)   # no iteration: the initial centroids


def test_kmeans_is_deterministic_and_does_not_raise_the_objective():
    x, init = _blobs()
    one = _lib.ivf_kmeans(x, init, 1)
    ten, again = _lib.ivf_kmeans(x, init, 10), _lib.ivf_kmeans(x, init, 10)
    np.testing.assert_array_equal(_bits(ten), _bits(again))
    o1, o10 = _objective(x, one), _objective(x, ten)
    print("k-means objective: %.6f after 1 iteration, %.6f after 10" % (o1, o10))
    assert o10 <= o1 * (1 + 1e-6)       # (the margin covers the float32 rounding of the centroids)


def test_kmeans_empty_list_keeps_its_centroid():
    x, init = _blobs()
    init[5] = 1000.0                                                     # nothing is nearest to it
    for iters in (1, 10):
        got = _lib.ivf_kmeans(x, init, iters)
        np.testing.assert_array_equal(_bits(got[5]), _bits(init[5]))
        assert not np.array_equal(got[4], init[4])
    want, a = _lloyd_step(x, init)
    assert (a != 5).all() and _ulps(_lib.ivf_kmeans(x, init, 1), want).max() <= 1
    with pytest.raises(_lib.HipError, match="cannot train"):
        _lib.ivf_kmeans(x[:10], init, 1)                                 # n < nlist


KW_N, KW_D, KW_LISTS = 3000, 100, 40
_wide_blobs = []


def _blobs_wide():
    """(x, init, assignment under init): d = 100 is two dimension blocks of the update kernel, the second of 36 lanes.
    37 blobs, and far from them three clusters of exactly 1, 2 and 3 rows, each with an initial centroid of its own: lists
    that leave three, two and one of the kernel's four waves without a row."""
    if not _wide_blobs:
        rng = np.random.default_rng(78)
        centres = (rng.standard_normal((KW_LISTS - 3, KW_D)) * 4).astype(np.float32)
        x = (centres[rng.integers(0, KW_LISTS - 3, KW_N)] + rng.standard_normal((KW_N, KW_D))).astype(np.float32)
        far = rng.choice(KW_N, 6, replace=False)
        for rows, at in ((far[:1], 500.0), (far[1:3], -500.0), (far[3:], 900.0)):
            x[rows] = (at + rng.standard_normal((len(rows), KW_D))).astype(np.float32)
        near = np.setdiff1d(np.arange(KW_N), far)
        init = np.vstack([x[rng.choice(near, KW_LISTS - 3, replace=False)], x[far[[0, 1, 3]]]])
        a = C.assign(init, x)
        for arr in (x, init, a):
            arr.setflags(write=False)
        _wide_blobs.append((x, init, a))
    return _wide_blobs[0]


def test_kmeans_two_dimension_blocks_and_lists_of_one_two_three_rows():
    """The bound is test_kmeans_one_iteration_equals_numpy's: float64 sums that differ from numpy's only in order, so at
    most one float32 step per element after the one rounding."""
    x, init, a = _blobs_wide()
    assert KW_D > 64 and KW_D % 64 == 36
    assert np.bincount(a, minlength=KW_LISTS)[-3:].tolist() == [1, 2, 3] and np.bincount(a, minlength=KW_LISTS).min() == 1
    got = _lib.ivf_kmeans(x, init, 1)
    want, a1 = _lloyd_step(x, init)
    assert np.array_equal(a1, a) and got.dtype == np.float32 and got.shape == init.shape
    worst = _ulps(got, want).max()
    print("k-means at d = 100, one iteration: largest difference %d ulp" % worst)
    assert worst <= 1
    np.testing.assert_array_equal(_bits(got[-3]), _bits(x[a == KW_LISTS - 3][0]))      # the mean of one row is the row
    # three single iterations, each from numpy's previous centroids
    c = want
    for step in (2, 3, 4):
        got = _lib.ivf_kmeans(x, c, 1)
        c, a_step = _lloyd_step(x, c)
        worst = _ulps(got, c).max()
        print("k-means at d = 100, iteration %d: largest difference %d ulp" % (step, worst))
        assert worst <= 1, step
        assert np.bincount(a_step, minlength=KW_LISTS)[-3:].tolist() == [1, 2, 3]


def test_kmeans_two_dimension_blocks_is_deterministic():
    x, init, _ = _blobs_wide()
    five, again = _lib.ivf_kmeans(x, init, 5), _lib.ivf_kmeans(x, init, 5)
    np.testing.assert_array_equal(_bits(five), _bits(again))
    assert not np.array_equal(five[:KW_LISTS - 3], init[:KW_LISTS - 3])


# ------------------------------------------------------------------------------------ the plugin class
def _descriptors(vecs, start=0):
    out = []
    for i, v in enumerate(vecs):
        e = DescriptorMemoryElement(start + i)
        e.set_vector(v)
        out.append(e)
    return out


def _plugin_data(dtype):
    rng = np.random.default_rng(21)
    centres = rng.standard_normal((40, 16)) * 3
    return (centres[rng.integers(0, 40, 3000)] + rng.standard_normal((3000, 16))).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_plugin_build_update_remove_nn(dtype):
    vecs = _plugin_data(dtype)
    descr = _descriptors(vecs)
    ivf = HipIvfFlatNearestNeighborsIndex(nlist=32, nprobe=32, train_iters=5, random_seed=4)
    bf = HipBruteForceNearestNeighborsIndex()
    ivf.build_index(descr[:2000])
    ivf.update_index(descr[2000:])                                       # joins the existing lists
    bf.build_index(descr)
    assert ivf.count() == bf.count() == 3000
    queries = _descriptors(np.vstack([vecs[7], vecs[2500] + 0.01, np.zeros(16)]).astype(dtype), start=10_000)

    def compare(n):
        for q in queries:
            with warnings.catch_warnings():
                warnings.simplefilter("error")                           # every list probed: n neighbours come back
                ie, idist = ivf.nn(q, n)
            be, bdist = bf.nn(q, n)
            assert [e.uuid() for e in ie] == [e.uuid() for e in be] and idist == bdist

    compare(1)
    compare(50)
    # a replaced uuid and a removal: the lists are rebuilt with the same centroids
    moved = DescriptorMemoryElement(7)
    moved.set_vector((vecs[7] + 5).astype(dtype))
    for index in (ivf, bf):
        index.update_index([moved])
        index.remove_from_index(list(range(100, 200)))
    assert ivf.count() == bf.count() == 2900
    compare(50)
    with pytest.raises(KeyError):
        ivf.remove_from_index([5, 150])                                  # 150 is gone: nothing changes
    assert ivf.count() == 2900
    compare(3)


def test_plugin_kth_distance_never_grows_with_nprobe_and_the_warning():
    vecs = _plugin_data(np.float32)
    ivf = HipIvfFlatNearestNeighborsIndex(nlist=32, nprobe=1, train_iters=5, random_seed=4)
    ivf.build_index(_descriptors(vecs))
    rng = np.random.default_rng(5)
    queries = np.vstack([vecs[:20] + np.float32(0.02), rng.standard_normal((20, 16)).astype(np.float32) * 3])
    last = None
    for nprobe in (1, 4, 16, 32):                                        # nested candidate sets
        ivf.nprobe = nprobe
        idx, dist = ivf.nn_many(queries, 25)
        assert ((idx >= 0) == np.isfinite(dist)).all()
        if last is not None:
            assert (dist[:, -1] <= last).all(), nprobe
        last = dist[:, -1]
    bf = HipBruteForceNearestNeighborsIndex()
    bf.build_index(_descriptors(vecs))
    bi, bd = bf.nn_many(queries, 25)
    np.testing.assert_array_equal(idx, bi)
    np.testing.assert_array_equal(_bits(dist), _bits(bd))
    # one list cannot hold all 3000 rows: fewer than n come back, with the reference's warning
    ivf.nprobe = 1
    q = _descriptors(vecs[:1], start=20_000)[0]
    with pytest.warns(RuntimeWarning, match="nprobe"):
        elems, dists = ivf.nn(q, 3000)
    assert 0 < len(elems) == len(dists) < 3000 and list(dists) == sorted(dists) and elems[0].uuid() == 0
