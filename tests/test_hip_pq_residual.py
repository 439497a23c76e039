"""
GPU tests of the IVF-PQ index's residual mode (`sq_pq_create_residual`, `sq_pq_residuals`, `_lib.PqIndex(...,
residual=True)`, `_lib.pq_residuals`, `HipIvfPqResidualNearestNeighborsIndex`).

Every answer is compared with the numpy restatement of tests/pq_residual_cases.py (list, residual, code, one table set
per query and probed list, left-to-right distance, result), ids exactly and distances in float32 bits; the cases'
preconditions are proven on the CPU by tests/test_pq_residual_cases_cpu.py.  The restatement of a case is computed once
and shared by the tests here.  Nothing here skips when the library is missing: the first call fails.
"""
import warnings

import numpy as np
import pytest

from oracle import cpu_ref as O
from smqtk_indexing_amd import _lib
from smqtk_indexing_amd._compat import DescriptorMemoryElement
from smqtk_indexing_amd.impls.nn_index.hip_ivf_pq_residual import HipIvfPqResidualNearestNeighborsIndex
from tests import pq_cases as C
from tests import pq_residual_cases as R

pytestmark = pytest.mark.gpu

NPROBES = (1, 3, 8, 100)         # 100 clamps to nlist = 8
KS = (1, 10, 5000)               # 5000 is beyond the 3001 rows: padding
M_LIST = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 33, 64)
DSUBS = (1, 4, 129, 8193, 16384)
_indexes = {}


@pytest.fixture(scope="module", autouse=True)
def _close_the_shared_indexes():
    yield
    for idx in _indexes.values():
        idx.close()
    _indexes.clear()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _index(d, m, ksub=C.KSUB):
    """The main case's residual index, built once: one add of all rows."""
    key = (d, m, ksub)
    if key not in _indexes:
        case = R.make_case(d, m, ksub)
        idx = _lib.PqIndex(case.centroids, case.codebooks, residual=True)
        idx.add(case.x)
        _indexes[key] = idx
    return _indexes[key]


def _same(got_dist, got_idx, want_idx, want_dist, what):
    np.testing.assert_array_equal(got_idx, want_idx, err_msg=what)
    np.testing.assert_array_equal(_bits(got_dist), _bits(want_dist), err_msg=what)


def _stride(m):
    return -(-m // 4) * 4


def _lists_equal(idx, case, what=""):
    off, ids, codes = idx.lists()
    np.testing.assert_array_equal(off, case.off, err_msg=what)
    np.testing.assert_array_equal(ids, case.order, err_msg=what)
    assert codes.dtype == np.uint8 and codes.shape == (case.n, case.m)
    np.testing.assert_array_equal(codes, case.codes_by_list(), err_msg=what)


# ------------------------------------------------------------------------------------ the main case
@pytest.mark.parametrize("d,m", R.SHAPES)
def test_codes_and_lists_equal_the_restatement(d, m):
    case, idx = R.make_case(d, m), _index(d, m)
    _lists_equal(idx, case)
    assert idx.residual and idx.info()["rows"] == C.N and idx.info()["codes_bytes"] == C.N * _stride(m)


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("nq", [1, 33])
@pytest.mark.parametrize("nprobe", NPROBES)
@pytest.mark.parametrize("d,m", R.SHAPES)
def test_search_equals_the_restatement(d, m, nprobe, nq, mem):
    """The first nq pool queries -- x[7] (41 rows share every code), the query at the far centroid (its first list is
    empty), the zero vector (the zero-centroid list of more than 1024 rows), the query at the list of 5 rows, then
    random ones -- for every k, from host and from device memory."""
    case, idx = R.make_case(d, m), _index(d, m)
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
            dist, ids = od.cpu().numpy(), oi.cpu().numpy()
            assert not (ids == -77).any() and not (dist == -3.0).any(), "a sentinel survived"
        _same(dist, ids, want_idx, want_dist, f"d={d} m={m} nprobe={nprobe} nq={nq} k={k} {mem}")
        if k == 5000:
            assert (ids[:, -1] == -1).all() and np.isposinf(dist[:, -1]).all()
    st = idx.stats()
    counts = [case.count(qi, nprobe) for qi in range(nq)]
    assert st["candidates"] == sum(counts) and st["bytes_scanned"] == sum(counts) * _stride(m)
    assert st["scan_launches"] == R.res_plan(nq, min(nprobe, C.NLIST), max(counts), KS[-1], m, C.KSUB)[2] == (1 if sum(counts) else 0)
    if nprobe == 1 and nq == 1:                                          # (e) the tie group, by id
        assert ids[0, :41].tolist() == [7] + list(range(100, 140)) and (dist[0, :41] == dist[0, 0]).all()


def test_id_base_the_empty_index_and_the_overflowing_query():
    d, m = 32, 8
    case = R.make_case(d, m)
    with _lib.PqIndex(case.centroids, case.codebooks, id_base=R.ID_BASE, residual=True) as idx:
        dist, ids = idx.search(case.pool[:3], 5, 4)                       # an empty index: padding only
        assert (ids == -1).all() and np.isposinf(dist).all() and idx.stats()["scan_launches"] == 0
        off, ids_l, codes = idx.lists()
        assert not off.any() and ids_l.shape == (0,) and codes.shape == (0, m) and idx.info()["codes_bytes"] == 0
        idx.add(case.x)
        for nprobe, k in ((1, 10), (3, 10), (8, 5000)):
            dist, ids = idx.search(case.pool, k, nprobe)
            _same(dist, ids, *case.expected(C.POOL, nprobe, k, id_base=R.ID_BASE), f"id_base nprobe={nprobe} k={k}")
        assert (ids[:, C.N:] == -1).all() and (ids[:, :C.N] >= R.ID_BASE).all()
        np.testing.assert_array_equal(idx.lists()[1], case.order + R.ID_BASE)
        dist, ids = idx.search(case.pool[C.Q_FAR], 10, 1)                 # a probe of the empty list alone
        assert (ids == -1).all() and np.isposinf(dist).all() and idx.stats()["candidates"] == 0
        # 1e30 everywhere: every distance is +inf, the real ids ascend, -1 only behind the last candidate
        q = R.huge_query(d)
        for nprobe in (3, 8):
            with np.errstate(over="ignore", invalid="ignore"):
                want = case.answer_of(q, nprobe)
            cands = want[0].shape[0]
            for k in (10, C.N + 3):
                dist, ids = idx.search(q, k, nprobe)
                oi, od = C.pad(*want, k, R.ID_BASE)
                _same(dist[0], ids[0], oi, od, f"overflowing query nprobe={nprobe} k={k}")
                n_real = min(k, cands)
                assert np.isposinf(dist).all() and (np.diff(ids[0, :n_real]) > 0).all() and (ids[0, :n_real] >= R.ID_BASE).all()
                assert (ids[0, cands:] == -1).all()


@pytest.mark.parametrize("d,m", [(32, 8), (12, 12), (516, 4)])
def test_three_adds_are_one_add(d, m):
    case, one = R.make_case(d, m), _index(d, m)
    with _lib.PqIndex(case.centroids, case.codebooks, residual=True) as idx:
        for lo, hi in ((0, 1), (1, 1201), (1201, C.N)):
            idx.add(case.x[lo:hi])
            for got, want in zip(idx.lists(), case.lists_after(hi)):
                np.testing.assert_array_equal(got, want, err_msg=f"after {hi} rows")
        for a, b in zip(idx.lists(), one.lists()):
            np.testing.assert_array_equal(a, b)
        dist, ids = idx.search(case.pool, 10, 3)
        _same(dist, ids, *case.expected(C.POOL, 3, 10), f"d={d} m={m} after three adds")
        assert idx.info() == {**one.info(), "add_us": idx.info()["add_us"]}


def test_info_counts_the_device_centroids():
    """Word 7 of sq_pq_info: what a plain index over the same centroids and codebooks reports, and the residual handle's
    copy of the centroids, [nlist][round_up(d, 4)] float32."""
    for d, m in ((32, 8), (12, 12)):
        case = R.make_case(d, m)
        with _lib.PqIndex(case.centroids, case.codebooks) as plain:
            want = plain.info()["books_coarse_bytes"] + C.NLIST * (-(-d // 4) * 4) * 4
        assert _index(d, m).info()["books_coarse_bytes"] == want
    rng = np.random.default_rng(2)
    cent, books = rng.standard_normal((3, 35)).astype(np.float32), rng.standard_normal((5, 4, 7)).astype(np.float32)
    with _lib.PqIndex(cent, books) as plain, _lib.PqIndex(cent, books, residual=True) as res:
        assert res.info()["books_coarse_bytes"] - plain.info()["books_coarse_bytes"] == 3 * 36 * 4
        assert len(res.info()) == _lib.SQ_PQ_INFO_FIELDS == 10


# ------------------------------------------------------------------------------------ the scan's stride loop
@pytest.mark.parametrize("nq", R.S_NQS)
@pytest.mark.parametrize("d,m", R.S_SHAPES)
def test_strided_scan(d, m, nq):
    """pq_scan_res_kernel's loop over chunks g, g + groups, ...: a list of 8100 rows (32 chunks, the last one partial)
    beside a 5-row list and an empty list, three lists probed.  600 queries: groups = ceil(chunks / 16) = 2, every
    workgroup of the long list walks 16 chunks; 64 queries: two workgroups per compute unit, 3 groups.  Every chunk of the
    long list holds one of some query's 100 results (proven on the CPU), so a chunk left out changes an answer.  The
    index is fresh and this is its first search: no earlier call has left keys in its scratch."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case = R.make_strided_case(d, m)
    queries, qis = R.strided_queries(case, nq)
    plan = R.strided_plan(case, nq, cus)
    what = f"d={d} m={m} nq={nq} on {cus} compute units"
    R.assert_regime(plan, nq, what)                                      # (a partitioned device says so here)
    with _lib.PqIndex(case.centroids, case.codebooks, residual=True) as idx:
        idx.add(case.x)
        _lists_equal(idx, case, what)
        dist, ids = idx.search(queries, R.S_K, R.S_NPROBE)
        _same(dist, ids, *case.expected(qis, R.S_NPROBE, R.S_K), what)
        st = idx.stats()
        cands = sum(case.count(qi, R.S_NPROBE) for qi in qis)
        assert st["candidates"] == cands and st["bytes_scanned"] == cands * _stride(m) and st["scan_launches"] == 1


# ------------------------------------------------------------------------------------ pair ranges
@pytest.mark.parametrize("nq", [3, 5])
def test_pair_ranges_under_a_small_budget(nq):
    """64 KiB of tables per pair (m = 64, ksub = 256), 8 lists probed, 1 MiB of key budget: what the budget leaves beside
    the slice's keys holds 14 pairs' tables, so the 24 (40) pairs go in 2 (3) ranges and a range boundary falls inside a
    query.  scan_launches is the plan's count; the answers are the bits of the default budget's one launch."""
    d, m, ksub = C.LDS_SHAPE
    case, idx = R.make_case(d, m, ksub), _index(d, m, ksub)
    _lists_equal(idx, case)
    qis = list(range(R.RANGE_Q0, R.RANGE_Q0 + nq))                       # pool queries whose range boundaries fall on lists with rows
    queries, other = case.pool[qis], case.pool[R.RANGE_OTHER:R.RANGE_OTHER + nq]
    for k in (10, 5000):
        want_idx, want_dist = case.expected(qis, 8, k)
        idx.set_option("ivf_key_budget_mb", 1)
        try:
            slice_, ppl, launches = R.res_plan(nq, 8, C.N, k, m, ksub, 1 << 20)
            starts = R.range_starts(nq, 8, ppl)
            assert slice_ == nq and launches == len(starts) >= 2 and any(pos for _, pos in starts[1:])
            assert k != 10 or launches == (2 if nq == 3 else 3)
            for ql, pos in starts[1:]:                                   # a range begins at a list with rows: a pair lost there is rows lost
                assert case.rows_of(R.probe(case.centroids, queries[ql], 8)[pos]).shape[0] > 0
            # other queries first: the key scratch then holds THEIR keys, so a pair that no launch scans leaves wrong keys
            # behind, not the keys an earlier search of the same queries wrote
            idx.search(other, k, 8)
            dist, ids = idx.search(queries, k, 8)
            assert idx.stats()["scan_launches"] == launches
            _same(dist, ids, want_idx, want_dist, f"nq={nq} k={k}, {launches} ranges of {ppl} pairs")
        finally:
            idx.reset_options()
        idx.search(other, k, 8)
        dist1, ids1 = idx.search(queries, k, 8)
        assert idx.stats()["scan_launches"] == 1
        _same(dist1, ids1, want_idx, want_dist, f"nq={nq} k={k}, one launch")
    dist, ids = idx.search(case.pool, 10, 3)                             # all 33 queries, three lists
    _same(dist, ids, *case.expected(C.POOL, 3, 10), "64 KiB of tables, nprobe 3")


# ------------------------------------------------------------------------------------ widths
def _recoded_checks(case, idx, nprobes, ks, npool, what):
    _lists_equal(idx, case, what)
    for nprobe in nprobes:
        for k in ks:
            dist, ids = idx.search(case.pool, k, nprobe)
            _same(dist, ids, *case.expected(npool, nprobe, k), f"{what} nprobe={nprobe} k={k}")
        cands = sum(case.count(qi, nprobe) for qi in range(npool))
        assert idx.stats()["candidates"] == cands and idx.stats()["bytes_scanned"] == cands * _stride(case.m)


@pytest.mark.parametrize("ksub", C.M_KSUBS)
@pytest.mark.parametrize("m", M_LIST)
def test_code_widths(m, ksub):
    """Code strides of 1 to 16 dwords with 0 to 3 padding bytes, both loads, both ways of staging the tables (dsub = 2);
    two adds split at an odd row; all 1049 distances of every query compared at k = 1049."""
    case = R.from_plain(C.make_m_case(m, ksub))
    with _lib.PqIndex(case.centroids, case.codebooks, residual=True) as idx:
        idx.add(case.x[:C.M_SPLIT])
        for got, want in zip(idx.lists(), case.lists_after(C.M_SPLIT)):
            np.testing.assert_array_equal(got, want, err_msg=case.what + " after the first add")
        idx.add(case.x[C.M_SPLIT:])
        _recoded_checks(case, idx, C.M_NPROBES, C.M_KS, C.M_POOL, f"m={m} ksub={ksub}")


@pytest.mark.parametrize("dsub", DSUBS)
def test_sub_vector_widths(dsub):
    """pq_tables_res_kernel at m = 3: sub-vectors of the query and of the centroid from offsets dsub and 2 dsub (unaligned
    for odd dsub), rq staged in up to 65 536 bytes of LDS, summed in numpy's order; all 300 distances compared."""
    case = R.from_plain(C.make_dsub_case(dsub))
    with _lib.PqIndex(case.centroids, case.codebooks, residual=True) as idx:
        idx.add(case.x)
        _recoded_checks(case, idx, (C.D_NLIST,), (C.D_N,), C.D_POOL, f"dsub={dsub}")


# ------------------------------------------------------------------------------------ sq_pq_residuals
@pytest.mark.parametrize("d,m", [(32, 8), (516, 4)])
def test_residuals_in_host_memory(d, m):
    case = R.make_case(d, m)
    got = _lib.pq_residuals(case.x, case.centroids)
    assert got.dtype == np.float32 and got.shape == case.x.shape
    np.testing.assert_array_equal(_bits(got), _bits(case.x - case.centroids[case.assignment]))
    np.testing.assert_array_equal(_bits(got), _bits(case.res))
    np.testing.assert_array_equal(_bits(_lib.pq_residuals(case.x[:1], case.centroids)), _bits(case.res[:1]))


def test_residuals_in_device_memory_from_an_unaligned_base():
    """d = 35 from a base 4 bytes into an allocation; the output to a second buffer and then in place."""
    import torch
    m, ksub, dsub = C.M_DEVICE
    case = R.from_plain(C.make_m_case(m, ksub, dsub))
    dev = torch.device("cuda:0")
    flat = torch.zeros(case.n * case.d + 1, dtype=torch.float32, device=dev)
    flat[1:].copy_(torch.from_numpy(np.array(case.x)).reshape(-1))
    out = torch.full((case.n * case.d + 2,), -5.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    assert flat.data_ptr() % 16 == 0 and case.d == 35
    _lib.pq_residuals_device(flat.data_ptr() + 4, case.n, case.d, case.centroids, out.data_ptr() + 4)
    got = out.cpu().numpy()
    assert got[0] == -5.0 and got[-1] == -5.0                             # nothing written outside [n, d]
    np.testing.assert_array_equal(_bits(got[1:-1].reshape(case.n, case.d)), _bits(case.res))
    _lib.pq_residuals_device(flat.data_ptr() + 4, case.n, case.d, case.centroids, flat.data_ptr() + 4)
    got = flat.cpu().numpy()
    assert got[0] == 0.0
    np.testing.assert_array_equal(_bits(got[1:].reshape(case.n, case.d)), _bits(case.res))
    # ... and rows added to a residual index from that base (m = 1: no 2-D copy, the residual buffer goes to the codebook's index)
    flat[1:].copy_(torch.from_numpy(np.array(case.x)).reshape(-1))
    torch.cuda.synchronize()
    with _lib.PqIndex(case.centroids, case.codebooks, residual=True) as idx:
        idx.add(flat.data_ptr() + 4, n=C.M_SPLIT, device_ptr=True)
        idx.add(flat.data_ptr() + 4 + C.M_SPLIT * case.d * 4, n=case.n - C.M_SPLIT, device_ptr=True)
        _recoded_checks(case, idx, (1, 8), (10, C.M_N), C.M_POOL, "m=1 d=35 device rows")


# ------------------------------------------------------------------------------------ against the plain index
@pytest.mark.parametrize("m,ksub", [(5, 13), (16, 16)])
def test_one_list_with_a_zero_centroid_is_the_plain_index(m, ksub):
    """nlist = 1 and a zero centroid: residuals are the rows and rq is q, so the residual index answers with the bits of
    the plain index, which is code of the parent commit."""
    plain = C.make_m_case(m, ksub)
    zero = np.zeros((1, plain.d), np.float32)
    with _lib.PqIndex(zero, plain.codebooks) as a, _lib.PqIndex(zero, plain.codebooks, residual=True) as b:
        a.add(plain.x)
        b.add(plain.x)
        for x, y in zip(a.lists(), b.lists()):
            np.testing.assert_array_equal(x, y)
        for k in (1, 10, C.M_N + 3):
            da, ia = a.search(plain.pool, k, 1)
            db, ib = b.search(plain.pool, k, 1)
            _same(db, ib, ia, da, f"m={m} ksub={ksub} k={k}")


def test_option_profile_changes_no_bit():
    case = R.from_plain(C.make_m_case(5, 13))
    with _lib.PqIndex(case.centroids, case.codebooks, residual=True) as idx:
        idx.add(case.x)
        calls = ((3, 10), (8, C.M_N))
        base = [idx.search(case.pool, k, nprobe) for nprobe, k in calls]
        for (nprobe, k), (dist, ids) in zip(calls, base):
            _same(dist, ids, *case.expected(C.M_POOL, nprobe, k), f"nprobe={nprobe} k={k}")
        assert idx.stats()["scan_ms"] == 0
        for mode in (1, 2):                                              # 2 behaves as 1
            idx.set_option("profile", mode)
            for (nprobe, k), (dist0, ids0) in zip(calls, base):
                dist, ids = idx.search(case.pool, k, nprobe)
                _same(dist, ids, ids0, dist0, f"profile={mode} nprobe={nprobe} k={k}")
                st = idx.stats()
                assert st["scan_ms"] > 0 and st["rerank_ms"] > 0 and st["scan_launches"] == 1 and st["total_ms"] > 0
        idx.set_option("ivf_key_budget_mb", 1)                           # a budget option beside the profile option
        dist, ids = idx.search(case.pool, C.M_N, 8)
        _same(dist, ids, base[1][1], base[1][0], "profile with a small budget")
        idx.reset_options()
        dist, ids = idx.search(case.pool, C.M_N, 8)
        _same(dist, ids, base[1][1], base[1][0], "after reset_options")
        assert idx.stats()["scan_ms"] == 0


# ------------------------------------------------------------------------------------ the recall case
def test_recall_case_bits():
    """The small clustered set on which residual codes find 1.5 times the plain codes' true neighbours (asserted on the
    CPU): here only the bits are compared."""
    case, _, r_res, r_plain = R.make_recall_case()
    with _lib.PqIndex(case.centroids, case.codebooks, residual=True) as idx:
        idx.add(case.x)
        _lists_equal(idx, case)
        for nprobe, k in ((R.R_NLIST, 10), (2, 100)):
            dist, ids = idx.search(case.pool, k, nprobe)
            _same(dist, ids, *case.expected(R.R_NQ, nprobe, k), f"recall case nprobe={nprobe} k={k}")


# ------------------------------------------------------------------------------------ the plugin class
def _descriptors(vecs, start=0):
    out = []
    for i, v in enumerate(vecs):
        e = DescriptorMemoryElement(start + i)
        e.set_vector(v)
        out.append(e)
    return out


def _check_nn(index, vecs_by_uuid, q, n):
    """`nn` re-ranks as the parent does: elements of the index with metrics.euclidean_distance of their ORIGINAL vectors
    to the float32 query, ascending."""
    elems, dists = index.nn(q, n)
    assert len(elems) == len(dists) == n and len({e.uuid() for e in elems}) == n
    q32 = np.asarray(q.vector()).astype(np.float32)
    for e, dv in zip(elems, dists):
        v = np.asarray(vecs_by_uuid[e.uuid()])
        assert np.array_equal(e.vector(), v) and dv == float(O.euclidean_distance(v, q32))
    assert list(dists) == sorted(dists)
    return elems, dists


def test_plugin_build_update_replace_remove_nn():
    case, _, _, _ = R.make_recall_case()
    vecs = np.array(case.x)
    descr = _descriptors(vecs)
    by_uuid = {i: vecs[i] for i in range(R.R_N)}
    pq = HipIvfPqResidualNearestNeighborsIndex(nlist=8, nprobe=8, m=8, train_iters=4, random_seed=4)
    pq.build_index(descr[:2000])
    try:
        dev = pq._dev
        assert dev.residual and dev.info()["rows"] == 2000 and dev.info()["ksub"] == 256
        # the codebooks are pq_train over pq_residuals of the training sample, from the residuals of the same draw
        sample, init, entries = pq.training_plan(2000)
        train = vecs[:2000][sample]
        cent = _lib.ivf_kmeans(train, train[init], 4)
        np.testing.assert_array_equal(_bits(pq._centroids), _bits(cent))
        res = _lib.pq_residuals(train, cent)
        books0 = np.ascontiguousarray(res[entries].reshape(len(entries), 8, 4).transpose(1, 0, 2))
        np.testing.assert_array_equal(_bits(pq._codebooks), _bits(_lib.pq_train(res, books0, 4)))
        assert not np.array_equal(pq._codebooks, _lib.pq_train(train, np.ascontiguousarray(train[entries].reshape(len(entries), 8, 4).transpose(1, 0, 2)), 4))
        pq.update_index(descr[2000:])                                    # joins the existing lists: the same device index
        assert pq.count() == R.R_N and pq._dev is dev and dev.info()["rows"] == R.R_N
        queries = _descriptors(np.vstack([vecs[7], vecs[2500] + np.float32(0.01), np.zeros(R.R_D, np.float32)]), start=10_000)
        with warnings.catch_warnings():
            warnings.simplefilter("error")                               # every list probed: n neighbours come back
            for q in queries:
                _check_nn(pq, by_uuid, q, 1)
                _check_nn(pq, by_uuid, q, 50)
            elems, _ = _check_nn(pq, by_uuid, descr[2500], 20)
            assert 2500 in [e.uuid() for e in elems]
        # nn_many: the device's coded answer, the bits of a residual index over the same training
        idx, dist = pq.nn_many(vecs[:5], 25)
        with _lib.PqIndex(pq._centroids, pq._codebooks, residual=True) as ref:
            ref.add(vecs)
            rd, ri = ref.search(vecs[:5], 25, 8)
        _same(dist, idx, ri, rd, "nn_many")
        # a replaced uuid and a removal: the lists are coded again with the same centroids and codebooks
        cent0, books = pq._centroids.copy(), pq._codebooks.copy()
        moved = DescriptorMemoryElement(7)
        moved.set_vector(vecs[7] + np.float32(0.5))
        by_uuid[7] = moved.vector()
        pq.update_index([moved])
        pq.remove_from_index(list(range(100, 200)))
        assert pq.count() == R.R_N - 100 and pq._dev is not dev and pq._dev.residual and pq._dev.info()["rows"] == R.R_N - 100
        assert np.array_equal(pq._centroids, cent0) and np.array_equal(pq._codebooks, books)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            elems, _ = _check_nn(pq, by_uuid, moved, 30)
            assert elems[0].uuid() == 7
            for q in queries:
                got, _ = _check_nn(pq, by_uuid, q, 50)
                assert not {e.uuid() for e in got} & set(range(100, 200))
        with pytest.raises(KeyError):
            pq.remove_from_index([5, 150])
        assert pq.count() == R.R_N - 100
    finally:
        if pq._dev is not None:
            pq._dev.close()
