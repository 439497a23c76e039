"""
GPU tests of the IVF-PQ index (`sq_pq_*`, `_lib.PqIndex`, `_lib.pq_train`, `HipIvfPqNearestNeighborsIndex`).

Every answer is compared with the numpy restatement of tests/pq_cases.py (list, code, tables, left-to-right distance and
result over `oracle.cpu_ref`), ids exactly and distances in float32 bits; the cases' preconditions -- a table sum in
another order changes a compared distance, the 41-way tie, the duplicated codebook entry, two empty lists, a list longer
than 1024 rows, a list of 5 rows; for the strided scan a result in every chunk, for every m and every sub-vector width a
sum in another order that shows in the bits -- are proven on the CPU by tests/test_pq_cases_cpu.py.  The restatement of
a case is computed once and shared by all tests here.  Nothing here skips when the library is missing: the first call
fails.
"""
import warnings

import numpy as np
import pytest

from oracle import cpu_ref as O
from smqtk_indexing_amd import _lib
from smqtk_indexing_amd._compat import DescriptorMemoryElement
from smqtk_indexing_amd.impls.nn_index.hip_ivf_pq import HipIvfPqNearestNeighborsIndex
from tests import pq_cases as C
from tests import width_cases as W

pytestmark = pytest.mark.gpu

NPROBES = (1, 3, 8, 100)         # 100 clamps to nlist = 8
KS = (1, 10, 5000)               # 5000 is beyond the 3001 rows: padding
ALL = [(d, m, C.KSUB) for d, m in C.SHAPES] + [(*C.KSUB_SHAPE, ksub) for ksub in C.KSUBS]
_indexes = {}


@pytest.fixture(scope="module", autouse=True)
def _close_the_shared_indexes():
    """The indexes `_index` builds are shared by the tests of this module and closed when the module is done."""
    yield
    for idx in _indexes.values():
        idx.close()
    _indexes.clear()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _index(d, m, ksub=C.KSUB):
    """The case's index, built once: one add of all rows."""
    key = (d, m, ksub)
    if key not in _indexes:
        case = C.make_case(d, m, ksub)
        idx = _lib.PqIndex(case.centroids, case.codebooks)
        idx.add(case.x)
        _indexes[key] = idx
    return _indexes[key]


def _same(got_dist, got_idx, want_idx, want_dist, what):
    np.testing.assert_array_equal(got_idx, want_idx, err_msg=what)
    np.testing.assert_array_equal(_bits(got_dist), _bits(want_dist), err_msg=what)


def _stride(m):
    return -(-m // 4) * 4


# ------------------------------------------------------------------------------------ codes and lists
@pytest.mark.parametrize("d,m,ksub", ALL)
def test_codes_and_lists_equal_the_restatement(d, m, ksub):
    case, idx = C.make_case(d, m, ksub), _index(d, m, ksub)
    off, ids, codes = idx.lists()
    np.testing.assert_array_equal(off, case.off)
    np.testing.assert_array_equal(ids, case.order)                      # list-major, ascending inside a list
    assert codes.dtype == np.uint8 and codes.shape == (C.N, m)
    np.testing.assert_array_equal(codes, case.codes_by_list())
    if ksub > C.DUP_HI:                                                  # the duplicated entry: the lower one wins
        col = codes[:, C.DUP_J]
        assert (col == C.DUP_LO).any() and not (col == C.DUP_HI).any()


# ------------------------------------------------------------------------------------ search
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("nq", [1, 33])
@pytest.mark.parametrize("nprobe", NPROBES)
@pytest.mark.parametrize("d,m", C.SHAPES)
def test_search_equals_the_restatement(d, m, nprobe, nq, mem):
    """The first nq pool queries -- x[7] (41 rows share every code), the query at the far centroid (its first list is
    empty), the zero vector (the list of more than 1024 rows), the query at the list of 5 rows, then random ones -- for
    every k, from host and from device memory."""
    case, idx = C.make_case(d, m), _index(d, m)
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
        _same(dist, ids, want_idx, want_dist, f"d={d} m={m} nprobe={nprobe} nq={nq} k={k} {mem}")
        if k == 5000:
            assert (ids[:, -1] == -1).all() and np.isposinf(dist[:, -1]).all()
    st = idx.stats()
    cands = sum(case.answer(qi, nprobe)[0].shape[0] for qi in range(nq))
    assert st["candidates"] == cands and st["bytes_scanned"] == cands * _stride(m)
    assert st["scan_launches"] == (1 if cands else 0)
    if nprobe == 1 and nq == 1:                                          # the tie group, by id
        assert ids[0, :41].tolist() == [7] + list(range(100, 140)) and (dist[0, :41] == dist[0, 0]).all()


@pytest.mark.parametrize("ksub", C.KSUBS)
def test_search_at_other_codebook_sizes(ksub):
    d, m = C.KSUB_SHAPE
    case, idx = C.make_case(d, m, ksub), _index(d, m, ksub)
    for nprobe, k in ((1, 10), (3, 1), (8, 5000)):
        dist, ids = idx.search(case.pool, k, nprobe)
        _same(dist, ids, *case.expected(C.POOL, nprobe, k), f"ksub={ksub} nprobe={nprobe} k={k}")


def test_id_base_and_the_empty_cases():
    d, m = C.KSUB_SHAPE
    case = C.make_case(d, m)
    with _lib.PqIndex(case.centroids, case.codebooks, id_base=1000) as idx:
        # an empty index: padding only
        dist, ids = idx.search(case.pool[:3], 5, 4)
        assert (ids == -1).all() and np.isposinf(dist).all() and idx.stats()["scan_launches"] == 0
        assert idx.info()["rows"] == 0 and idx.info()["codes_bytes"] == 0
        off, ids_l, codes = idx.lists()
        assert not off.any() and ids_l.shape == (0,) and codes.shape == (0, m)
        idx.add(case.x)
        for nprobe, k in ((1, 10), (3, 10), (8, 5000)):
            dist, ids = idx.search(case.pool, k, nprobe)
            _same(dist, ids, *case.expected(C.POOL, nprobe, k, id_base=1000), f"id_base nprobe={nprobe} k={k}")
        # a probe of the empty list alone
        dist, ids = idx.search(case.pool[C.Q_FAR], 10, 1)
        assert (ids == -1).all() and np.isposinf(dist).all() and idx.stats()["candidates"] == 0
        # the list of 5 rows alone: shorter than k
        dist, ids = idx.search(case.pool[C.Q_SMALL], 10, 1)
        assert sorted(ids[0, :C.SMALL_ROWS].tolist()) == [1000 + r for r in range(C.SMALL_AT, C.SMALL_AT + C.SMALL_ROWS)]
        assert (ids[0, C.SMALL_ROWS:] == -1).all() and np.isposinf(dist[0, C.SMALL_ROWS:]).all()
        _, ids_l, _ = idx.lists()
        np.testing.assert_array_equal(ids_l, case.order + 1000)


# ------------------------------------------------------------------------------------ add
@pytest.mark.parametrize("d,m", [(32, 8), (12, 12), (516, 4)])
def test_three_adds_are_one_add(d, m):
    case, one = C.make_case(d, m), _index(d, m)
    with _lib.PqIndex(case.centroids, case.codebooks) as idx:
        for lo, hi in ((0, 1), (1, 1201), (1201, C.N)):
            idx.add(case.x[lo:hi])
        for a, b in zip(idx.lists(), one.lists()):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(idx.lists()[2], case.codes_by_list())
        dist, ids = idx.search(case.pool, 10, 3)
        _same(dist, ids, *case.expected(C.POOL, 3, 10), f"d={d} m={m} after three adds")
        assert idx.info() == {**one.info(), "add_us": idx.info()["add_us"]} and idx.info()["add_us"] > 0


def test_rows_added_from_device_memory():
    torch = pytest.importorskip("torch")
    d, m = C.KSUB_SHAPE
    case = C.make_case(d, m)
    x_t = torch.from_numpy(np.array(case.x)).to(torch.device("cuda:0"))
    torch.cuda.synchronize()
    with _lib.PqIndex(case.centroids, case.codebooks) as idx:
        idx.add(x_t.data_ptr(), n=C.N, device_ptr=True)
        for a, b in zip(idx.lists(), _index(d, m).lists()):
            np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------------------------ info
@pytest.mark.parametrize("d,m,ksub", [(32, 8, 64), (12, 12, 64), (512, 64, 64), (32, 8, 3)])
def test_info_is_the_layout(d, m, ksub):
    """The footprint follows from the layout.  Per row: round_up(m, 4) code bytes and a 4-byte insertion number; 8 bytes per
    list offset.  Codebooks and coarse index do not grow with the rows and are what include/smqtk_hip.h's sq_dense_info
    reports for m + 1 dense L2 indexes without scan copies -- float32 rows at round_up(width, 4) floats, and the row
    statistics of the dense layout: two float32 per row padded to tiles of 32 rows and the origin of round_up(width, 128)
    floats, each in a growable block of b + b / 8 + 256 bytes -- plus the padded copy of the codebooks the tables kernel
    reads, m * ksub entries of round_up(dsub, 4) floats."""
    case, idx = C.make_case(d, m, ksub), _index(d, m, ksub)
    info = idx.info()
    assert (info["rows"], info["d"], info["nlist"], info["m"], info["ksub"]) == (C.N, d, C.NLIST, m, ksub)
    assert info["codes_bytes"] == C.N * _stride(m)
    assert info["ids_offsets_bytes"] == C.N * 4 + (C.NLIST + 1) * 8
    up = lambda v, a: -(-v // a) * a
    block = lambda b: b + b // 8 + 256

    def dense_bytes(rows, width):
        return rows * up(width, 4) * 4 + 2 * block(up(rows, 32) * 4) + block(up(width, 128) * 4)

    dsub = d // m
    assert info["books_coarse_bytes"] == dense_bytes(C.NLIST, d) + m * dense_bytes(ksub, dsub) + m * ksub * up(dsub, 4) * 4
    assert info["key_budget_bytes"] == 256 << 20 and info["add_us"] > 0
    with _lib.PqIndex(case.centroids, case.codebooks) as empty:
        assert empty.info()["books_coarse_bytes"] == info["books_coarse_bytes"]
        assert empty.info()["ids_offsets_bytes"] == (C.NLIST + 1) * 8
    # against the float32 matrix: (m + 4) / (4 d) of it at m % 4 == 0
    assert info["codes_bytes"] + C.N * 4 == C.N * (_stride(m) + 4)


# ------------------------------------------------------------------------------------ training
@pytest.mark.parametrize("d,m", [(4, 4), (32, 8), (516, 4)])
def test_training_is_kmeans_per_sub_matrix(d, m):
    """dsub = 1, 4 and 129: codebook j is `_lib.ivf_kmeans` over the contiguous copy of x[:, j dsub:(j+1) dsub], bit for
    bit, and two runs are equal."""
    dsub, ksub, iters = d // m, 16, 3
    assert dsub in (1, 4, 129)
    rng = np.random.default_rng([11, d, m])
    x = rng.standard_normal((C.N, d)).astype(np.float32)
    books0 = np.ascontiguousarray(x[rng.choice(C.N, ksub, replace=False)].reshape(ksub, m, dsub).transpose(1, 0, 2))
    got, again = _lib.pq_train(x, books0, iters), _lib.pq_train(x, books0, iters)
    assert got.shape == (m, ksub, dsub) and got.dtype == np.float32
    np.testing.assert_array_equal(_bits(got), _bits(again))
    for j in range(m):
        want = _lib.ivf_kmeans(np.ascontiguousarray(x[:, j * dsub:(j + 1) * dsub]), books0[j], iters)
        np.testing.assert_array_equal(_bits(got[j]), _bits(want), err_msg=f"codebook {j}")
    assert not np.array_equal(got, books0)
    np.testing.assert_array_equal(_lib.pq_train(x, books0, 0), books0)  # no iteration: the initial entries


# ------------------------------------------------------------------------------------ the slice budget
def test_a_small_key_budget_runs_the_batch_in_slices():
    d, m = C.KSUB_SHAPE
    case = C.make_case(d, m)
    queries = np.ascontiguousarray(np.tile(case.pool, (3, 1))[:C.SLICE_NQ])
    qis = [i % C.POOL for i in range(C.SLICE_NQ)]
    want_idx, want_dist = case.expected(qis, C.NLIST, C.SLICE_K)
    with _lib.PqIndex(case.centroids, case.codebooks) as idx:
        idx.add(case.x)
        dist1, ids1 = idx.search(queries, C.SLICE_K, C.NLIST)
        assert idx.stats()["scan_launches"] == 1
        idx.set_option("ivf_key_budget_mb", C.SLICE_BUDGET_MB)
        assert idx.info()["key_budget_bytes"] == C.SLICE_BUDGET_MB << 20
        dist, ids = idx.search(queries, C.SLICE_K, C.NLIST)
        # every list probed: 3001 candidates per query; (3001 + 10) * 8 bytes of keys and m * ksub * 4 of tables each
        per = (C.N + C.SLICE_K) * 8 + m * C.KSUB * 4
        slices = -(-C.SLICE_NQ // ((C.SLICE_BUDGET_MB << 20) // per))
        assert slices > 1 and idx.stats()["scan_launches"] == slices
        _same(dist, ids, want_idx, want_dist, f"{C.SLICE_NQ} queries in {slices} slices")
        _same(dist, ids, ids1, dist1, "slices against one slice")
        idx.reset_options()
        idx.search(queries, C.SLICE_K, C.NLIST)
        assert idx.stats()["scan_launches"] == 1


# ------------------------------------------------------------------------------------ the scan's stride loop
@pytest.mark.parametrize("nq", C.S_NQS)
@pytest.mark.parametrize("d,m", C.S_SHAPES)
def test_strided_scan(d, m, nq):
    """pq_scan_kernel's loop over chunks blockIdx.x, blockIdx.x + gridDim.x, ...: 12 000 rows, 50 distinct queries tiled
    to 600 (every workgroup walks 16 chunks, the last one fewer) and to 64 (two workgroups per compute unit), with the
    16-byte loads (32, 16) and the dword loads (12, 6).  Every chunk holds one of some query's 100 results (proven on
    the CPU), so a chunk left out or a workgroup that stops early changes an answer.  With three lists probed the
    queries have different candidate counts: the strides end at different trips, and at 64 queries the planted query's
    last workgroups return at entry while the others' walk on.  The index is fresh and these are its first searches;
    three lists come first, so no earlier call of this handle has left the keys of a search in its scratch."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case = C.make_strided_case(d, m)
    queries, qis = C.strided_queries(case, nq)
    with _lib.PqIndex(case.centroids, case.codebooks) as idx:
        idx.add(case.x)
        for nprobe in sorted(C.S_NPROBES):
            plan = C.strided_plan(case, nprobe, nq, cus)
            what = f"d={d} m={m} nq={nq} nprobe={nprobe} on {cus} compute units"
            C.assert_regime(plan, nq, what)                              # (a partitioned device says so here)
            if nprobe == 3 and nq == C.S_NQS[1]:
                assert plan["early"].get(C.S_Q_SHORT) and len(plan["early"]) < C.S_POOL // 2, f"{what}: {plan['early']}"
            else:
                assert not plan["early"], f"{what}: {plan['early']}"
            dist, ids = idx.search(queries, C.S_K, nprobe)
            _same(dist, ids, *case.expected(qis, nprobe, C.S_K), what)
            st = idx.stats()
            cands = sum(plan["counts"][qi] for qi in qis)
            assert st["candidates"] == cands and st["bytes_scanned"] == cands * _stride(m) and st["scan_launches"] == 1


# ------------------------------------------------------------------------------------ every m
def _m_checks(case, idx, what):
    off, ids, codes = idx.lists()
    np.testing.assert_array_equal(off, case.off, err_msg=what)
    np.testing.assert_array_equal(ids, case.order, err_msg=what)
    assert codes.dtype == np.uint8 and codes.shape == (case.n, case.m)
    np.testing.assert_array_equal(codes, case.codes_by_list(), err_msg=what)         # (without the padding bytes)
    assert idx.info()["codes_bytes"] == case.n * _stride(case.m)
    for nprobe in C.M_NPROBES:
        for k in C.M_KS:
            dist, ids = idx.search(case.pool, k, nprobe)
            _same(dist, ids, *case.expected(C.M_POOL, nprobe, k), f"{what} nprobe={nprobe} k={k}")
        cands = sum(case.answer(qi, nprobe)[0].shape[0] for qi in range(C.M_POOL))
        st = idx.stats()
        assert st["candidates"] == cands and st["bytes_scanned"] == cands * _stride(case.m)


def _two_adds(case):
    idx = _lib.PqIndex(case.centroids, case.codebooks)
    try:
        idx.add(case.x[:C.M_SPLIT])
        off, ids, codes = idx.lists()
        for got, want in zip((off, ids, codes), C.lists_after(case, C.M_SPLIT)):
            np.testing.assert_array_equal(got, want, err_msg=case.what + " after the first add")
        idx.add(case.x[C.M_SPLIT:])                                      # moves the first add's rows at this code stride
    except BaseException:
        idx.close()
        raise
    return idx


@pytest.mark.parametrize("ksub", C.M_KSUBS)
@pytest.mark.parametrize("m", range(1, 65))
def test_every_m(m, ksub):
    """Every m from 1 to 64 (dsub = 2), at ksub 13 and 16: code strides of 1 to 16 dwords with 0 to 3 zero bytes behind
    the codes -- `j < m` false in the last dword and in the last 16 bytes --, the dword loop with up to 15 trips and the
    16-byte loop with 1 to 4, the tables staged 16 bytes at a time and one float at a time.  Two adds split at an odd
    row.  All 1049 distances of every query are compared at k = 1049; a pairwise sum of the table entries changes one
    of them exactly when m >= 8 (asserted on the CPU)."""
    case = C.make_m_case(m, ksub)
    with _two_adds(case) as idx:
        _m_checks(case, idx, f"m={m} ksub={ksub}")


@pytest.mark.parametrize("m,ksub", C.M_EXTRA)
def test_one_entry_and_255_entries(m, ksub):
    """ksub = 1 (m = 1 and 5): every code is 0 and every candidate of a query ties, so the answer is the candidates by
    id.  ksub = 255 at m = 5: 1275 table floats, staged one float at a time in five passes of the 256 lanes."""
    case = C.make_m_case(m, ksub)
    with _two_adds(case) as idx:
        _m_checks(case, idx, f"m={m} ksub={ksub}")
        if ksub == 1:
            dist, ids = idx.search(case.pool, 10, 3)
            assert (np.diff(ids, axis=1) > 0).all() and (dist == dist[:, :1]).all()


def test_one_sub_quantiser_with_rows_from_device_memory():
    """m = 1: pq_add_part makes no 2-D copy and hands the caller's rows to the codebook's index as they are -- here
    device rows of 35 floats from a base 4 bytes into an allocation, in two adds."""
    import torch
    m, ksub, dsub = C.M_DEVICE
    case = C.make_m_case(m, ksub, dsub)
    flat = torch.zeros(case.n * case.d + 1, dtype=torch.float32, device=torch.device("cuda:0"))
    flat[1:].copy_(torch.from_numpy(np.array(case.x)).reshape(-1))
    ptr = flat.data_ptr() + 4
    torch.cuda.synchronize()
    assert flat.data_ptr() % 16 == 0 and ptr % 16 == 4 and case.d == 35
    with _lib.PqIndex(case.centroids, case.codebooks) as idx:
        idx.add(ptr, n=C.M_SPLIT, device_ptr=True)
        idx.add(ptr + C.M_SPLIT * case.d * 4, n=case.n - C.M_SPLIT, device_ptr=True)
        _m_checks(case, idx, "m=1 d=35 device rows")


# ------------------------------------------------------------------------------------ every sub-vector width
def _dsub_checks(dsub):
    case = C.make_dsub_case(dsub)
    with _lib.PqIndex(case.centroids, case.codebooks) as idx:
        idx.add(case.x)
        off, ids, codes = idx.lists()
        np.testing.assert_array_equal(off, case.off)
        np.testing.assert_array_equal(ids, case.order)
        np.testing.assert_array_equal(codes, case.codes_by_list())
        dist, ids = idx.search(case.pool, C.D_N, C.D_NLIST)
        _same(dist, ids, *case.expected(C.D_POOL, C.D_NLIST, C.D_N), f"dsub={dsub}")
        assert (np.sort(ids, axis=1) == np.arange(C.D_N)).all()        # every row's distance was compared


@pytest.mark.parametrize("dsub", W.WIDTHS)
def test_tables_at_sub_vector_width(dsub):
    """pq_tables_kernel sums in numpy's order (SqLeafLane over entries padded to a multiple of four floats, the query's
    sub-vectors staged from offsets dsub and 2 dsub, unaligned for odd dsub) at every width where that code branches.
    Every list probed and k = 300: all distances, and so every table entry some row's code selects, are compared;
    tables summed left to right (dsub >= 8) or as one leaf (dsub >= 129) fail here (tests/test_pq_cases_cpu.py)."""
    _dsub_checks(dsub)


@pytest.mark.parametrize("dsub", C.D_BEYOND)
def test_tables_at_sub_vector_width_beyond_numpys_buffer(dsub):
    """Sub-vectors longer than numpy's 8192-element buffer, up to the documented limit of 16384 floats: 65 536 bytes of
    dynamic LDS for the staged sub-vector."""
    _dsub_checks(dsub)


def test_sub_vectors_beyond_the_limit_are_refused():
    with pytest.raises(_lib.HipError, match=r"code -4\).*sub-vectors"):
        _lib.PqIndex(np.zeros((2, 2 * 16385), np.float32), np.zeros((2, 4, 16385), np.float32))
    with _lib.PqIndex(np.zeros((2, 8), np.float32), np.zeros((2, 4, 4), np.float32)) as idx:    # (the refusal left nothing behind)
        assert idx.info()["rows"] == 0


# ------------------------------------------------------------------------------------ the scan's LDS limit
def test_scan_with_64_kib_of_tables():
    """m = 64 with ksub = 256: 65 536 bytes of tables per workgroup, the value pq_scan_kernel's launch_lds is given as
    the kernel's maximum.  The order of searches in a process does not matter for it: launch_lds sets the kernel's
    dynamic-LDS attribute to that maximum before the first launch of each instantiation on a device, whatever that
    launch asks for, so a process that began with a small shape is no different from one that begins here (the module
    runs this shape after smaller ones with the same instantiation, m = 16 and m = 64 at ksub = 64)."""
    d, m, ksub = C.LDS_SHAPE
    case, idx = C.make_case(d, m, ksub), _index(d, m, ksub)
    off, ids, codes = idx.lists()
    np.testing.assert_array_equal(off, case.off)
    np.testing.assert_array_equal(ids, case.order)
    np.testing.assert_array_equal(codes, case.codes_by_list())
    for nprobe in (1, 8):
        for k in (10, 5000):
            dist, ids = idx.search(case.pool, k, nprobe)
            _same(dist, ids, *case.expected(C.POOL, nprobe, k), f"64 KiB of tables nprobe={nprobe} k={k}")


# ------------------------------------------------------------------------------------ 700 lists
def test_many_lists_three_adds_and_search():
    """700 lists of fewer than 256 coded rows (m = 5, stride 8 bytes): after each of three adds the lists are the
    restatement's -- the second and third run pq_scatter_old_kernel's ivf_locate over 700 old offsets with empty lists
    among them --, a scan chunk spans dozens of lists, and the planted query meets its empty lists at probe positions 63,
    255 and 257."""
    case = C.make_many_lists_case()
    with _lib.PqIndex(case.centroids, case.codebooks) as idx:
        for lo, hi in C.ML_ADDS:
            idx.add(case.x[lo:hi])
            for got, want in zip(idx.lists(), C.lists_after(case, hi)):
                np.testing.assert_array_equal(got, want, err_msg=f"after {hi} rows")
        for nprobe in C.ML_NPROBES:
            for k in C.ML_KS:
                dist, ids = idx.search(case.pool, k, nprobe)
                _same(dist, ids, *case.expected(C.POOL, nprobe, k), f"700 lists nprobe={nprobe} k={k}")
            cands = sum(case.answer(qi, nprobe)[0].shape[0] for qi in range(C.POOL))
            assert idx.stats()["candidates"] == cands and idx.stats()["bytes_scanned"] == cands * _stride(C.ML_M)
        from tests.ivf_cases import Q_PLANT
        for nprobe in (63, 64, 255, 256, 257, 258):                      # the planted query alone: an empty list probed last
            dist, ids = idx.search(case.pool[Q_PLANT], 10, nprobe)
            _same(dist, ids, *case.expected([Q_PLANT], nprobe, 10), f"700 lists, the planted query, nprobe={nprobe}")


# ------------------------------------------------------------------------------------ small things that belong
@pytest.mark.parametrize("m,ksub", [(5, 13), (64, 16)])
def test_option_profile_changes_no_answer(m, ksub):
    """Option "profile" = 1 times the kernels, = 2 launches pq_scan_kernel a first time to stage the tables only (it
    indexes s_t[lane % (m ksub)]: 65 floats here, fewer than lanes, and 1024) and stores into the key buffer ahead of
    the real scan: the answers are the bits of profile = 0."""
    case = C.make_m_case(m, ksub)
    with _two_adds(case) as idx:
        calls = ((3, 10), (8, C.M_N))
        base = [idx.search(case.pool, k, nprobe) for nprobe, k in calls]
        for (nprobe, k), (dist, ids) in zip(calls, base):
            _same(dist, ids, *case.expected(C.M_POOL, nprobe, k), f"m={m} nprobe={nprobe} k={k}")
        assert idx.stats()["scan_ms"] == 0
        for mode in (1, 2):
            idx.set_option("profile", mode)
            for (nprobe, k), (dist0, ids0) in zip(calls, base):
                dist, ids = idx.search(case.pool, k, nprobe)
                _same(dist, ids, ids0, dist0, f"m={m} profile={mode} nprobe={nprobe} k={k}")
                assert idx.stats()["scan_ms"] > 0 and idx.stats()["scan_launches"] == 1
        idx.reset_options()
        for (nprobe, k), (dist0, ids0) in zip(calls, base):
            dist, ids = idx.search(case.pool, k, nprobe)
            _same(dist, ids, ids0, dist0, f"m={m} after reset_options nprobe={nprobe} k={k}")
        assert idx.stats()["scan_ms"] == 0


def test_id_base_beyond_32_bits():
    case = C.make_m_case(5, 13)
    with _lib.PqIndex(case.centroids, case.codebooks, id_base=C.ID_BASE) as idx:
        idx.add(case.x[:C.M_SPLIT])
        idx.add(case.x[C.M_SPLIT:])
        off, ids, _ = idx.lists()
        np.testing.assert_array_equal(off, case.off)
        np.testing.assert_array_equal(ids, case.order + C.ID_BASE)
        for nprobe, k in ((1, 10), (8, C.M_N + 3)):
            dist, ids = idx.search(case.pool, k, nprobe)
            want_idx, want_dist = case.expected(C.M_POOL, nprobe, k, id_base=C.ID_BASE)
            _same(dist, ids, want_idx, want_dist, f"id_base nprobe={nprobe} k={k}")
        assert (ids[:, C.M_N:] == -1).all() and (ids[:, :C.M_N] >= C.ID_BASE).all()      # padding stays -1


def test_a_query_whose_tables_overflow():
    """1e30 everywhere: every table entry, and so every candidate's distance, is +inf.  The answer is the candidates'
    real ids in ascending order at +inf, and -1 only behind the last candidate."""
    case = C.make_m_case(5, 13)
    q = C.huge_query(case.d)
    with _two_adds(case) as idx:
        for nprobe in (3, 8):
            with np.errstate(over="ignore"):
                want = C.answer_of(case, q, nprobe)
            cands = want[0].shape[0]
            for k in (10, C.M_N + 3):
                dist, ids = idx.search(q, k, nprobe)
                oi, od = C.pad(*want, k)
                _same(dist[0], ids[0], oi, od, f"overflowing query nprobe={nprobe} k={k}")
                assert np.isposinf(dist).all() and (np.diff(ids[0, :min(k, cands)]) > 0).all() and (ids[0, :min(k, cands)] >= 0).all()
                assert (ids[0, cands:] == -1).all()
            assert idx.stats()["candidates"] == cands


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


def _check_nn(index, vecs_by_uuid, q, n):
    """`nn` returns elements of the index with metrics.euclidean_distance of their ORIGINAL vectors to the float32 query,
    ascending."""
    elems, dists = index.nn(q, n)
    assert len(elems) == len(dists) == n and len({e.uuid() for e in elems}) == n
    q32 = np.asarray(q.vector()).astype(np.float32)
    for e, dv in zip(elems, dists):
        v = np.asarray(vecs_by_uuid[e.uuid()])
        assert np.array_equal(e.vector(), v)
        want = O.euclidean_distance(v, q32 if v.dtype == np.float32 else q32.astype(v.dtype))
        assert dv == float(want)
    assert list(dists) == sorted(dists)
    return elems, dists


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_plugin_build_update_remove_nn(dtype):
    vecs = _plugin_data(dtype)
    descr = _descriptors(vecs)
    by_uuid = {i: vecs[i] for i in range(3000)}
    pq = HipIvfPqNearestNeighborsIndex(nlist=32, nprobe=32, m=4, train_iters=5, random_seed=4)
    pq.build_index(descr[:2000])
    dev = pq._dev
    pq.update_index(descr[2000:])                                        # joins the existing lists: the same device index
    assert pq.count() == 3000 and pq._dev is dev and dev.info()["rows"] == 3000
    assert dev.info()["codes_bytes"] == 3000 * 4 and dev.info()["ksub"] == 256
    queries = _descriptors(np.vstack([vecs[7], vecs[2500] + 0.01, np.zeros(16)]).astype(dtype), start=10_000)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                   # every list probed: n neighbours come back
        for q in queries:
            _check_nn(pq, by_uuid, q, 1)
            _check_nn(pq, by_uuid, q, 50)
        # a row added by the update is found from its own vector, the coded distances of nn_many are ascending
        elems, _ = _check_nn(pq, by_uuid, descr[2500], 20)
        assert 2500 in [e.uuid() for e in elems]
    idx, dist = pq.nn_many(vecs[:5].astype(np.float32), 25)
    assert (idx >= 0).all() and (np.diff(dist, axis=1) >= 0).all()
    # a replaced uuid and a removal: the lists are coded again with the same centroids and codebooks
    cent, books = pq._centroids.copy(), pq._codebooks.copy()
    moved = DescriptorMemoryElement(7)
    moved.set_vector((vecs[7] + 5).astype(dtype))
    by_uuid[7] = moved.vector()
    pq.update_index([moved])
    pq.remove_from_index(list(range(100, 200)))
    assert pq.count() == 2900 and pq._dev is not dev and pq._dev.info()["rows"] == 2900
    assert np.array_equal(pq._centroids, cent) and np.array_equal(pq._codebooks, books)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        elems, _ = _check_nn(pq, by_uuid, moved, 30)
        assert elems[0].uuid() == 7
        for q in queries:
            got, _ = _check_nn(pq, by_uuid, q, 50)
            assert not {e.uuid() for e in got} & set(range(100, 200))
    with pytest.raises(KeyError):
        pq.remove_from_index([5, 150])                                   # 150 is gone: nothing changes
    assert pq.count() == 2900
    with pytest.raises(ValueError, match="sub-vectors"):
        HipIvfPqNearestNeighborsIndex(m=3).build_index(descr[:100])      # 16 % 3 != 0


def test_plugin_warns_when_the_probed_lists_run_short():
    vecs = _plugin_data(np.float32)
    pq = HipIvfPqNearestNeighborsIndex(nlist=32, nprobe=1, m=8, train_iters=5, random_seed=4)
    pq.build_index(_descriptors(vecs))
    q = _descriptors(vecs[:1], start=20_000)[0]
    with pytest.warns(RuntimeWarning, match="nprobe"):
        elems, dists = pq.nn(q, 3000)                                    # one list cannot hold all 3000 rows
    assert 0 < len(elems) == len(dists) < 3000 and list(dists) == sorted(dists)
    assert elems[0].uuid() == 0 and dists[0] == 0.0


def test_plugin_with_fewer_descriptors_than_256():
    """40 descriptors: the training sample is all of them, the codebooks have ksub = 40 entries, and with every list
    probed `nn` returns 1 and all 40 neighbours."""
    rng = np.random.default_rng(23)
    vecs = (rng.standard_normal((40, 16)) * 2).astype(np.float32)
    by_uuid = {i: vecs[i] for i in range(40)}
    pq = HipIvfPqNearestNeighborsIndex(nlist=8, nprobe=8, m=4, train_iters=3, random_seed=2)
    assert pq.training_plan(40)[2].shape == (40,)
    pq.build_index(_descriptors(vecs))
    try:
        assert pq.count() == 40 and pq._dev.info()["ksub"] == 40 and pq._dev.info()["rows"] == 40 and pq._codebooks.shape == (4, 40, 4)
        queries = _descriptors(np.vstack([vecs[3], vecs[17] + 0.01, np.zeros(16)]).astype(np.float32), start=1000)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            for q in queries:
                _check_nn(pq, by_uuid, q, 1)
                elems, _ = _check_nn(pq, by_uuid, q, 40)
                assert {e.uuid() for e in elems} == set(range(40))
            elems, dists = _check_nn(pq, by_uuid, queries[0], 1)
            assert elems[0].uuid() == 3 and dists[0] == 0.0
    finally:
        pq._dev.close()
