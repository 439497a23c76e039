"""
GPU tests of the IVF-PQ index's packed mode (`sq_pq_create_packed`, the plugin classes of hip_ivf_pq4.py) against the numpy
restatements of tests/pq_cases.py (plain) and tests/pq_residual_cases.py (residual) as they stand: ids exactly, distances in
float32 bits, `lists()` one byte per code.  Nothing here skips when the library is missing.
"""
import numpy as np
import pytest

from oracle import cpu_ref as O
from smqtk_indexing_amd import _lib
from smqtk_indexing_amd._compat import DescriptorMemoryElement
from smqtk_indexing_amd.impls.nn_index.hip_ivf_pq4 import HipIvfPq4NearestNeighborsIndex, HipIvfPq4ResidualNearestNeighborsIndex
from tests import pq_cases as C
from tests import pq_residual_cases as R

pytestmark = pytest.mark.gpu

MODES = ("plain", "residual")
M_LIST = tuple(range(1, 18)) + (24, 25, 32, 33, 40, 41, 48, 49, 56, 57, 63, 64)     # every stride 4 .. 32 bytes, both nibble parities
NPROBES, KS = (1, 3, 8, 100), (1, 10, 5000)
TAIL_SHAPES = ((64, 16), (12, 12))               # (d, m) at ksub = 16: a 5-row list, two empty lists, one beyond 1024 rows
_indexes = {}


@pytest.fixture(scope="module", autouse=True)
def _close_the_shared_indexes():
    yield
    for idx in _indexes.values():
        idx.close()
    _indexes.clear()


def _in_mode(plain, mode):
    return plain if mode == "plain" else R.from_plain(plain)


def _main_case(d, m, mode):
    return C.make_case(d, m, 16) if mode == "plain" else R.make_case(d, m, 16)


def _new(case, mode, packed=True, **kw):
    return _lib.PqIndex(case.centroids, case.codebooks, residual=mode == "residual", packed=packed, **kw)


def _shared(d, m, mode):
    """The main case's packed index at ksub = 16 with ids beyond 2^32, built once: one add of all rows."""
    if (d, m, mode) not in _indexes:
        _indexes[(d, m, mode)] = _new(_main_case(d, m, mode), mode, id_base=C.ID_BASE)
        _indexes[(d, m, mode)].add(_main_case(d, m, mode).x)
    return _indexes[(d, m, mode)]


def _same(got_dist, got_idx, want_idx, want_dist, what):
    np.testing.assert_array_equal(got_idx, want_idx, err_msg=what)
    np.testing.assert_array_equal(*(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) for a in (got_dist, want_dist)), err_msg=what)


def _check(idx, case, nprobes, ks, queries=None, qis=None, id_base=0):
    """`lists()` and the packed bytes against the case, then every (nprobe, k) of the pool (or of `queries`) in bits."""
    stride = -(-(-(-case.m // 2)) // 4) * 4
    for got, want in zip(idx.lists(), (case.off, case.order + id_base, case.codes_by_list())):
        np.testing.assert_array_equal(got, want, err_msg=case.what)
    assert idx.info()["codes_bytes"] == case.n * stride and idx.info()["rows"] == case.n
    qis = range(case.pool.shape[0]) if qis is None else qis
    for nprobe in nprobes:
        for k in ks:
            dist, ids = idx.search(case.pool if queries is None else queries, k, nprobe)
            _same(dist, ids, *case.expected(qis, nprobe, k, id_base), f"{case.what} nprobe={nprobe} k={k}")
        assert idx.stats()["bytes_scanned"] == sum(case.answer(qi, nprobe)[0].shape[0] for qi in qis) * stride


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ksub", C.M_KSUBS)
@pytest.mark.parametrize("m", M_LIST)
def test_every_stride_and_nibble_parity(m, ksub, mode):
    """Rows of 1 to 8 dwords (every scan instance, both load widths), half-filled last bytes, two adds; all 1049 distances."""
    case = _in_mode(C.make_m_case(m, ksub), mode)
    with _new(case, mode) as idx:
        idx.add(case.x[:C.M_SPLIT])
        idx.add(case.x[C.M_SPLIT:])
        _check(idx, case, C.M_NPROBES, C.M_KS)


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("nq", [1, 33])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d,m", TAIL_SHAPES)
def test_inactive_lanes_and_tails(d, m, mode, nq, mem):
    """The 5-row list (251 of 256 lanes behind the end must still serve the lookups), empty lists, the long list's tail."""
    case, idx = _main_case(d, m, mode), _shared(d, m, mode)
    if mem == "host":
        return _check(idx, case, NPROBES, KS, case.pool[:nq], range(nq), C.ID_BASE)
    import torch
    q_t = torch.from_numpy(np.array(case.pool[:nq])).to("cuda:0")
    for nprobe in NPROBES:
        for k in KS:
            od = torch.full((nq, k), -3.0, dtype=torch.float32, device="cuda:0")
            oi = torch.full((nq, k), -77, dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            idx.search_device(q_t.data_ptr(), nq, k, nprobe, od.data_ptr(), oi.data_ptr(), torch.cuda.current_stream().cuda_stream)
            _same(od.cpu().numpy(), oi.cpu().numpy(), *case.expected(nq, nprobe, k, id_base=C.ID_BASE), f"{case.what} nprobe={nprobe} nq={nq} k={k}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("what,v", [("ksub", v) for v in (1, 2, 3)] + [("dsub", v) for v in (1, 4, 129, 1024, 1028)])
def test_small_codebooks_and_both_tables_kernels(what, v, mode):
    """ksub 1, 2, 3 at KSUB_SHAPE (registers behind ksub are never read; at ksub = 1 ids decide); m = 3, ksub = 16 at d / m up
    to 1024 (pq4_tables_kernel: unaligned starts, several pairwise leaves, 64 KiB of LDS) and 1028 (the one-byte kernels)."""
    case = _in_mode(C.make_case(*C.KSUB_SHAPE, v) if what == "ksub" else C.make_m_case(3, 16, dsub=v), mode)
    with _new(case, mode) as idx:
        idx.add(case.x)
        _check(idx, case, (1, 3, 8), (10, 5000))


@pytest.mark.parametrize("nq", C.S_NQS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d,m", C.S_SHAPES)
def test_stride_loop(d, m, mode, nq):
    """Workgroups walking chunks g, g + groups, ...: 16 each with 600 queries, a spread call with 64 (the existing cases)."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if mode == "plain":
        case, nprobes = C.make_strided_case(d, m), C.S_NPROBES
        for nprobe in nprobes:
            C.assert_regime(C.strided_plan(case, nprobe, nq, cus), nq, f"{case.what} on {cus} compute units")
    else:
        case, nprobes = R.make_strided_case(d, m), (R.S_NPROBE,)
        R.assert_regime(R.strided_plan(case, nq, cus), nq, f"{case.what} on {cus} compute units")
    queries, qis = C.strided_queries(case, nq)
    with _new(case, mode) as idx:
        idx.add(case.x)
        _check(idx, case, nprobes, (C.S_K,), queries, qis)


@pytest.mark.parametrize("k", [1000, 5000])
def test_pair_ranges_under_a_small_budget(k):
    """264 pairs under 1 MiB of key budget: ranges that begin inside a query at a list with rows; other queries run first."""
    (d, m), nq = TAIL_SHAPES[0], C.POOL
    case, idx = _main_case(d, m, "residual"), _shared(d, m, "residual")
    slice_, ppl, launches = R.res_plan(nq, 8, C.N, k, m, 16, 1 << 20)
    starts = [(q0 + ql, pos) for q0 in range(0, nq, slice_) for ql, pos in R.range_starts(min(slice_, nq - q0), 8, ppl)]
    assert launches == len(starts) >= 2
    assert any(pos and case.rows_of(R.probe(case.centroids, case.pool[qi], 8)[pos]).shape[0] for qi, pos in starts)
    idx.set_option("ivf_key_budget_mb", 1)
    try:
        idx.search(case.pool[::-1], k, 8)
        dist, ids = idx.search(case.pool, k, 8)
        assert idx.stats()["scan_launches"] == launches
    finally:
        idx.reset_options()
    _same(dist, ids, *case.expected(nq, 8, k, id_base=C.ID_BASE), f"k={k}: {launches} ranges of {ppl} pairs")


@pytest.mark.parametrize("mode", MODES)
def test_empty_index_three_adds_overflow_and_the_one_byte_index(mode):
    d, m = TAIL_SHAPES[1]
    case, one = _main_case(d, m, mode), _shared(d, m, mode)
    with _new(case, mode, id_base=C.ID_BASE) as idx, _new(case, mode, packed=False, id_base=C.ID_BASE) as wide:
        dist, ids = idx.search(case.pool[:3], 5, 4)                          # an empty index: padding only
        assert (ids == -1).all() and np.isposinf(dist).all() and idx.stats()["scan_launches"] == 0 and idx.info()["codes_bytes"] == 0
        for lo, hi in ((0, 1), (1, 1201), (1201, C.N)):
            idx.add(case.x[lo:hi])
        wide.add(case.x)
        for a, b, c in zip(idx.lists(), one.lists(), wide.lists()):          # three adds leave what one add leaves, and what one byte per code holds
            np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(a, c)
        for nprobe, k in ((1, 10), (3, 100), (8, 5000)):                      # ... whose bits a packed index gives
            _same(*idx.search(case.pool, k, nprobe), *wide.search(case.pool, k, nprobe)[::-1], f"{mode} nprobe={nprobe} k={k}")
        q = C.huge_query(d)                                                   # every distance +inf: ids ascend, -1 only behind the last candidate
        with np.errstate(over="ignore", invalid="ignore"):
            want = case.answer_of(q, 3) if mode == "residual" else C.answer_of(case, q, 3)
        for k in (10, C.N + 3):
            dist, ids = idx.search(q, k, 3)
            _same(dist[0], ids[0], *C.pad(*want, k, C.ID_BASE), f"{mode} overflowing query k={k}")
            n_real = min(k, want[0].shape[0])
            assert np.isposinf(dist).all() and (np.diff(ids[0, :n_real]) > 0).all() and (ids[0, n_real:] == -1).all()


@pytest.mark.parametrize("cls", [HipIvfPq4NearestNeighborsIndex, HipIvfPq4ResidualNearestNeighborsIndex])
@pytest.mark.parametrize("n", [40, 10])
def test_plugin_classes(n, cls):
    """ksub = min(16, sample rows), a packed device index, and `nn` re-ranked by the original vectors as the parents do."""
    vecs = np.random.default_rng(n).standard_normal((n, 8)).astype(np.float32)
    descr = [DescriptorMemoryElement(i) for i in range(n)]
    for e, v in zip(descr, vecs):
        e.set_vector(v)
    pq = cls(nlist=2, nprobe=2, m=4, train_iters=3, random_seed=1)
    pq.build_index(descr)
    try:
        info = pq._dev.info()
        assert pq._dev.packed and pq._dev.residual == (cls is HipIvfPq4ResidualNearestNeighborsIndex)
        assert info["ksub"] == min(16, n) == pq.training_plan(n)[2].shape[0] and info["codes_bytes"] == n * 4
        elems, dists = pq.nn(descr[3], 5)
        assert elems[0].uuid() == 3 and dists[0] == 0.0 and list(dists) == sorted(dists)
        assert all(dv == float(O.euclidean_distance(vecs[e.uuid()], vecs[3])) for e, dv in zip(elems, dists))
    finally:
        pq._dev.close()
