"""
GPU tests of the IVF-SQ index (`sq_isq_*`, `_lib.IsqIndex`, the two plugin classes of impls/nn_index/hip_ivf_sq.py).

Every answer is compared with the numpy restatement of tests/isq_cases.py -- tests/ivf_cases.py's search over the decoded
matrix with the lists of the original one -- ids exactly and distances in float32 bits; the codes read back through
`lists()` are numpy's.  What the cases must have (clipping at both ends, another summation order changing a distance at
every width) is proven on the CPU by tests/test_isq_cases_cpu.py.
"""
import numpy as np
import pytest

from smqtk_indexing_amd import _lib
from smqtk_indexing_amd._compat import DescriptorMemoryElement
from smqtk_indexing_amd.impls.nn_index.hip_bruteforce import HipBruteForceNearestNeighborsIndex
from smqtk_indexing_amd.impls.nn_index.hip_ivf_sq import HipIvfSq8NearestNeighborsIndex, HipIvfSqFp16NearestNeighborsIndex
from tests import isq_cases as S
from tests import ivf_cases as C
from tests import width_cases as W

pytestmark = pytest.mark.gpu

ID_BASE = 2 ** 40 + 5
KINDS = pytest.mark.parametrize("kind", sorted(S.KINDS))
_indexes = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got_dist, got_idx, want_idx, want_dist, what):
    np.testing.assert_array_equal(got_idx, want_idx, err_msg=what)
    np.testing.assert_array_equal(_bits(got_dist), _bits(want_dist), err_msg=what)


def _open(sc, **kw):
    return _lib.IsqIndex(sc.case.centroids, sc.kind, sc.vmin, sc.step, **kw)


def _built(name, kind):
    """(restatement, index) of the main or the many-lists case, built once: one add of all rows."""
    sc = S.make(C.make_case(36) if name == "main" else C.make_many_lists_case(), S.KINDS[kind])
    if (name, kind) not in _indexes:
        idx = _open(sc, id_base=ID_BASE)
        idx.add(sc.case.x)
        _indexes[name, kind] = idx
    return sc, _indexes[name, kind]


def _stride(d, kind):
    return -(-d * (2 if kind == "f16" else 1) // 16) * 16


# ------------------------------------------------------------------------------------ encode
@KINDS
def test_encode_of_a_hand_made_matrix(kind):
    """Half-to-even (0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 254.5 -> 254), both clips (255.5, +inf -> 255; -0.3, NaN -> 0) and a
    column with step 0; for float16 a subnormal half, the largest half, overflow to inf and two ties."""
    if kind == "sq8":
        values = np.array([0.5, 1.5, 2.5, 254.5, 255.5, -0.3, np.inf, np.nan], np.float32)
    else:
        values = np.array([1e-6, 65504, 65520, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -1e-6, -65520, 0.1], np.float32)
    x = np.ascontiguousarray(values[(np.arange(16)[:, None] + np.arange(9)[None, :]) % 8])
    vmin, step = (np.zeros(9, np.float32), np.ones(9, np.float32)) if kind == "sq8" else (None, None)
    if kind == "sq8":
        step[4] = 0
    with _lib.IsqIndex(np.zeros((1, 9), np.float32), S.KINDS[kind], vmin, step) as idx:
        idx.add(x[:5])
        idx.add(x[5:])
        off, ids, codes = idx.lists()
        assert off.tolist() == [0, 16] and ids.tolist() == list(range(16))
        np.testing.assert_array_equal(codes, S.encode(x, S.KINDS[kind], vmin, step))
        if kind == "sq8":
            assert codes[0].tolist() == [0, 2, 2, 254, 0, 0, 255, 0, 0]
        else:
            assert codes[0, :5].view(np.float16).tolist() == [np.float16(1e-6), 65504.0, np.inf, 1.0, 1 + 2.0 ** -9] and 0 < codes[0, 0] < 0x400


@KINDS
def test_main_case_codes_and_lists_are_numpys(kind):
    sc, idx = _built("main", kind)
    off, ids, codes = idx.lists()
    np.testing.assert_array_equal(off, sc.case.off)
    np.testing.assert_array_equal(ids, sc.case.order + ID_BASE)
    np.testing.assert_array_equal(codes, sc.codes[sc.case.order])
    if kind == "sq8":
        np.testing.assert_array_equal(np.stack(_lib.isq_train(sc.case.x[:S.TRAIN_ROWS])).view(np.uint32), np.stack([sc.vmin, sc.step]).view(np.uint32))


# ------------------------------------------------------------------------------------ every width where the code branches
@pytest.mark.parametrize("kind,d", [("sq8", d) for d in list(W.WIDTHS) + [8193, 8199, 8200]] + [("f16", d) for d in S.F16_WIDTHS])
def test_scan_at_width(kind, d):
    """8- and 16-byte loads, tails of 1 .. 7, leaves below 8, the first pairwise split, padded strides, staging beyond
    64 KiB; two adds, so that the second moves the first one's code rows at this stride."""
    sc = S.make(C.make_width_case(d), S.KINDS[kind])
    with _open(sc) as idx:
        idx.add(sc.case.x[:500])
        idx.add(sc.case.x[500:])
        _, _, codes = idx.lists()
        np.testing.assert_array_equal(codes, sc.codes[sc.case.order])
        dist, ids = idx.search(sc.case.pool, 300, 8)
        _same(dist, ids, *sc.dec.expected(C.W_POOL, 8, 300), f"{kind} d={d}")
        assert idx.stats()["bytes_scanned"] == C.W_POOL * sc.case.n * _stride(d, kind)


# ------------------------------------------------------------------------------------ the main case
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("nq", [1, 33])
@pytest.mark.parametrize("nprobe", [1, 3, 64])
@KINDS
def test_search_equals_the_restatement(kind, nprobe, nq, mem):
    sc, idx = _built("main", kind)
    for k in (1, 200):
        if mem == "host":
            dist, ids = idx.search(sc.case.pool[:nq], k, nprobe)
        else:
            torch = pytest.importorskip("torch")
            dev = torch.device("cuda:0")
            q_t = torch.from_numpy(np.array(sc.case.pool[:nq])).to(dev)
            od = torch.full((nq, k), -3.0, dtype=torch.float32, device=dev)
            oi = torch.full((nq, k), -77, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            idx.search_device(q_t.data_ptr(), nq, k, nprobe, od.data_ptr(), oi.data_ptr())
            dist, ids = od.cpu().numpy(), oi.cpu().numpy()
        _same(dist, ids, *sc.dec.expected(nq, nprobe, k, id_base=ID_BASE), f"{kind} nprobe={nprobe} nq={nq} k={k} {mem}")
    cands = sum(sc.dec.answer(qi, nprobe)[0].shape[0] for qi in range(nq))
    st = idx.stats()
    assert st["candidates"] == cands and st["bytes_scanned"] == cands * _stride(36, kind) and st["scan_launches"] == (1 if cands else 0)


@KINDS
def test_every_list_probed_equals_the_dense_search_over_the_decoded_matrix(kind):
    sc, idx = _built("main", kind)
    dense = _lib.DenseIndex(sc.dec.x)
    try:
        dd, di = dense.search(sc.case.pool, 200)
        dist, ids = idx.search(sc.case.pool, 200, C.NLIST + 36)
        _same(dist, ids, di + ID_BASE, dd, f"{kind}: every list probed")
    finally:
        dense.close()


@pytest.mark.parametrize("nprobe", [64, 257, 700])
@KINDS
def test_many_lists(kind, nprobe):
    """700 lists of fewer than 256 rows: every full scan chunk crosses list boundaries."""
    sc, idx = _built("many", kind)
    dist, ids = idx.search(sc.case.pool, 300, nprobe)
    _same(dist, ids, *sc.dec.expected(C.POOL, nprobe, 300, id_base=ID_BASE), f"{kind} many lists nprobe={nprobe}")


# ------------------------------------------------------------------------------------ adds and budgets
@KINDS
def test_three_adds_are_one_add_and_an_empty_index_pads(kind):
    sc, one = _built("main", kind)
    with _open(sc, id_base=ID_BASE) as idx:
        dist, ids = idx.search(sc.case.pool[:3], 5, 4)
        assert (ids == -1).all() and np.isposinf(dist).all() and idx.info()["rows"] == 0 and idx.stats()["scan_launches"] == 0
        for lo, hi in ((0, 1), (1, 7001), (7001, C.N)):
            idx.add(sc.case.x[lo:hi])
        for got, want in zip(idx.lists(), one.lists()):
            np.testing.assert_array_equal(got, want)
        dist, ids = idx.search(sc.case.pool, 200, 3)
        _same(dist, ids, *sc.dec.expected(C.POOL, 3, 200, id_base=ID_BASE), f"{kind} after three adds")


@KINDS
def test_device_rows_padded_and_from_an_unaligned_base(kind):
    torch = pytest.importorskip("torch")
    sc = S.make(C.make_width_case(35), S.KINDS[kind])
    n, d = sc.case.n, 35
    flat = torch.zeros(n * d + 1, dtype=torch.float32, device=torch.device("cuda:0"))
    flat[1:].copy_(torch.from_numpy(np.array(sc.case.x)).reshape(-1))
    torch.cuda.synchronize()
    assert flat.data_ptr() % 16 == 0
    with _open(sc) as idx:
        idx.add(flat.data_ptr() + 4, n=500, device_ptr=True)
        idx.add(flat.data_ptr() + 4 + 500 * d * 4, n=n - 500, device_ptr=True)
        off, ids, codes = idx.lists()
        np.testing.assert_array_equal(ids, sc.case.order)
        np.testing.assert_array_equal(codes, sc.codes[sc.case.order])
        dist, ids = idx.search(sc.case.pool, C.W_K, 3)
        _same(dist, ids, *sc.dec.expected(C.W_POOL, 3, C.W_K), f"{kind} device rows")


@KINDS
def test_a_small_key_budget_runs_70_queries_in_slices(kind):
    """Every list probed: (20 011 + 10) * 8 bytes of keys per query, 6 queries per MiB, 12 slices for 70 queries."""
    sc, idx = _built("main", kind)
    queries = np.tile(sc.case.pool, (3, 1))[:70]
    want_idx, want_dist = (np.tile(a, (3, 1))[:70] for a in sc.dec.expected(C.POOL, C.NLIST, 10, id_base=ID_BASE))
    idx.set_option("ivf_key_budget_mb", 1)
    try:
        dist, ids = idx.search(queries, 10, C.NLIST)
        assert idx.info()["key_budget_bytes"] == 1 << 20 and idx.stats()["scan_launches"] == 12
        _same(dist, ids, want_idx, want_dist, f"{kind} in 12 slices")
    finally:
        idx.reset_options()


# ------------------------------------------------------------------------------------ info and plugins
@KINDS
def test_info_is_the_layout_arithmetic(kind):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((300, 128)).astype(np.float32)
    vmin, step = S.train(x) if kind == "sq8" else (None, None)
    for d, per_row in ((128, 132 if kind == "sq8" else 260), (35, 4 + _stride(35, kind))):
        par = [None if p is None else p[:d] for p in (vmin, step)]
        with _lib.IsqIndex(x[:4, :d], S.KINDS[kind], *par) as idx:
            idx.add(x[:, :d])
            info = idx.info()
            assert (info["rows"], info["d"], info["nlist"], info["kind"], info["row_stride_bytes"]) == (300, d, 4, S.KINDS[kind], _stride(d, kind))
            assert info["codes_bytes"] == 300 * _stride(d, kind) and info["codes_bytes"] + 300 * 4 == 300 * per_row
            assert info["ids_offsets_bytes"] >= 300 * 4 + 5 * 8 and info["coarse_params_bytes"] >= 4 * d * 4 + 2 * -(-d // 4) * 16
            assert info["add_us"] > 0 and info["key_budget_bytes"] == 256 << 20 and info["longest_list"] + info["empty_lists"] > 0


def _descriptors(vecs, start=0):
    out = []
    for i, v in enumerate(vecs):
        e = DescriptorMemoryElement(start + i)
        e.set_vector(v)
        out.append(e)
    return out


@pytest.mark.parametrize("cls", [HipIvfSq8NearestNeighborsIndex, HipIvfSqFp16NearestNeighborsIndex])
def test_plugin_build_update_remove_nn(cls):
    """40 descriptors, every list probed and every element asked for: `nn` re-ranks by the original vectors, so the
    answer is the brute-force index's; one probe returns fewer and warns."""
    vecs = (np.random.default_rng(21).standard_normal((46, 16)) * 3).astype(np.float32)
    descr = _descriptors(vecs)
    sq, bf = cls(nlist=4, nprobe=4, train_iters=3, random_seed=4), HipBruteForceNearestNeighborsIndex()
    sq.build_index(descr[:40])
    sq.update_index(descr[40:])
    bf.build_index(descr)
    q = _descriptors(vecs[7:8] + np.float32(0.01), start=1000)[0]

    def compare():
        se, sdist = sq.nn(q, sq.count())
        be, bdist = bf.nn(q, bf.count())
        assert [e.uuid() for e in se] == [e.uuid() for e in be] and sdist == bdist

    compare()
    idx, dist = sq.nn_many(vecs[:3], 46)
    assert sorted(idx[0].tolist()) == list(range(46)) and (np.diff(dist, axis=1) >= 0).all() and (dist[:, 0] < 0.5).all()
    moved = DescriptorMemoryElement(7)
    moved.set_vector(vecs[7] + np.float32(5))
    for index in (sq, bf):
        index.update_index([moved])
        index.remove_from_index(list(range(10, 20)))
    assert sq.count() == bf.count() == 36
    compare()
    with pytest.raises(KeyError):
        sq.remove_from_index([5, 15])
    sq.nprobe = 1
    with pytest.warns(RuntimeWarning, match="nprobe"):
        elems, dists = sq.nn(q, 36)
    assert 0 < len(elems) < 36 and list(dists) == sorted(dists)
