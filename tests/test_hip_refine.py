"""
GPU tests of the refine stage (`sq_refine_*`, `_lib.RefineStore`, impls/nn_index/hip_ivf_refine.py).

Re-ranks are compared with the numpy restatement of tests/refine_cases.py, searches with the exact list indexes they must
equal (`IvfIndex.search`, `IsqIndex.search`): ids exactly, distances in float32 bits.
"""
import numpy as np
import pytest
import torch

from smqtk_indexing_amd import _lib
from smqtk_indexing_amd._compat import DescriptorMemoryElement
from smqtk_indexing_amd.impls.nn_index.hip_ivf_refine import HipIvfPqRefineNearestNeighborsIndex
from tests import refine_cases as R

pytestmark = pytest.mark.gpu

KINDS = pytest.mark.parametrize("kind", sorted(R.KINDS))


def _same(got, want, what=""):
    np.testing.assert_array_equal(got[1], want[1], err_msg=what)
    np.testing.assert_array_equal(got[0].view(np.uint32), np.ascontiguousarray(want[0], dtype=np.float32).view(np.uint32), err_msg=what)


def _store(x, kind, vmin=None, step=None, id_base=0, adds=1):
    par = (vmin, step) if kind == "sq8" else ()
    store = _lib.RefineStore(x.shape[1], R.KINDS[kind], *par, id_base=id_base)
    for part in np.array_split(x, adds):
        store.add(part)
    return store


def _decoded(x, kind, vmin, step):
    return R.decode(R.encode(x, R.KINDS[kind], vmin, step), R.KINDS[kind], vmin, step)


@pytest.mark.parametrize("direct", [0, 1])
@pytest.mark.parametrize("d", R.WIDTHS)
@KINDS
def test_rerank_at_width(kind, d, direct):
    x, vmin, step, q, cand = R.width_case(d)
    with _store(x, kind, vmin, step, R.ID_BASE, adds=2) as store:
        store.set_option("refine_direct", direct)
        got = store.rerank(q, cand, R.K)
        assert store.stats()["candidates"] == R.NQ * (R.KB - 4) and store.stats()["bytes_scanned"] == R.NQ * (R.KB - 4) * store.info()["row_stride_bytes"]
    _same(got, R.rerank(_decoded(x, kind, vmin, step), R.ID_BASE, q, cand, R.K))


@pytest.mark.parametrize("direct", [0, 1])
@KINDS
def test_ties_ascend_by_id_and_padding_follows_the_last_candidate(kind, direct):
    """Every row four times, the candidates in descending id order: equal distances come out by ascending id; k beyond the
    valid candidates pads behind them only."""
    x, vmin, step, q, _ = R.width_case(33)
    x4 = np.tile(x[:10], (4, 1))
    cand = np.tile(np.arange(39, -3, -1, dtype=np.int64), (R.NQ, 1))       # 39 .. 0, -1, -2
    with _store(x4, kind, vmin, step) as store:
        store.set_option("refine_direct", direct)
        got = store.rerank(q, cand, 42)
    want = R.rerank(_decoded(x4, kind, vmin, step), 0, q, cand, 42)
    assert (want[1][:, :4] % 10 == want[1][:, :1] % 10).all() and (np.diff(want[1][:, :4]) > 0).all() and (want[1][:, 40:] == -1).all()
    _same(got, want)


@pytest.fixture(scope="module")
def bases():
    """The four bases over the list case, built once and closed with the module."""
    x, cent, books, vmin, step, _ = R.list_case()
    made = dict(plain=_lib.PqIndex(cent, books), residual=_lib.PqIndex(cent, books, residual=True),
                packed=_lib.PqIndex(cent, books, residual=True, packed=True), sq8=_lib.IsqIndex(cent, _lib.SQ_ISQ_SQ8, vmin, step))
    for b in made.values():
        b.add(x)
    yield made
    for b in made.values():
        b.close()


@pytest.mark.parametrize("base", ["plain", "residual", "packed", "sq8"])
@KINDS
def test_search_equals_the_exact_lists(bases, base, kind):
    x, cent, _, vmin, step, q = R.list_case()
    exact = _lib.IvfIndex(cent) if kind == "f32" else _lib.IsqIndex(cent, R.KINDS[kind], *((vmin, step) if kind == "sq8" else ()))
    with exact, _store(x, kind, vmin, step) as store:
        exact.add(x)
        off = exact.lists()[0]
        assert off[R.LIST_EMPTY + 1] == off[R.LIST_EMPTY] and off[R.LIST_SMALL + 1] - off[R.LIST_SMALL] == 5
        for nprobe in (1, 3, 13):
            for nq in (1, 33):
                _same(store.search(bases[base], q[:nq], 10, len(x), nprobe), exact.search(q[:nq], 10, nprobe), f"nprobe={nprobe} nq={nq}")


def test_search_with_a_short_candidate_list(bases):
    x, cent, _, vmin, step, q = R.list_case()
    k, nprobe = 10, 6
    with _store(x, "f16") as store:
        got = store.search(bases["residual"], q, k, 2 * k, nprobe)
        assert store.stats()["candidates"] < bases["residual"].stats()["candidates"]
    _, cand = bases["residual"].search(q, 2 * k, nprobe)
    _same(got, R.rerank(_decoded(x, "f16", None, None), 0, q, cand, k))


def test_a_batch_in_query_slices(bases):
    """A key budget of 1 MB holds 31 queries of 1400 candidates: 33 queries go in two slices, outputs and counts in place."""
    x, _, _, _, _, q = R.list_case()
    cand = np.full((33, 1400), -1, np.int64)
    cand[:, 100:140] = np.stack([np.random.default_rng(i).permutation(len(x))[:40] for i in range(33)])
    with _store(x, "f16") as store:
        store.set_option("ivf_key_budget_mb", 1)
        _same(store.rerank(q, cand, 10), R.rerank(_decoded(x, "f16", None, None), 0, q, cand, 10))
        assert store.stats()["candidates"] == 33 * 40 and store.stats()["scan_launches"] == 2
        got = store.search(bases["packed"], q, 10, 1400, 3)
        assert store.stats()["scan_launches"] == 2
        store.reset_options()
        _same(got, store.search(bases["packed"], q, 10, 1400, 3))


def test_device_memory_equals_host_memory():
    x, vmin, step, q, cand = R.width_case(300)
    with _store(x, "sq8", vmin, step, R.ID_BASE) as store:
        want = store.rerank(q, cand, R.K)
        qd, cd = torch.from_numpy(np.array(q)).cuda(), torch.from_numpy(np.array(cand)).cuda()
        od, oi = torch.empty((R.NQ, R.K), dtype=torch.float32, device="cuda"), torch.empty((R.NQ, R.K), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        store.rerank_device(qd.data_ptr(), R.NQ, cd.data_ptr(), R.KB, R.K, od.data_ptr(), oi.data_ptr())
    _same((od.cpu().numpy(), oi.cpu().numpy()), want)


def test_id_base_beyond_32_bits():
    x, vmin, step, q, cand = R.width_case(17)
    base = 2 ** 40 + 5
    with _store(x, "f16", id_base=base) as store:
        got = store.rerank(q, cand - R.ID_BASE + base, R.K)
    _same(got, R.rerank(_decoded(x, "f16", None, None), base, q, cand - R.ID_BASE + base, R.K))


@KINDS
def test_three_adds_leave_the_rows_of_one(kind):
    x, vmin, step, _, _ = R.width_case(100)
    with _store(x, kind, vmin, step, adds=3) as three, _store(x, kind, vmin, step) as one:
        np.testing.assert_array_equal(three.rows().view(np.uint8), one.rows().view(np.uint8))
        np.testing.assert_array_equal(one.rows().view(np.uint8), R.encode(x, R.KINDS[kind], vmin, step).view(np.uint8))
        assert three.info()["rows"] == 70 and three.info()["codes_bytes"] == 70 * three.info()["row_stride_bytes"] and three.info()["add_us"] > 0


def test_empty_store_and_empty_base_answer_with_padding():
    _, cent, books, _, _, q = R.list_case()
    with _lib.RefineStore(32, _lib.SQ_REFINE_F16) as store, _lib.PqIndex(cent, books) as base:
        for dist, idx in (store.rerank(q[:2], np.zeros((2, 5), np.int64), 3), store.search(base, q[:2], 3, 5, 2)):
            assert (idx == -1).all() and np.isinf(dist).all()


def test_search_refuses_a_base_that_does_not_match(bases):
    x, cent, books, _, _, q = R.list_case()
    with _store(x[:500], "f16") as short, _store(x, "f16", id_base=7) as shifted, _store(np.ascontiguousarray(x[:, :16]), "f16") as narrow, \
            _store(x, "f16") as store:
        for bad in (short, shifted, narrow):
            with pytest.raises(_lib.HipError, match="code -1"):
                bad.search(bases["plain"], q[:1, :bad.d], 3, 5, 2)
        dense = _lib.DenseIndex(np.array(x))
        with pytest.raises(_lib.HipError, match="code -4"):
            store.search(dense, q[:1], 3, 5, 2)
        dense.close()


def test_sq8_zero_step_column_and_non_finite_row():
    x, vmin, step, q, cand = R.width_case(9)
    x, step = x.copy(), step.copy()
    step[4] = 0
    x[3, :3] = (np.nan, np.inf, -np.inf)
    with _store(x, "sq8", vmin, step, R.ID_BASE) as store:
        np.testing.assert_array_equal(store.rows(), R.encode(x, _lib.SQ_REFINE_SQ8, vmin, step))
        got = store.rerank(q, cand, R.K)
    _same(got, R.rerank(_decoded(x, "sq8", vmin, step), R.ID_BASE, q, cand, R.K))


@pytest.mark.parametrize("refine,packed", [("fp16", False), ("sq8", True), ("f32", False)])
def test_plugin_follows_a_store_built_by_hand(refine, packed):
    """After build, update with new and with replaced uuids, and remove: `nn_many` is a RefineStore.search over the same
    centroids, codebooks and rows; `nn` orders its elements by the original vectors."""
    vecs = (np.random.default_rng(31).standard_normal((300, 16)) * 3).astype(np.float32)
    descr = [DescriptorMemoryElement(i) for i in range(300)]
    for e, v in zip(descr, vecs):
        e.set_vector(v)
    index = HipIvfPqRefineNearestNeighborsIndex(nlist=8, nprobe=3, m=4, packed=packed, refine=refine, k_factor=3, train_iters=3, random_seed=4)

    def check():
        rows = np.vstack([e.vector() for e in index._elements]).astype(np.float32)
        kind = {"fp16": "f16"}.get(refine, refine)
        with _lib.PqIndex(index._centroids, index._codebooks, residual=True, packed=packed) as base, \
                _store(rows, kind, *(index._ranges or (None, None))) as store:
            base.add(rows)
            want = store.search(base, vecs[:5], 7, 21, 3)
        idx, dist = index.nn_many(vecs[:5], 7)
        _same((dist, idx), want)

    index.build_index(descr[:250])
    check()
    index.update_index(descr[250:])
    check()
    moved = DescriptorMemoryElement(7)
    moved.set_vector(vecs[7] + np.float32(5))
    index.update_index([moved])
    check()
    index.remove_from_index(list(range(10, 20)))
    assert index.count() == 290
    check()
    elems, dists = index.nn(descr[30], 5)
    rows = index.nn_many(vecs[30:31], 5)[0][0]
    assert sorted(e.uuid() for e in elems) == sorted(index._elements[i].uuid() for i in rows) and list(dists) == sorted(dists)
