"""
CPU tests of the host side of dense removal: the three new entry points are declared, bound
and exported; the brute-force plugin hands removals to the device index (a recording stand-in here) and searches with
plain k; MutableShardedIndex does the same with a local index that offers `remove`.  Nothing here launches a kernel:
the device side is tests/test_hip_dense_remove.py.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import cpu_ref as O
from smqtk_indexing_amd import _lib
from smqtk_indexing_amd._compat import DescriptorMemoryElement, ReadOnlyError
from smqtk_indexing_amd.impls.nn_index.hip_bruteforce import HipBruteForceNearestNeighborsIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sq_dense_remove", "sq_dense_compact", "sq_dense_count")


# --------------------------------------------------------------------------------------------------------- ABI
def test_new_entry_points_are_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "smqtk_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(sq_[a-z0-9_]+)\s*\(", code)))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name
        assert getattr(_lib.load(), name).restype is ctypes.c_int
    # each documented in the style of its neighbours: the comment in front of the prototype cites the reference
    for name in NEW:
        doc = src[:src.index("int %s(" % name)]
        doc = doc[doc.rindex("/*"):]
        assert "faiss.py:644-694" in doc, name
    # header count = export count, as VERDICT.md checks it: the library's dynamic sq_* symbols are the declared ones
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = sorted({ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("sq_")})
    assert exported == declared
    assert len(declared) == len(_lib.EXPORTS) == 44
    # sq_dense_info keeps its fields
    assert re.search(r"#define SQ_DENSE_INFO_FIELDS 10\b", src)
    for meth in ("remove", "compact", "count"):
        assert callable(getattr(_lib.DenseIndex, meth))


def test_raw_abi_refuses_unknown_handles_and_bad_arguments():
    lib = _lib.load()
    ids = (ctypes.c_int64 * 2)(1, 2)
    n = ctypes.c_int64(0)
    assert lib.sq_dense_remove(12345, ids, 2) == -1
    assert b"unknown handle" in lib.sq_last_error()
    assert lib.sq_dense_compact(12345, None) == -1
    assert lib.sq_dense_count(12345, ctypes.byref(n), ctypes.byref(n)) == -1


# ------------------------------------------------------------------------------------------------------ plugin
class RecordingDense:
    """Stands where `_lib.DenseIndex` stands in the plugin: records the calls, answers with the oracle."""

    def __init__(self, matrix, metric="euclidean"):
        self.rows = np.array(matrix, dtype=np.float32)
        self.dead = np.zeros(len(self.rows), dtype=bool)
        self.metric = metric
        self.calls = []
        self.closed = False

    @property
    def n(self):
        return len(self.rows)

    def search(self, q, k):
        self.calls.append(("search", int(k)))
        live = np.flatnonzero(~self.dead)
        dist = np.full((len(q), k), np.inf, dtype=np.float32 if self.metric == "euclidean" else np.float64)
        idx = np.full((len(q), k), -1, dtype=np.int64)
        for j, v in enumerate(np.asarray(q, dtype=np.float32)):
            rd, ri = O.dense_topk(self.rows[live], v, k, self.metric)
            dist[j, :len(rd)], idx[j, :len(ri)] = rd, live[ri]
        return dist, idx

    def remove(self, ids):
        ids = np.asarray(ids, dtype=np.int64)
        self.calls.append(("remove", ids.tolist()))
        assert len(set(ids.tolist())) == len(ids) and (ids >= 0).all() and (ids < self.n).all() and not self.dead[ids].any()
        self.dead[ids] = True

    def append(self, rows):
        self.calls.append(("append", len(rows)))
        self.rows = np.concatenate([self.rows, np.asarray(rows, dtype=np.float32)])
        self.dead = np.concatenate([self.dead, np.zeros(len(rows), dtype=bool)])

    def compact(self):
        self.calls.append(("compact",))
        old_to_new = np.where(self.dead, -1, np.cumsum(~self.dead) - 1).astype(np.int64)
        self.rows, self.dead = self.rows[~self.dead], np.zeros(int((~self.dead).sum()), dtype=bool)
        return old_to_new

    def count(self):
        return self.n, int((~self.dead).sum())

    def close(self):
        self.closed = True


def _elems(x, base=0):
    return [DescriptorMemoryElement(base + i).set_vector(v) for i, v in enumerate(x)]


def _plugin(x, metric="euclidean"):
    index = HipBruteForceNearestNeighborsIndex(metric)
    index.build_index(_elems(x))
    index._dev = RecordingDense(index._matrix, metric)
    return index, index._dev


def _agrees(index, vectors, live_uuid_to_vec, k, metric="euclidean"):
    uu = np.array(sorted(live_uuid_to_vec))
    mat = np.stack([live_uuid_to_vec[u] for u in uu]).astype(np.float32)
    for qv in vectors:
        idx, dist = index.nn_many(qv[None, :], k)
        rd, ri = O.dense_topk(mat, qv, k, metric)
        assert [e.uuid() for e in index.elements_of(idx[0])] == uu[ri].tolist()
        np.testing.assert_array_equal(dist[0], rd)


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_plugin_removes_on_the_device_and_searches_with_plain_k(metric):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((400, 12)).astype(np.float32)
    index, dev = _plugin(x, metric)
    live = {i: x[i] for i in range(400)}
    gone = [7, 300, 8, 120]
    index.remove_from_index(gone)
    assert dev.calls == [("remove", sorted(gone))]          # the rows of those uuids, once, nothing else
    assert index._dev is dev and index.count() == 396 and not dev.closed
    for g in gone:
        del live[g]
    dev.calls.clear()
    index.nn_many(x[:3], 10)
    assert dev.calls == [("search", 10)]                    # plain k: no k + dead, nothing filtered on the host
    _agrees(index, [x[7], x[5]], live, 10, metric)
    index.nn_many(x[:2], 1000)                              # k is clamped to the live count, as it was to n
    assert dev.calls[-1] == ("search", 396)
    # KeyError before any change (nearest_neighbor_index.py:84-94), for unknown and for already removed uuids
    dev.calls.clear()
    for bad in ([5, 9999], [5, 7]):
        with pytest.raises(KeyError):
            index.remove_from_index(bad)
    assert dev.calls == [] and index.count() == 396
    _agrees(index, [x[5]], live, 3, metric)
    # an append goes behind the removed rows; ids are stable
    index.update_index(_elems(x[:4] + 0.5, base=1000))
    assert ("append", 4) in dev.calls and ("compact",) not in dev.calls
    live.update({1000 + i: x[i] + 0.5 for i in range(4)})
    _agrees(index, [x[0] + 0.5, x[7]], live, 5, metric)


def test_plugin_compacts_past_a_quarter_and_renumbers():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((200, 8)).astype(np.float32)
    index, dev = _plugin(x)
    live = {i: x[i] for i in range(200)}
    index.remove_from_index(list(range(0, 100, 2)))         # 50 of 200: exactly a quarter, not past it
    assert ("compact",) not in dev.calls and len(index._dead) == 50
    for g in range(0, 100, 2):
        del live[g]
    _agrees(index, [x[0], x[150]], live, 7)
    index.remove_from_index([199])                          # 51 of 200: the device compacts, the host follows
    del live[199]
    assert dev.calls[-1] == ("compact",) and index._dev is dev and not dev.closed
    assert not index._dead and index.count() == 149 and dev.count() == (149, 149)
    assert len(index._elements) == 149 and all(e is not None for e in index._elements)
    assert index._matrix.shape == (149, 8)
    # elements_of still returns the right descriptors: row r of the device is _elements[r] is row r of the host blocks
    for r, e in enumerate(index._elements):
        assert index._row_of[e.uuid()] == r
        np.testing.assert_array_equal(index._matrix[r], x[e.uuid()])
        np.testing.assert_array_equal(dev.rows[r], x[e.uuid()])
    _agrees(index, [x[0], x[150], x[199]], live, 9)
    # and the renumbered index keeps mutating in place
    index.update_index(_elems(x[:3] + 2.0, base=500))
    index.remove_from_index([1, 500])
    live.update({501: x[1] + 2.0, 502: x[2] + 2.0})
    del live[1]
    assert dev.calls[-1][0] == "remove" and len(dev.calls[-1][1]) == 2 and ("compact",) not in dev.calls[-3:]
    _agrees(index, [x[1], x[2] + 2.0], live, 6)


def test_plugin_read_only_and_no_device_paths_are_unchanged():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((50, 6)).astype(np.float32)
    ro = HipBruteForceNearestNeighborsIndex(read_only=True)
    with pytest.raises(ReadOnlyError):
        ro.remove_from_index([1])
    # without a device index the host rebuilds its state, as before (no GPU is needed to remove)
    index = HipBruteForceNearestNeighborsIndex()
    index.build_index(_elems(x))
    index.remove_from_index([3, 4])
    assert index._dev is None and index.count() == 48 and not index._dead
    assert [e.uuid() for e in index._elements] == [i for i in range(50) if i not in (3, 4)]
    # removing every row leaves the device index behind (it holds at least one row) and an empty plugin
    index, dev = _plugin(x)
    index.remove_from_index(list(range(50)))
    assert index.count() == 0 and index._dev is None and dev.closed and ("remove", list(range(50))) not in dev.calls


# ------------------------------------------------------------------------------------------------------ shards
def test_mutable_sharded_index_with_a_local_index_that_removes(tmp_path):
    import torch
    import torch.distributed as dist
    from smqtk_indexing_amd.distributed import MutableShardedIndex

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = "29533"
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        rng = np.random.default_rng(6)
        d, k = 8, 10
        db = rng.standard_normal((6000, d)).astype(np.float32)
        qs = rng.standard_normal((3, d)).astype(np.float32)
        log = []

        def build_local(rows, removes=True):
            mat = rows.numpy().copy()
            dead = np.zeros(len(mat), dtype=bool)
            log.append(("build", len(mat)))

            def search(queries, kk):
                log.append(("search", int(kk)))
                live = np.flatnonzero(~dead)
                dd = np.full((len(queries), kk), np.inf, np.float32)
                ii = np.full((len(queries), kk), -1, np.int64)
                for j, q in enumerate(np.asarray(queries, dtype=np.float32)):
                    a, b = O.dense_topk(mat[live], q, kk)
                    dd[j, :len(a)], ii[j, :len(b)] = a, live[b]
                return torch.from_numpy(dd), torch.from_numpy(ii)

            def remove(local_rows):
                local_rows = np.asarray(local_rows)
                log.append(("remove", len(local_rows)))
                assert not dead[local_rows].any()
                dead[local_rows] = True
            if removes:
                search.remove = remove
            return search

        def check(idx, live):
            ids = np.array(sorted(live))
            mat = np.stack([live[i] for i in ids])
            dd, ii = idx.search(torch.from_numpy(qs), k)
            for j in range(len(qs)):
                rd, ri = O.dense_topk(mat, qs[j], k)
                np.testing.assert_array_equal(ii[j], ids[ri])
                np.testing.assert_array_equal(dd[j].view(np.uint32), rd.view(np.uint32))

        idx = MutableShardedIndex(torch.from_numpy(db.copy()), 0, len(db), build_local)
        live = {i: db[i] for i in range(len(db))}
        top = set()
        for q in qs:
            top.update(int(r) for r in O.dense_topk(db, q, k)[1])
        gone = sorted(top | set([r for r in range(2000, 3100) if r not in top][:1025 - len(top)]))
        assert len(gone) == 1025                               # past max_dead = 1024, under compact_at = 25 %
        log.clear()
        idx.remove(gone)
        assert log == [("remove", 1025)]                       # no rebuild
        for g in gone:
            del live[g]
        check(idx, live)
        assert log[-1] == ("search", k) and ("build", 6000) not in log   # k passed through, not k + dead
        with pytest.raises(KeyError):
            idx.remove([gone[0]])
        # an append rebuilds the local index from all local rows: the dead ones are removed from it again
        log.clear()
        nid = idx.append(torch.from_numpy(qs + np.float32(0.01)))
        assert log == [("build", 6003), ("remove", 1025)]
        live.update({int(a): v for a, v in zip(nid, qs + np.float32(0.01))})
        check(idx, live)
        # compact_at still compacts
        log.clear()
        more = [r for r in range(3100, 3800) if r not in top][:600]
        idx.remove(more)
        assert log == [("build", 6003 - 1625)] and int(idx.dead.sum()) == 0
        for g in more:
            del live[g]
        check(idx, live)
        # a local index without `remove` keeps today's behaviour: k + dead, rebuild past max_dead
        idx2 = MutableShardedIndex(torch.from_numpy(db.copy()), 0, len(db), lambda rows: build_local(rows, removes=False))
        log.clear()
        idx2.remove(gone[:1000])
        idx2.search(torch.from_numpy(qs), k)
        assert log == [("search", k + 1000)]
        log.clear()
        idx2.remove(gone[1000:])
        assert log == [("build", 6000 - 1025)]
    finally:
        dist.destroy_process_group()
