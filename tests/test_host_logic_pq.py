"""
The host side of the IVF-PQ index, without a GPU.

1. `HipIvfPqNearestNeighborsIndex`'s own logic: the configuration round trip, the constructor's `ValueError`s,
   `read_only`, the training plan (the IVF-Flat class's sample and centroids, then one further draw for the codebook
   entries), and the build / update / remove state machine against a recording stand-in for the device index -- new
   uuids are one `add`, a replaced uuid and a removal code the elements' vectors again with the same centroids and
   codebooks, `KeyError` before anything changes; `nn` orders by the original vectors' distances for every dtype; and
   without a usable device `is_usable()` is False and nothing falls back to the CPU.
2. The third library: include/smqtk_hip_pq.h, `_lib.PQ_EXPORTS` and the dynamic sq_pq_* symbols of libsmqtk_hip_pq.so
   are one set, disjoint from the other two libraries' sets; and every refusal of the header's limits through the raw ABI,
   made before a device is touched.
3. tests/host/pq_plan_main.cpp over smqtk_indexing_amd/csrc/sq_pq_plan.hpp (plain C++), compiled with ROCm's clang++
   under AddressSanitizer and UndefinedBehaviorSanitizer and linked statically against the sanitizer runtime: nothing is
   preloaded and nothing is loaded into Python.
"""
import ctypes
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

from smqtk_indexing_amd import NearestNeighborsIndex, _lib
from smqtk_indexing_amd._compat import DescriptorMemoryElement, ReadOnlyError, from_config_dict, to_config_dict
from smqtk_indexing_amd.impls.nn_index.hip_ivf import HipIvfFlatNearestNeighborsIndex
from smqtk_indexing_amd.impls.nn_index.hip_ivf_pq import HipIvfPqNearestNeighborsIndex
from tests.test_host_logic_buffers import HOST, _clangxx


def _descr(uid, vec):
    d = DescriptorMemoryElement(uid)
    d.set_vector(np.asarray(vec))
    return d


class _FakePq:
    """Stands in for `_lib.PqIndex`: records what the plugin asks of the device."""
    made = []

    def __init__(self, centroids, codebooks, id_base=0):
        self.centroids, self.codebooks = np.array(centroids), np.array(codebooks)
        self.added, self.closed, self.searches = [], False, []
        self.answer = None
        _FakePq.made.append(self)

    def add(self, rows):
        self.added.append(np.array(rows))

    def search(self, q, k, nprobe):
        self.searches.append((np.array(q), k, nprobe))
        if self.answer is not None:
            return self.answer
        idx = np.full((q.shape[0], k), -1, np.int64)
        dist = np.full((q.shape[0], k), np.inf, np.float32)
        idx[:, 0], dist[:, 0] = 0, 0.5
        return dist, idx

    def close(self):
        self.closed = True


@pytest.fixture
def fake_device(monkeypatch):
    _FakePq.made = []
    trained = {"kmeans": [], "pq": []}

    def kmeans(x, centroids, iters=10):
        trained["kmeans"].append((np.array(x), np.array(centroids), iters))
        return np.array(centroids, dtype=np.float32) + np.float32(1)

    def pq_train(x, codebooks, iters=10):
        trained["pq"].append((np.array(x), np.array(codebooks), iters))
        return np.array(codebooks, dtype=np.float32) + np.float32(2)

    monkeypatch.setattr(_lib, "usable", lambda: True)
    monkeypatch.setattr(_lib, "PqIndex", _FakePq)
    monkeypatch.setattr(_lib, "ivf_kmeans", kmeans)
    monkeypatch.setattr(_lib, "pq_train", pq_train)
    monkeypatch.setattr(_lib, "dense_distances", lambda q, rows, metric: np.sqrt(((np.asarray(rows, np.float64) - q) ** 2).sum(1)))
    return trained


# ------------------------------------------------------------------ the plugin's host logic
def test_config_round_trip_and_interface():
    assert issubclass(HipIvfPqNearestNeighborsIndex, NearestNeighborsIndex)
    i = HipIvfPqNearestNeighborsIndex()
    assert i.get_config() == {"nlist": None, "nprobe": 1, "m": 8, "train_iters": 10, "random_seed": 0, "read_only": False}
    assert HipIvfPqNearestNeighborsIndex.get_default_config() == i.get_config()
    j = HipIvfPqNearestNeighborsIndex(nlist=50, nprobe=7, m=4, train_iters=3, random_seed=11, read_only=True)
    c = j.get_config()
    assert c == {"nlist": 50, "nprobe": 7, "m": 4, "train_iters": 3, "random_seed": 11, "read_only": True}
    assert HipIvfPqNearestNeighborsIndex.from_config(c).get_config() == c
    k = from_config_dict(to_config_dict(j), [HipIvfPqNearestNeighborsIndex])
    assert isinstance(k, HipIvfPqNearestNeighborsIndex) and k.get_config() == c
    assert i.count() == 0 and len(i) == 0
    assert HipIvfPqNearestNeighborsIndex.is_usable() == _lib.pq_usable()


def test_constructor_value_errors():
    for bad in (0, -3):
        with pytest.raises(ValueError, match="nprobe"):
            HipIvfPqNearestNeighborsIndex(nprobe=bad)
    for bad in (0, -1, _lib.SQ_IVF_MAX_LISTS + 1):
        with pytest.raises(ValueError, match="nlist"):
            HipIvfPqNearestNeighborsIndex(nlist=bad)
    for bad in (0, -1, _lib.SQ_PQ_MAX_M + 1):
        with pytest.raises(ValueError, match="m must"):
            HipIvfPqNearestNeighborsIndex(m=bad)
    with pytest.raises(ValueError, match="train_iters"):
        HipIvfPqNearestNeighborsIndex(train_iters=-1)
    with pytest.raises(TypeError):
        HipIvfPqNearestNeighborsIndex(distance_method="cosine")          # there is no such choice: L2 only
    HipIvfPqNearestNeighborsIndex(nlist=_lib.SQ_IVF_MAX_LISTS, nprobe=1, m=_lib.SQ_PQ_MAX_M, train_iters=0)
    assert (_lib.SQ_PQ_MAX_M, _lib.SQ_PQ_MAX_KSUB, _lib.SQ_PQ_INFO_FIELDS) == (64, 256, 10)


def test_training_plan_extends_the_ivf_flat_plan():
    for n, nlist, seed in ((5000, 4, 9), (700, 4, 9), (3, 64, 0), (100_000, None, 2)):
        pq = HipIvfPqNearestNeighborsIndex(nlist=nlist, random_seed=seed)
        flat = HipIvfFlatNearestNeighborsIndex(nlist=nlist, random_seed=seed)
        assert pq.effective_nlist(n) == flat.effective_nlist(n)
        sample, init, entries = pq.training_plan(n)
        f_sample, f_init = flat.training_plan(n)
        assert np.array_equal(sample, f_sample) and np.array_equal(init, f_init)
        ksub = min(256, len(sample))
        assert entries.shape == (ksub,) and np.unique(entries).shape == (ksub,) and entries.max() < len(sample)
        # one further draw from the same generator
        rs = np.random.RandomState(seed)
        m = len(sample)
        if m < n:
            rs.choice(n, size=m, replace=False)
        rs.choice(m, size=pq.effective_nlist(n), replace=False)
        assert np.array_equal(entries, rs.choice(m, size=ksub, replace=False))


def test_build_update_remove_state_machine(fake_device):
    rng = np.random.default_rng(3)
    vecs = rng.standard_normal((40, 6)).astype(np.float32)
    idx = HipIvfPqNearestNeighborsIndex(nlist=5, nprobe=2, m=3, train_iters=4, random_seed=1)
    with pytest.raises(ValueError):
        idx.build_index([])
    with pytest.raises(ValueError, match="sub-vectors"):                 # d % m != 0, at build
        HipIvfPqNearestNeighborsIndex(m=4).build_index([_descr(i, vecs[i]) for i in range(30)])
    assert not _FakePq.made and not fake_device["kmeans"] and not fake_device["pq"]
    idx.build_index([_descr(i, vecs[i]) for i in range(30)] + [_descr(3, vecs[3])])     # a repeated uuid counts once
    assert idx.count() == 30 and len(fake_device["kmeans"]) == 1 and len(fake_device["pq"]) == 1 and len(_FakePq.made) == 1
    sample, init, entries = idx.training_plan(30)
    x, c0, iters = fake_device["kmeans"][0]
    assert iters == 4 and np.array_equal(x, vecs[:30][sample]) and np.array_equal(c0, vecs[:30][sample][init])
    x, b0, iters = fake_device["pq"][0]
    assert iters == 4 and np.array_equal(x, vecs[:30][sample]) and b0.shape == (3, 30, 2)          # ksub = min(256, 30 sample rows)
    for j in range(3):                                                   # the same draw serves every sub-quantiser
        assert np.array_equal(b0[j], vecs[:30][sample][entries][:, 2 * j:2 * j + 2])
    dev = _FakePq.made[0]
    assert np.array_equal(dev.centroids, c0 + 1) and np.array_equal(dev.codebooks, b0 + 2)
    assert len(dev.added) == 1 and np.array_equal(dev.added[0], vecs[:30])
    assert not hasattr(idx, "_blocks") and not hasattr(idx, "_matrix")   # no host copy of the matrix
    # new uuids join the existing lists: one add, no training, no new device index
    idx.update_index([_descr(i, vecs[i]) for i in range(30, 36)])
    assert idx.count() == 36 and len(fake_device["kmeans"]) == 1 and len(fake_device["pq"]) == 1 and len(_FakePq.made) == 1
    assert len(dev.added) == 2 and np.array_equal(dev.added[1], vecs[30:36]) and not dev.closed
    assert [e.uuid() for e in idx.elements_of(range(36))] == list(range(36))
    # a replaced uuid codes the elements' vectors again with the same centroids and codebooks
    repl = vecs[5] + np.float32(2)
    idx.update_index([_descr(5, repl), _descr(36, vecs[36])])
    assert idx.count() == 37 and len(fake_device["pq"]) == 1 and len(_FakePq.made) == 2 and dev.closed
    dev2 = _FakePq.made[1]
    assert np.array_equal(dev2.centroids, dev.centroids) and np.array_equal(dev2.codebooks, dev.codebooks) and len(dev2.added) == 1
    keep = [i for i in range(36) if i != 5]
    assert np.array_equal(dev2.added[0], np.vstack([vecs[keep], repl[None], vecs[36][None]]))
    assert [e.uuid() for e in idx.elements_of(range(37))] == keep + [5, 36]
    # unknown uuids: KeyError before anything changes
    with pytest.raises(KeyError):
        idx.remove_from_index([0, 1, 999])
    assert idx.count() == 37 and len(_FakePq.made) == 2 and not dev2.closed
    with pytest.raises(ValueError):
        idx.remove_from_index([])
    idx.remove_from_index([0, 36])
    assert idx.count() == 35 and len(_FakePq.made) == 3 and dev2.closed and len(fake_device["kmeans"]) == 1
    dev3 = _FakePq.made[2]
    assert np.array_equal(dev3.codebooks, dev.codebooks)
    assert np.array_equal(dev3.added[0], np.vstack([vecs[[i for i in keep if i != 0]], repl[None]]))
    # searches carry k = min(n, count) and the configured nprobe; -1 entries are dropped and warned about; the distance
    # is the original vectors', not the coded 0.5
    q = _descr("q", vecs[1])
    with pytest.warns(RuntimeWarning, match="nprobe"):
        elems, dists = idx.nn(q, 3)
    assert dev3.searches[-1][1:] == (3, 2) and [e.uuid() for e in elems] == [1] and dists == (0.0,)
    idx.nn_many(vecs[:4], 1000)
    assert dev3.searches[-1][1:] == (35, 2) and dev3.searches[-1][0].shape == (4, 6)
    # float32 descriptors too are ordered by their own distances: the coded order (row 2 first) is overruled
    dev3.answer = (np.array([[0.25, 0.5]], np.float32), np.array([[2, 0]], np.int64))
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                # enough neighbours: no warning
        elems, dists = idx.nn(q, 2)
    d_of = {u: float(np.sqrt(((vecs[u].astype(np.float64) - vecs[1]) ** 2).sum())) for u in (1, 3)}
    assert [e.uuid() for e in idx.elements_of([2, 0])] == [3, 1]
    assert [e.uuid() for e in elems] == [1, 3] and dists == (d_of[1], d_of[3]) and dists[0] == 0.0
    # removing everything empties the index; an update then builds (and trains) afresh
    idx.remove_from_index([e.uuid() for e in idx.elements_of(range(35))])
    assert idx.count() == 0 and len(_FakePq.made) == 3 and dev3.closed
    with pytest.raises(ValueError, match="No index"):
        idx.nn(q, 1)
    idx.update_index([_descr(i, vecs[i]) for i in range(8)])
    assert idx.count() == 8 and len(fake_device["pq"]) == 2 and len(_FakePq.made) == 4
    with pytest.raises(ValueError, match="dimensions"):
        idx.update_index([_descr(100, np.zeros(7, np.float32))])
    assert idx.count() == 8


def test_nn_hands_the_float32_query_and_the_original_vectors_to_dense_distances(fake_device, monkeypatch):
    vecs = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 3.0]])
    idx = HipIvfPqNearestNeighborsIndex(nlist=1, m=2)
    idx.build_index([_descr(i, vecs[i]) for i in range(3)])          # float64 vectors
    seen = []

    def distances(q, rows, metric):
        seen.append((q.dtype, rows.dtype, metric))
        return np.array([9.0, 4.0])

    monkeypatch.setattr(_lib, "dense_distances", distances)
    _FakePq.made[-1].answer = (np.array([[1.0, 2.0]], np.float32), np.array([[1, 2]], np.int64))
    elems, dists = idx.nn(_descr("q", np.zeros(2)), 2)
    assert seen == [(np.float32, np.float64, _lib.SQ_METRIC_L2)]
    assert [e.uuid() for e in elems] == [2, 1] and dists == (4.0, 9.0)


def test_read_only(fake_device):
    idx = HipIvfPqNearestNeighborsIndex(read_only=True)
    d = [_descr(0, np.zeros(8, np.float32))]
    for call in (idx.build_index, idx.update_index):
        with pytest.raises(ReadOnlyError):
            call(d)
    with pytest.raises(ReadOnlyError):
        idx.remove_from_index([0])
    assert idx.count() == 0 and not fake_device["pq"] and not _FakePq.made


def test_without_a_usable_device_nothing_falls_back(monkeypatch):
    monkeypatch.setattr(_lib, "usable", lambda: False)
    assert not HipIvfPqNearestNeighborsIndex.is_usable()
    idx = HipIvfPqNearestNeighborsIndex(nlist=2, m=2)
    with pytest.raises(_lib.HipError, match="no CPU fallback"):
        idx.build_index([_descr(i, np.full(4, i, np.float32)) for i in range(5)])
    assert idx.count() == 0
    with pytest.raises(ValueError, match="No index"):
        idx.nn(_descr("q", np.zeros(4, np.float32)), 1)


def test_without_the_third_library_the_class_is_not_usable(monkeypatch):
    monkeypatch.setattr(_lib, "usable", lambda: True)
    monkeypatch.setattr(_lib, "PQ_LIB_PATH", os.path.join(os.path.dirname(_lib.PQ_LIB_PATH), "no_such_library.so"))
    assert not _lib.pq_usable() and not HipIvfPqNearestNeighborsIndex.is_usable()


# ------------------------------------------------------------------ the third library
def test_third_library_exports_what_its_header_declares():
    root = os.path.dirname(os.path.dirname(HOST))

    def declared(header):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", header)).read(), flags=re.S)
        return sorted(set(re.findall(r"\b(sq_[a-z0-9_]+)\s*\(", src)))

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
        return sorted({ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("sq_")})

    assert declared("smqtk_hip_pq.h") == sorted(_lib.PQ_EXPORTS) == exported(_lib.PQ_LIB_PATH)
    assert all(name.startswith("sq_pq_") for name in _lib.PQ_EXPORTS) and len(set(_lib.PQ_EXPORTS)) == len(_lib.PQ_EXPORTS)
    for other_exports, other_path, header in ((_lib.EXPORTS, _lib.LIB_PATH, "smqtk_hip.h"), (_lib.IVF_EXPORTS, _lib.IVF_LIB_PATH, "smqtk_hip_ivf.h")):
        assert not set(_lib.PQ_EXPORTS) & set(other_exports)
        assert not set(_lib.PQ_EXPORTS) & set(exported(other_path)) and not set(_lib.PQ_EXPORTS) & set(declared(header))
    pq = _lib.load_pq()
    assert all(getattr(pq, name).restype is ctypes.c_int for name in _lib.PQ_EXPORTS)
    # found beside the libraries it is built on
    dyn = subprocess.run(["readelf", "-d", _lib.PQ_LIB_PATH], check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
    assert "libsmqtk_hip.so" in dyn and "libsmqtk_hip_ivf.so" in dyn and "$ORIGIN" in dyn


def test_abi_refuses_bad_calls_before_touching_a_device():
    core, lib = _lib.load(), _lib.load_pq()
    h = ctypes.c_int64(0)
    x = np.zeros((300, 8), np.float32)
    p = x.ctypes.data

    def create(nlist, d, m, ksub):
        return lib.sq_pq_create(p, nlist, d, p, m, ksub, 0, ctypes.byref(h))

    def train(n, d, m, ksub, mem=0):
        return lib.sq_pq_train(p, n, d, m, ksub, p, 1, mem)

    # d % m != 0
    assert create(4, 8, 3, 16) == -1 and b"no multiple" in core.sq_last_error()
    assert train(300, 8, 3, 16) == -1 and b"no multiple" in core.sq_last_error()
    # m outside 1 .. 64
    for m in (0, -1, 65):
        assert create(4, 130, m, 16) == -1 and b"m = " in core.sq_last_error()
        assert train(300, 130, m, 16) == -1 and b"m = " in core.sq_last_error()
    # ksub outside 1 .. 256
    for ksub in (0, -2, 257):
        assert create(4, 8, 2, ksub) == -1 and b"ksub" in core.sq_last_error()
        assert train(300, 8, 2, ksub) == -1 and b"ksub" in core.sq_last_error()
    # sub-vectors beyond 16384 floats: the tables kernel stages one in 64 KiB of LDS
    assert create(4, 16385, 1, 16) == -4 and b"sub-vectors" in core.sq_last_error()
    assert train(300, 2 * 16385, 2, 16) == -4 and b"sub-vectors" in core.sq_last_error()
    # nlist > 65536: the coarse rule
    assert create(_lib.SQ_IVF_MAX_LISTS + 1, 8, 2, 16) == -4 and b"lists" in core.sq_last_error()
    # training with fewer rows than entries
    assert train(15, 8, 2, 16) == -1 and b"cannot train" in core.sq_last_error()
    assert train(300, 8, 2, 16, mem=_lib.SQ_MEM_DEVICE_ASYNC) == -4
    # a search in any mode but the two blocking ones, whatever the handle
    for mem in (_lib.SQ_MEM_DEVICE_ASYNC, _lib.SQ_MEM_PLAN, _lib.SQ_MEM_PLAN_ASYNC, 9, -1):
        assert lib.sq_pq_search(12345, p, 1, 1, 1, p, p, mem, None) == -4 and b"blocking calls only" in core.sq_last_error()
    # null pointers and unknown handles
    assert lib.sq_pq_create(None, 4, 8, p, 2, 16, 0, ctypes.byref(h)) == -1
    assert lib.sq_pq_create(p, 4, 8, None, 2, 16, 0, ctypes.byref(h)) == -1
    for call in (lambda: lib.sq_pq_add(12345, p, 4, 0), lambda: lib.sq_pq_lists(12345, None, None, None),
                 lambda: lib.sq_pq_search(12345, p, 1, 1, 1, p, p, 0, None), lambda: lib.sq_pq_destroy(12345)):
        assert call() == -1 and b"unknown handle" in core.sq_last_error()
    out = (ctypes.c_int64 * _lib.SQ_PQ_INFO_FIELDS)()
    assert lib.sq_pq_info(12345, out, _lib.SQ_PQ_INFO_FIELDS) == -1
    assert h.value == 0


@pytest.mark.gpu
def test_search_modes_other_than_blocking_are_refused():
    """`mem` of a search other than SQ_MEM_HOST / SQ_MEM_DEVICE: SQ_ERR_UNSUPPORTED (the check needs a handle, and a
    handle needs a device)."""
    lib = _lib.load_pq()
    rng = np.random.default_rng(1)
    x = rng.standard_normal((64, 8)).astype(np.float32)
    books = np.ascontiguousarray(x[:16].reshape(16, 2, 4).transpose(1, 0, 2))
    with _lib.PqIndex(x[:4], books) as idx:
        idx.add(x)
        dist, ids = np.empty((1, 4), np.float32), np.empty((1, 4), np.int64)
        for mem in (_lib.SQ_MEM_DEVICE_ASYNC, _lib.SQ_MEM_PLAN, 9):
            assert lib.sq_pq_search(idx.handle, x.ctypes.data, 1, 4, 1, dist.ctypes.data, ids.ctypes.data, mem, None) == -4
        assert lib.sq_pq_search(idx.handle, x.ctypes.data, 1, 4, 0, dist.ctypes.data, ids.ctypes.data, 0, None) == -1   # nprobe < 1


# ------------------------------------------------------------------ sq_pq_plan.hpp under sanitizers
@pytest.mark.skipif(_clangxx() is None, reason="ROCm's clang++ is not installed: nothing to compile the program with")
def test_plan_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pq_plan_main")
    cmd = [_clangxx(), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libsan",
           os.path.join(HOST, "pq_plan_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, "compiling tests/host/pq_plan_main.cpp failed:\n" + r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0, "status %d:\n%s" % (r.returncode, r.stdout[-4000:])
    assert "pq plan ok" in r.stdout, r.stdout[-4000:]
    for word in ("Sanitizer", "runtime error"):
        assert word not in r.stdout, r.stdout[-4000:]
    fields = dict(w.split("=") for w in r.stdout.split("pq plan ok:")[1].split())
    assert (int(fields["max_m"]), int(fields["max_ksub"]), int(fields["lds_max"])) == (_lib.SQ_PQ_MAX_M, _lib.SQ_PQ_MAX_KSUB, 65536)
    # the Python restatement of pq_scan_groups (tests/pq_cases.py) against the real function, line by line
    from tests import pq_cases
    real = {tuple(map(int, ln.split()[1:4])): int(ln.split()[4]) for ln in r.stdout.splitlines() if ln.startswith("groups ")}
    assert len(real) > 3000
    for (chunks, nq, cus), g in real.items():
        assert pq_cases.pq_scan_groups(chunks, nq, cus) == g, (chunks, nq, cus, g)
    # ... and the triples the strided-scan tests run are among them, in the regime each is meant for
    for d, m in pq_cases.S_SHAPES:
        case = pq_cases.make_strided_case(d, m)
        for nprobe in pq_cases.S_NPROBES:
            for nq in pq_cases.S_NQS:
                plan = pq_cases.strided_plan(case, nprobe, nq, pq_cases.S_CUS)
                assert real[(plan["chunks"], nq, pq_cases.S_CUS)] == plan["groups"]
                pq_cases.assert_regime(plan, nq, case.what)
