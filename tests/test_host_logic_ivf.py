"""
The host side of the IVF-Flat index, without a GPU.

1. `HipIvfFlatNearestNeighborsIndex`'s own logic: the configuration round trip, the constructor's `ValueError`s,
   `read_only`, the `nlist` rule and the training plan, and the build / update / remove state machine -- which calls
   join the existing lists (`add`), which rebuild them with the same centroids, `KeyError` before anything changes --
   against a recording stand-in for the device index; and what happens without a usable device: `is_usable()` is
   False and nothing falls back to the CPU.
2. tests/host/ivf_plan_main.cpp over smqtk_indexing_amd/csrc/sq_ivf_plan.hpp (plain C++), compiled with ROCm's clang++
   under AddressSanitizer and UndefinedBehaviorSanitizer and linked statically against the sanitizer runtime: nothing is
   preloaded and nothing is loaded into Python.  It checks the counting sort's offsets against a direct sort, the scan's
   chunks at list lengths 0, 1, chunk - 1, chunk, chunk + 1, `ivf_locate` over prefix arrays of 65, 257 and 700 entries
   with runs of empty lists, the slice sizes under the key budget, and the 64-bit products at 2^32 - 1 rows.
"""
import math
import os
import subprocess
import warnings

import numpy as np
import pytest

from smqtk_indexing_amd import NearestNeighborsIndex, _lib
from smqtk_indexing_amd._compat import DescriptorMemoryElement, ReadOnlyError, from_config_dict, to_config_dict
from smqtk_indexing_amd.impls.nn_index import hip_ivf
from smqtk_indexing_amd.impls.nn_index.hip_ivf import HipIvfFlatNearestNeighborsIndex
from tests.test_host_logic_buffers import HOST, _clangxx


def _descr(uid, vec):
    d = DescriptorMemoryElement(uid)
    d.set_vector(np.asarray(vec))
    return d


class _FakeIvf:
    """Stands in for `_lib.IvfIndex`: records what the plugin asks of the device."""
    made = []

    def __init__(self, centroids, id_base=0, metric=_lib.SQ_METRIC_L2):
        self.centroids = np.array(centroids)
        self.added, self.closed, self.searches = [], False, []
        self.answer = None
        _FakeIvf.made.append(self)

    def add(self, rows):
        self.added.append(np.array(rows))

    @property
    def n(self):
        return sum(a.shape[0] for a in self.added)

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
    _FakeIvf.made = []
    trained = []

    def kmeans(x, centroids, iters=10):
        trained.append((np.array(x), np.array(centroids), iters))
        return np.array(centroids, dtype=np.float32) + np.float32(1)

    monkeypatch.setattr(_lib, "usable", lambda: True)
    monkeypatch.setattr(_lib, "IvfIndex", _FakeIvf)
    monkeypatch.setattr(_lib, "ivf_kmeans", kmeans)
    return trained


# ------------------------------------------------------------------ the plugin's host logic
def test_config_round_trip_and_interface():
    assert issubclass(HipIvfFlatNearestNeighborsIndex, NearestNeighborsIndex)
    i = HipIvfFlatNearestNeighborsIndex()
    assert i.get_config() == {"nlist": None, "nprobe": 1, "train_iters": 10, "random_seed": 0,
                              "distance_method": "euclidean", "read_only": False}
    assert HipIvfFlatNearestNeighborsIndex.get_default_config() == i.get_config()
    j = HipIvfFlatNearestNeighborsIndex(nlist=50, nprobe=7, train_iters=3, random_seed=11, read_only=True)
    c = j.get_config()
    assert c == {"nlist": 50, "nprobe": 7, "train_iters": 3, "random_seed": 11, "distance_method": "euclidean", "read_only": True}
    assert HipIvfFlatNearestNeighborsIndex.from_config(c).get_config() == c
    k = from_config_dict(to_config_dict(j), [HipIvfFlatNearestNeighborsIndex])
    assert isinstance(k, HipIvfFlatNearestNeighborsIndex) and k.get_config() == c
    assert i.count() == 0 and len(i) == 0
    assert HipIvfFlatNearestNeighborsIndex.is_usable() == _lib.ivf_usable()


def test_constructor_value_errors():
    for bad in (0, -3):
        with pytest.raises(ValueError, match="nprobe"):
            HipIvfFlatNearestNeighborsIndex(nprobe=bad)
    for method in ("cosine", "hik", ""):
        with pytest.raises(ValueError, match="euclidean"):
            HipIvfFlatNearestNeighborsIndex(distance_method=method)
    for bad in (0, -1, _lib.SQ_IVF_MAX_LISTS + 1):
        with pytest.raises(ValueError, match="nlist"):
            HipIvfFlatNearestNeighborsIndex(nlist=bad)
    with pytest.raises(ValueError, match="train_iters"):
        HipIvfFlatNearestNeighborsIndex(train_iters=-1)
    HipIvfFlatNearestNeighborsIndex(nlist=_lib.SQ_IVF_MAX_LISTS, nprobe=1, train_iters=0)


def test_nlist_rule_and_training_plan():
    auto = HipIvfFlatNearestNeighborsIndex()
    for n in (1, 2, 3, 15, 16, 17, 3000, 20_011, 10_000_000):
        assert auto.effective_nlist(n) == hip_ivf.default_nlist(n) == max(1, min(n, int(4 * math.sqrt(n))))
    assert [auto.effective_nlist(n) for n in (1, 2, 3, 16, 17, 3000, 10_000_000)] == [1, 2, 3, 16, 16, 219, 12649]
    given = HipIvfFlatNearestNeighborsIndex(nlist=64)
    assert [given.effective_nlist(n) for n in (1, 63, 64, 65, 10 ** 6)] == [1, 63, 64, 64, 64]      # clamped to n
    # the sample: at most 256 rows per list, without replacement, from RandomState(random_seed); then nlist distinct
    # sample rows from the same generator
    idx = HipIvfFlatNearestNeighborsIndex(nlist=4, random_seed=9)
    sample, init = idx.training_plan(5000)
    assert sample.shape == (1024,) and np.unique(sample).shape == (1024,) and 0 <= sample.min() and sample.max() < 5000
    assert init.shape == (4,) and np.unique(init).shape == (4,) and init.max() < 1024
    rs = np.random.RandomState(9)
    assert np.array_equal(sample, np.sort(rs.choice(5000, size=1024, replace=False)))
    assert np.array_equal(init, rs.choice(1024, size=4, replace=False))
    s2, i2 = HipIvfFlatNearestNeighborsIndex(nlist=4, random_seed=9).training_plan(5000)
    assert np.array_equal(s2, sample) and np.array_equal(i2, init)
    s3, _ = HipIvfFlatNearestNeighborsIndex(nlist=4, random_seed=10).training_plan(5000)
    assert not np.array_equal(s3, sample)
    sample, init = idx.training_plan(700)                             # fewer rows than 256 per list: all of them
    assert np.array_equal(sample, np.arange(700)) and np.unique(init).shape == (4,)
    sample, init = HipIvfFlatNearestNeighborsIndex(nlist=64).training_plan(3)
    assert sample.tolist() == [0, 1, 2] and sorted(init.tolist()) == [0, 1, 2]


def test_build_update_remove_state_machine(fake_device):
    rng = np.random.default_rng(3)
    vecs = rng.standard_normal((40, 6)).astype(np.float32)
    idx = HipIvfFlatNearestNeighborsIndex(nlist=5, nprobe=2, train_iters=4, random_seed=1)
    with pytest.raises(ValueError):
        idx.build_index([])
    idx.build_index([_descr(i, vecs[i]) for i in range(30)] + [_descr(3, vecs[3])])     # a repeated uuid counts once
    assert idx.count() == 30 and len(fake_device) == 1 and len(_FakeIvf.made) == 1
    x, c0, iters = fake_device[0]
    sample, init = idx.training_plan(30)
    assert iters == 4 and np.array_equal(x, vecs[:30][sample]) and np.array_equal(c0, vecs[:30][sample][init])
    dev = _FakeIvf.made[0]
    assert np.array_equal(dev.centroids, c0 + 1) and len(dev.added) == 1 and np.array_equal(dev.added[0], vecs[:30])
    # new uuids join the existing lists: one add, no training, no new device index
    idx.update_index([_descr(i, vecs[i]) for i in range(30, 36)])
    assert idx.count() == 36 and len(fake_device) == 1 and len(_FakeIvf.made) == 1
    assert len(dev.added) == 2 and np.array_equal(dev.added[1], vecs[30:36]) and not dev.closed
    assert [e.uuid() for e in idx.elements_of(range(36))] == list(range(36))
    # a replaced uuid rebuilds the lists from the host copy with the same centroids
    repl = vecs[5] + np.float32(2)
    idx.update_index([_descr(5, repl), _descr(36, vecs[36])])
    assert idx.count() == 37 and len(fake_device) == 1 and len(_FakeIvf.made) == 2 and dev.closed
    dev2 = _FakeIvf.made[1]
    assert np.array_equal(dev2.centroids, dev.centroids) and len(dev2.added) == 1
    keep = [i for i in range(36) if i != 5]
    assert np.array_equal(dev2.added[0], np.vstack([vecs[keep], repl[None], vecs[36][None]]))
    assert [e.uuid() for e in idx.elements_of(range(37))] == keep + [5, 36]
    # unknown uuids: KeyError before anything changes
    with pytest.raises(KeyError):
        idx.remove_from_index([0, 1, 999])
    assert idx.count() == 37 and len(_FakeIvf.made) == 2 and not dev2.closed
    with pytest.raises(ValueError):
        idx.remove_from_index([])
    # removal: the lists again, same centroids, the remaining rows in their order
    idx.remove_from_index([0, 36])
    assert idx.count() == 35 and len(_FakeIvf.made) == 3 and dev2.closed and len(fake_device) == 1
    dev3 = _FakeIvf.made[2]
    assert np.array_equal(dev3.centroids, dev.centroids)
    assert np.array_equal(dev3.added[0], np.vstack([vecs[[i for i in keep if i != 0]], repl[None]]))
    # searches carry k = min(n, count) and the configured nprobe; -1 entries are dropped and warned about
    q = _descr("q", vecs[1])
    with pytest.warns(RuntimeWarning, match="nprobe"):
        elems, dists = idx.nn(q, 3)
    assert dev3.searches[-1][1:] == (3, 2) and [e.uuid() for e in elems] == [1] and dists == (0.5,)
    idx.nn_many(vecs[:4], 1000)
    assert dev3.searches[-1][1:] == (35, 2) and dev3.searches[-1][0].shape == (4, 6)
    dev3.answer = (np.array([[0.25, 0.5]], np.float32), np.array([[2, 0]], np.int64))
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                # enough neighbours: no warning
        elems, dists = idx.nn(q, 2)
    assert [e.uuid() for e in elems] == [3, 1] and dists == (0.25, 0.5)
    # removing everything empties the index; an update then builds (and trains) afresh
    idx.remove_from_index([e.uuid() for e in idx.elements_of(range(35))])
    assert idx.count() == 0 and len(_FakeIvf.made) == 3 and dev3.closed
    with pytest.raises(ValueError, match="No index"):
        idx.nn(q, 1)
    idx.update_index([_descr(i, vecs[i]) for i in range(8)])
    assert idx.count() == 8 and len(fake_device) == 2 and len(_FakeIvf.made) == 4
    with pytest.raises(ValueError, match="dimensions"):
        idx.update_index([_descr(100, np.zeros(7, np.float32))])
    assert idx.count() == 8


def test_float64_descriptors_are_ranked_by_their_own_distances(fake_device, monkeypatch):
    vecs = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 3.0]])
    idx = HipIvfFlatNearestNeighborsIndex(nlist=1)
    idx.build_index([_descr(i, vecs[i]) for i in range(3)])          # float64 vectors
    seen = []

    def distances(q, rows, metric):
        seen.append((q.dtype, rows.dtype, metric))
        return np.array([9.0, 4.0])

    monkeypatch.setattr(_lib, "dense_distances", distances)
    _FakeIvf.made[-1].answer = (np.array([[1.0, 2.0]], np.float32), np.array([[1, 2]], np.int64))
    elems, dists = idx.nn(_descr("q", np.zeros(2)), 2)
    assert seen == [(np.float32, np.float64, _lib.SQ_METRIC_L2)]     # float32 query against the original vectors
    assert [e.uuid() for e in elems] == [2, 1] and dists == (4.0, 9.0)


def test_read_only(fake_device):
    idx = HipIvfFlatNearestNeighborsIndex(read_only=True)
    d = [_descr(0, np.zeros(3, np.float32))]
    for call in (idx.build_index, idx.update_index):
        with pytest.raises(ReadOnlyError):
            call(d)
    with pytest.raises(ReadOnlyError):
        idx.remove_from_index([0])
    assert idx.count() == 0 and not fake_device and not _FakeIvf.made


def test_without_a_usable_device_nothing_falls_back(monkeypatch):
    monkeypatch.setattr(_lib, "usable", lambda: False)
    assert not HipIvfFlatNearestNeighborsIndex.is_usable()
    idx = HipIvfFlatNearestNeighborsIndex(nlist=2)
    with pytest.raises(_lib.HipError, match="no CPU fallback"):
        idx.build_index([_descr(i, np.full(4, i, np.float32)) for i in range(5)])
    assert idx.count() == 0
    with pytest.raises(ValueError, match="No index"):
        idx.nn(_descr("q", np.zeros(4, np.float32)), 1)


def test_extension_library_exports_what_its_header_declares():
    """include/smqtk_hip_ivf.h, `_lib.IVF_EXPORTS` and the dynamic sq_* symbols of libsmqtk_hip_ivf.so are one set, and
    none of them is an entry point of the main library, whose own set stays what include/smqtk_hip.h declares."""
    import re
    root = os.path.dirname(os.path.dirname(HOST))

    def declared(header):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", header)).read(), flags=re.S)
        return sorted(set(re.findall(r"\b(sq_[a-z0-9_]+)\s*\(", src)))

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
        return sorted({ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("sq_")})

    assert declared("smqtk_hip_ivf.h") == sorted(_lib.IVF_EXPORTS) == exported(_lib.IVF_LIB_PATH)
    assert len(_lib.IVF_EXPORTS) == 7 and not set(_lib.IVF_EXPORTS) & set(_lib.EXPORTS)
    assert declared("smqtk_hip.h") == sorted(_lib.EXPORTS) == exported(_lib.LIB_PATH)
    ivf = _lib.load_ivf()
    assert all(getattr(ivf, name).restype is __import__("ctypes").c_int for name in _lib.IVF_EXPORTS)


def test_abi_refuses_bad_calls_before_touching_a_device():
    core, lib = _lib.load(), _lib.load_ivf()
    import ctypes
    h = ctypes.c_int64(0)
    x = np.zeros((4, 8), np.float32)
    assert lib.sq_ivf_create(None, 4, 8, 0, 0, ctypes.byref(h)) == -1
    assert lib.sq_ivf_create(x.ctypes.data, 4, 8, _lib.SQ_METRIC_COSINE, 0, ctypes.byref(h)) == -4     # L2 only
    assert b"L2 only" in core.sq_last_error()
    assert lib.sq_ivf_create(x.ctypes.data, _lib.SQ_IVF_MAX_LISTS + 1, 8, 0, 0, ctypes.byref(h)) == -4
    assert lib.sq_ivf_kmeans(x.ctypes.data, 3, 8, x.ctypes.data, 4, 1, 0) == -1                        # n < nlist
    assert b"cannot train" in core.sq_last_error()
    assert lib.sq_ivf_kmeans(x.ctypes.data, 4, 8, x.ctypes.data, _lib.SQ_IVF_MAX_LISTS + 1, 1, 0) != 0
    for call in (lambda: lib.sq_ivf_add(12345, x.ctypes.data, 4, 0), lambda: lib.sq_ivf_lists(12345, None, None),
                 lambda: lib.sq_ivf_search(12345, x.ctypes.data, 1, 1, 1, x.ctypes.data, x.ctypes.data, 0, None),
                 lambda: lib.sq_ivf_destroy(12345)):
        assert call() == -1 and b"unknown handle" in core.sq_last_error()
    out = (ctypes.c_int64 * _lib.SQ_IVF_INFO_FIELDS)()
    assert lib.sq_ivf_info(12345, out, _lib.SQ_IVF_INFO_FIELDS) == -1
    with pytest.raises(_lib.HipError):
        _lib.set_option("ivf_no_such_option", 1)
    _lib.set_option("ivf_key_budget_mb", 0)                          # the slice budget's option is known; 0 = the default


# ------------------------------------------------------------------ sq_ivf_plan.hpp under sanitizers
@pytest.mark.skipif(_clangxx() is None, reason="ROCm's clang++ is not installed: nothing to compile the program with")
def test_plan_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "ivf_plan_main")
    cmd = [_clangxx(), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libsan",
           os.path.join(HOST, "ivf_plan_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, "compiling tests/host/ivf_plan_main.cpp failed:\n" + r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0, "status %d:\n%s" % (r.returncode, r.stdout[-4000:])
    assert "ivf plan ok" in r.stdout, r.stdout[-4000:]
    for word in ("Sanitizer", "runtime error"):
        assert word not in r.stdout, r.stdout[-4000:]
    fields = dict(w.split("=") for w in r.stdout.split("ivf plan ok:")[1].split())
    assert (int(fields["chunk"]), int(fields["budget"]), int(fields["max_lists"])) == (256, 256 << 20, _lib.SQ_IVF_MAX_LISTS)
