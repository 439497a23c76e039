"""
The host side of the IVF-PQ index's residual mode, without a GPU.

1. The two new entry points through the raw ABI: every refusal is made before a device is touched.
2. `HipIvfPqResidualNearestNeighborsIndex`'s host logic against recording stand-ins: the parent's configuration and
   state machine, the codebooks trained on `pq_residuals` of the training sample from the residuals of the parent's
   `entries` draw, the device index created with `residual=True`; the parent class itself asks for neither.
3. tests/host/pq_residual_plan_main.cpp over the residual plan of smqtk_indexing_amd/csrc/sq_pq_plan.hpp (plain C++),
   compiled with ROCm's clang++ under AddressSanitizer and UndefinedBehaviorSanitizer, linked statically against the
   sanitizer runtime and run as its own program; the lines it prints are compared with the Python restatement of
   tests/pq_residual_cases.py.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from smqtk_indexing_amd import NearestNeighborsIndex, _lib
from smqtk_indexing_amd._compat import DescriptorMemoryElement, from_config_dict, to_config_dict
from smqtk_indexing_amd.impls.nn_index.hip_ivf_pq import HipIvfPqNearestNeighborsIndex
from smqtk_indexing_amd.impls.nn_index.hip_ivf_pq_residual import HipIvfPqResidualNearestNeighborsIndex
from tests import pq_residual_cases as R
from tests.test_host_logic_buffers import HOST, _clangxx


def _descr(uid, vec):
    d = DescriptorMemoryElement(uid)
    d.set_vector(np.asarray(vec))
    return d


# ------------------------------------------------------------------ the raw ABI
def test_abi_refuses_bad_calls_before_touching_a_device():
    core, lib = _lib.load(), _lib.load_pq()
    assert {"sq_pq_create_residual", "sq_pq_residuals"} <= set(_lib.PQ_EXPORTS) and _lib.SQ_PQ_INFO_FIELDS == 10
    h = ctypes.c_int64(0)
    x = np.zeros((300, 8), np.float32)
    p = x.ctypes.data

    def create(nlist, d, m, ksub):
        return lib.sq_pq_create_residual(p, nlist, d, p, m, ksub, 0, ctypes.byref(h))

    def residuals(n, d, nlist, mem=0, xp=p, cp=p, op=p):
        return lib.sq_pq_residuals(xp, n, d, cp, nlist, op, mem)

    # sq_pq_create_residual: what sq_pq_create refuses, under its own name
    assert create(4, 8, 3, 16) == -1 and b"sq_pq_create_residual" in core.sq_last_error() and b"no multiple" in core.sq_last_error()
    for m in (0, -1, 65):
        assert create(4, 130, m, 16) == -1 and b"m = " in core.sq_last_error()
    for ksub in (0, -2, 257):
        assert create(4, 8, 2, ksub) == -1 and b"ksub" in core.sq_last_error()
    assert create(4, 16385, 1, 16) == -4 and b"sub-vectors" in core.sq_last_error()
    assert create(_lib.SQ_IVF_MAX_LISTS + 1, 8, 2, 16) == -4 and b"lists" in core.sq_last_error()
    assert create(0, 8, 2, 16) == -1 and create(4, 0, 2, 16) == -1
    assert lib.sq_pq_create_residual(None, 4, 8, p, 2, 16, 0, ctypes.byref(h)) == -1
    assert lib.sq_pq_create_residual(p, 4, 8, None, 2, 16, 0, ctypes.byref(h)) == -1
    assert lib.sq_pq_create_residual(p, 4, 8, p, 2, 16, 0, None) == -1
    assert h.value == 0
    # sq_pq_residuals
    assert residuals(300, 8, _lib.SQ_IVF_MAX_LISTS + 1) == -4 and b"sq_pq_residuals" in core.sq_last_error() and b"lists" in core.sq_last_error()
    assert residuals(2 ** 26 + 1, 8, 4) == -4 and b"2^26" in core.sq_last_error()
    for mem in (_lib.SQ_MEM_DEVICE_ASYNC, _lib.SQ_MEM_PLAN, _lib.SQ_MEM_PLAN_ASYNC, 9, -1):
        assert residuals(300, 8, 4, mem=mem) == -4 and b"host or device memory only" in core.sq_last_error()
    for bad in (dict(n=0), dict(n=-5), dict(d=0), dict(nlist=0), dict(xp=None), dict(cp=None), dict(op=None)):
        args = dict(n=300, d=8, nlist=4)
        args.update(bad)
        assert residuals(**args) == -1 and b"bad argument" in core.sq_last_error()


def test_python_wrappers_check_their_shapes():
    with pytest.raises(ValueError, match="centroids"):
        _lib.pq_residuals(np.zeros((5, 8), np.float32), np.zeros((2, 7), np.float32))
    with pytest.raises(ValueError):
        _lib.pq_residuals(np.zeros(8, np.float32), np.zeros((2, 8), np.float32))
    out = _lib.pq_residuals(np.zeros((0, 8), np.float32), np.zeros((2, 8), np.float32))       # no rows: no call
    assert out.shape == (0, 8) and out.dtype == np.float32
    with pytest.raises(ValueError, match="centroids"):
        _lib.pq_residuals_device(0, 5, 8, np.zeros((2, 7), np.float32), 0)
    with pytest.raises(ValueError, match="codebooks"):
        _lib.PqIndex(np.zeros((2, 8), np.float32), np.zeros((3, 4, 2), np.float32), residual=True)


# ------------------------------------------------------------------ the plugin's host logic
class _FakePq:
    made = []

    def __init__(self, centroids, codebooks, id_base=0, **kw):
        self.centroids, self.codebooks, self.kw = np.array(centroids), np.array(codebooks), kw
        self.added, self.closed = [], False
        _FakePq.made.append(self)

    def add(self, rows):
        self.added.append(np.array(rows))

    def search(self, q, k, nprobe):
        idx = np.zeros((q.shape[0], k), np.int64)
        return np.full((q.shape[0], k), 0.5, np.float32), idx

    def close(self):
        self.closed = True


@pytest.fixture
def fake_device(monkeypatch):
    _FakePq.made = []
    calls = {"kmeans": [], "pq": [], "residuals": []}

    def kmeans(x, centroids, iters=10):
        calls["kmeans"].append((np.array(x), np.array(centroids), iters))
        return np.array(centroids, dtype=np.float32) + np.float32(1)

    def pq_train(x, codebooks, iters=10):
        calls["pq"].append((np.array(x), np.array(codebooks), iters))
        return np.array(codebooks, dtype=np.float32) + np.float32(2)

    def pq_residuals(x, centroids):
        calls["residuals"].append((np.array(x), np.array(centroids)))
        return np.array(x, dtype=np.float32) * np.float32(0.5) - np.float32(3)

    monkeypatch.setattr(_lib, "usable", lambda: True)
    monkeypatch.setattr(_lib, "PqIndex", _FakePq)
    monkeypatch.setattr(_lib, "ivf_kmeans", kmeans)
    monkeypatch.setattr(_lib, "pq_train", pq_train)
    monkeypatch.setattr(_lib, "pq_residuals", pq_residuals)
    monkeypatch.setattr(_lib, "dense_distances", lambda q, rows, metric: np.sqrt(((np.asarray(rows, np.float64) - q) ** 2).sum(1)))
    return calls


def test_config_is_the_parents():
    assert issubclass(HipIvfPqResidualNearestNeighborsIndex, HipIvfPqNearestNeighborsIndex)
    assert issubclass(HipIvfPqResidualNearestNeighborsIndex, NearestNeighborsIndex)
    i = HipIvfPqResidualNearestNeighborsIndex()
    assert i.get_config() == HipIvfPqNearestNeighborsIndex().get_config() == HipIvfPqResidualNearestNeighborsIndex.get_default_config()
    j = HipIvfPqResidualNearestNeighborsIndex(nlist=50, nprobe=7, m=4, train_iters=3, random_seed=11, read_only=True)
    c = j.get_config()
    assert c == {"nlist": 50, "nprobe": 7, "m": 4, "train_iters": 3, "random_seed": 11, "read_only": True}
    k = from_config_dict(to_config_dict(j), [HipIvfPqNearestNeighborsIndex, HipIvfPqResidualNearestNeighborsIndex])
    assert type(k) is HipIvfPqResidualNearestNeighborsIndex and k.get_config() == c
    assert HipIvfPqResidualNearestNeighborsIndex.is_usable() == _lib.pq_usable()
    with pytest.raises(ValueError, match="m must"):
        HipIvfPqResidualNearestNeighborsIndex(m=65)
    a, b = j.training_plan(5000), HipIvfPqNearestNeighborsIndex(nlist=50, random_seed=11).training_plan(5000)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


def test_build_trains_on_residuals_and_makes_a_residual_index(fake_device):
    rng = np.random.default_rng(3)
    vecs = rng.standard_normal((40, 6)).astype(np.float32)
    idx = HipIvfPqResidualNearestNeighborsIndex(nlist=5, nprobe=2, m=3, train_iters=4, random_seed=1)
    idx.build_index([_descr(i, vecs[i]) for i in range(30)])
    sample, init, entries = idx.training_plan(30)
    train = vecs[:30][sample]
    assert len(fake_device["kmeans"]) == len(fake_device["residuals"]) == len(fake_device["pq"]) == len(_FakePq.made) == 1
    x, c0, iters = fake_device["kmeans"][0]
    assert iters == 4 and np.array_equal(x, train) and np.array_equal(c0, train[init])
    # the residuals of the training sample against the TRAINED centroids
    x, cent = fake_device["residuals"][0]
    assert np.array_equal(x, train) and np.array_equal(cent, c0 + 1)
    coded = train * np.float32(0.5) - np.float32(3)
    x, b0, iters = fake_device["pq"][0]
    assert iters == 4 and np.array_equal(x, coded) and b0.shape == (3, 30, 2)
    for j in range(3):                                                   # the residuals of the same `entries` draw
        assert np.array_equal(b0[j], coded[entries][:, 2 * j:2 * j + 2])
    dev = _FakePq.made[0]
    assert dev.kw == {"residual": True} and np.array_equal(dev.centroids, c0 + 1) and np.array_equal(dev.codebooks, b0 + 2)
    assert len(dev.added) == 1 and np.array_equal(dev.added[0], vecs[:30])          # the rows themselves: the device takes the residuals
    # new uuids join the lists; a replaced uuid and a removal make a new residual index with the same training
    idx.update_index([_descr(i, vecs[i]) for i in range(30, 36)])
    assert len(_FakePq.made) == 1 and len(dev.added) == 2 and np.array_equal(dev.added[1], vecs[30:36])
    idx.update_index([_descr(5, vecs[5] + np.float32(2))])
    idx.remove_from_index([0])
    assert idx.count() == 35 and len(_FakePq.made) == 3 and len(fake_device["pq"]) == len(fake_device["residuals"]) == 1
    assert all(d.kw == {"residual": True} and np.array_equal(d.codebooks, dev.codebooks) for d in _FakePq.made)
    with pytest.raises(KeyError):
        idx.remove_from_index([0])
    elems, dists = idx.nn(_descr("q", vecs[1]), 1)
    assert len(elems) == 1 and dists[0] >= 0


def test_the_parent_class_asks_for_neither(fake_device):
    vecs = np.random.default_rng(4).standard_normal((20, 4)).astype(np.float32)
    idx = HipIvfPqNearestNeighborsIndex(nlist=2, m=2, train_iters=1)
    idx.build_index([_descr(i, vecs[i]) for i in range(20)])
    assert not fake_device["residuals"] and _FakePq.made[0].kw == {}
    sample, _, entries = idx.training_plan(20)
    x, b0, _ = fake_device["pq"][0]
    assert np.array_equal(x, vecs[sample]) and np.array_equal(b0[1], vecs[sample][entries][:, 2:4])


def test_without_a_usable_device_nothing_falls_back(monkeypatch):
    monkeypatch.setattr(_lib, "usable", lambda: False)
    assert not HipIvfPqResidualNearestNeighborsIndex.is_usable()
    idx = HipIvfPqResidualNearestNeighborsIndex(nlist=2, m=2)
    with pytest.raises(_lib.HipError, match="no CPU fallback"):
        idx.build_index([_descr(i, np.full(4, i, np.float32)) for i in range(5)])
    assert idx.count() == 0


# ------------------------------------------------------------------ the residual plan under sanitizers
@pytest.mark.skipif(_clangxx() is None, reason="ROCm's clang++ is not installed: nothing to compile the program with")
def test_residual_plan_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pq_residual_plan_main")
    cmd = [_clangxx(), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libsan",
           os.path.join(HOST, "pq_residual_plan_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, "compiling tests/host/pq_residual_plan_main.cpp failed:\n" + r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0, "status %d:\n%s" % (r.returncode, r.stdout[-4000:])
    assert "pq residual plan ok" in r.stdout, r.stdout[-4000:]
    for word in ("Sanitizer", "runtime error"):
        assert word not in r.stdout, r.stdout[-4000:]
    fields = dict(w.split("=") for w in r.stdout.split("pq residual plan ok:")[1].split())
    assert int(fields["max_pairs"]) == R.MAX_PAIRS
    # the Python restatement against the real functions, line by line
    real = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("plan "):
            v = list(map(int, ln.split()[1:]))
            real[tuple(v[:7])] = tuple(v[7:])
    assert len(real) == int(fields["lines"]) > 20000
    for key, want in real.items():
        assert R.res_plan(*key) == want, (key, want, R.res_plan(*key))
    # ... and the plans the GPU tests lean on are among the lines
    assert real[(3, 8, 3001, 10, 64, 256, 1 << 20)] == (3, 14, 2) and real[(5, 8, 3001, 10, 64, 256, 1 << 20)][2] == 3
    assert real[(600, 3, 12000, 100, 16, 16, R.DEFAULT_BUDGET)][2] == 1 and real[(64, 3, 12000, 100, 6, 16, R.DEFAULT_BUDGET)][2] == 1
