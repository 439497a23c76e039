"""The host side of the PCA front stage without a GPU: export set, refusals, plugin classes, the GPU tests' preconditions in
numpy, and sq_pca_plan.hpp under the host sanitizers (a stand-alone program: nothing sanitised is loaded into Python)."""
import ctypes
import os
import pickle
import subprocess

import numpy as np
import pytest

from smqtk_indexing_amd import NearestNeighborsIndex, _lib
from smqtk_indexing_amd._compat import DescriptorMemoryElement
from smqtk_indexing_amd.impls.nn_index import hip_ivf_pca as H
from tests import pca_cases as C
from tests.test_host_logic_isq import _declared, _exported
from tests.test_host_logic_pq import HOST, _clangxx


def test_seventh_library_exports_what_its_header_declares():
    assert _declared("smqtk_hip_pca.h") == sorted(_lib.PCA_EXPORTS) == _exported(_lib.PCA_LIB_PATH)
    others = (_lib.EXPORTS, _lib.IVF_EXPORTS, _lib.PQ_EXPORTS, _lib.ISQ_EXPORTS, _lib.REFINE_EXPORTS, _lib.OPQ_EXPORTS)
    assert not any(set(_lib.PCA_EXPORTS) & set(names) for names in others)


def test_abi_refuses_bad_calls_before_touching_a_device():
    core, lib = _lib.load(), _lib.load_pca()
    h = ctypes.c_int64(0)
    a = np.ones(64, np.float32)
    s = np.ones(16, np.float64)
    p, p2, ps = a.ctypes.data, a.ctypes.data + 128, s.ctypes.data
    for d_in, d_out, why in ((4, 5, b"does not widen"), (600, 513, b"beyond 512"), (8193, 4, b"beyond 8192")):
        assert lib.sq_pca_create(p, None, d_in, d_out, ctypes.byref(h)) == -4 and why in core.sq_last_error() and h.value == 0
    for args in ((None, None, 4, 2, ctypes.byref(h)), (p, None, 0, 0, ctypes.byref(h)), (p, None, 4, 0, ctypes.byref(h)), (p, None, 4, 2, None)):
        assert lib.sq_pca_create(*args) == -1
    for mem in (_lib.SQ_MEM_DEVICE_ASYNC, _lib.SQ_MEM_PLAN, 9, -1):
        assert lib.sq_pca_apply(12345, p, 1, p2, mem, None) == -4 and b"host or device memory only" in core.sq_last_error()
        assert lib.sq_pca_moments(p, 4, 2, p2, ps, mem) == -4 and b"host or device memory only" in core.sq_last_error()
    assert lib.sq_pca_apply(12345, p, 1, p, 0, None) == -1 and b"overlap" in core.sq_last_error()
    for x, y, n in ((None, p2, 1), (p, None, 1), (p, p2, -1)):
        assert lib.sq_pca_apply(12345, x, n, y, 0, None) == -1 and b"bad argument" in core.sq_last_error()
    for n in (1, 0, -3):
        assert lib.sq_pca_moments(p, n, 2, p2, ps, 0) == -1 and b"at least 2 rows" in core.sq_last_error()
    for x, m, sc in ((None, p2, ps), (p, None, ps), (p, p2, None)):
        assert lib.sq_pca_moments(x, 4, 2, m, sc, 0) == -1 and b"bad argument" in core.sq_last_error()
    assert lib.sq_pca_moments(p, 4, 2, p + 16, ps, 0) == -1 and b"overlap" in core.sq_last_error()
    assert lib.sq_pca_moments(p, 4, 8193, p2, ps, 0) == -4 and lib.sq_pca_moments(p, 2 ** 26 + 1, 1, p2, ps, 0) == -4
    out = (ctypes.c_int64 * _lib.SQ_PCA_INFO_FIELDS)()
    for call in (lambda: lib.sq_pca_apply(12345, p, 1, p2, 0, None), lambda: lib.sq_pca_info(12345, out, _lib.SQ_PCA_INFO_FIELDS),
                 lambda: lib.sq_pca_destroy(12345)):
        assert call() == -1 and b"unknown handle" in core.sq_last_error()


@pytest.mark.parametrize("cls,extra", [(H.HipPcaIvfFlatNearestNeighborsIndex, {}), (H.HipPcaIvfPqNearestNeighborsIndex, {"m": 4})])
def test_plugin_classes(cls, extra, monkeypatch):
    assert issubclass(cls, H._PcaFront) and issubclass(cls, NearestNeighborsIndex) and not cls.is_usable()
    index = cls(pca_dims=16, nlist=50, nprobe=7, train_iters=3, random_seed=11, **extra)
    c = index.get_config()
    assert c == dict({"pca_dims": 16, "nlist": 50, "nprobe": 7, "train_iters": 3, "random_seed": 11, "read_only": False}, **extra)
    assert cls.from_config(c).get_config() == c and cls().count() == 0
    index._pca_matrix, index._pca_mean = np.ones((16, 24), np.float32), np.arange(24, dtype=np.float32)
    back = pickle.loads(pickle.dumps(index))
    assert back.get_config() == c and back.count() == 0 and back._dev is None and back._pca is None
    assert np.array_equal(back._pca_matrix, index._pca_matrix) and np.array_equal(back._pca_mean, index._pca_mean)
    for bad in ({"pca_dims": 0}, {"pca_dims": 513}, {"nprobe": 0}) + (({"pca_dims": 18, "m": 4},) if extra else ()):
        with pytest.raises(ValueError):
            cls(**bad)
    # a width that is not the model's is refused on the host, before any device call (there is no device here)
    monkeypatch.setattr(_lib, "PcaTransform", lambda *a: pytest.fail("a device call"))
    e = DescriptorMemoryElement(0)
    e.set_vector(np.ones(25, np.float32))
    index._elements, index._centroids = [e], np.ones((2, 16), np.float32)
    for call in (lambda: index._to_matrix([e]), lambda: index.nn_many(np.ones((2, 23), np.float32), 1), lambda: index.update_index([e])):
        with pytest.raises(ValueError, match="projection of 24"):
            call()
    monkeypatch.setattr(_lib, "usable", lambda: True)
    assert _lib.pca_usable()
    monkeypatch.setattr(_lib, "PCA_LIB_PATH", os.path.join(os.path.dirname(_lib.PCA_LIB_PATH), "no_such_library.so"))
    assert not _lib.pca_usable() and not cls.is_usable()


@pytest.mark.parametrize("d_in,d_out", C.APPLY_SHAPES)
def test_the_apply_bound_holds_for_float32_and_bites(d_in, d_out):
    """numpy's float32 evaluation is inside the bound; a missing mean (and, where A is square, a transposed A) is outside it
    by more than 10 x somewhere: the mean alone is a term of order 1 / (8193 u) = 2000 bounds at the widest."""
    a, mean = C.model(d_in, d_out)
    for n in C.row_counts(d_out):
        x = C.rows(n, d_in)
        y64, bound = C.apply_reference(x, a, mean)
        assert (np.abs(((x - mean) @ a.T).astype(np.float64) - y64) <= bound).all(), n
        for y in [x @ a.T] + ([(x - mean) @ a] if d_in == d_out > 1 else []):
            assert (np.abs(y.astype(np.float64) - y64) / bound).max() > 10, n


@pytest.mark.parametrize("d,n", C.MOMENT_CASES)
def test_the_moments_bound_holds_for_float32_and_bites(d, n):
    """A float32 numpy scatter about the float32 mean is inside the bound; without the last row it is outside it where that
    row's centred square, of order 1, exceeds gamma_1026 n: n of a few thousand.  The integer case stays below 2^24."""
    x = C.rows(n, d)
    mean = (x.astype(np.float64).sum(axis=0) / n).astype(np.float32)
    c = x - mean
    C.check_moments(x, mean, (c.T @ c).astype(np.float64), (d, n))
    if d >= 5 and 2 < n <= 4 * C.RUN:
        _, s64, bound = C.moments_reference(x, mean)
        assert (np.abs((c[:-1].T @ c[:-1]).astype(np.float64) - s64) / bound).max() > 10
    xi, centre, s_int = C.integer_case()
    assert np.array_equal(xi.mean(axis=0), centre) and int(np.abs(s_int).max()) < 2 ** 24


def test_training_quality_of_a_float32_scatter():
    x, _ = C.index_case()
    mean = (x.astype(np.float64).sum(axis=0) / len(x)).astype(np.float32)
    c = x - mean
    scatter = (c.T @ c).astype(np.float64)
    C.check_training_quality(H.principal_axes(scatter, len(x), 16), x, mean, scatter)


@pytest.mark.skipif(_clangxx() is None, reason="ROCm's clang++ is not installed: nothing to compile the program with")
def test_plan_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pca_plan_main")
    cmd = [_clangxx(), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libsan", os.path.join(HOST, "pca_plan_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, "compiling tests/host/pca_plan_main.cpp failed:\n" + r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]
    assert "pca plan ok: widest_lds=82944 most_tiles_per_wave=8" in r.stdout, r.stdout[-4000:]
