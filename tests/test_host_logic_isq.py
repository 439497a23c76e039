"""
The host side of the IVF-SQ index, without a GPU: include/smqtk_hip_isq.h, `_lib.ISQ_EXPORTS` and the dynamic sq_isq_*
symbols of libsmqtk_hip_isq.so are one set, disjoint from the other three libraries' sets; every refusal of the header's
limits through the raw ABI, made before a device is touched; and `is_usable()` of the two plugin classes.
"""
import ctypes
import os
import re
import subprocess

import numpy as np

from smqtk_indexing_amd import NearestNeighborsIndex, _lib
from smqtk_indexing_amd.impls.nn_index.hip_ivf_sq import HipIvfSq8NearestNeighborsIndex, HipIvfSqFp16NearestNeighborsIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sq_[a-z0-9_]+)\s*\(", src)))


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
    return sorted({ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("sq_")})


def test_fourth_library_exports_what_its_header_declares():
    assert _declared("smqtk_hip_isq.h") == sorted(_lib.ISQ_EXPORTS) == _exported(_lib.ISQ_LIB_PATH)
    assert all(name.startswith("sq_isq_") for name in _lib.ISQ_EXPORTS) and len(set(_lib.ISQ_EXPORTS)) == len(_lib.ISQ_EXPORTS) == 7
    for other, path, header in ((_lib.EXPORTS, _lib.LIB_PATH, "smqtk_hip.h"), (_lib.IVF_EXPORTS, _lib.IVF_LIB_PATH, "smqtk_hip_ivf.h"),
                                (_lib.PQ_EXPORTS, _lib.PQ_LIB_PATH, "smqtk_hip_pq.h")):
        assert not set(_lib.ISQ_EXPORTS) & (set(other) | set(_exported(path)) | set(_declared(header)))
    isq = _lib.load_isq()
    assert all(getattr(isq, name).restype is ctypes.c_int for name in _lib.ISQ_EXPORTS)
    dyn = subprocess.run(["readelf", "-d", _lib.ISQ_LIB_PATH], check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
    assert "libsmqtk_hip.so" in dyn and "libsmqtk_hip_ivf.so" in dyn and "$ORIGIN" in dyn and "libsmqtk_hip_pq.so" not in dyn


def test_abi_refuses_bad_calls_before_touching_a_device():
    core, lib = _lib.load(), _lib.load_isq()
    h = ctypes.c_int64(0)
    big = np.ones(41_000, np.float32)                 # centroids, vmin or step of any width asked for below
    p = big.ctypes.data
    bad = np.ones(8, np.float32)

    def create(kind, vmin, step, nlist=1, d=8, metric=_lib.SQ_METRIC_L2):
        return lib.sq_isq_create(p, nlist, d, kind, vmin, step, metric, 0, ctypes.byref(h))

    for kind in (-1, 2):
        assert create(kind, p, p) == -1 and b"kind" in core.sq_last_error()
    for vmin, step in ((None, p), (p, None), (None, None)):
        assert create(_lib.SQ_ISQ_SQ8, vmin, step) == -1 and b"needs vmin and step" in core.sq_last_error()
    for vmin, step in ((None, p), (p, None), (p, p)):
        assert create(_lib.SQ_ISQ_F16, vmin, step) == -1 and b"no parameters" in core.sq_last_error()
    for value in (np.nan, np.inf, -np.inf):
        bad[:] = 1
        bad[5] = value
        assert create(_lib.SQ_ISQ_SQ8, p, bad.ctypes.data) == -1 and b"dimension 5" in core.sq_last_error()
        assert create(_lib.SQ_ISQ_SQ8, bad.ctypes.data, p) == -1 and b"dimension 5" in core.sq_last_error()
    bad[:] = 1
    bad[3] = -0.5
    assert create(_lib.SQ_ISQ_SQ8, p, bad.ctypes.data) == -1 and b"dimension 3" in core.sq_last_error()
    assert create(_lib.SQ_ISQ_SQ8, p, p, metric=_lib.SQ_METRIC_COSINE) == -4 and b"L2 only" in core.sq_last_error()
    assert create(_lib.SQ_ISQ_F16, None, None, nlist=_lib.SQ_IVF_MAX_LISTS + 1) == -4 and b"lists" in core.sq_last_error()
    # the scan stages 3 round_up(d, 4) floats (SQ8) or round_up(d, 4) (F16) in at most 160 KiB of LDS
    assert create(_lib.SQ_ISQ_SQ8, p, p, d=13_653) == -4 and b"LDS" in core.sq_last_error()
    assert create(_lib.SQ_ISQ_F16, None, None, d=40_961) == -4 and b"LDS" in core.sq_last_error()
    for mem in (_lib.SQ_MEM_DEVICE_ASYNC, _lib.SQ_MEM_PLAN, 9, -1):
        assert lib.sq_isq_search(12345, p, 1, 1, 1, p, p, mem, None) == -4 and b"blocking calls only" in core.sq_last_error()
        assert lib.sq_isq_train(p, 4, 2, p, p, mem) == -4
    for call in (lambda: lib.sq_isq_add(12345, p, 4, 0), lambda: lib.sq_isq_lists(12345, None, None, None),
                 lambda: lib.sq_isq_search(12345, p, 1, 1, 1, p, p, 0, None), lambda: lib.sq_isq_destroy(12345)):
        assert call() == -1 and b"unknown handle" in core.sq_last_error()
    out = (ctypes.c_int64 * _lib.SQ_ISQ_INFO_FIELDS)()
    assert lib.sq_isq_info(12345, out, _lib.SQ_ISQ_INFO_FIELDS) == -1 and h.value == 0


def test_plugin_classes(monkeypatch):
    for cls, kind in ((HipIvfSq8NearestNeighborsIndex, _lib.SQ_ISQ_SQ8), (HipIvfSqFp16NearestNeighborsIndex, _lib.SQ_ISQ_F16)):
        assert issubclass(cls, NearestNeighborsIndex) and cls.KIND == kind and cls.is_usable() == _lib.isq_usable()
        c = cls(nlist=50, nprobe=7, train_iters=3, random_seed=11).get_config()
        assert c == {"nlist": 50, "nprobe": 7, "train_iters": 3, "random_seed": 11, "read_only": False}
        assert cls.from_config(c).get_config() == c and cls().count() == 0
    monkeypatch.setattr(_lib, "usable", lambda: True)
    assert _lib.isq_usable()
    monkeypatch.setattr(_lib, "ISQ_LIB_PATH", os.path.join(os.path.dirname(_lib.ISQ_LIB_PATH), "no_such_library.so"))
    assert not _lib.isq_usable() and not HipIvfSq8NearestNeighborsIndex.is_usable() and not HipIvfSqFp16NearestNeighborsIndex.is_usable()
