"""
The host side of the refine stage, without a GPU: include/smqtk_hip_refine.h, `_lib.REFINE_EXPORTS` and the dynamic
sq_refine_* symbols of libsmqtk_hip_refine.so are one set, and the other four libraries export what they did; every
refusal of the header's limits that needs no handle, through the raw ABI, made before a device is touched (a base that
does not match needs two handles: tests/test_hip_refine.py); and the plugin class's configuration.
"""
import ctypes
import os

import numpy as np
import pytest

from smqtk_indexing_amd import NearestNeighborsIndex, _lib
from smqtk_indexing_amd.impls.nn_index.hip_ivf_refine import HipIvfPqRefineNearestNeighborsIndex
from tests.test_host_logic_isq import _declared, _exported


def test_fifth_library_exports_what_its_header_declares():
    assert _declared("smqtk_hip_refine.h") == sorted(_lib.REFINE_EXPORTS) == _exported(_lib.REFINE_LIB_PATH)
    for exports, path, header in ((_lib.EXPORTS, _lib.LIB_PATH, "smqtk_hip.h"), (_lib.IVF_EXPORTS, _lib.IVF_LIB_PATH, "smqtk_hip_ivf.h"),
                                  (_lib.PQ_EXPORTS, _lib.PQ_LIB_PATH, "smqtk_hip_pq.h"), (_lib.ISQ_EXPORTS, _lib.ISQ_LIB_PATH, "smqtk_hip_isq.h")):
        assert sorted(exports) == _exported(path) == _declared(header) and not set(_lib.REFINE_EXPORTS) & set(exports)
    lib = _lib.load_refine()
    assert all(getattr(lib, name).restype is ctypes.c_int for name in _lib.REFINE_EXPORTS)


def test_abi_refuses_bad_calls_before_touching_a_device():
    core, lib = _lib.load(), _lib.load_refine()
    h = ctypes.c_int64(0)
    big = np.ones(41_000, np.float32)
    p = big.ctypes.data
    bad = np.ones(8, np.float32)

    def create(kind, vmin, step, d=8):
        return lib.sq_refine_create(d, kind, vmin, step, 0, ctypes.byref(h))

    for kind in (-1, 3):
        assert create(kind, p, p) == -1 and b"kind" in core.sq_last_error()
    for vmin, step in ((None, p), (p, None), (None, None)):
        assert create(_lib.SQ_REFINE_SQ8, vmin, step) == -1 and b"needs vmin and step" in core.sq_last_error()
    for kind in (_lib.SQ_REFINE_F16, _lib.SQ_REFINE_F32):
        for vmin, step in ((None, p), (p, None), (p, p)):
            assert create(kind, vmin, step) == -1 and b"no parameters" in core.sq_last_error()
    for value in (np.nan, np.inf, -np.inf, -0.5):
        bad[:] = 1
        bad[5] = value
        assert create(_lib.SQ_REFINE_SQ8, p, bad.ctypes.data) == -1 and b"dimension 5" in core.sq_last_error()
        if value != -0.5:
            assert create(_lib.SQ_REFINE_SQ8, bad.ctypes.data, p) == -1 and b"dimension 5" in core.sq_last_error()
    assert create(_lib.SQ_REFINE_F16, None, None, d=0) == -1
    # 128 bytes of row numbers, the staging of 3 round_up(d, 4) floats (SQ8) or round_up(d, 4), and 32 slabs of 1056 bytes in 160 KiB
    assert create(_lib.SQ_REFINE_SQ8, p, p, d=10_825) == -4 and b"LDS" in core.sq_last_error()
    for kind in (_lib.SQ_REFINE_F16, _lib.SQ_REFINE_F32):
        assert create(kind, None, None, d=32_481) == -4 and b"LDS" in core.sq_last_error()
    for mem in (_lib.SQ_MEM_DEVICE_ASYNC, _lib.SQ_MEM_PLAN, 9, -1):
        assert lib.sq_refine_rerank(12345, p, 1, p, 1, 1, p, p, mem, None) == -4 and b"blocking calls only" in core.sq_last_error()
        assert lib.sq_refine_search(12345, 12346, p, 1, 1, 1, 1, p, p, mem, None) == -4 and b"blocking calls only" in core.sq_last_error()
        assert lib.sq_refine_add(12345, p, 4, mem) == -4
    for k, kb in ((5, 4), (0, 4), (4, 0), (-1, -1)):
        assert lib.sq_refine_rerank(12345, p, 1, p, kb, k, p, p, 0, None) == -1 and b"unknown handle" not in core.sq_last_error()
        assert lib.sq_refine_search(12345, 12346, p, 1, k, kb, 1, p, p, 0, None) == -1 and b"unknown handle" not in core.sq_last_error()
    for call in (lambda: lib.sq_refine_add(12345, p, 4, 0), lambda: lib.sq_refine_rows(12345, 0, 0, None),
                 lambda: lib.sq_refine_rerank(12345, p, 1, p, 1, 1, p, p, 0, None),
                 lambda: lib.sq_refine_search(12345, 12346, p, 1, 1, 1, 1, p, p, 0, None), lambda: lib.sq_refine_destroy(12345)):
        assert call() == -1 and b"unknown handle" in core.sq_last_error()
    out = (ctypes.c_int64 * _lib.SQ_REFINE_INFO_FIELDS)()
    assert lib.sq_refine_info(12345, out, _lib.SQ_REFINE_INFO_FIELDS) == -1 and h.value == 0


def test_plugin_class(monkeypatch):
    cls = HipIvfPqRefineNearestNeighborsIndex
    assert issubclass(cls, NearestNeighborsIndex) and cls.is_usable() == _lib.refine_usable() and not cls.is_usable()
    c = cls(nlist=50, nprobe=7, m=4, residual=False, packed=True, refine="sq8", k_factor=8, train_iters=3, random_seed=11).get_config()
    assert c == {"nlist": 50, "nprobe": 7, "m": 4, "residual": False, "packed": True, "refine": "sq8", "k_factor": 8, "train_iters": 3,
                 "random_seed": 11, "read_only": False}
    assert cls.from_config(c).get_config() == c and cls().count() == 0 and cls().get_config()["refine"] == "fp16"
    assert cls(packed=True).MAX_ENTRIES == _lib.SQ_PQ_PACKED_MAX_KSUB and cls().MAX_ENTRIES == _lib.SQ_PQ_MAX_KSUB
    for bad in ({"refine": "bf16"}, {"k_factor": 0}, {"nprobe": 0}, {"m": 0}):
        with pytest.raises(ValueError):
            cls(**bad)
    monkeypatch.setattr(_lib, "usable", lambda: True)
    assert _lib.refine_usable()
    monkeypatch.setattr(_lib, "REFINE_LIB_PATH", os.path.join(os.path.dirname(_lib.REFINE_LIB_PATH), "no_such_library.so"))
    assert not _lib.refine_usable() and not cls.is_usable()
