"""The packed mode's host side without a GPU: `sq_pq_create_packed`'s refusals before a device is touched, the plugin classes."""
import ctypes
import os

import numpy as np

from smqtk_indexing_amd import _lib
from smqtk_indexing_amd.impls.nn_index.hip_ivf_pq import HipIvfPqNearestNeighborsIndex
from smqtk_indexing_amd.impls.nn_index.hip_ivf_pq4 import HipIvfPq4NearestNeighborsIndex, HipIvfPq4ResidualNearestNeighborsIndex

CLASSES = (HipIvfPq4NearestNeighborsIndex, HipIvfPq4ResidualNearestNeighborsIndex)


def test_abi_refuses_bad_calls_before_touching_a_device():
    core, lib = _lib.load(), _lib.load_pq()
    h = ctypes.c_int64(0)
    p = np.zeros((300, 8), np.float32).ctypes.data

    def create(nlist, d, m, ksub, residual, cent=p, books=p, out=ctypes.byref(h)):
        return lib.sq_pq_create_packed(cent, nlist, d, books, m, ksub, residual, 0, out), core.sq_last_error()

    for residual in (0, 1):
        for ksub in (0, 17, 256):
            assert create(4, 8, 2, ksub, residual)[0] == -1 and b"ksub" in core.sq_last_error()
        for m in (0, 65):
            assert create(4, 130, m, 16, residual)[0] == -1 and b"m = " in core.sq_last_error()
        assert create(4, 8, 3, 16, residual)[0] == -1 and b"no multiple" in core.sq_last_error()
        assert create(4, 16385, 1, 16, residual)[0] == -4 and b"sub-vectors" in core.sq_last_error()
        assert create(_lib.SQ_IVF_MAX_LISTS + 1, 8, 2, 16, residual)[0] == -4 and b"lists" in core.sq_last_error()
        assert create(4, 8, 2, 16, residual, cent=None)[0] == -1 and create(4, 8, 2, 16, residual, books=None)[0] == -1
        assert create(4, 8, 2, 16, residual, out=None)[0] == -1
    assert h.value == 0


def test_classes_without_a_device_or_the_third_library(monkeypatch):
    assert [c.MAX_ENTRIES for c in CLASSES] == [16, 16] and HipIvfPqNearestNeighborsIndex.MAX_ENTRIES == 256
    for cls in CLASSES:
        assert cls.is_usable() == _lib.pq_usable()
        sample, _, entries = cls(nlist=4, random_seed=9).training_plan(700)
        assert entries.shape == (16,) and np.unique(entries).shape == (16,) and entries.max() < len(sample)
        assert cls(nlist=4).training_plan(10)[2].shape == (10,)
    monkeypatch.setattr(_lib, "usable", lambda: False)
    assert not any(cls.is_usable() for cls in CLASSES)
    monkeypatch.setattr(_lib, "usable", lambda: True)
    monkeypatch.setattr(_lib, "PQ_LIB_PATH", os.path.join(os.path.dirname(_lib.PQ_LIB_PATH), "no_such_library.so"))
    assert not _lib.pq_usable() and not any(cls.is_usable() for cls in CLASSES)
