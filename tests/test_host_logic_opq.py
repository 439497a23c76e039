"""
The host side of the OPQ transform and its index, without a GPU: export sets, the raw ABI's refusals (a handle of another
kind needs a device: tests/test_hip_opq.py), the plugin class, the GPU tests' preconditions proven on the CPU, and
sq_opq_plan.hpp under the host sanitizers (a stand-alone program, linked statically: nothing is loaded into Python).
"""
import ctypes
import os
import pickle
import subprocess

import numpy as np
import pytest

from smqtk_indexing_amd import NearestNeighborsIndex, _lib
from smqtk_indexing_amd.impls.nn_index import hip_ivf_opq as H
from smqtk_indexing_amd.impls.nn_index.hip_ivf_pq import HipIvfPqNearestNeighborsIndex
from tests import opq_cases as C
from tests.test_host_logic_isq import _declared, _exported
from tests.test_host_logic_pq import HOST, _clangxx


def test_sixth_library_exports_what_its_header_declares():
    assert _declared("smqtk_hip_opq.h") == sorted(_lib.OPQ_EXPORTS) == _exported(_lib.OPQ_LIB_PATH)
    assert sorted(_lib.EXPORTS) == _exported(_lib.LIB_PATH) == _declared("smqtk_hip.h") and not set(_lib.OPQ_EXPORTS) & set(_lib.EXPORTS)
    lib = _lib.load_opq()
    assert all(getattr(lib, name).restype is ctypes.c_int for name in _lib.OPQ_EXPORTS)


def test_abi_refuses_bad_calls_before_touching_a_device():
    core, lib = _lib.load(), _lib.load_opq()
    h = ctypes.c_int64(0)
    a = np.ones(16, np.float32)
    p, p2 = a.ctypes.data, a.ctypes.data + 32
    assert lib.sq_opq_create(p, 0, ctypes.byref(h)) == -1 and lib.sq_opq_create(None, 4, ctypes.byref(h)) == -1
    assert lib.sq_opq_create(p, 4, None) == -1
    assert lib.sq_opq_create(p, _lib.SQ_OPQ_MAX_D + 1, ctypes.byref(h)) == -4 and b"beyond 4096" in core.sq_last_error() and h.value == 0
    for mem in (_lib.SQ_MEM_DEVICE_ASYNC, _lib.SQ_MEM_PLAN, 9, -1):
        assert lib.sq_opq_apply(12345, p, 1, p2, mem, None) == -4 and b"host or device memory only" in core.sq_last_error()
    assert lib.sq_opq_apply(12345, p, 1, p, 0, None) == -1 and b"overlap" in core.sq_last_error()
    for x, y, n in ((None, p2, 1), (p, None, 1), (p, p2, -1)):
        assert lib.sq_opq_apply(12345, x, n, y, 0, None) == -1 and b"bad argument" in core.sq_last_error()
    out = (ctypes.c_int64 * _lib.SQ_OPQ_INFO_FIELDS)()
    for call in (lambda: lib.sq_opq_apply(12345, p, 1, p2, 0, None), lambda: lib.sq_opq_info(12345, out, _lib.SQ_OPQ_INFO_FIELDS),
                 lambda: lib.sq_opq_destroy(12345)):
        assert call() == -1 and b"unknown handle" in core.sq_last_error()


def test_plugin_class(monkeypatch):
    cls = H.HipOpqIvfPqNearestNeighborsIndex
    assert issubclass(cls, HipIvfPqNearestNeighborsIndex) and issubclass(cls, NearestNeighborsIndex)
    assert cls.is_usable() == _lib.opq_usable() and not cls.is_usable()
    index = cls(nlist=50, nprobe=7, m=4, pq_mode="packed", opq_iters=3, train_iters=3, random_seed=11)
    c = index.get_config()
    assert c == {"nlist": 50, "nprobe": 7, "m": 4, "pq_mode": "packed", "opq_iters": 3, "train_iters": 3, "random_seed": 11, "read_only": False}
    assert cls.from_config(c).get_config() == c and cls().count() == 0
    assert (cls().get_config()["pq_mode"], cls().get_config()["opq_iters"]) == ("residual", C.T_ITERS) and H.OPQ_INNER_ITERS == C.T_INNER
    index._rotation = C.matrix(8, "orthonormal")
    index._centroids, index._codebooks = np.ones((2, 8), np.float32), np.ones((4, 16, 2), np.float32)
    back = pickle.loads(pickle.dumps(index))
    assert back.get_config() == c and back.count() == 0 and back._dev is None and back._opq is None
    assert all(np.array_equal(getattr(back, k), getattr(index, k)) for k in ("_rotation", "_centroids", "_codebooks"))
    made = []
    monkeypatch.setattr(_lib, "PqIndex", lambda cent, books, **kw: made.append(kw))
    for mode, (residual, packed) in H.PQ_MODES.items():
        one = cls(pq_mode=mode)
        one._new_device_index()
        assert made[-1] == {"residual": residual, "packed": packed} and (mode.startswith("packed"), "residual" in mode) == (packed, residual)
        assert one.MAX_ENTRIES == (_lib.SQ_PQ_PACKED_MAX_KSUB if packed else _lib.SQ_PQ_MAX_KSUB)
    assert sorted(H.PQ_MODES) == ["packed", "packed_residual", "plain", "residual"]
    for bad in ({"pq_mode": "opq"}, {"pq_mode": None}, {"opq_iters": -1}, {"m": 0}):
        with pytest.raises(ValueError):
            cls(**bad)
    monkeypatch.setattr(_lib, "usable", lambda: True)
    assert _lib.opq_usable()
    monkeypatch.setattr(_lib, "OPQ_LIB_PATH", os.path.join(os.path.dirname(_lib.OPQ_LIB_PATH), "no_such_library.so"))
    assert not _lib.opq_usable() and not cls.is_usable()


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("d", C.WIDTHS)
def test_the_bound_holds_for_float32_and_bites(d, kind):
    """numpy's float32 product is inside the bound on every case of the GPU test; a transposed A and a sum without its
    last k element are outside it by more than a factor of 10 somewhere in every case (the smallest measured: 29, where
    the dropped element of a one-row case is a small one; a mean-sized term alone is 1 / (d^2 u) bounds, 16 at d = 1027)."""
    a = C.matrix(d, kind)
    for n in C.ROWS:
        x = C.rows(n, d)
        y64, bound = C.reference(x, a)
        assert (np.abs((x @ a.T).astype(np.float64) - y64) <= bound).all(), (d, kind, n)
        wrong = [x[:, :-1] @ a[:, :-1].T] + ([x @ a] if d > 1 else [])
        for y in wrong:
            assert (np.abs(y.astype(np.float64) - y64) / bound).max() > 10, (d, kind, n)


def test_the_training_restatement_beats_the_identity():
    x, entries = C.make_training_case()
    r = C.train_rotation(x, entries, H.initial_rotation(np.random.RandomState(0), C.T_D), C.T_M, C.T_ITERS)
    r64 = r.astype(np.float64)
    assert np.abs(r64 @ r64.T - np.eye(C.T_D)).max() <= C.T_D * 2.0 ** -23
    trained, plain = C.budget_mse(x, r, entries, C.T_M), C.budget_mse(x, np.eye(C.T_D, dtype=np.float32), entries, C.T_M)
    assert trained < 0.5 * plain, (trained, plain)         # measured: 0.365 against 1.102


@pytest.mark.skipif(_clangxx() is None, reason="ROCm's clang++ is not installed: nothing to compile the program with")
def test_plan_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "opq_plan_main")
    cmd = [_clangxx(), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libsan", os.path.join(HOST, "opq_plan_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, "compiling tests/host/opq_plan_main.cpp failed:\n" + r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]
    assert "opq plan ok: widest_lds=150528 resident_up_to=512" in r.stdout, r.stdout[-4000:]
