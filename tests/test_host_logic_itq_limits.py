"""HipItqFunctor.fit chooses the device fit by the library's limits (SQ_ITQFIT_MAX_D / SQ_ITQFIT_MAX_BITS), not by a
literal of its own.  Host logic only: the device is a recording stand-in."""
import os
import re

import numpy as np
import pytest

from smqtk_indexing_amd import _lib
from smqtk_indexing_amd._compat import DescriptorMemoryElement
from smqtk_indexing_amd.impls.lsh_functor import hip_itq
from smqtk_indexing_amd.impls.lsh_functor.hip_itq import HipItqFunctor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Recorder:
    """Stands in for _fit_device and get_hash: records which path fit() took."""

    def __init__(self):
        self.device_shapes = []

    def fit_device(self, functor, x_in):
        self.device_shapes.append(x_in.shape)
        d = x_in.shape[1]
        return np.zeros(d, dtype=x_in.dtype), np.eye(d)[:, :functor.bit_length]


def _fit(monkeypatch, n, d, bits, **kw):
    rec = _Recorder()
    monkeypatch.setattr(hip_itq._lib, "usable", lambda: True)
    monkeypatch.setattr(HipItqFunctor, "_fit_device", lambda self, x: rec.fit_device(self, x))
    monkeypatch.setattr(HipItqFunctor, "get_hash", lambda self, x: np.zeros((len(x), self.bit_length), dtype=bool))
    rng = np.random.default_rng(d)
    elems = [DescriptorMemoryElement(i).set_vector(row) for i, row in enumerate(rng.standard_normal((n, d)).astype(np.float32))]
    f = HipItqFunctor(bit_length=bits, itq_iterations=1, random_seed=0, **kw)
    f.fit(elems)
    return rec, f


@pytest.mark.parametrize("d", [512, 513, 1000, 2048])
def test_fit_takes_the_device_path_up_to_the_library_limit(monkeypatch, d):
    rec, f = _fit(monkeypatch, 12, d, 8)
    assert rec.device_shapes == [(12, d)]
    assert f.rotation.shape == (d, 8)


def test_fit_falls_back_to_the_host_beyond_the_library_limit(monkeypatch):
    monkeypatch.setattr(_lib, "SQ_ITQFIT_MAX_D", 40)       # (a host fit at 8193 dimensions would take minutes)
    rec, f = _fit(monkeypatch, 60, 48, 8)
    assert rec.device_shapes == [] and f.rotation.shape == (48, 8)
    rec, _ = _fit(monkeypatch, 60, 40, 8)
    assert rec.device_shapes == [(60, 40)]
    monkeypatch.setattr(_lib, "SQ_ITQFIT_MAX_BITS", 4)
    rec, _ = _fit(monkeypatch, 60, 40, 8)
    assert rec.device_shapes == []
    rec, _ = _fit(monkeypatch, 60, 40, 8, fit_on_device=False)
    assert rec.device_shapes == []


def test_python_limits_are_the_header_limits():
    text = open(os.path.join(ROOT, "include", "smqtk_hip.h")).read()
    assert int(re.search(r"#define\s+SQ_ITQFIT_MAX_D\s+(\d+)", text).group(1)) == _lib.SQ_ITQFIT_MAX_D == 8192
    assert int(re.search(r"#define\s+SQ_ITQFIT_MAX_BITS\s+(\d+)", text).group(1)) == _lib.SQ_ITQFIT_MAX_BITS == 256
