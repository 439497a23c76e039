"""Host side of option "dense_int8_wide" (the int8 first stage for rows of 513 to 8192 dimensions): the
library and `_lib` know the name, `DenseIndex(options=...)` marshals it to sq_dense_create_opts, the brute-force plugin
hands an index the process-wide choice as its own, and the header documents it.  Nothing here launches a kernel: the
device side is tests/test_hip_dense_int8_wide.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from smqtk_indexing_amd import _lib
from smqtk_indexing_amd._compat import DescriptorMemoryElement
from smqtk_indexing_amd.impls.nn_index import hip_bruteforce
from smqtk_indexing_amd.impls.nn_index.hip_bruteforce import HipBruteForceNearestNeighborsIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dense_int8_wide"


def test_the_library_and_lib_know_the_option():
    assert NAME in _lib.DENSE_CREATE_OPTIONS
    lib = _lib.load()
    try:
        assert lib.sq_set_option(NAME.encode(), 1) == 0, lib.sq_last_error()
    finally:
        assert lib.sq_set_option(NAME.encode(), 0) == 0
    assert lib.sq_set_option(b"dense_int8_wider", 1) == -1 and b"unknown option" in lib.sq_last_error()
    # sq_dense_create_opts resolves the names before anything else: a known one gets as far as the argument check
    names = (ctypes.c_char_p * 1)(NAME.encode())
    values = (ctypes.c_int64 * 1)(1)
    h = ctypes.c_int64(0)
    assert lib.sq_dense_create_opts(None, 0, 0, _lib.SQ_METRIC_L2, _lib.SQ_MEM_HOST, 0, names, values, 1, ctypes.byref(h)) == -1
    assert b"bad argument" in lib.sq_last_error()
    names = (ctypes.c_char_p * 1)(b"dense_int8_wider")
    assert lib.sq_dense_create_opts(None, 0, 0, _lib.SQ_METRIC_L2, _lib.SQ_MEM_HOST, 0, names, values, 1, ctypes.byref(h)) == -1
    assert b"unknown option" in lib.sq_last_error()


def test_set_option_remembers_the_process_wide_value(monkeypatch):
    monkeypatch.setattr(_lib, "_process_options", {})
    assert _lib.process_option(NAME) is None and _lib.process_option(NAME, 0) == 0
    try:
        _lib.set_option(NAME, 1)
        assert _lib.process_option(NAME, 0) == 1
    finally:
        _lib.set_option(NAME, 0)
    assert _lib.process_option(NAME, 5) == 0


class _StubLibrary:
    """Stands where the loaded library stands: records what DenseIndex hands to the create calls."""

    def __init__(self):
        self.calls = []

    def sq_dense_create(self, ptr, n, d, metric, mem, id_base, out):
        self.calls.append(("sq_dense_create", n, d, metric, mem, id_base))
        out._obj.value = 41
        return 0

    def sq_dense_create_opts(self, ptr, n, d, metric, mem, id_base, names, values, n_opts, out):
        self.calls.append(("sq_dense_create_opts", n, d, metric, mem, id_base, [names[i] for i in range(n_opts)],
                           [values[i] for i in range(n_opts)], n_opts))
        out._obj.value = 42
        return 0

    def sq_dense_destroy(self, h):
        self.calls.append(("sq_dense_destroy", h))
        return 0


def test_dense_index_marshals_create_options(monkeypatch):
    stub = _StubLibrary()
    monkeypatch.setattr(_lib, "load", lambda: stub)
    db = np.zeros((3, 600), dtype=np.float32)
    idx = _lib.DenseIndex(db, metric=_lib.SQ_METRIC_COSINE, options={NAME: 1, "dense_int8": -1})
    assert idx.handle == 42
    assert stub.calls == [("sq_dense_create_opts", 3, 600, _lib.SQ_METRIC_COSINE, _lib.SQ_MEM_HOST, 0, [NAME.encode(), b"dense_int8"], [1, -1], 2)]
    idx.close()
    plain = _lib.DenseIndex(db)
    assert plain.handle == 41 and stub.calls[-1][0] == "sq_dense_create"
    plain.close()


@pytest.mark.parametrize("process_value,expected", [(None, {}), (0, {}), (1, {"options": {NAME: 1}})])
def test_plugin_hands_the_process_wide_choice_to_its_index(monkeypatch, process_value, expected):
    made = []

    class _Dense:
        def __init__(self, matrix, metric=None, **kw):
            made.append((matrix.shape, metric, kw))

        def close(self):
            pass

    monkeypatch.setattr(hip_bruteforce._lib, "DenseIndex", _Dense)
    monkeypatch.setattr(hip_bruteforce, "_require_usable", lambda self: None)
    monkeypatch.setattr(_lib, "_process_options", {} if process_value is None else {NAME: process_value})
    index = HipBruteForceNearestNeighborsIndex("cosine")
    assert index.get_config() == {"distance_method": "cosine", "read_only": False}
    rows = np.random.default_rng(0).standard_normal((4, 600)).astype(np.float32)
    index._set([DescriptorMemoryElement(i).set_vector(r) for i, r in enumerate(rows)], rows)
    index._device()
    assert made == [((4, 600), _lib.SQ_METRIC_COSINE, expected)]


def test_the_header_documents_the_option():
    src = open(os.path.join(ROOT, "include", "smqtk_hip.h")).read()
    comments = " ".join(re.findall(r"/\*.*?\*/", src, flags=re.S))
    at = comments.index('Option "%s"' % NAME)
    doc = comments[at:at + 1200]
    # beside "dense_int8": the default, the widths, the row floor and where it is read
    assert comments.index('Option "dense_int8"') < at < comments.index('Option "dense_int8_batch"')
    for word in ("0 by default", "513 to 8192", "65536", "sq_dense_create_opts", "32 queries"):
        assert word in doc, word
    # the options table of the library itself
    core = open(os.path.join(ROOT, "smqtk_indexing_amd", "csrc", "sq_core.hip")).read()
    assert '{"%s", &Options::%s}' % (NAME, NAME) in core
    common = open(os.path.join(ROOT, "smqtk_indexing_amd", "csrc", "sq_common.hpp")).read()
    assert re.search(r"int %s = 0;" % NAME, common)
