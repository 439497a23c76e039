"""Host side of option "dense_bf16" (whether a dense index keeps its bfloat16 scan copy: 1 always, -1 on demand, 0 never;
DESIGN.md 4.8): the library and `_lib` know the name, `DenseIndex(options=...)` marshals it to sq_dense_create_opts, the
brute-force plugin hands an index the process-wide choice as its own, the distributed helpers pass options through, and the
header documents it.  Nothing here launches a kernel: the device side is tests/test_hip_dense_bf16_on_demand.py."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest

from smqtk_indexing_amd import _lib, distributed
from smqtk_indexing_amd._compat import DescriptorMemoryElement
from smqtk_indexing_amd.impls.nn_index import hip_bruteforce
from smqtk_indexing_amd.impls.nn_index.hip_bruteforce import HipBruteForceNearestNeighborsIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dense_bf16"


def test_the_library_and_lib_know_the_option():
    assert NAME in _lib.DENSE_CREATE_OPTIONS
    lib = _lib.load()
    try:
        for value in (-1, 0, 1):
            assert lib.sq_set_option(NAME.encode(), value) == 0, lib.sq_last_error()
    finally:
        assert lib.sq_set_option(NAME.encode(), 1) == 0
    # sq_dense_create_opts resolves the names before anything else: a known one gets as far as the argument check
    names = (ctypes.c_char_p * 1)(NAME.encode())
    values = (ctypes.c_int64 * 1)(-1)
    h = ctypes.c_int64(0)
    assert lib.sq_dense_create_opts(None, 0, 0, _lib.SQ_METRIC_L2, _lib.SQ_MEM_HOST, 0, names, values, 1, ctypes.byref(h)) == -1
    assert b"bad argument" in lib.sq_last_error()


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


def test_dense_index_marshals_the_option(monkeypatch):
    stub = _StubLibrary()
    monkeypatch.setattr(_lib, "load", lambda: stub)
    db = np.zeros((3, 128), dtype=np.float32)
    idx = _lib.DenseIndex(db, options={NAME: -1})
    assert idx.handle == 42
    assert stub.calls == [("sq_dense_create_opts", 3, 128, _lib.SQ_METRIC_L2, _lib.SQ_MEM_HOST, 0, [NAME.encode()], [-1], 1)]
    idx.close()


@pytest.mark.parametrize("process,expected", [
    ({}, {}),
    ({NAME: 1}, {}),
    ({NAME: -1}, {"options": {NAME: -1}}),
    ({NAME: 0}, {"options": {NAME: 0}}),
    ({"dense_int8_wide": 1}, {"options": {"dense_int8_wide": 1}}),
    ({"dense_int8_wide": 1, NAME: 1}, {"options": {"dense_int8_wide": 1}}),
    ({"dense_int8_wide": 1, NAME: -1}, {"options": {"dense_int8_wide": 1, NAME: -1}}),
    ({"dense_int8_wide": 0, NAME: 0}, {"options": {NAME: 0}}),
])
def test_plugin_hands_the_process_wide_choice_to_its_index(monkeypatch, process, expected):
    made = []

    class _Dense:
        def __init__(self, matrix, metric=None, **kw):
            made.append((matrix.shape, metric, kw))

        def close(self):
            pass

    monkeypatch.setattr(hip_bruteforce._lib, "DenseIndex", _Dense)
    monkeypatch.setattr(hip_bruteforce, "_require_usable", lambda self: None)
    monkeypatch.setattr(_lib, "_process_options", dict(process))
    index = HipBruteForceNearestNeighborsIndex("cosine")
    assert index.get_config() == {"distance_method": "cosine", "read_only": False}
    rows = np.random.default_rng(0).standard_normal((4, 600)).astype(np.float32)
    index._set([DescriptorMemoryElement(i).set_vector(r) for i, r in enumerate(rows)], rows)
    index._device()
    assert made == [((4, 600), _lib.SQ_METRIC_COSINE, expected)]


class _Tensor:
    """As much of a device tensor as the helpers touch before they hand it to DenseIndex."""
    shape = (5, 128)

    def data_ptr(self):
        return 4096


@pytest.mark.parametrize("options,expected", [(None, {}), ({}, {}), ({NAME: 0}, {"options": {NAME: 0}}),
                                              ({NAME: -1, "dense_int8": 1}, {"options": {NAME: -1, "dense_int8": 1}})])
def test_distributed_helpers_pass_options(monkeypatch, options, expected):
    made = []

    class _Dense:
        def __init__(self, ptr, **kw):
            made.append((ptr, kw))

    monkeypatch.setattr(_lib, "DenseIndex", _Dense)
    if "torch" not in sys.modules:   # (the helpers import it for dtypes only before the first search)
        monkeypatch.setitem(sys.modules, "torch", types.SimpleNamespace(float32="f32", float64="f64", int64="i64"))
    t = _Tensor()
    shard = distributed.dense_shard(t, 1000, metric=_lib.SQ_METRIC_COSINE, options=options)
    common = {"n": 5, "d": 128, "metric": _lib.SQ_METRIC_COSINE, "device_ptr": True, "keepalive": t}
    assert made == [(4096, dict(common, id_base=1000, **expected))]
    assert isinstance(shard.index, _Dense)
    del made[:]
    search = distributed.dense_local_builder(_lib.SQ_METRIC_COSINE, options=options)(t)
    assert made == [(4096, dict(common, **expected))]
    assert isinstance(search.index, _Dense)
    if options:   # the caller's dict is not kept: a later change of it does not reach indexes built afterwards
        assert made[0][1]["options"] is not options


def test_distributed_helpers_default_to_no_options():
    import inspect
    assert inspect.signature(distributed.dense_shard).parameters["options"].default is None
    assert inspect.signature(distributed.dense_local_builder).parameters["options"].default is None


def test_the_header_documents_the_option():
    src = open(os.path.join(ROOT, "include", "smqtk_hip.h")).read()
    comments = " ".join(re.findall(r"/\*.*?\*/", src, flags=re.S))
    at = comments.index('Option "%s"' % NAME)
    assert comments.index('Option "dense_mid_tier"') < at
    doc = " ".join(comments[at:at + 2400].replace("*", " ").split())   # (the comment block's line prefixes out)
    for word in ("1 by default", "-1, on demand", "0, never", "1: sq_dense_create and sq_dense_compact build", "sq_dense_compact sheds",
                 "sq_dense_info reports 0 bytes", "sq_dense_create_opts", "nothing is freed"):
        assert word in doc, word
    # the paragraphs other tests read stay where they were
    assert comments.index('Option "dense_int8"') < comments.index('Option "dense_int8_wide"') < comments.index('Option "dense_int8_batch"') < at


def test_the_option_table_and_the_default():
    core = open(os.path.join(ROOT, "smqtk_indexing_amd", "csrc", "sq_core.hip")).read()
    assert '{"%s", &Options::%s}' % (NAME, NAME) in core
    common = open(os.path.join(ROOT, "smqtk_indexing_amd", "csrc", "sq_common.hpp")).read()
    assert re.search(r"int %s = 1;" % NAME, common)
