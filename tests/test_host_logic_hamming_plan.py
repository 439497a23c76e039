"""The plan view of the Hamming search (sq_hamming_search with mem = SQ_MEM_PLAN) without a device: the header and the
ctypes layer agree on its constants, and an unknown handle is refused before anything touches the GPU."""
import ctypes
import os
import re

from smqtk_indexing_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_field_count_matches_the_header():
    src = open(os.path.join(ROOT, "include", "smqtk_hip.h")).read()
    m = re.search(r"#define\s+SQ_HAMMING_PLAN_FIELDS\s+(\d+)", src)
    assert m and int(m.group(1)) == _lib.SQ_HAMMING_PLAN_FIELDS == len(_lib.HammingIndex.PLAN_FIELDS)
    for name in ("SQ_MEM_PLAN", "SQ_MEM_PLAN_ASYNC"):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, src)
        assert m and int(m.group(1)) == getattr(_lib, name)
    assert len({_lib.SQ_MEM_HOST, _lib.SQ_MEM_DEVICE, _lib.SQ_MEM_DEVICE_ASYNC, _lib.SQ_MEM_PLAN, _lib.SQ_MEM_PLAN_ASYNC}) == 5


def test_plan_of_an_unknown_handle_fails_without_a_device():
    lib = _lib.load()
    out = (ctypes.c_int64 * _lib.SQ_HAMMING_PLAN_FIELDS)()
    for mem in (_lib.SQ_MEM_PLAN, _lib.SQ_MEM_PLAN_ASYNC):
        rc = lib.sq_hamming_search(123456789, None, 4, 10, None, out, mem, None)
        assert rc != _lib.SQ_OK
        assert "sq_hamming_plan: unknown handle" in lib.sq_last_error().decode()
