"""
The list-major scan of the IVF-SQ index (handle option "isq_scan" = 1: isq_scan_shared_kernel behind ivf_pair_group)
against the numpy restatement of tests/isq_cases.py and against the per-query scan ("isq_scan" = 0) on the same handle:
ids equal, float32 distance bits equal.  stats()["mid_tier_queries"] is the number of (query, list) pairs of non-empty
lists the list-major scan served, and 0 when the per-query scan ran.
"""
import numpy as np
import pytest

from smqtk_indexing_amd import _lib
from tests import isq_cases as S
from tests import ivf_cases as C
from tests import width_cases as W
from tests.test_hip_ivf_shared_scan import _live_pairs, _same

pytestmark = pytest.mark.gpu
KINDS = pytest.mark.parametrize("kind", sorted(S.KINDS))
# The widest row the scan stages in 160 KiB - 256 bytes (isq_shared_lds_bytes, sq_isq_plan.hpp): (2 + G) round_up(d, 4)
# floats for SQ8 -- 4088 for G = 8 --, G round_up(d, 4) floats for F16: IVF-Flat's 5112
G = C.plan_constant("kIvfSharedGroup")
EDGE = {"sq8": (160 * 1024 - 256) // ((2 + G) * 4) // 4 * 4, "f16": (160 * 1024 - 256) // (G * 4) // 4 * 4}
_indexes = {}


def _index(key, kind, case):
    """(restatement, index over the case's rows); under a key the index is built once and kept."""
    sc = S.make(case, S.KINDS[kind])
    idx = None if key is None else _indexes.get((key, kind))
    if idx is None:
        idx = _lib.IsqIndex(case.centroids, sc.kind, sc.vmin, sc.step)
        idx.add(case.x)
        if key is not None:
            _indexes[key, kind] = idx
    return sc, idx


def _both_scans(idx, case, queries, k, nprobe, want, what, routed=True):
    """Option 1 and option 0 on one handle: the same answer; the stats say which scan ran."""
    idx.set_option("isq_scan", 1)
    got = idx.search(queries, k, nprobe)
    served = idx.stats()["mid_tier_queries"]
    idx.set_option("isq_scan", 0)
    old = idx.search(queries, k, nprobe)
    assert idx.stats()["mid_tier_queries"] == 0
    _same(got, *want, what + " (list-major)")
    _same(old, *want, what + " (per query)")
    assert served == (_live_pairs(case, queries, nprobe) if routed else 0), what


@KINDS
@pytest.mark.parametrize("nq", [1, 9, 33])
@pytest.mark.parametrize("nprobe", [1, 5, 64, 100])
@pytest.mark.parametrize("d", C.DIMS)
def test_search_equals_the_restatement(d, nprobe, nq, kind):
    """33 queries at nprobe 64 share every list in groups of 8, 8, 8, 8, 1; nq = 9 is one full group and one of one;
    nprobe 5 shares lists among one to several queries; the far query's first list is empty."""
    case = C.make_case(d)
    sc, idx = _index(d, kind, case)
    for k in (1, 200, 30_000):
        _both_scans(idx, case, case.pool[:nq], k, nprobe, sc.dec.expected(nq, nprobe, k), f"{kind} d={d} nprobe={nprobe} nq={nq} k={k}")


@KINDS
@pytest.mark.parametrize("nq", [1, 33])
@pytest.mark.parametrize("nprobe", [63, 64, 65, 257, 700])
def test_many_lists(nprobe, nq, kind):
    """700 lists of fewer than 256 rows: one chunk per group, many groups, empty lists at probe ranks 63 / 255 / 257."""
    case = C.make_many_lists_case()
    sc, idx = _index("many", kind, case)
    for k in (10, 7000):
        _both_scans(idx, case, case.pool[:nq], k, nprobe, sc.dec.expected(nq, nprobe, k), f"{kind} many lists nprobe={nprobe} nq={nq} k={k}")


WIDTHS = sorted(set(W.WIDTHS) | {35})   # 35: a float16 row padded to 80 bytes, an 8-bit row to 48
SQ8_EDGE = [4085, 4088, 4089, 4092]     # (2 + 8) * 4088 * 4 = 163 520 <= 160 KiB - 256 < (2 + 8) * 4092 * 4


@pytest.mark.parametrize("kind,d", [(kind, d) for kind in sorted(S.KINDS) for d in WIDTHS] + [("sq8", d) for d in SQ8_EDGE])
def test_widths(kind, d):
    """Every width at which the summation branches, and the edges of both kinds' LDS rule.  Beyond a kind's edge option 1
    answers through the per-query scan and serves no pair."""
    case = C.make_width_case(d)
    sc, idx = _index(None, kind, case)
    with idx:
        for nprobe in (3, 8):
            _both_scans(idx, case, case.pool, C.W_K, nprobe, sc.dec.expected(C.W_POOL, nprobe, C.W_K), f"{kind} d={d} nprobe={nprobe}",
                        routed=d <= EDGE[kind])


@KINDS
def test_slices(kind):
    """A key budget of 1 MB: 33 queries run a few to a slice (ivf_slice_queries); each slice is grouped and scanned."""
    case = C.make_case(128)
    sc, idx = _index(None, kind, case)
    with idx:
        idx.set_option("ivf_key_budget_mb", 1)
        idx.set_option("isq_scan", 1)
        for nprobe, k in ((C.NLIST, 10), (5, 200)):
            got = idx.search(case.pool, k, nprobe)
            st = idx.stats()
            _same(got, *sc.dec.expected(C.POOL, nprobe, k), f"{kind} nprobe={nprobe} in slices")
            maxc = max(sc.dec.answer(qi, nprobe)[0].shape[0] for qi in range(C.POOL))
            assert st["scan_launches"] == -(-C.POOL // ((1 << 20) // ((maxc + min(k, maxc)) * 8))) > 1
            assert st["mid_tier_queries"] == _live_pairs(case, case.pool, nprobe)


@KINDS
def test_repeated_query_and_refine_base(kind):
    """One query 17 times in a batch: every list it probes is shared by 17 pairs (8 + 8 + 1).  Then a float32 refine
    store over the index, every probed row a candidate: sq_refine_search takes the scan by the base handle's option,
    the list-major scan chooses the per-query scan's candidates, and the re-ranked answer is IVF-Flat's restatement."""
    case = C.make_case(36)
    sc, idx = _index(36, kind, case)
    idx.set_option("isq_scan", 1)
    for qi in (C.Q_ROW7, 4):
        one = idx.search(case.pool[qi:qi + 1], 200, 5)
        _same(one, *(a[qi:] for a in sc.dec.expected(qi + 1, 5, 200)), f"{kind} one query")
        got = idx.search(np.repeat(case.pool[qi:qi + 1], 17, axis=0), 200, 5)
        assert idx.stats()["mid_tier_queries"] == 17 * _live_pairs(case, case.pool[qi:qi + 1], 5)
        _same(got, np.repeat(one[1], 17, axis=0), np.repeat(one[0], 17, axis=0), f"{kind} 17 copies")
    with _lib.RefineStore(36, _lib.SQ_REFINE_F32) as store:
        store.add(case.x)
        for opt in (1, 0):
            idx.set_option("isq_scan", opt)
            _same(store.search(idx, case.pool, 200, case.n, 5), *case.expected(C.POOL, 5, 200), f"{kind} refined, isq_scan {opt}")
            assert idx.stats()["mid_tier_queries"] == (_live_pairs(case, case.pool, 5) if opt else 0)
