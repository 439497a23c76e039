"""
The int8 stream loop (smqtk_indexing_amd/csrc/sq_dense_i8.hpp: dense8_stream) against the oracle, at the places where
its bookkeeping can go wrong: how many units a wave gets (none, one, two, many; a share that is no whole number of
units), the last unit of the index, the unit on either side of the cache-policy boundary, every geometry of the loop
(128-, 256- and 512-byte rows; the head's, the sample pass's, the scan's and the body's use of it), blocking calls and
pipelined ones (the captured graph).  The loop keeps 64-bit unit numbers throughout -- 32-bit ones were measured and
gained nothing (profiles/int8_stream_loop_before_after.txt) -- so there is no host-side choice of a loop to test.

Every GPU case compares ids and float32 distance bits with oracle.cpu_ref.dense_topk (cosine: 1e-12, ties tolerated as
tests/test_hip_scan_variants.py does) and -- the data being N(0, 1) -- requires that no query left the first stage:
fallback_queries == 0 and mid_tier_queries == 0, so that a stream that loses rows cannot hide behind the later tiers.
The one exception is the tight-cluster case, whose point is a survivor segment that overflows: its answers must still
be the oracle's, by whatever tier.

An index born below 65 536 rows has no int8 copy: every shape starts there.
"""
import numpy as np
import pytest

from oracle import cpu_ref as O
from smqtk_indexing_amd import _lib
from tests.test_hip_scan_variants import _check_every_query

pytestmark = pytest.mark.gpu

BASE = 65536
NQ = 32
_data = {}


def _metric_id(metric):
    return _lib.SQ_METRIC_L2 if metric == "euclidean" else _lib.SQ_METRIC_COSINE


def _edge_rows(n, qi):
    """The ten rows planted as query qi's nearest: query 0 the first and last row of units 0, 1, 127 and 128 (row 8192 between the
    last two), the last row of the last whole unit and the index's last row; the others the first and last rows of five units of their own."""
    if qi == 0:
        return [0, 63, 64, 127, 8128, 8191, 8192, 8255, 64 * ((n - 1) // 64) - 1, n - 1]
    first = 64 * (140 + 30 * qi)
    return [first + 64 * u + e for u in range(5) for e in (0, 63)]


def _dataset(n, d, metric, plant="none"):
    """(db, qs, per-query oracle top-100) of a shape, computed once for all the cases that share it.  Rows and queries are
    N(0, 1); `plant` = "edges": the ten nearest rows of every fourth query sit in the first and last row of a unit, in the
    last unit of the index and in the units on either side of row 8192 (the cache-policy boundary of 128-byte rows with
    one cacheable MB); "cluster": rows 32 768 .. n - 32 769 within 1e-3 of the 32 queries."""
    key = (n, d, metric, plant)
    if key not in _data:
        rng = np.random.default_rng(1000 * d + (n - BASE) + (7 if metric == "cosine" else 0) + len(plant))
        db = rng.standard_normal((n, d)).astype(np.float32)
        qs = rng.standard_normal((NQ, d)).astype(np.float32)
        if plant == "edges":
            for qi in range(0, NQ, 4):
                for j, r in enumerate(_edge_rows(n, qi)):
                    db[r] = qs[qi] + np.float32(1e-3 * (j + 1)) * rng.standard_normal(d).astype(np.float32)
        elif plant == "cluster":
            c = rng.standard_normal(d).astype(np.float32)
            db[32768:n - 32768] = c + np.float32(1e-3) * rng.standard_normal((n - 65536, d)).astype(np.float32)
            qs = (c + np.float32(1e-3) * rng.standard_normal((NQ, d))).astype(np.float32)
        refs = [O.dense_topk(db, q, 100, metric) for q in qs]
        _data[key] = (db, qs, refs)
    return _data[key]


_indexes = {}


def _index(n, d, metric, plant="none"):
    """One index per dataset for the whole module: the cases differ in per-index options, reset before each."""
    key = (n, d, metric, plant)
    if key not in _indexes:
        db, _, _ = _dataset(*key)
        idx = _lib.DenseIndex(db, metric=_metric_id(metric), options={"dense_int8": 1})
        assert idx.info()["int8_in_use"], "no int8 copy: the stream loop is not reached"
        _indexes[key] = idx
    idx = _indexes[key]
    idx.reset_options()
    idx.set_option("dense_int8", 1)
    return idx


@pytest.fixture(scope="module", autouse=True)
def _close_indexes():
    yield
    for idx in _indexes.values():
        idx.close()
    _indexes.clear()
    _data.clear()


def _refs_k(refs, nq, k):
    return [(rd[:k], ri[:k]) for rd, ri in refs[:nq]]


def _blocking(idx, db, qs, refs, nq, k, metric, certify=True):
    dist, ids = idx.search(qs[:nq], k)
    st = idx.stats()
    print("blocking nq=%d k=%d" % (nq, k), {w: st[w] for w in ("fallback_queries", "mid_tier_queries", "candidates", "scan_launches")})
    _check_every_query(db, qs[:nq], dist, ids, k, metric, _refs_k(refs, nq, k))
    if certify:
        assert st["fallback_queries"] == 0 and st["mid_tier_queries"] == 0, st
        assert st["scan_launches"] >= 1, st


def _pipelined(idx, db, qs, refs, nq, k, metric, calls=7):
    """Depth 2: two slots; a slot's first call of a shape runs eagerly, its second captures the graph, later ones replay it."""
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    ddt = torch.float64 if metric == "cosine" else torch.float32
    qd = torch.from_numpy(np.ascontiguousarray(qs[:nq])).to(dev)
    idx.set_option("dense_async_depth", 2)
    outs = [(torch.empty((nq, k), dtype=ddt, device=dev), torch.empty((nq, k), dtype=torch.int64, device=dev)) for _ in range(calls)]
    for od, oi in outs:
        idx.search_device_async(qd.data_ptr(), nq, k, od.data_ptr(), oi.data_ptr(), stream)
    idx.sync()
    torch.cuda.synchronize()
    st = idx.stats()
    for od, oi in outs:
        _check_every_query(db, qs[:nq], od.cpu().numpy(), oi.cpu().numpy(), k, metric, _refs_k(refs, nq, k))
    assert st["fallback_queries"] == 0 and st["mid_tier_queries"] == 0, st


# ---- ring edge counts: rows 65 536 + r; 8 workgroups (about 16 units per wave), 256 (2048 waves share about 1025 units: none,
# one or two each), 136 (a workgroup's share is no whole number of units)
@pytest.mark.parametrize("blocks", [8, 256, 136])
@pytest.mark.parametrize("r", [0, 1, 63, 64, 65])
def test_ring_edge_counts(r, blocks):
    n = BASE + r
    db, qs, refs = _dataset(n, 128, "euclidean")
    idx = _index(n, 128, "euclidean")
    idx.set_option("dense_blocks", blocks)
    _blocking(idx, db, qs, refs, NQ, 10, "euclidean")
    _pipelined(idx, db, qs, refs, NQ, 10, "euclidean")


# ---- the cache-policy boundary: all cacheable, all non-temporal, and non-temporal behind one cacheable MB -- row 8192 of
# 128-byte rows (unit 128: inside every workgroup's share at 8 workgroups, ahead of most at 256), row 4096 / 2048 of wider ones
@pytest.mark.parametrize("blocks", [8, 256])
@pytest.mark.parametrize("nt", [0, 1, 2])
@pytest.mark.parametrize("d", [128, 200, 512])
def test_cache_policy_boundary(d, nt, blocks):
    n = BASE + 65
    db, qs, refs = _dataset(n, d, "euclidean")
    idx = _index(n, d, "euclidean")
    idx.set_option("dense_blocks", blocks)
    idx.set_option("dense_nt", nt)
    if nt == 2:
        idx.set_option("dense_nt_keep_mb", 1)
    _blocking(idx, db, qs, refs, NQ, 10, "euclidean")
    _pipelined(idx, db, qs, refs, NQ, 10, "euclidean", calls=5)


# ---- every geometry of the loop: the fused call's head and body (with and without the tightened threshold), the six-launch
# chain's sample pass and scan
@pytest.mark.parametrize("fused,tighten", [(0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("d", [128, 200, 512])
def test_every_geometry(d, metric, fused, tighten):
    n = BASE + 65
    db, qs, refs = _dataset(n, d, metric)
    idx = _index(n, d, metric)
    idx.set_option("dense_fused", fused)
    idx.set_option("dense_tighten", tighten)
    for nq in (1, 31, 32):
        for k in (1, 100):
            _blocking(idx, db, qs, refs, nq, k, metric)
    _pipelined(idx, db, qs, refs, 31, 100, metric, calls=5)


# ---- survivors at the edges of units, of the index and of the cache-policy boundary
@pytest.mark.parametrize("blocks,nt", [(8, 2), (256, 2), (136, 0), (8, 1)])
def test_survivors_at_the_edges(blocks, nt):
    n = BASE + 65
    db, qs, refs = _dataset(n, 128, "euclidean", "edges")
    for qi in range(0, NQ, 4):      # the planted rows ARE the ten nearest
        assert set(_edge_rows(n, qi)) == set(refs[qi][1][:10].tolist())
    idx = _index(n, 128, "euclidean", "edges")
    idx.set_option("dense_blocks", blocks)
    idx.set_option("dense_nt", nt)
    if nt == 2:
        idx.set_option("dense_nt_keep_mb", 1)
    _blocking(idx, db, qs, refs, NQ, 10, "euclidean")
    _pipelined(idx, db, qs, refs, NQ, 10, "euclidean", calls=5)


CLUSTER_N = BASE + 98304        # 65 536 N(0, 1) rows around a cluster of 98 304 = 1536 units


def test_tight_cluster_overflows_a_segment():
    """Rows 32 768 .. 131 071 (units 512 .. 2047) lie within 1e-3 of all 32 queries, inside the int8 slack: every lane of
    every tile of those units has a survivor, 128 entries per unit.  At 8 workgroups the ticket map gives each workgroup 8 of
    every 64 units, 192 of the cluster's; whichever way its eight waves share them, one takes 24 or more -- 3072 entries
    against the 2048 a wave's segment holds.  The positions beyond the segment must be dropped, counted and flagged: the
    queries are then answered by the later tiers (asserted), and the answers are the oracle's.  Exempt from the first-stage
    condition, as its point is the overflow."""
    n = CLUSTER_N
    db, qs, refs = _dataset(n, 128, "euclidean", "cluster")
    idx = _index(n, 128, "euclidean", "cluster")
    idx.set_option("dense_blocks", 8)
    for fused in (1, 0):            # the body's and the scan's use of the loop
        idx.set_option("dense_fused", fused)
        _blocking(idx, db, qs, refs, NQ, 10, "euclidean", certify=False)
        st = idx.stats()
        assert st["scan_launches"] >= 1 and st["bytes_scanned"] >= (-(-n // 64) * 64) * 132, st    # the int8 pass ran
        assert st["fallback_queries"] + st["mid_tier_queries"] > 0, st                             # ... and overflowed
