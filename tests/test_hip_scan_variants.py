"""
Every launched build of the dense first-stage scan against the oracle.

SCAN_VARIANTS maps each template instantiation of the scan kernels (dense_scan_kernel, dense_wide_scan_kernel,
dense8_scan_kernel, dense8_scan_mt_kernel, dense8_body_kernel; SAMPLE builds included) to the per-index options and
shapes that make the library launch it.  tests/test_isa_hazards.py checks on the CPU that the table names every
instantiation compiled into sq_dense.hip.

Each case fixes the grid (dense_blocks = 8) and picks n so that the waves of the full pass own c or c + 1 row tiles
(c = 0, 2, 4, 9: waves with no tile, with fewer tiles than the ring has stages, exactly a group, a few groups and a
tail), with a partial last tile.  Queries are planted on rows of the last tile of a wave's range, on row n - 1 and on a
tie group that straddles a tile boundary.  Every query is checked: L2 ids and float32 bits equal to the oracle; cosine
distances within 1e-12 with ties tolerated; and no query may have left the scan for the exact path.
"""
import zlib
from dataclasses import dataclass

import numpy as np
import pytest

from oracle import cpu_ref as O
from smqtk_indexing_amd import _lib

pytestmark = pytest.mark.gpu


@dataclass(frozen=True)
class Recipe:
    options: dict                    # per-index options (DenseIndex(..., options=...))
    dims: tuple                      # row widths that reach the build
    batches: tuple                   # queries per call that reach the build
    waves: int = 4                   # waves per workgroup of the full pass (sizes the tail shapes)
    int8: bool = False               # the int8 first stage (its copy needs 65536 rows or more)
    metrics: tuple = ("euclidean", "cosine")
    unreachable: str = ""            # compiled but never launched: why (no GPU case)


SCAN_VARIANTS = {}


def _add(fmt, recipe, sample=(False, True)):
    for s in sample:
        SCAN_VARIANTS[fmt.format(S="true" if s else "false")] = recipe


BF16 = {"dense_int8": 0, "dense_blocks": 8}
NO_NT = dict(BF16, dense_nt=0)

# ---- d_pad = 128 (one k-unit)
# one query tile per wave: eight waves, two stages (the default), or four waves with 2 / 3 / 4 stages
_add("dense_scan_kernel<8,2,1,1,2,false,{S},false>", Recipe(dict(NO_NT, dense_qt=1), (1, 100, 128), (33, 97, 257), waves=8))
for _st in (2, 3, 4):
    _add("dense_scan_kernel<4,%d,1,1,2,false,{S},false>" % _st,
         Recipe(dict(NO_NT, dense_qt=1, dense_waves=4, dense_stages=_st), (1, 100, 128), (33, 65, 130)))
# four query tiles per wave, q_hi only: the skewed epilogue (SKEW); its non-temporal build for one query group
_add("dense_scan_kernel<4,4,1,4,1,true,{S},false>", Recipe(dict(NO_NT), (100, 128), (65, 97, 130, 257)))
_add("dense_scan_kernel<4,4,1,4,1,true,{S},true>", Recipe(dict(BF16, dense_nt=1), (100, 128), (65, 97, 128)))
_add("dense_scan_kernel<4,4,1,4,2,true,{S},false>", Recipe(dict(NO_NT, dense_qplanes=2), (100, 128), (65, 130, 257)))
# two query tiles per wave: eight waves (q_hi only; non-temporal for one group), four waves, two planes
_add("dense_scan_kernel<8,2,1,2,1,true,{S},false>", Recipe(dict(NO_NT, dense_qt=2), (100, 128), (33, 64, 97), waves=8))
_add("dense_scan_kernel<8,2,1,2,1,true,{S},true>", Recipe(dict(BF16, dense_nt=1), (100, 128), (33, 64), waves=8))
_add("dense_scan_kernel<4,4,1,2,1,true,{S},false>", Recipe(dict(NO_NT, dense_qt=2, dense_waves=4), (100, 128), (33, 64, 130)))
_add("dense_scan_kernel<4,4,1,2,2,true,{S},false>", Recipe(dict(NO_NT, dense_qt=2, dense_qplanes=2), (100, 128), (33, 64, 97)))
# ---- d_pad = 256 .. 512 (two to four k-units)
_KU_DIMS = {2: (129, 256), 3: (300, 384), 4: (400, 512)}
for _ku, _dims in _KU_DIMS.items():
    # one query tile: the LDS copy of the query tile leaves room for 3 stages (KU 2, 3) or 2 (KU 4)
    _add("dense_scan_kernel<4,2,%d,1,2,false,{S},false>" % _ku, Recipe(dict(NO_NT, dense_qt=1, dense_stages=2), _dims, (33, 65, 130)))
    if _ku < 4:
        _add("dense_scan_kernel<4,3,%d,1,2,false,{S},false>" % _ku, Recipe(dict(NO_NT, dense_qt=1), _dims, (33, 97, 257)))
    _add("dense_scan_kernel<4,4,%d,2,1,true,{S},false>" % _ku, Recipe(dict(NO_NT), _dims, (33, 64, 65, 97, 128, 130, 257)))
_NOROOM = "scan_geometry: the LDS copy of the query tile leaves the ring fewer than 4 stages (3 for KU 4)"
for _ku in (2, 3, 4):
    _add("dense_scan_kernel<4,4,%d,1,2,false,{S},false>" % _ku, Recipe({}, (), (), unreachable=_NOROOM))
_add("dense_scan_kernel<4,3,4,1,2,false,{S},false>", Recipe({}, (), (), unreachable=_NOROOM))
# ---- rows beyond 512 dimensions: query planes 1 / 2, query tiles 1 / 2 / 4 per wave
for _qp in (1, 2):
    for _qt in (1, 2, 4):
        _add("dense_wide_scan_kernel<%d,%d,{S}>" % (_qp, _qt),
             Recipe(dict(BF16, dense_qt=_qt, dense_qplanes=_qp), (600, 700), (33, 65, 130) if _qt > 1 else (33, 64),
                    waves=8))
# ---- the int8 first stage (128 / 256 / 512-byte rows)
I8 = {"dense_int8": 1, "dense_blocks": 8, "dense_nt": 0}
_I8_DIMS = {4: (100, 128), 8: (129, 256), 16: (400, 512)}
for _ks, _dims in _I8_DIMS.items():
    # one query tile: the six-launch chain (sample pass + full pass) and the fused call's body (L2 / cosine)
    _add("dense8_scan_kernel<%d,{S}>" % _ks, Recipe(dict(I8, dense_fused=0), _dims, (17, 32), waves=8 if _ks <= 8 else 4, int8=True))
    for _cos in (False, True):
        SCAN_VARIANTS["dense8_body_kernel<%d,%s>" % (_ks, "true" if _cos else "false")] = Recipe(
            dict(I8), _dims, (17, 32), waves=8 if _ks <= 8 else 4, int8=True, metrics=("cosine",) if _cos else ("euclidean",))
# two / four query tiles per wave over 128-byte rows
_add("dense8_scan_mt_kernel<2,{S}>", Recipe(dict(I8, dense_qt=2), (100, 128), (33, 64), waves=8, int8=True))
_add("dense8_scan_mt_kernel<4,{S}>", Recipe(dict(I8, dense_qt=4, dense_int8_batch=256), (100, 128), (65, 97, 130), waves=8, int8=True))

TAILS = (0, 2, 4, 9)     # the full pass's waves own c or c + 1 row tiles
K = 10


def _cases():
    out = []
    for name, r in SCAN_VARIANTS.items():
        if r.unreachable:
            continue
        for c in ((0, 9) if r.int8 else TAILS):
            for metric in r.metrics:
                out.append(pytest.param(name, c, metric, id="%s-c%d-%s" % (name, c, metric[:3])))
    return out


def _dedupe(cases):
    """SAMPLE = true and false share a recipe (one call launches both): one case per (recipe, tail, metric)."""
    seen, out = set(), []
    for p in cases:
        name, c, metric = p.values
        key = (id(SCAN_VARIANTS[name]), c, metric)
        if key not in seen:
            seen.add(key)
            out.append(p)
    return out


def _shape(r, c, metric):
    """(n, d, nq) of a case: n puts c or c + 1 row tiles on every wave of the full pass, the last tile partial."""
    pick = c + (metric == "cosine")
    dims = [x for x in r.dims if metric == "euclidean" or x > 1]     # (cosine of one-dimensional rows: two values, all ties)
    d = dims[pick % len(dims)]
    nq = r.batches[pick % len(r.batches)]
    nwaves = 8 * r.waves
    if r.int8:
        n = 65536 + c * 4099 + 17
    else:
        n_tiles = c * nwaves + nwaves // 2 + 1
        n = n_tiles * 32 - 7
    return n, d, nq


def _plant(rng, n, d, nq, nwaves):
    """Rows and queries: each query near a row of the last tile of some wave's range, one on row n - 1, one on a tie
    group across a tile boundary, the rest random."""
    db = rng.standard_normal((n, d)).astype(np.float32)
    qs = rng.standard_normal((nq, d)).astype(np.float32)
    n_tiles = -(-n // 32)
    last = []
    for w in range(min(nwaves, n_tiles)):
        t = w + ((n_tiles - 1 - w) // nwaves) * nwaves          # the last tile of wave w
        last.append(t)
    noise = np.float32(1e-3)
    for qi in range(0, nq, 2):
        t = last[(qi // 2) % len(last)]
        row = min(n - 1, 32 * t + (qi * 7) % 32)
        qs[qi] = db[row] + noise * rng.standard_normal(d).astype(np.float32)
    if n > 64:
        b = 32 * (n_tiles // 2)                                  # tie group: rows b - 2 .. b + 1
        db[b - 2:b + 2] = db[b - 2]
        qs[1 % nq] = db[b - 2] + noise * rng.standard_normal(d).astype(np.float32)
    qs[nq - 1] = db[n - 1]
    return db, qs


def _check_every_query(db, qs, dist, ids, k, metric, refs=None):
    """`refs`: the oracle's (distances, ids) per query where several cases share them."""
    for qi, q in enumerate(qs):
        rd, ri = refs[qi] if refs is not None else O.dense_topk(db, q, k, metric)
        kk = len(rd)
        if metric == "euclidean":
            assert dist.dtype == np.float32
            np.testing.assert_array_equal(ids[qi, :kk], ri, err_msg="query %d" % qi)
            np.testing.assert_array_equal(dist[qi, :kk].view(np.uint32), rd.view(np.uint32), err_msg="query %d" % qi)
        else:
            np.testing.assert_allclose(dist[qi, :kk], rd, rtol=1e-12, atol=1e-15, err_msg="query %d" % qi)
            mism = ids[qi, :kk] != ri
            if mism.any():
                full = O.dense_distances(db, q, "cosine")
                assert np.abs(full[ids[qi, :kk][mism]] - full[ri[mism]]).max() < 1e-14, "query %d" % qi


@pytest.mark.parametrize("name,c,metric", _dedupe(_cases()))
def test_scan_variant_against_oracle(name, c, metric):
    r = SCAN_VARIANTS[name]
    n, d, nq = _shape(r, c, metric)
    rng = np.random.default_rng(zlib.crc32(("%s %d %d %d %s" % (name.split("<")[0], n, d, nq, metric)).encode()))
    db, qs = _plant(rng, n, d, nq, 8 * r.waves)
    opts = dict(r.options)
    if not r.int8:
        opts["candidate_cap"] = n - 1          # the scan path down to the smallest shapes (n > cap)
    m = _lib.SQ_METRIC_L2 if metric == "euclidean" else _lib.SQ_METRIC_COSINE
    idx = _lib.DenseIndex(db, metric=m, options=opts)
    try:
        if r.int8:
            assert idx.info()["int8_in_use"], "no int8 copy: the int8 builds are not reached"
        dist, ids = idx.search(qs, K)
        st = idx.stats()
        assert st["fallback_queries"] == 0, st     # the answer checked is the scan's, not the exact path's
        assert st["scan_launches"] >= 1, st
        _check_every_query(db, qs, dist, ids, K, metric)
    finally:
        idx.close()


# ---- option "dense_rerank_segments": survivor segments per re-rank workgroup of the chains' shared tail
# (bf16 chain: any divisor of the scan workgroup's waves, 8 segments run on the kernel's 512-thread limit; int8 six-launch
# chain: L2 only, four at the most -- its cosine cases run the same launch three times and are kept as the fixed point:
# the option must not change a cosine answer).  n as _shape builds it (c row tiles per wave + a partial last tile).
TAIL_GROUPS = {
    # name: (options, scan waves, n, d, nq, segments)
    "bf16-8w": (dict(dense_int8=0, dense_blocks=8, candidate_cap=2048, dense_qt=1), 8, (9 * 64 + 33) * 32 - 7, 100, 33, (1, 2, 4, 8)),
    "bf16-4w": (dict(dense_int8=0, dense_blocks=8, candidate_cap=2048), 4, (18 * 32 + 17) * 32 - 7, 128, 130, (1, 2, 4)),
    "int8-six": (dict(dense_int8=1, dense_fused=0), 8, 65536 + 17, 100, 17, (1, 2, 4)),
}
_tail_data = {}


def _tail_case(group, metric):
    """(db, qs, oracle answers) of a group, computed once for all its segment counts."""
    if (group, metric) not in _tail_data:
        _, waves, n, d, nq, _ = TAIL_GROUPS[group]
        rng = np.random.default_rng(zlib.crc32(("tail %s %s" % (group, metric)).encode()))
        db, qs = _plant(rng, n, d, nq, 8 * waves)
        _tail_data[(group, metric)] = (db, qs, [O.dense_topk(db, q, K, metric) for q in qs])
    return _tail_data[(group, metric)]


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("group,segments", [(g, s) for g, v in TAIL_GROUPS.items() for s in v[5]])
def test_rerank_segments_against_oracle(group, segments, metric):
    db, qs, refs = _tail_case(group, metric)
    opts = dict(TAIL_GROUPS[group][0], dense_rerank_segments=segments)
    m = _lib.SQ_METRIC_L2 if metric == "euclidean" else _lib.SQ_METRIC_COSINE
    idx = _lib.DenseIndex(db, metric=m, options=opts)
    try:
        if opts.get("dense_int8") == 1:
            assert idx.info()["int8_in_use"], "no int8 copy: the six-launch int8 chain is not reached"
        dist, ids = idx.search(qs, K)
        st = idx.stats()
        print(group, segments, metric, st)
        # the answers checked are the chain's own: sample pass + full pass, every query certified by the tail's select
        # (a later tier would add a pass per group of queries and count them here)
        assert st["scan_launches"] == 2 and st["fallback_queries"] == 0 and st["mid_tier_queries"] == 0, st
        _check_every_query(db, qs, dist, ids, K, metric, refs)
    finally:
        idx.close()
