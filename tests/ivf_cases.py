"""
Case builder and numpy restatement for the tests of the IVF-Flat index (`sq_ivf_*`): no GPU.

The restatement is the contract of include/smqtk_hip_ivf.h over `oracle.cpu_ref`:

    assignment  list of a row      = O.dense_topk(centroids, row, 1)       (nearest centroid, ties to the lowest list)
    probe       lists of a query   = O.dense_topk(centroids, q, nprobe)    (min(nprobe, nlist) of them)
    result      the k smallest (distance, id) over the rows of the probed lists, distances those of
                O.euclidean_distance(row, q) in float32; -1 / +inf behind the last candidate

`make_case(d)` builds the case the GPU tests run (n = 20 011 rows, 64 lists, seeded standard_normal) and ASSERTS what
those tests lean on, so a seed that misses a condition fails on the CPU (tests/test_ivf_cases_cpu.py):

1. exactly two empty lists: 9 (its centroid equals centroid 3, and ties go to the lower list) and 11 (its centroid is 1000
   everywhere);
2. a list longer than one scan chunk (256 candidates: kIvfChunk of sq_ivf_plan.hpp) -- and longer than 1024, so one
   query's scan has several work items inside ONE list;
3. a list shorter than k = 200 (a probe of it alone pads);
4. rows 100 .. 139 are copies of row 7: the query x[7] has 41 candidates at distance 0, ordered by id.

`make_many_lists_case()` (6007 rows, d = 20, 700 lists) is the shape where a query probes more lists than a wave has
lanes and a scan chunk spans many lists.  It asserts:

1. no list reaches one scan chunk (256 rows), so every full chunk crosses list boundaries; some list has exactly 1 row;
2. four empty lists: M_LIST_FAR (its centroid is 1000 everywhere) and the three M_TWINS, copies of lower-numbered
   centroids, which lose every tie and so probe directly behind their originals;
3. for the planted query (Q_PLANT) the twins sit at the probe positions M_TWIN_AT = 63, 255 and 257: the last lane of
   the first wave, the last entry of the first block of 256, and inside the second block of the prefix kernel;
4. the 41-way tie of x[7] and the far query's empty first list, as in make_case.

`make_width_case(d)` (1049 rows, 8 lists, 5 queries, any d) is what the scan is walked with over the widths of
tests/width_cases.py.  Its purpose is that a kernel summing in another order than numpy's fails, so it asserts that over
the 50 distances of the five queries' 10 nearest rows a left-to-right float32 sum (d >= 8) and an eight-accumulator sum
without the pairwise tree (d >= 129) each differ from O.euclidean_distance in at least one distance's bits; below those
widths the orders are the same arithmetic.  One list is empty (W_TWIN, a copy of W_TWIN_OF) and row 700 is a copy of
row 20 (query 0 is that row).
"""
import functools
import os
import re
from typing import Dict, Tuple

import numpy as np

from oracle import cpu_ref as O
from tests.width_cases import N_INDEX

N, NLIST = 20_011, 64
DIMS = (36, 128, 600)
SCAN_CHUNK = 256                 # kIvfChunk
POOL = 33
Q_ROW7, Q_FAR, Q_ZERO = 0, 1, 2  # where the special queries sit in the pool
LIST_TWIN, LIST_TWIN_OF, LIST_FAR = 9, 3, 11


def plan_constant(name: str) -> int:
    """An integer constant of smqtk_indexing_amd/csrc/sq_ivf_plan.hpp (the cases are cut for the scan's chunk size)."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "smqtk_indexing_amd", "csrc", "sq_ivf_plan.hpp")
    m = re.search(r"\b%s\s*=\s*(\d+)\s*;" % re.escape(name), open(path).read())
    assert m, f"{name} not found in {path}"
    return int(m.group(1))


def assign(centroids: np.ndarray, x: np.ndarray) -> np.ndarray:
    """List of every row: the oracle's nearest centroid, one row at a time."""
    return np.fromiter((O.dense_topk(centroids, row, 1)[1][0] for row in x), dtype=np.int64, count=x.shape[0])


def lists_of(assignment: np.ndarray, nlist: int) -> Tuple[np.ndarray, np.ndarray]:
    """(list_off[nlist + 1], row numbers list by list, ascending inside a list): a stable sort by list."""
    order = np.argsort(assignment, kind="stable").astype(np.int64)
    off = np.searchsorted(assignment[order], np.arange(nlist + 1)).astype(np.int64)
    return off, order


def probe(centroids: np.ndarray, q: np.ndarray, nprobe: int) -> np.ndarray:
    return O.dense_topk(centroids, q, min(int(nprobe), centroids.shape[0]))[1]


def pad(ids: np.ndarray, dist: np.ndarray, k: int, id_base: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """The first k of an answer in the ABI's shape: ids + id_base, -1 / +inf behind the last candidate."""
    oi = np.full(k, -1, dtype=np.int64)
    od = np.full(k, np.inf, dtype=np.float32)
    m = min(k, ids.shape[0])
    oi[:m] = ids[:m] + id_base
    od[:m] = dist[:m]
    return oi, od


def search(x: np.ndarray, centroids: np.ndarray, off: np.ndarray, order: np.ndarray, q: np.ndarray, nprobe: int,
           dist_all: np.ndarray = None) -> Tuple[np.ndarray, np.ndarray]:
    """(ids, float32 distances) of EVERY candidate of q, in (distance, id) order; `dist_all`: the distances of all rows
    from q when the caller has them (each is a function of its row and q alone)."""
    cand = np.concatenate([order[off[l]:off[l + 1]] for l in probe(centroids, q, nprobe)] + [np.zeros(0, np.int64)])
    if cand.shape[0] == 0:
        return cand, np.zeros(0, np.float32)
    dist = O.dense_distances(x[cand], q, "euclidean") if dist_all is None else dist_all[cand]
    o = np.lexsort((cand, dist))
    return cand[o], dist[o]


class Case:
    """What the builders return (rows `x` [n, d], `centroids` [nlist, d], `assignment`, `off`, `order`, the query
    `pool`, and `n`, `nlist`, `d`); arrays are read-only."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self._dist: Dict[int, np.ndarray] = {}
        self._answers: Dict[tuple, Tuple[np.ndarray, np.ndarray]] = {}

    def dist_all(self, qi: int) -> np.ndarray:
        if qi not in self._dist:
            self._dist[qi] = O.dense_distances(self.x, self.pool[qi], "euclidean")
        return self._dist[qi]

    def answer(self, qi: int, nprobe: int) -> Tuple[np.ndarray, np.ndarray]:
        """Every candidate of pool query qi at this nprobe, (distance, id) order; computed once."""
        key = (qi, min(int(nprobe), self.nlist))
        if key not in self._answers:
            self._answers[key] = search(self.x, self.centroids, self.off, self.order, self.pool[qi], key[1], self.dist_all(qi))
        return self._answers[key]

    def expected(self, nq: int, nprobe: int, k: int, id_base: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """(ids [nq, k], dist [nq, k]) of the first nq pool queries, padded as the ABI pads."""
        rows = [pad(*self.answer(qi, nprobe), k, id_base) for qi in range(nq)]
        return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


@functools.lru_cache(maxsize=4)
def make_case(d: int, seed: int = 5) -> Case:
    what = f"ivf case d={d} seed={seed}"
    rng = np.random.default_rng(seed * 1000 + d)
    x = rng.standard_normal((N, d)).astype(np.float32)
    x[100:140] = x[7]
    # 64 distinct data rows, none of them row 7 or one of its copies
    rows = 140 + rng.choice(N - 140, size=NLIST, replace=False)
    centroids = x[rows].copy()
    centroids[LIST_TWIN] = centroids[LIST_TWIN_OF]
    centroids[LIST_FAR] = 1000.0
    a = assign(centroids, x)
    off, order = lists_of(a, NLIST)
    pool = rng.standard_normal((POOL, d)).astype(np.float32)
    near = rng.integers(0, N, size=POOL)
    half = np.arange(POOL) % 2 == 0                                  # every other random query lies next to a row
    pool[half] = x[near[half]] + (rng.standard_normal((int(half.sum()), d)) * 0.05).astype(np.float32)
    pool[Q_ROW7] = x[7]
    pool[Q_FAR] = np.float32(1000.0) + (rng.standard_normal(d) * 0.5).astype(np.float32)
    pool[Q_ZERO] = 0
    for arr in (x, centroids, a, off, order, pool):
        arr.setflags(write=False)
    case = Case(x=x, centroids=centroids, assignment=a, off=off, order=order, pool=pool, d=d, n=N, nlist=NLIST, what=what)
    sizes = np.diff(off)
    assert np.flatnonzero(sizes == 0).tolist() == [LIST_TWIN, LIST_FAR], f"{what}: empty lists {np.flatnonzero(sizes == 0)}"
    assert sizes.max() > 4 * SCAN_CHUNK, f"{what}: longest list {sizes.max()}"
    assert 0 < sizes[sizes > 0].min() < 200, f"{what}: shortest list {sizes[sizes > 0].min()}"
    ids, dist = case.answer(Q_ROW7, 1)
    assert (dist[:41] == 0).all() and ids[:41].tolist() == [7] + list(range(100, 140)) and dist[41] > 0, f"{what}: the tie group"
    assert probe(centroids, pool[Q_FAR], 1)[0] == LIST_FAR, f"{what}: the far query's first list"
    return case


# ------------------------------------------------------------------------------------ many short lists
M_N, M_D, M_NLIST = 6007, 20, 700
M_LIST_FAR = 350
M_TWINS = (697, 698, 699)
M_TWIN_AT = (63, 255, 257)       # the twins' places in the planted query's probe order
Q_PLANT = 3


@functools.lru_cache(maxsize=1)
def make_many_lists_case(seed: int = 5) -> Case:
    what = f"ivf many-lists case seed={seed}"
    rng = np.random.default_rng([seed, M_N, M_NLIST])
    x = rng.standard_normal((M_N, M_D)).astype(np.float32)
    x[100:140] = x[7]
    rows = 140 + rng.choice(M_N - 140, size=M_NLIST, replace=False)   # distinct data rows, none of them row 7 or a copy
    centroids = x[rows].copy()
    pool = rng.standard_normal((POOL, M_D)).astype(np.float32)
    near = rng.integers(0, M_N, size=POOL)
    half = np.arange(POOL) % 2 == 0
    pool[half] = x[near[half]] + (rng.standard_normal((int(half.sum()), M_D)) * 0.05).astype(np.float32)
    pool[Q_ROW7] = x[7]
    pool[Q_FAR] = np.float32(1000.0) + (rng.standard_normal(M_D) * 0.5).astype(np.float32)
    pool[Q_ZERO] = 0
    pool[Q_PLANT] = rng.standard_normal(M_D).astype(np.float32)
    # The twins.  With their slots out of the way the planted query ranks the other centroids; twin t becomes a copy of
    # the centroid that ends up directly in front of M_TWIN_AT[t] once the t twins before it have moved in.
    centroids[[M_LIST_FAR, *M_TWINS]] = 1000.0
    ranked = probe(centroids, pool[Q_PLANT], M_NLIST)
    twin_of = tuple(int(ranked[at - 1 - t]) for t, at in enumerate(M_TWIN_AT))
    for twin, orig in zip(M_TWINS, twin_of):
        centroids[twin] = centroids[orig]
    a = assign(centroids, x)
    off, order = lists_of(a, M_NLIST)
    for arr in (x, centroids, a, off, order, pool):
        arr.setflags(write=False)
    case = Case(x=x, centroids=centroids, assignment=a, off=off, order=order, pool=pool, d=M_D, n=M_N, nlist=M_NLIST,
                twin_of=twin_of, what=what)
    sizes = np.diff(off)
    assert sizes.max() < SCAN_CHUNK, f"{what}: longest list {sizes.max()}"
    assert (sizes == 1).any(), f"{what}: no list of exactly one row"
    assert np.flatnonzero(sizes == 0).tolist() == sorted((M_LIST_FAR,) + M_TWINS), f"{what}: empty lists {np.flatnonzero(sizes == 0)}"
    assert 1 <= M_TWIN_AT[0] < 64 <= M_TWIN_AT[1] < 256 <= M_TWIN_AT[2] < M_NLIST
    ranked = probe(centroids, pool[Q_PLANT], M_NLIST)
    for twin, orig, at in zip(M_TWINS, twin_of, M_TWIN_AT):
        assert orig < twin and ranked[at - 1] == orig and ranked[at] == twin, f"{what}: twin {twin} probes at {np.flatnonzero(ranked == twin)}"
        assert sizes[twin] == 0 and sizes[orig] > 0, f"{what}: twin {twin} of {orig}"
    ids, dist = case.answer(Q_ROW7, 1)
    assert (dist[:41] == 0).all() and ids[:41].tolist() == [7] + list(range(100, 140)) and dist[41] > 0, f"{what}: the tie group"
    assert probe(centroids, pool[Q_FAR], 1)[0] == M_LIST_FAR, f"{what}: the far query's first list"
    return case


# ------------------------------------------------------------------------------------ every row width
W_N, W_NLIST, W_POOL, W_K = N_INDEX, 8, 5, 10
W_TWIN, W_TWIN_OF = 5, 2
W_ROW, W_ROW_COPY = 20, 700
DEVICE_ROW_DIMS = (35, 36)       # rows added from device memory: a padded stride (35 -> 36) and an unaligned base at ld == d
# the batch beyond 65 536 queries: 50 distinct queries tiled over the d = 8 case
BATCH_D, BATCH_NQ, BATCH_DISTINCT, BATCH_NPROBE, BATCH_K, BATCH_BUDGET_MB = 8, 70_000, 50, 2, 3, 1024


def batch_queries(case: "Case") -> np.ndarray:
    """The 50 distinct queries of the large batch: the case's five, then rows plus noise and random ones in turn."""
    rng = np.random.default_rng([7, case.d])
    q = (rng.standard_normal((BATCH_DISTINCT, case.d)) * 3).astype(np.float32)
    q[::2] = case.x[rng.choice(case.n, size=BATCH_DISTINCT // 2, replace=False)] + np.float32(1e-3) * rng.standard_normal(
        (BATCH_DISTINCT // 2, case.d)).astype(np.float32)
    q[:W_POOL] = case.pool
    q.setflags(write=False)
    return q


def l2_left_to_right(rows: np.ndarray, q: np.ndarray) -> np.ndarray:
    """float32 distances with the squares added one after the other (np.cumsum accumulates in sequence)."""
    sq = np.square(rows - q)
    return np.sqrt(np.cumsum(sq, axis=1, dtype=np.float32)[:, -1])


def l2_one_leaf(rows: np.ndarray, q: np.ndarray) -> np.ndarray:
    """float32 distances with numpy's eight accumulators over the WHOLE row -- its leaf, but no pairwise tree above."""
    sq = np.square(rows - q)
    d = sq.shape[1]
    nfull = d - d % 8
    r = np.cumsum(sq[:, :nfull].reshape(sq.shape[0], -1, 8), axis=1, dtype=np.float32)[:, -1, :]
    res = ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))
    for i in range(nfull, d):
        res = res + sq[:, i]
    return np.sqrt(res)


def orders_that_differ(case: Case) -> Tuple[int, int]:
    """Of the 50 distances of the five queries' 10 nearest rows: how many a left-to-right sum, and how many a sum of one
    leaf, gives other bits than O.euclidean_distance."""
    seq = leaf = 0
    for q in case.pool:
        dist, ids = O.dense_topk(case.x, q, W_K)
        bits = dist.view(np.uint32)
        seq += int((l2_left_to_right(case.x[ids], q).view(np.uint32) != bits).sum())
        if case.d >= 8:
            leaf += int((l2_one_leaf(case.x[ids], q).view(np.uint32) != bits).sum())
    return seq, leaf


@functools.lru_cache(maxsize=2)
def make_width_case(d: int) -> Case:
    what = f"ivf width case d={d}"
    rng = np.random.default_rng([6, d])
    x = (rng.standard_normal((W_N, d)) * 3).astype(np.float32)
    x[W_ROW_COPY] = x[W_ROW]
    rows = rng.choice(np.setdiff1d(np.arange(W_N), (W_ROW, W_ROW_COPY)), size=W_NLIST, replace=False)
    centroids = x[rows].copy()
    centroids[W_TWIN] = centroids[W_TWIN_OF]
    pool = (rng.standard_normal((W_POOL, d)) * 3).astype(np.float32)
    for qi in (0, 2, 4):
        pool[qi] = x[(qi * 131 + 7) % W_N] + np.float32(1e-3) * rng.standard_normal(d).astype(np.float32)
    pool[0] = x[W_ROW]
    a = assign(centroids, x)
    off, order = lists_of(a, W_NLIST)
    for arr in (x, centroids, a, off, order, pool):
        arr.setflags(write=False)
    case = Case(x=x, centroids=centroids, assignment=a, off=off, order=order, pool=pool, d=d, n=W_N, nlist=W_NLIST, what=what)
    assert np.flatnonzero(np.diff(off) == 0).tolist() == [W_TWIN], f"{what}: empty lists {np.flatnonzero(np.diff(off) == 0)}"
    seq, leaf = orders_that_differ(case)
    assert seq > 0 or d < 8, f"{what}: a left-to-right sum gives numpy's bits in all 50 distances"
    assert leaf > 0 or d < 129, f"{what}: a sum of one leaf gives numpy's bits in all 50 distances"
    return case
