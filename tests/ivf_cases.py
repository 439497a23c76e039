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
"""
import functools
import os
import re
from typing import Dict, Tuple

import numpy as np

from oracle import cpu_ref as O

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
    """What make_case returns; arrays are read-only."""

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
        key = (qi, min(int(nprobe), NLIST))
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
    case = Case(x=x, centroids=centroids, assignment=a, off=off, order=order, pool=pool, d=d, what=what)
    sizes = np.diff(off)
    assert np.flatnonzero(sizes == 0).tolist() == [LIST_TWIN, LIST_FAR], f"{what}: empty lists {np.flatnonzero(sizes == 0)}"
    assert sizes.max() > 4 * SCAN_CHUNK, f"{what}: longest list {sizes.max()}"
    assert 0 < sizes[sizes > 0].min() < 200, f"{what}: shortest list {sizes[sizes > 0].min()}"
    ids, dist = case.answer(Q_ROW7, 1)
    assert (dist[:41] == 0).all() and ids[:41].tolist() == [7] + list(range(100, 140)) and dist[41] > 0, f"{what}: the tie group"
    assert probe(centroids, pool[Q_FAR], 1)[0] == LIST_FAR, f"{what}: the far query's first list"
    return case
