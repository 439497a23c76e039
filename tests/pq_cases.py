"""
Case builder and numpy restatement for the tests of the IVF-PQ index (`sq_pq_*`): no GPU.

The restatement is the contract of include/smqtk_hip_pq.h over `oracle.cpu_ref`, with dsub = d / m and
x_j = x[j * dsub:(j + 1) * dsub], everything float32:

    list      of a row   = O.dense_topk(centroids, row, 1)            (nearest centroid, ties to the lowest list)
    code[j]   of a row   = O.dense_topk(codebooks[j], row_j, 1)       (nearest entry, ties to the lowest entry)
    tables    of a query : T[j][c] = np.square(codebooks[j][c] - q_j).sum()          (numpy's pairwise order)
    distance  of a row   = sqrt(((T[0][code[0]] + T[1][code[1]]) + ...) + T[m-1][code[m-1]])   (left to right)
    result    the k smallest (distance, id) over the rows of the min(nprobe, nlist) probed lists; -1 / +inf behind

`make_case(d, m, ksub)` builds what the GPU tests run (3001 rows, 8 lists, seeded standard_normal, codebook entries
taken from rows of the set) and ASSERTS what those tests lean on, so a seed that misses a condition fails on the CPU
(tests/test_pq_cases_cpu.py):

1. sum order: over the 10 nearest rows of five queries, adding the m table entries in numpy's pairwise order instead
   of left to right changes at least one distance's bits when m >= 8 (so a scan that sums in another order fails), and
   none when m < 8, where the two orders are the same arithmetic -- (516, 4) is there for dsub = 129, a table entry
   beyond one pairwise leaf;
2. ties: rows 100 .. 139 are copies of row 7, so 41 rows share every code and the query x[7] gets them first, ordered
   by id; entry DUP_HI of codebook DUP_J is a copy of entry DUP_LO < DUP_HI -- some row's nearest entry is that pair, and
   every such row carries DUP_LO;
3. list shapes: two empty lists (LIST_TWIN, a copy of the lower LIST_TWIN_OF, and LIST_FAR, 1000 everywhere), list
   LIST_BIG longer than 1024 rows (its centroid is the origin), and list LIST_SMALL of SMALL_ROWS = 5 rows, shorter than
   k = 10 (a cluster of its own at 50).
"""
import functools
from typing import Dict, Tuple

import numpy as np

from oracle import cpu_ref as O
from tests.ivf_cases import assign, lists_of, pad, probe

N, NLIST, POOL = 3001, 8, 33
SHAPES = ((64, 16), (32, 8), (512, 64), (12, 12), (516, 4))     # (d, m)
KSUB = 64                                                        # of the five shapes above
KSUBS = (2, 3, 256)                                              # further codebook sizes, at KSUB_SHAPE
KSUB_SHAPE = (32, 8)
LIST_BIG, LIST_TWIN_OF, LIST_TWIN, LIST_FAR, LIST_SMALL = 0, 2, 5, 6, 7
SMALL_AT, SMALL_ROWS = 200, 5                                    # rows 200 .. 204 form the small list
Q_ROW7, Q_FAR, Q_ZERO, Q_SMALL = 0, 1, 2, 3                      # where the special queries sit in the pool
ORDER_QUERIES = (4, 5, 6, 7, 8)                                  # the five queries of the sum-order condition
DUP_J, DUP_LO, DUP_HI = 1, 0, 1
SLICE_NQ, SLICE_BUDGET_MB, SLICE_K = 70, 1, 10


def encode(codebooks: np.ndarray, x: np.ndarray) -> np.ndarray:
    """codes uint8 [n, m].  O.dense_topk(codebooks[j], row_j, 1) for every row, evaluated entry by entry: the distance
    of all rows to entry c is O.dense_distances(x_j, entry) -- (a - b)^2 == (b - a)^2 exactly and each row is summed in
    the same pairwise order -- and np.argmin keeps the first, i.e. the lowest, of equal entries."""
    m, ksub, dsub = codebooks.shape
    codes = np.empty((x.shape[0], m), dtype=np.uint8)
    for j in range(m):
        xj = np.ascontiguousarray(x[:, j * dsub:(j + 1) * dsub])
        dist = np.stack([O.dense_distances(xj, codebooks[j][c], "euclidean") for c in range(ksub)])
        codes[:, j] = np.argmin(dist, axis=0)
    return codes


def tables(codebooks: np.ndarray, q: np.ndarray) -> np.ndarray:
    """T float32 [m, ksub]: the square of metrics.euclidean_distance before its root."""
    m, ksub, dsub = codebooks.shape
    return np.stack([np.square(codebooks[j] - q[j * dsub:(j + 1) * dsub]).sum(1) for j in range(m)]).astype(np.float32, copy=False)


def picked(t: np.ndarray, codes: np.ndarray) -> np.ndarray:
    """[rows, m]: the table entry every code byte selects."""
    return np.ascontiguousarray(t[np.arange(t.shape[0])[None, :], codes.astype(np.int64)], dtype=np.float32)


def coded_distances(t: np.ndarray, codes: np.ndarray) -> np.ndarray:
    """float32 [rows]: the m entries added one after the other (np.cumsum accumulates in sequence), then the root."""
    return np.sqrt(np.cumsum(picked(t, codes), axis=1, dtype=np.float32)[:, -1])


def coded_distances_pairwise(t: np.ndarray, codes: np.ndarray) -> np.ndarray:
    """The same entries added in numpy's pairwise order: NOT the contract, the other order of condition 1."""
    return np.sqrt(picked(t, codes).sum(axis=1))


class Case:
    """What make_case returns (rows `x`, `centroids`, `codebooks` [m, ksub, dsub], `assignment`, `off`, `order`, `codes`
    [n, m] in insertion order, the query `pool`, and `n`, `nlist`, `d`, `m`, `ksub`); arrays are read-only."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self._dist: Dict[int, np.ndarray] = {}
        self._answers: Dict[tuple, Tuple[np.ndarray, np.ndarray]] = {}

    def dist_all(self, qi: int) -> np.ndarray:
        if qi not in self._dist:
            self._dist[qi] = coded_distances(tables(self.codebooks, self.pool[qi]), self.codes)
        return self._dist[qi]

    def answer(self, qi: int, nprobe: int) -> Tuple[np.ndarray, np.ndarray]:
        """Every candidate of pool query qi at this nprobe, (distance, id) order; computed once."""
        key = (qi, min(int(nprobe), self.nlist))
        if key not in self._answers:
            lists = probe(self.centroids, self.pool[qi], key[1])
            cand = np.concatenate([self.order[self.off[l]:self.off[l + 1]] for l in lists] + [np.zeros(0, np.int64)])
            dist = self.dist_all(qi)[cand]
            o = np.lexsort((cand, dist))
            self._answers[key] = (cand[o], dist[o])
        return self._answers[key]

    def expected(self, queries, nprobe: int, k: int, id_base: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """(ids [nq, k], dist [nq, k]) of the given pool queries (a count: the first ones), padded as the ABI pads."""
        qs = range(queries) if isinstance(queries, int) else queries
        rows = [pad(*self.answer(qi, nprobe), k, id_base) for qi in qs]
        return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])

    def codes_by_list(self) -> np.ndarray:
        return self.codes[self.order]


def orders_that_differ(case: Case) -> int:
    """Of the 50 distances of five queries' 10 nearest rows (every list probed): how many a pairwise sum of the table
    entries gives other bits than the contract's left-to-right sum."""
    differ = 0
    for qi in ORDER_QUERIES:
        ids, dist = case.answer(qi, case.nlist)
        other = coded_distances_pairwise(tables(case.codebooks, case.pool[qi]), case.codes[ids[:10]])
        differ += int((other.view(np.uint32) != dist[:10].view(np.uint32)).sum())
    return differ


@functools.lru_cache(maxsize=8)
def make_case(d: int, m: int, ksub: int = KSUB, seed: int = 5) -> Case:
    what = f"pq case d={d} m={m} ksub={ksub} seed={seed}"
    assert d % m == 0
    dsub = d // m
    rng = np.random.default_rng([seed, d, m, ksub])
    x = rng.standard_normal((N, d)).astype(np.float32)
    x[100:140] = x[7]
    x[SMALL_AT:SMALL_AT + SMALL_ROWS] = np.float32(50.0) + (rng.standard_normal((SMALL_ROWS, d)) * 0.5).astype(np.float32)
    free = np.arange(SMALL_AT + SMALL_ROWS, N)                     # rows that are neither row 7, a copy of it nor the small cluster
    centroids = x[rng.choice(free, size=NLIST, replace=False)].copy()
    centroids[LIST_BIG] = 0.0
    centroids[LIST_TWIN] = centroids[LIST_TWIN_OF]
    centroids[LIST_FAR] = 1000.0
    centroids[LIST_SMALL] = 50.0
    entries = rng.choice(free, size=ksub, replace=False)
    codebooks = np.ascontiguousarray(x[entries].reshape(ksub, m, dsub).transpose(1, 0, 2))
    if ksub > DUP_HI and m > DUP_J:
        codebooks[DUP_J, DUP_HI] = codebooks[DUP_J, DUP_LO]
    a = assign(centroids, x)
    off, order = lists_of(a, NLIST)
    codes = encode(codebooks, x)
    pool = rng.standard_normal((POOL, d)).astype(np.float32)
    near = rng.integers(0, N, size=POOL)
    half = np.arange(POOL) % 2 == 0                                  # every other random query lies next to a row
    pool[half] = x[near[half]] + (rng.standard_normal((int(half.sum()), d)) * 0.05).astype(np.float32)
    pool[Q_ROW7] = x[7]
    pool[Q_FAR] = np.float32(1000.0) + (rng.standard_normal(d) * 0.5).astype(np.float32)
    pool[Q_ZERO] = 0
    pool[Q_SMALL] = np.float32(50.0) + (rng.standard_normal(d) * 0.5).astype(np.float32)
    for arr in (x, centroids, codebooks, a, off, order, codes, pool):
        arr.setflags(write=False)
    case = Case(x=x, centroids=centroids, codebooks=codebooks, assignment=a, off=off, order=order, codes=codes, pool=pool,
                d=d, m=m, ksub=ksub, dsub=dsub, n=N, nlist=NLIST, what=what)
    # the entry-by-entry evaluation of `encode` is the literal rule
    for r in (0, 7, 100, SMALL_AT, 1500, N - 1):
        literal = [O.dense_topk(codebooks[j], x[r, j * dsub:(j + 1) * dsub], 1)[1][0] for j in range(m)]
        assert codes[r].tolist() == literal, f"{what}: codes of row {r}"
    # 3. list shapes
    sizes = np.diff(off)
    assert np.flatnonzero(sizes == 0).tolist() == [LIST_TWIN, LIST_FAR], f"{what}: empty lists {np.flatnonzero(sizes == 0)}"
    assert sizes[LIST_BIG] > 1024, f"{what}: longest list {sizes.max()}"
    assert order[off[LIST_SMALL]:off[LIST_SMALL + 1]].tolist() == list(range(SMALL_AT, SMALL_AT + SMALL_ROWS)), f"{what}: the small list"
    assert probe(centroids, pool[Q_FAR], 1)[0] == LIST_FAR and probe(centroids, pool[Q_SMALL], 1)[0] == LIST_SMALL, f"{what}: first lists"
    assert probe(centroids, pool[Q_ZERO], 1)[0] == LIST_BIG, f"{what}: the zero query's first list"
    # 2. ties
    assert (codes[100:140] == codes[7]).all()
    ids, dist = case.answer(Q_ROW7, 1)
    mine = order[off[a[7]]:off[a[7] + 1]]
    same = mine[(codes[mine] == codes[7]).all(axis=1)]               # row 7's codes are the nearest entries of the query x[7]
    assert ids[:same.shape[0]].tolist() == same.tolist() and (dist[:same.shape[0]] == dist[0]).all(), f"{what}: the tie group"
    assert set([7] + list(range(100, 140))) <= set(same.tolist()), f"{what}: the tie group's rows"
    if ksub >= KSUB:   # (smaller codebooks: other rows share the codes too)
        assert same.tolist() == [7] + list(range(100, 140)) and dist[41] > dist[40], f"{what}: {same.shape[0]} rows share row 7's codes"
    if ksub > DUP_HI and m > DUP_J:
        assert (codes[:, DUP_J] == DUP_LO).any() and not (codes[:, DUP_J] == DUP_HI).any(), f"{what}: the duplicated entry"
    # 1. sum order
    differ = orders_that_differ(case)
    assert (differ > 0) == (m >= 8), f"{what}: a pairwise sum changes {differ} of 50 distances"
    case.differ = differ
    return case
