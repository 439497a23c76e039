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

Further builders, each asserting its own conditions in the same way (their docstrings say which): `make_strided_case`
(12 000 rows: scan workgroups that walk several chunks, with `pq_scan_groups` restated), `make_m_case` (every m, two
adds), `make_dsub_case` (every sub-vector width, m = 3), `make_many_lists_case` (700 lists); `make_case` at LDS_SHAPE is
the scan's 64 KiB of tables.
"""
import functools
from typing import Dict, Tuple

import numpy as np

from oracle import cpu_ref as O
from tests.ivf_cases import assign, lists_of, pad, probe
from tests.width_cases import N_INDEX

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

    def candidates(self, qi: int, nprobe: int) -> np.ndarray:
        """The rows of the probed lists of pool query qi, concatenated in probe order: candidate p of the scan."""
        lists = probe(self.centroids, self.pool[qi], min(int(nprobe), self.nlist))
        return np.concatenate([self.order[self.off[l]:self.off[l + 1]] for l in lists] + [np.zeros(0, np.int64)])

    def answer(self, qi: int, nprobe: int) -> Tuple[np.ndarray, np.ndarray]:
        """Every candidate of pool query qi at this nprobe, (distance, id) order; computed once."""
        key = (qi, min(int(nprobe), self.nlist))
        if key not in self._answers:
            cand = self.candidates(qi, key[1])
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


# ------------------------------------------------------------------------------------ what the further builders share
def _case(what: str, x: np.ndarray, centroids: np.ndarray, codebooks: np.ndarray, pool: np.ndarray, assignment: np.ndarray = None, **extra) -> Case:
    """The restatement's lists and codes of `x` as a read-only Case."""
    nlist, (m, ksub, dsub) = centroids.shape[0], codebooks.shape
    assert x.shape[1] == m * dsub == centroids.shape[1] == pool.shape[1], what
    a = assign(centroids, x) if assignment is None else assignment
    off, order = lists_of(a, nlist)
    codes = encode(codebooks, x)
    for arr in (x, centroids, codebooks, a, off, order, codes, pool):
        arr.setflags(write=False)
    return Case(x=x, centroids=centroids, codebooks=codebooks, assignment=a, off=off, order=order, codes=codes, pool=pool,
                d=x.shape[1], m=m, ksub=ksub, dsub=dsub, n=x.shape[0], nlist=nlist, what=what, **extra)


def lists_after(case: Case, rows: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(list_off, ids list by list, codes list by list) of the index once the first `rows` rows are added."""
    off, order = lists_of(case.assignment[:rows], case.nlist)
    return off, order, case.codes[order]


def answer_of(case: Case, q: np.ndarray, nprobe: int) -> Tuple[np.ndarray, np.ndarray]:
    """Every candidate of ANY query vector, (distance, id) order: the restatement, nothing cached."""
    lists = probe(case.centroids, q, nprobe)
    cand = np.concatenate([case.order[case.off[l]:case.off[l + 1]] for l in lists] + [np.zeros(0, np.int64)])
    dist = coded_distances(tables(case.codebooks, q), case.codes[cand])
    o = np.lexsort((cand, dist))
    return cand[o], dist[o]


def sum_left_to_right(sq: np.ndarray) -> np.ndarray:
    """Rows of float32 added one element after the other (np.cumsum accumulates in sequence)."""
    return np.cumsum(sq, axis=1, dtype=np.float32)[:, -1]


def sum_one_leaf(sq: np.ndarray) -> np.ndarray:
    """Rows added with numpy's eight accumulators over the WHOLE row -- its leaf, but no pairwise tree above."""
    n = sq.shape[1]
    nfull = n - n % 8
    if nfull == 0:
        return sum_left_to_right(sq)
    r = np.cumsum(sq[:, :nfull].reshape(sq.shape[0], -1, 8), axis=1, dtype=np.float32)[:, -1, :]
    res = ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))
    for i in range(nfull, n):
        res = res + sq[:, i]
    return res


def tables_summed(codebooks: np.ndarray, q: np.ndarray, reduce) -> np.ndarray:
    """`tables` with the squares of an entry added by `reduce` instead of numpy's pairwise sum: NOT the contract."""
    m, ksub, dsub = codebooks.shape
    return np.stack([reduce(np.square(codebooks[j] - q[j * dsub:(j + 1) * dsub])) for j in range(m)]).astype(np.float32, copy=False)


def all_distances_that_differ(case: Case, other) -> int:
    """Over ALL rows and every pool query: how many distances `other(case, q)` gives other bits than the contract's."""
    differ = 0
    for qi in range(case.pool.shape[0]):
        differ += int((other(case, case.pool[qi]).view(np.uint32) != case.dist_all(qi).view(np.uint32)).sum())
    return differ


# ------------------------------------------------------------------------------------ the scan's stride loop
SCAN_CHUNK = 256                 # kIvfChunk
CHUNKS_PER_GROUP, GROUPS_PER_CU = 16, 2      # kPqChunksPerGroup, kPqGroupsPerCu of sq_pq_plan.hpp


def pq_scan_groups(chunks: int, nq: int, cus: int) -> int:
    """sq_pq_plan.hpp's pq_scan_groups, restated (tests/test_host_logic_pq.py proves the two equal on the triples used):
    the workgroups that share one query's chunks."""
    if chunks < 1:
        return 1
    want = -(-chunks // CHUNKS_PER_GROUP)
    fill = -(-(GROUPS_PER_CU * cus) // nq) if nq > 0 else 1
    g = max(want, fill)
    return max(g, 1) if g < chunks else chunks


S_N, S_NLIST, S_KSUB, S_POOL, S_K = 12_000, 8, 16, 50, 100
S_SHAPES = ((32, 16), (12, 6))   # (d, m): 16-byte loads with w = 4; dword loads with w = 2 and two padded bytes
S_NPROBES = (8, 3)               # every list: 12 000 candidates each, 47 chunks, the last one partial; three lists: uneven counts
S_NQS = (600, 64)                # 16 chunks per workgroup; two workgroups per CU
S_CUS = 256                      # the device the regimes are cut for (the GPU test asserts them for the device it runs on)
S_SMALL = (5, 6, 7)              # three short lists: their centroids lie S_FAR times as far out as a row
S_Q_SHORT = 0                    # the pool query that probes exactly those three first
S_FAR = {32: 1.15, 12: 1.6}


def strided_queries(case: Case, nq: int):
    """(the pool tiled to nq rows, the pool index of every row)."""
    qis = [i % S_POOL for i in range(nq)]
    return np.ascontiguousarray(case.pool[qis]), qis


def strided_plan(case: Case, nprobe: int, nq: int, cus: int) -> dict:
    """What pq_scan_kernel's grid is for this call: the candidates of every pool query, the chunks of the longest, the
    workgroups per query, and per pool query the workgroups that return at entry (blockIdx.x * 256 >= its candidates)."""
    counts = [int(case.answer(qi, nprobe)[0].shape[0]) for qi in range(S_POOL)]
    chunks = -(-max(counts) // SCAN_CHUNK)
    groups = pq_scan_groups(chunks, nq, cus)
    early = {qi: list(range(-(-c // SCAN_CHUNK), groups)) for qi, c in enumerate(counts) if -(-c // SCAN_CHUNK) < groups}
    return {"counts": counts, "chunks": chunks, "want": -(-chunks // CHUNKS_PER_GROUP), "groups": groups, "early": early}


def assert_regime(plan: dict, nq: int, what: str) -> None:
    """nq = 600: every workgroup walks 16 chunks (the last one fewer); nq = 64: the call is spread, fewer chunks each but
    more than one."""
    if nq == S_NQS[0]:
        assert plan["groups"] == plan["want"] < plan["chunks"], f"{what}: {plan['groups']} workgroups for {plan['chunks']} chunks"
    else:
        assert plan["want"] < plan["groups"] < plan["chunks"], f"{what}: {plan['groups']} workgroups for {plan['chunks']} chunks"


def chunks_without_a_result(case: Case, nprobe: int, k: int) -> list:
    """The chunk indices 0 .. chunks-1 of the batch in which NO pool query has one of its k results, a candidate's place
    being its position in the concatenation of the probed lists in probe order."""
    hit = np.zeros(-(-max(case.answer(qi, nprobe)[0].shape[0] for qi in range(S_POOL)) // SCAN_CHUNK), dtype=bool)
    for qi in range(S_POOL):
        top = case.answer(qi, nprobe)[0][:k]
        hit[np.flatnonzero(np.isin(case.candidates(qi, nprobe), top)) // SCAN_CHUNK] = True
    return np.flatnonzero(~hit).tolist()


@functools.lru_cache(maxsize=2)
def make_strided_case(d: int, m: int, seed: int = 6) -> Case:
    """12 000 rows in 8 lists, ksub = 16, 50 distinct queries: the batch whose scan workgroups walk several chunks each.
    Asserted: (1) at nprobe = 8 every query has 12 000 candidates = 47 chunks with a partial last one, at nprobe = 3 the
    counts differ from query to query; (2) for S_CUS compute units both batch sizes are in their regime at both nprobe;
    (3) every chunk index holds one of some query's k = 100 results, so a chunk that is skipped changes an answer;
    (4) at nprobe = 3 the planted query S_Q_SHORT probes the three short lists: with 64 queries (8 workgroups per query)
    its last workgroups return at entry while the other queries' stride, with 600 queries (3 workgroups) none returns."""
    what = f"pq strided case d={d} m={m} seed={seed}"
    assert d % m == 0
    dsub = d // m
    rng = np.random.default_rng([seed, d, m, S_N])
    x = rng.standard_normal((S_N, d)).astype(np.float32)
    rows = rng.choice(S_N, size=S_NLIST + S_KSUB, replace=False)
    centroids = x[rows[:S_NLIST]].copy()
    centroids[list(S_SMALL)] *= np.float32(S_FAR[d])
    codebooks = np.ascontiguousarray(x[rows[S_NLIST:]].reshape(S_KSUB, m, dsub).transpose(1, 0, 2))
    pool = rng.standard_normal((S_POOL, d)).astype(np.float32)
    near = rng.integers(0, S_N, size=S_POOL)
    half = np.arange(S_POOL) % 2 == 0
    pool[half] = x[near[half]] + (rng.standard_normal((int(half.sum()), d)) * 0.05).astype(np.float32)
    for a in np.arange(0.35, 1.2, 0.05, dtype=np.float32):        # a point between the three far centroids that probes them first
        pool[S_Q_SHORT] = a * centroids[list(S_SMALL)].sum(axis=0)
        if sorted(probe(centroids, pool[S_Q_SHORT], 3).tolist()) == list(S_SMALL):
            break
    case = _case(what, x, centroids, codebooks, pool)
    assert np.unique(pool, axis=0).shape[0] == S_POOL, f"{what}: the queries are not distinct"
    # (1)
    full = strided_plan(case, 8, S_NQS[0], S_CUS)
    assert set(full["counts"]) == {S_N} and full["chunks"] == 47 and S_N % SCAN_CHUNK != 0, f"{what}: every list probed"
    part = strided_plan(case, 3, S_NQS[0], S_CUS)
    assert len(set(part["counts"])) >= 5, f"{what}: candidate counts at nprobe 3: {sorted(set(part['counts']))}"
    for nprobe in S_NPROBES:
        for nq in S_NQS:
            plan = strided_plan(case, nprobe, nq, S_CUS)
            assert_regime(plan, nq, f"{what} nprobe={nprobe} nq={nq}")                     # (2)
            if nprobe == 8 or nq == S_NQS[0]:
                assert not plan["early"], f"{what} nprobe={nprobe} nq={nq}: workgroups return at entry: {plan['early']}"
        missed = chunks_without_a_result(case, nprobe, S_K)                                # (3)
        assert not missed, f"{what} nprobe={nprobe} k={S_K}: no result in chunks {missed}"
    # (4)
    assert sorted(probe(centroids, pool[S_Q_SHORT], 3).tolist()) == list(S_SMALL), f"{what}: the planted query's lists"
    spread = strided_plan(case, 3, S_NQS[1], S_CUS)
    assert min(part["counts"]) == part["counts"][S_Q_SHORT] and S_Q_SHORT in spread["early"], f"{what}: shortest {min(part['counts'])}"
    assert spread["early"][S_Q_SHORT][-1] == spread["groups"] - 1 and len(spread["early"]) < S_POOL // 2, f"{what}: {spread['early']}"
    case.shortest, case.longest = min(part["counts"]), max(part["counts"])
    return case


# ------------------------------------------------------------------------------------ every m
M_N, M_NLIST, M_POOL, M_SPLIT = N_INDEX, 8, 5, 523          # two adds, split at an odd row
M_KSUBS = (13, 16)               # m * ksub % 4 is decorrelated from m % 4
M_NPROBES, M_KS = (1, 3, 8), (10, N_INDEX)
M_TWIN, M_TWIN_OF = 5, 2         # an empty list among those the second add moves
M_EXTRA = ((1, 1), (5, 1), (5, 255))                        # (m, ksub): every code 0; 1275 table floats, staged one by one in five passes
M_DEVICE = (1, 16, 35)           # (m, ksub, dsub): rows from device memory, d = 35, from a base 4 bytes into an allocation


def pairwise_distances_of(case: Case, q: np.ndarray) -> np.ndarray:
    return coded_distances_pairwise(tables(case.codebooks, q), case.codes)


@functools.lru_cache(maxsize=4)
def make_m_case(m: int, ksub: int, dsub: int = 2, seed: int = 5) -> Case:
    """1049 rows in 8 lists (one empty), five queries, d = m * dsub.  Asserted, over the distances of ALL rows from the five
    queries (the tests compare them all at k = 1049): adding the m table entries in numpy's pairwise order changes some
    distance's bits exactly when m >= 8; with ksub = 1 every row of a query ties."""
    what = f"pq m case m={m} ksub={ksub} dsub={dsub} seed={seed}"
    d = m * dsub
    rng = np.random.default_rng([seed, m, ksub, dsub])
    x = rng.standard_normal((M_N, d)).astype(np.float32)
    rows = rng.choice(M_N, size=M_NLIST, replace=False)
    centroids = x[rows].copy()
    centroids[M_TWIN] = centroids[M_TWIN_OF]
    entries = rng.choice(M_N, size=ksub, replace=False)
    codebooks = np.ascontiguousarray(x[entries].reshape(ksub, m, dsub).transpose(1, 0, 2))
    pool = rng.standard_normal((M_POOL, d)).astype(np.float32)
    for qi in (0, 2, 4):
        pool[qi] = x[(qi * 131 + 7) % M_N] + np.float32(1e-2) * rng.standard_normal(d).astype(np.float32)
    case = _case(what, x, centroids, codebooks, pool)
    assert np.flatnonzero(np.diff(case.off) == 0).tolist() == [M_TWIN], f"{what}: empty lists {np.flatnonzero(np.diff(case.off) == 0)}"
    assert int(case.codes.max()) == ksub - 1, f"{what}: the last entry is nobody's code"
    case.differ = all_distances_that_differ(case, pairwise_distances_of)
    assert (case.differ > 0) == (m >= 8), f"{what}: a pairwise sum changes {case.differ} of {M_POOL * M_N} distances"
    if ksub == 1:
        assert not case.codes.any() and all(np.unique(case.dist_all(qi)).shape[0] == 1 for qi in range(M_POOL)), f"{what}: ties"
    return case


# ------------------------------------------------------------------------------------ every sub-vector width
D_M, D_N, D_KSUB, D_NLIST, D_POOL = 3, 300, 37, 4, 5
D_BEYOND = (8193, 8199, 8200, 16384)                        # numpy's 8192-element buffer; the documented limit of pq_tables_kernel


@functools.lru_cache(maxsize=1)
def make_dsub_case(dsub: int) -> Case:
    """m = 3 sub-vectors of `dsub` floats (they start at dsub and 2 dsub: unaligned for odd dsub), 300 rows in 4 lists,
    ksub = 37, five queries.  Asserted over the distances of ALL rows from the five queries (the tests compare them all
    at k = 300): tables summed left to right (dsub >= 8), and tables summed as one leaf of eight accumulators without the
    pairwise tree (dsub >= 129), each change at least one distance's bits."""
    what = f"pq dsub case dsub={dsub}"
    d = D_M * dsub
    rng = np.random.default_rng([8, dsub])
    x = rng.standard_normal((D_N, d), dtype=np.float32) * np.float32(3)
    rows = rng.choice(D_N, size=D_NLIST + D_KSUB, replace=False)
    centroids = x[rows[:D_NLIST]].copy()
    codebooks = np.ascontiguousarray(x[rows[D_NLIST:]].reshape(D_KSUB, D_M, dsub).transpose(1, 0, 2))
    pool = rng.standard_normal((D_POOL, d), dtype=np.float32) * np.float32(3)
    for qi in (0, 2, 4):
        pool[qi] = x[(qi * 31 + 7) % D_N] + np.float32(1e-3) * rng.standard_normal(d, dtype=np.float32)
    case = _case(what, x, centroids, codebooks, pool)
    assert (np.diff(case.off) > 0).all(), f"{what}: an empty list"
    case.seq = all_distances_that_differ(case, lambda c, q: coded_distances(tables_summed(c.codebooks, q, sum_left_to_right), c.codes))
    case.leaf = all_distances_that_differ(case, lambda c, q: coded_distances(tables_summed(c.codebooks, q, sum_one_leaf), c.codes))
    assert case.seq > 0 or dsub < 8, f"{what}: tables summed left to right give numpy's bits in all {D_POOL * D_N} distances"
    assert case.leaf > 0 or dsub < 129, f"{what}: tables summed as one leaf give numpy's bits in all {D_POOL * D_N} distances"
    return case


# ------------------------------------------------------------------------------------ the scan's LDS limit, 700 lists
LDS_SHAPE = (64, 64, 256)        # (d, m, ksub): 64 KiB of tables, what pq_scan_kernel's launch_lds is given as its maximum
ML_M, ML_KSUB = 5, 16            # over the d = 20 rows of ivf_cases.make_many_lists_case(): dsub = 4, stride 8 bytes
ML_ADDS = ((0, 1), (1, 2500), (2500, 6007))
ML_NPROBES, ML_KS = (1, 64, 256, 257, 700), (10, 5000)
ID_BASE = 2 ** 40 + 5


@functools.lru_cache(maxsize=1)
def make_many_lists_case(seed: int = 5) -> Case:
    """The 700 lists of tests/ivf_cases.py (rows, centroids, assignment and query pool with the planted query whose
    empty lists sit at probe positions 63, 255 and 257; that builder asserts those) with the rows coded by 5 codebooks
    of 16 entries."""
    from tests import ivf_cases
    base = ivf_cases.make_many_lists_case()
    assert ML_ADDS[-1][1] == base.n and base.d % ML_M == 0
    rng = np.random.default_rng([seed, ML_M, ML_KSUB])
    entries = rng.choice(base.n, size=ML_KSUB, replace=False)
    codebooks = np.ascontiguousarray(base.x[entries].reshape(ML_KSUB, ML_M, base.d // ML_M).transpose(1, 0, 2))
    case = _case(f"pq many-lists case seed={seed}", base.x, base.centroids, codebooks, base.pool, assignment=base.assignment)
    assert np.array_equal(case.off, base.off) and np.array_equal(case.order, base.order)
    for lo, hi in ML_ADDS[:-1]:      # the later adds move rows and meet empty lists among the old offsets
        assert (np.diff(lists_after(case, hi)[0]) == 0).sum() >= 4
    return case


def huge_query(d: int) -> np.ndarray:
    """1e30 everywhere: every square overflows, every table entry and so every candidate's distance is +inf."""
    return np.full(d, 1e30, dtype=np.float32)
