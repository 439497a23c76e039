"""
Case builders and numpy restatement for the tests of the IVF-PQ index in residual mode (`sq_pq_create_residual`,
`sq_pq_residuals`): no GPU.

The restatement is the residual contract of include/smqtk_hip_pq.h, written over tests/pq_cases.py (`encode`, `tables`,
`coded_distances`) and tests/ivf_cases.py (`assign`, `lists_of`, `probe`, `pad`), everything float32:

    list      l(x)       = assign(centroids, x)                              (unchanged)
    residual  r          = x - centroids[l(x)]
    code      of a row   = encode(codebooks, r)
    tables    of (q, l)  : T_l = tables(codebooks, q - centroids[l])         (one set per query and probed list)
    distance  of a row of list l = coded_distances(T_l, code)                (left to right, then the root)
    result    the k smallest (distance, id) over the rows of the probed lists; -1 / +inf behind

Every builder ASSERTS what the GPU tests lean on, so a seed that misses a condition fails on the CPU
(tests/test_pq_residual_cases_cpu.py).  `make_case(d, m, ksub)` takes rows, centroids, lists and query pool of
`pq_cases.make_case` (3001 rows, 8 lists: LIST_BIG with the zero centroid, a twin list, a far empty list, a 5-row list,
40 copies of row 7) with codebook entries taken from residuals of rows, and asserts (a) .. (e) of its docstring.
`make_strided_case` is the scan's stride loop, `make_recall_case` the small clustered set on which residual codes beat
plain codes, `from_plain` recodes any case of pq_cases.py (every m, every sub-vector width).  `res_plan` restates the
plan of sq_pq_plan.hpp (slice, pairs per launch, launches).
"""
import functools
from typing import Dict, Tuple

import numpy as np

from tests import pq_cases as C
from tests.ivf_cases import assign, lists_of, pad, probe

SHAPES = ((64, 16), (32, 8), (12, 12), (516, 4))          # (d, m), ksub = C.KSUB
CHECK_QUERIES = (C.Q_SMALL, 4, 5, 6, 7)                   # the five queries whose 10 nearest rows conditions (c) and (d) compare
ID_BASE = 2 ** 40 + 5


def residuals(centroids: np.ndarray, x: np.ndarray, a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(x - centroids[a], dtype=np.float32)


def tables_of(codebooks: np.ndarray, centroids: np.ndarray, q: np.ndarray, l: int) -> np.ndarray:
    """T_l of the contract: rq = q - centroids[l] first, then the plain tables against rq."""
    return C.tables(codebooks, q - centroids[l])


def tables_regrouped(codebooks: np.ndarray, centroids: np.ndarray, q: np.ndarray, l: int) -> np.ndarray:
    """NOT the contract: the centroid added to the entry, np.square((codebooks[j] + c_j) - q_j) -- condition (c)."""
    m, ksub, dsub = codebooks.shape
    c = centroids[l]
    return np.stack([np.square((codebooks[j] + c[j * dsub:(j + 1) * dsub]) - q[j * dsub:(j + 1) * dsub]).sum(1)
                     for j in range(m)]).astype(np.float32, copy=False)


class ResCase:
    """Rows `x`, `centroids`, `codebooks`, `assignment`, `off`, `order`, residual `codes` [n, m] in insertion order, the
    query `pool`, and `n`, `nlist`, `d`, `m`, `ksub`, `dsub`; arrays are read-only.  Answers are computed once."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self._answers: Dict[tuple, Tuple[np.ndarray, np.ndarray]] = {}

    def rows_of(self, l: int) -> np.ndarray:
        return self.order[self.off[l]:self.off[l + 1]]

    def candidates_of(self, q: np.ndarray, nprobe: int, tables_fn=tables_of, all_from_first: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """(rows, distances) of the probed lists' rows in probe order: candidate p of the select.  `tables_fn` and
        `all_from_first` (the first probed list's tables for every list) are the wrong ways of conditions (b), (c)."""
        lists = probe(self.centroids, q, min(int(nprobe), self.nlist))
        rows, dist = [np.zeros(0, np.int64)], [np.zeros(0, np.float32)]
        for l in lists:
            r = self.rows_of(l)
            if r.shape[0]:
                t = tables_fn(self.codebooks, self.centroids, q, lists[0] if all_from_first else l)
                rows.append(r)
                dist.append(self.reduce(t, self.codes[r]))
        return np.concatenate(rows), np.concatenate(dist)

    reduce = staticmethod(C.coded_distances)

    def answer_of(self, q: np.ndarray, nprobe: int, **kw) -> Tuple[np.ndarray, np.ndarray]:
        cand, dist = self.candidates_of(q, nprobe, **kw)
        o = np.lexsort((cand, dist))
        return cand[o], dist[o]

    def answer(self, qi: int, nprobe: int) -> Tuple[np.ndarray, np.ndarray]:
        key = (qi, min(int(nprobe), self.nlist))
        if key not in self._answers:
            self._answers[key] = self.answer_of(self.pool[qi], key[1])
        return self._answers[key]

    def expected(self, queries, nprobe: int, k: int, id_base: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """(ids [nq, k], dist [nq, k]) of the given pool queries (a count: the first ones), padded as the ABI pads."""
        qs = range(queries) if isinstance(queries, int) else queries
        rows = [pad(*self.answer(qi, nprobe), k, id_base) for qi in qs]
        return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])

    def count(self, qi: int, nprobe: int) -> int:
        return int(self.answer(qi, nprobe)[0].shape[0])

    def codes_by_list(self) -> np.ndarray:
        return self.codes[self.order]

    def lists_after(self, rows: int):
        off, order = lists_of(self.assignment[:rows], self.nlist)
        return off, order, self.codes[order]


def _res_case(what, x, centroids, codebooks, pool, a, **extra) -> ResCase:
    nlist, (m, ksub, dsub) = centroids.shape[0], codebooks.shape
    assert x.shape[1] == m * dsub == centroids.shape[1] == pool.shape[1], what
    off, order = lists_of(a, nlist)
    res = residuals(centroids, x, a)
    codes = C.encode(codebooks, res)
    for arr in (codebooks, codes, res):
        arr.setflags(write=False)
    return ResCase(x=x, centroids=centroids, codebooks=codebooks, assignment=a, off=off, order=order, codes=codes, res=res, pool=pool,
                   d=x.shape[1], m=m, ksub=ksub, dsub=dsub, n=x.shape[0], nlist=nlist, what=what, **extra)


def from_plain(plain: C.Case, codebooks: np.ndarray = None) -> ResCase:
    """A case of tests/pq_cases.py coded again as residuals (its rows, centroids, lists and pool; its codebooks unless
    others are given).  Asserted: some row's residual code differs from its plain code."""
    case = _res_case("residual " + plain.what, plain.x, plain.centroids, plain.codebooks if codebooks is None else codebooks,
                     plain.pool, plain.assignment)
    if codebooks is None and plain.ksub > 1:
        assert (case.codes != plain.codes).any(), f"{case.what}: the residual codes are the plain codes"
    return case


def distances_that_differ(case: ResCase, queries, **wrong) -> int:
    """Of the 10 nearest rows of each of `queries` (every list probed): how many distances the wrong way changes."""
    differ = 0
    for qi in queries:
        ids, dist = case.answer(qi, case.nlist)
        cand, other = case.candidates_of(case.pool[qi], case.nlist, **wrong)
        at = {int(r): i for i, r in enumerate(cand)}
        got = other[[at[int(r)] for r in ids[:10]]]
        differ += int((got.view(np.uint32) != dist[:10].view(np.uint32)).sum())
    return differ


@functools.lru_cache(maxsize=8)
def make_case(d: int, m: int, ksub: int = C.KSUB, seed: int = 5) -> ResCase:
    """pq_cases.make_case's rows, centroids, lists and pool; codebook entry c of sub-quantiser j is sub-vector j of the
    residual of a row drawn outside the planted rows.  Asserted:
    (a) in every non-empty list but LIST_BIG some row's code differs from the plain code encode(codebooks, x); in LIST_BIG
        (zero centroid: the residual is the row) every code equals it;
    (b) for some pool query at some nprobe >= 2, the first probed list's tables used for every list change its 10 nearest
        ids (`case.wrong_pair` = (query, nprobe)): a kernel staging the wrong pair's tables fails;
    (c) tables computed as np.square((codebooks[j] + c_j) - q_j) change at least one of the 50 distances of the
        CHECK_QUERIES' 10 nearest rows: a kernel regrouping the subtraction fails;
    (d) the entries added in numpy's pairwise order change one of those 50 distances exactly when m >= 8;
    (e) x[7] at nprobe 1: the 41 rows 7, 100 .. 139 come first, equal distances, ordered by id."""
    args = (d, m) + ((ksub,) if (ksub, seed) != (C.KSUB, 5) else ()) + ((seed,) if seed != 5 else ())
    plain = C.make_case(*args)                           # (spelled as the plain tests spell it: one cached build for both)
    what = f"residual pq case d={d} m={m} ksub={ksub} seed={seed}"
    rng = np.random.default_rng([seed, d, m, ksub, 1])
    free = np.arange(C.SMALL_AT + C.SMALL_ROWS, C.N)
    entries = rng.choice(free, size=ksub, replace=False)
    res = residuals(plain.centroids, plain.x, plain.assignment)
    codebooks = np.ascontiguousarray(res[entries].reshape(ksub, m, d // m).transpose(1, 0, 2))
    case = from_plain(plain, codebooks)
    case.what = what
    sizes = np.diff(case.off)
    assert np.flatnonzero(sizes == 0).tolist() == [C.LIST_TWIN, C.LIST_FAR] and sizes[C.LIST_BIG] > 1024 and sizes[C.LIST_SMALL] == 5, what
    assert not case.centroids[C.LIST_BIG].any(), what
    # (a)
    plain_codes = C.encode(codebooks, case.x)
    for l in range(case.nlist):
        rows = case.rows_of(l)
        if l == C.LIST_BIG:
            assert np.array_equal(case.codes[rows], plain_codes[rows]), f"{what}: codes of LIST_BIG"
        elif rows.shape[0]:
            assert (case.codes[rows] != plain_codes[rows]).any(), f"{what}: list {l}'s residual codes are its plain codes"
    # (b)
    case.wrong_pair = None
    for nprobe in (2, 3, case.nlist):
        for qi in range(C.POOL):
            ids, _ = case.answer(qi, nprobe)
            wrong, _ = case.answer_of(case.pool[qi], nprobe, all_from_first=True)
            if ids.shape[0] >= 10 and ids[:10].tolist() != wrong[:10].tolist():
                case.wrong_pair = (qi, nprobe)
                break
        if case.wrong_pair:
            break
    assert case.wrong_pair is not None, f"{what}: the first list's tables for every list change no query's 10 nearest"
    # (c)
    case.regrouped = distances_that_differ(case, CHECK_QUERIES, tables_fn=tables_regrouped)
    assert case.regrouped > 0, f"{what}: the regrouped subtraction changes none of 50 distances"
    # (d)
    case.differ = 0
    for qi in CHECK_QUERIES:
        ids, dist = case.answer(qi, case.nlist)
        pw = ResCase(**{**case.__dict__, "_answers": {}})
        pw.reduce = C.coded_distances_pairwise
        cand, other = pw.candidates_of(case.pool[qi], case.nlist)
        at = {int(r): i for i, r in enumerate(cand)}
        got = other[[at[int(r)] for r in ids[:10]]]
        case.differ += int((got.view(np.uint32) != dist[:10].view(np.uint32)).sum())
    assert (case.differ > 0) == (m >= 8), f"{what}: a pairwise sum changes {case.differ} of 50 distances"
    # (e)
    ids, dist = case.answer(C.Q_ROW7, 1)
    if ksub >= C.KSUB:
        assert ids[:41].tolist() == [7] + list(range(100, 140)) and (dist[:41] == dist[0]).all() and dist[41] > dist[40], f"{what}: the tie group"
    return case


def huge_query(d: int) -> np.ndarray:
    return C.huge_query(d)


# ------------------------------------------------------------------------------------ the plan, restated
TABLE_BYTES = lambda m, ksub: m * ksub * 4
MAX_PAIRS = 65535                # kPqMaxPairsPerLaunch: the scan grid's second dimension
SELECT_LDS_KEYS, SORT_CHUNK = 16384, 4096
DEFAULT_BUDGET = 256 << 20


def query_scratch_bytes(maxc: int, k: int) -> int:
    """ivf_query_scratch_bytes of sq_ivf_plan.hpp."""
    mc = max(maxc, 1)
    ks = k if k < maxc else mc
    b = (mc + ks) * 8
    if ks > SELECT_LDS_KEYS:
        span = SORT_CHUNK
        while span < mc:
            span <<= 1
        b += 2 * span * 8
    return b


def res_plan(nq: int, np_: int, maxc: int, k: int, m: int, ksub: int, budget: int = DEFAULT_BUDGET) -> Tuple[int, int, int]:
    """(queries per slice, pairs per launch, launches) of a residual search: pq_slice_queries, pq_res_pairs_per_launch
    (before the cap at the slice's pairs) and pq_res_launches of sq_pq_plan.hpp."""
    per, tb = query_scratch_bytes(maxc, k), TABLE_BYTES(m, ksub)
    slice_ = min(max(budget // (per + tb), 1), nq)
    ppl = min(max((budget - slice_ * per) // tb, 1), MAX_PAIRS)
    if maxc < 1 or nq < 1 or np_ < 1:
        return slice_, ppl, 0
    eff = min(ppl, slice_ * np_)
    full, rest = divmod(nq, slice_)                      # whole slices, and the queries of a last shorter one
    launches = full * -(-(slice_ * np_) // eff) + -(-(rest * np_) // eff)
    return slice_, ppl, launches


RANGE_Q0, RANGE_OTHER = 11, 20        # at LDS_SHAPE: the pool queries of the pair-range test, and the ones run before them


def range_starts(ns: int, np_: int, ppl: int):
    """(query, position) at which every range of a slice of ns queries begins."""
    return [divmod(p0, np_) for p0 in range(0, ns * np_, min(ppl, ns * np_))]


# ------------------------------------------------------------------------------------ the scan's stride loop
S_N, S_NLIST, S_KSUB, S_POOL, S_K, S_NPROBE = 12_000, 4, 16, 50, 100, 3
S_SHAPES = ((32, 16), (12, 6))   # (d, m): 16-byte loads with w = 4; dword loads with w = 2 and two padded bytes
S_NQS = (600, 64)
S_CUS = 256
S_LONG, S_SMALL, S_EMPTY, S_MID = 0, 1, 2, 3
S_LONG_ROWS, S_SMALL_ROWS = 8100, 5          # 32 chunks, the last one of 164 rows
S_Q_SMALL, S_Q_EMPTY = 0, 1                  # pool queries at the 5-row list and at the empty list


def strided_plan(case: ResCase, nq: int, cus: int) -> dict:
    """pq_scan_res_kernel's grid for nq queries at S_NPROBE: chunks of the longest list, pairs, workgroups per pair."""
    chunks = -(-int(np.diff(case.off).max()) // C.SCAN_CHUNK)
    pairs = nq * S_NPROBE
    maxc = max(case.count(qi, S_NPROBE) for qi in range(S_POOL))
    slice_, ppl, launches = res_plan(nq, S_NPROBE, maxc, S_K, case.m, case.ksub)
    return {"chunks": chunks, "pairs": pairs, "want": -(-chunks // C.CHUNKS_PER_GROUP), "groups": C.pq_scan_groups(chunks, pairs, cus),
            "slice": slice_, "ppl": ppl, "launches": launches}


def assert_regime(plan: dict, nq: int, what: str) -> None:
    """One launch holds every pair.  600 queries: groups = ceil(chunks / 16), every workgroup of the long list walks 16
    chunks; 64 queries: the call is spread over two workgroups per CU, fewer chunks each but more than one."""
    assert plan["slice"] == nq and plan["launches"] == 1 and plan["ppl"] >= plan["pairs"], f"{what}: {plan}"
    if nq == S_NQS[0]:
        assert plan["groups"] == plan["want"] < plan["chunks"], f"{what}: {plan}"
    else:
        assert plan["want"] < plan["groups"] < plan["chunks"], f"{what}: {plan}"


def strided_queries(case: ResCase, nq: int):
    qis = [i % S_POOL for i in range(nq)]
    return np.ascontiguousarray(case.pool[qis]), qis


@functools.lru_cache(maxsize=2)
def make_strided_case(d: int, m: int, seed: int = 6) -> ResCase:
    """12 000 rows in 4 lists: S_LONG (zero centroid, 8100 rows = 32 chunks), S_SMALL (5 rows at 50), S_EMPTY (its
    centroid at 1000) and S_MID (the rest, around -20), ksub = 16, 50 distinct queries, three lists probed.  Asserted:
    the list sizes; for S_CUS compute units both batch sizes are in their regime; every chunk of the long list holds one
    of some query's k = 100 results; the planted queries probe the 5-row list and the empty list first."""
    what = f"residual strided case d={d} m={m} seed={seed}"
    dsub = d // m
    rng = np.random.default_rng([seed, d, m, S_N, 1])
    x = rng.standard_normal((S_N, d)).astype(np.float32)
    x[S_LONG_ROWS:] -= np.float32(20.0)
    small = rng.choice(np.arange(S_LONG_ROWS, S_N), size=S_SMALL_ROWS, replace=False)     # from the middle list: the long list keeps its rows
    x[small] = np.float32(50.0) + (rng.standard_normal((S_SMALL_ROWS, d)) * 0.5).astype(np.float32)
    centroids = np.zeros((S_NLIST, d), np.float32)
    centroids[S_SMALL], centroids[S_EMPTY], centroids[S_MID] = 50.0, 1000.0, -20.0
    a = assign(centroids, x)
    res = residuals(centroids, x, a)
    codebooks = np.ascontiguousarray(res[rng.choice(S_N, size=S_KSUB, replace=False)].reshape(S_KSUB, m, dsub).transpose(1, 0, 2))
    pool = rng.standard_normal((S_POOL, d)).astype(np.float32)
    near = rng.integers(0, S_N, size=S_POOL)
    half = np.arange(S_POOL) % 2 == 0
    pool[half] = x[near[half]] + (rng.standard_normal((int(half.sum()), d)) * 0.05).astype(np.float32)
    pool[S_Q_SMALL] = np.float32(50.0) + (rng.standard_normal(d) * 0.5).astype(np.float32)
    pool[S_Q_EMPTY] = np.float32(1000.0) + (rng.standard_normal(d) * 0.5).astype(np.float32)
    for arr in (x, centroids, a, pool):
        arr.setflags(write=False)
    case = _res_case(what, x, centroids, codebooks, pool, a)
    sizes = np.diff(case.off)
    assert sizes[S_LONG] == S_LONG_ROWS >= 8000 and sizes[S_EMPTY] == 0 and sizes[S_SMALL] == S_SMALL_ROWS, f"{what}: lists {sizes}"
    assert np.unique(pool, axis=0).shape[0] == S_POOL, f"{what}: the queries are not distinct"
    assert probe(centroids, pool[S_Q_SMALL], 3)[0] == S_SMALL and probe(centroids, pool[S_Q_EMPTY], 3)[0] == S_EMPTY, f"{what}: planted queries"
    for nq in S_NQS:
        assert_regime(strided_plan(case, nq, S_CUS), nq, f"{what} nq={nq}")
    assert strided_plan(case, S_NQS[0], S_CUS)["chunks"] >= 32
    # every chunk of the long list holds one of some query's results (a row's chunk: its place in the list // 256)
    place = np.full(S_N, -1, np.int64)
    place[case.rows_of(S_LONG)] = np.arange(S_LONG_ROWS)
    hit = np.zeros(-(-S_LONG_ROWS // C.SCAN_CHUNK), dtype=bool)
    for qi in range(S_POOL):
        top = case.answer(qi, S_NPROBE)[0][:S_K]
        p = place[top]
        hit[p[p >= 0] // C.SCAN_CHUNK] = True
    assert hit.all(), f"{what}: no result in chunks {np.flatnonzero(~hit).tolist()} of the long list"
    return case


# ------------------------------------------------------------------------------------ recall: residual against plain codes
R_N, R_D, R_M, R_KSUB, R_NLIST, R_NQ, R_ITERS, R_SEED = 3000, 32, 8, 16, 8, 32, 8, 3


def kmeans(x: np.ndarray, c0: np.ndarray, iters: int) -> np.ndarray:
    """Plain Lloyd iterations in numpy (an empty cluster keeps its centre): trains the recall case's centroids and
    codebooks.  The lists and codes of the case come from `assign` / `encode`, not from here."""
    c = np.array(c0, dtype=np.float32)
    for _ in range(iters):
        a = ((x[:, None, :] - c[None]) ** 2).sum(2).argmin(1)
        for l in range(c.shape[0]):
            if (a == l).any():
                c[l] = x[a == l].mean(0)
    return c


def train_books(x: np.ndarray, m: int, ksub: int, entries: np.ndarray, iters: int) -> np.ndarray:
    dsub = x.shape[1] // m
    return np.stack([kmeans(np.ascontiguousarray(x[:, j * dsub:(j + 1) * dsub]), x[entries, j * dsub:(j + 1) * dsub], iters) for j in range(m)])


def recall_at(found: np.ndarray, exact: np.ndarray) -> float:
    return float(np.mean([len(set(f.tolist()) & set(e.tolist())) / e.shape[0] for f, e in zip(found, exact)]))


@functools.lru_cache(maxsize=1)
def make_recall_case(seed: int = R_SEED):
    """3000 rows, d = 32, 8 clusters of sigma 0.25 around centres of scale 2, m = 8, ksub = 16, 32 queries next to rows,
    every list probed; centroids and both sets of codebooks trained by `kmeans`.  Returns (residual case, plain case,
    recall@10 of the residual codes, of the plain codes) and asserts the first recall at least 1.5 times the second."""
    from oracle import cpu_ref as O
    what = f"recall case seed={seed}"
    rng = np.random.default_rng([seed, R_N])
    centres = (rng.standard_normal((R_NLIST, R_D)) * 2).astype(np.float32)
    x = (centres[rng.integers(0, R_NLIST, R_N)] + rng.standard_normal((R_N, R_D)) * 0.25).astype(np.float32)
    pool = (x[rng.choice(R_N, R_NQ, replace=False)] + rng.standard_normal((R_NQ, R_D)) * 0.05).astype(np.float32)
    centroids = kmeans(x, x[rng.choice(R_N, R_NLIST, replace=False)], R_ITERS)
    entries = rng.choice(R_N, R_KSUB, replace=False)
    a = assign(centroids, x)
    res = residuals(centroids, x, a)
    books_res = train_books(res, R_M, R_KSUB, entries, R_ITERS)
    books_plain = train_books(x, R_M, R_KSUB, entries, R_ITERS)
    for arr in (x, centroids, a, pool, books_plain):
        arr.setflags(write=False)
    case = _res_case(what, x, centroids, books_res, pool, a)
    plain = C._case(what + " (plain codes)", x, centroids, books_plain, pool, assignment=a)
    exact = np.stack([O.dense_topk(x, q, 10)[1] for q in pool])
    got_res = np.stack([case.answer(qi, R_NLIST)[0][:10] for qi in range(R_NQ)])
    got_plain = np.stack([plain.answer(qi, R_NLIST)[0][:10] for qi in range(R_NQ)])
    r_res, r_plain = recall_at(got_res, exact), recall_at(got_plain, exact)
    assert r_plain > 0 and r_res >= 1.5 * r_plain, f"{what}: recall@10 residual {r_res:.3f} against plain {r_plain:.3f}"
    return case, plain, r_res, r_plain
