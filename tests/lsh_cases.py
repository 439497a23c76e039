"""
Case builder for the tests of the one-call LSH query (`sq_lsh_query`): pure numpy, no GPU.

`make_case(dtype, d, bits, normalize, seed)` builds a clustered descriptor matrix, an ITQ-shaped model, the bucket map
the way `HipLSHNearestNeighborIndex` builds it (codes from the ORACLE's hash, so the device never grades itself) and a
pool of 70 queries; `Case.oracle` answers a (query, m, metric) once and caches it.  The builder ASSERTS the conditions
the GPU tests lean on (module docstring of tests/test_hip_lsh_composite.py):

1. margin   every bit of every pool query has |z| > 1e-9 |x - mean| |R_j|: float64 rounding of the dot product is
            below d * 2^-53 ~ 1e-12 of that product at d = 8192, so numpy's summation order and the device's cannot
            disagree about a bit;
2. buckets  at least a quarter of the buckets hold two or more rows, the largest five or more, and there are at least
            6000 unique codes (a Hamming handle with candidate_cap = 2048 is then off the all-keys chain);
3. ties     the oracle's answer for the planted query `c` has two adjacent bit-equal distances whose row ids DESCEND:
            equal distances are ordered by candidate position (code order, then row order in the bucket), not by id.

No query is dropped to make a condition hold: a seed that misses one fails here, on the CPU.
"""
import functools
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from oracle import cpu_ref as O

POOL = 70
# where the special queries sit in the pool (call sizes take the first nq rows, so every call of 4 or more has them)
Q_ROW7, Q_CENTRE, Q_PAIR, Q_ZERO = 0, 1, 2, 3
MIN_CODES = 6000
# 6400 centres, 65 % of them alone in their bucket: ~13 000 rows, ~6400 codes.  (Codes follow centres -- a copy with
# noise of 2^-12 rarely flips a bit -- so the 6000 unique codes of condition 2 need that many centres.)
N_CENTRES = 6400


def lsh_nn_fast(q_vec: np.ndarray, n: int, mean_vec: np.ndarray, rotation: np.ndarray, normalize,
                uniq_codes: np.ndarray, code_rows: Sequence[Sequence[int]], db: np.ndarray, metric: str,
                k: Optional[int] = None, q_code: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
    """`oracle.cpu_ref.lsh_nn` with the candidates' distances from one `O.dense_distances` call in place of the
    per-row Python loop: hash -> n nearest codes in (distance, code id) order -> buckets concatenated in that order ->
    distances -> stable sort -> the first `k` (default n, as lsh_nn).  `q_code`: the query's packed code when the
    caller already has it (the oracle's, of the same arguments)."""
    if q_code is None:
        q_code = O.pack_bits_msb(O.itq_get_hash(q_vec, mean_vec, rotation, normalize)[None, :])[0]
    _, near = O.hamming_topk(uniq_codes, q_code, n)
    cand: List[int] = []
    for u in near.tolist():
        cand.extend(code_rows[u])
    cand_a = np.asarray(cand, dtype=np.int64)
    k = n if k is None else k
    if cand_a.shape[0] == 0:
        return cand_a, np.zeros(0, dtype=db.dtype if metric == "euclidean" else np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        dist = O.dense_distances(db[cand_a], q_vec, metric)
    order = np.argsort(dist, kind="stable")[:k]
    return cand_a[order], dist[order]


def csr_of(inv: np.ndarray, n_codes: int, live: Optional[np.ndarray] = None):
    """(off, order, buckets) of rows grouped by code id, row order inside a bucket -- as HipLSHNearestNeighborIndex
    builds its map; `live`: the rows the map lists (default all)."""
    rows = np.arange(inv.shape[0], dtype=np.int64) if live is None else np.asarray(live, dtype=np.int64)
    o = np.argsort(inv[rows], kind="stable")
    order = rows[o].astype(np.int64)
    off = np.searchsorted(inv[rows][o], np.arange(n_codes + 1)).astype(np.int64)
    buckets = [order[off[u]:off[u + 1]].tolist() for u in range(n_codes)]
    return off, order, buckets


class Case:
    """What make_case returns; arrays are read-only."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self._oracle: Dict[tuple, Tuple[np.ndarray, np.ndarray]] = {}

    @property
    def words(self) -> int:
        return O.words_for_bits(self.bits)

    def oracle(self, qi: int, m: int, metric: str, k: Optional[int] = None, buckets=None, tag=None):
        """(row ids, distances) of pool query `qi` for the m nearest codes, first k (default m) rows; computed once per
        (query, m, metric) -- every row of the list is kept, so any k is a slice of it.  `buckets` (with a `tag` for
        the cache) replaces the case's bucket lists: a partial map."""
        key = (qi, m, metric, tag)
        if key not in self._oracle:
            self._oracle[key] = lsh_nn_fast(self.pool[qi], m, self.mean, self.rot, self.normalize, self.uniq,
                                            self.buckets if buckets is None else buckets, self.db, metric,
                                            k=self.db.shape[0], q_code=self.pool_codes[qi])
        ids, dist = self._oracle[key]
        k = m if k is None else k
        return ids[:k], dist[:k]


def _model(rng, db, d, bits, normalize):
    # the float64 mean of the first 500 rows as the functor sees them (normalised rows when it normalises: the raw
    # rows' mean would dwarf x / |x|_1 and collapse the codes)
    mean = O.itq_norm_vector(db[:500].astype(np.float64), normalize).mean(axis=0)
    if bits <= d:
        q, _ = np.linalg.qr(rng.standard_normal((d, d)))
        rot = np.ascontiguousarray(q[:, :bits])
    else:
        rot = rng.standard_normal((d, bits))
    return mean, rot


def check_margin(x, mean, rot, normalize, what):
    xn = O.itq_norm_vector(x, normalize)
    z = O.itq_z(x, mean, rot, normalize)
    scale = np.linalg.norm(xn.astype(np.float64) - mean, axis=1)[:, None] * np.linalg.norm(rot, axis=0)[None, :]
    worst = (np.abs(z) / scale).min()
    assert worst > 1e-9, f"{what}: a query bit sits {worst:.3e} of |x - mean||R_j| from zero"


@functools.lru_cache(maxsize=16)
def make_case(dtype, d: int, bits: int, normalize, seed: int, n_centres: int = N_CENTRES) -> Case:
    dt = np.dtype(dtype).type
    what = f"case {np.dtype(dtype).name} {d}->{bits} normalize={normalize} seed={seed}"
    rng = np.random.default_rng(seed)
    # ---- rows: centres repeated 1 .. 6 times, a repeat an exact copy or the centre plus noise of relative size 2^-12
    centres = rng.standard_normal((n_centres, d)).astype(dt)
    reps = rng.choice(np.arange(1, 7), size=n_centres, p=[0.65, 0.07, 0.07, 0.07, 0.07, 0.07])
    src = np.repeat(np.arange(n_centres), reps)
    first = np.r_[True, src[1:] != src[:-1]]
    noisy = ~first & (rng.random(src.shape[0]) < 0.5)
    body = centres[src]
    body[noisy] += (rng.standard_normal((int(noisy.sum()), d)) * 2.0 ** -12).astype(dt)
    perm = rng.permutation(src.shape[0])                # buckets are scattered over the row ids
    body, src, first = body[perm], src[perm], first[perm]
    mean, rot = _model(rng, body, d, bits, normalize)
    assert np.abs(mean).max() > 0
    # ---- the zero row and company for its bucket: x = -s mean gives x - mean = -(1 + s) mean (with normalize as well:
    # x / |x| is a negative multiple of the mean again), the signs of the zero row's own -mean
    company = np.stack([(-s * mean).astype(dt) for s in (0.5, 1.0, 2.0)])
    # ---- the planted pair c + e, c - e: small multiples of 2^-8, so both sums and both differences from c are exact
    # in float32 and the two L2 distances are the same bits
    c = (np.rint(rng.standard_normal(d) * 256) / 256).astype(dt)
    e = (np.rint(rng.standard_normal(d) * 0.3 * 256) / 256).astype(dt)
    assert np.abs(c).max() < 8 and np.abs(e).max() < 8 and (e != 0).any()
    pair = np.stack([c + e, c - e])
    db = np.ascontiguousarray(np.vstack([body, np.zeros((1, d), dt), company, pair]).astype(dt))
    n = db.shape[0]
    zero_row, pair_rows = body.shape[0], (n - 2, n - 1)
    # ---- codes and buckets, from the oracle's hash
    packed = O.pack_bits_msb(O.itq_get_hash(db, mean, rot, normalize))
    uniq, inv = np.unique(packed, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    # candidate order is (Hamming distance, code id): the pair's row that comes FIRST in it takes the higher row id
    q_code = O.pack_bits_msb(O.itq_get_hash(c, mean, rot, normalize)[None, :])[0]
    hd = O.popcount_u64(uniq[inv[list(pair_rows)]] ^ q_code[None, :]).sum(axis=1)
    assert inv[pair_rows[0]] != inv[pair_rows[1]], f"{what}: the planted pair shares a bucket"
    if (hd[0], inv[pair_rows[0]]) < (hd[1], inv[pair_rows[1]]):
        db[[pair_rows[0], pair_rows[1]]] = db[[pair_rows[1], pair_rows[0]]]
        inv[[pair_rows[0], pair_rows[1]]] = inv[[pair_rows[1], pair_rows[0]]]
    off, order, buckets = csr_of(inv, uniq.shape[0])
    # ---- the query pool
    centre_row = int(np.flatnonzero(first & (reps[src] >= 3))[0])     # a noise-free centre with copies
    pool = rng.standard_normal((POOL, d)).astype(dt)
    near = rng.integers(0, body.shape[0], size=POOL)
    half = np.arange(POOL) % 2 == 0                                   # every other random query lies next to a row
    pool[half] = db[near[half]] + (rng.standard_normal((int(half.sum()), d)) * 0.05).astype(dt)
    pool[Q_ROW7], pool[Q_CENTRE], pool[Q_PAIR], pool[Q_ZERO] = db[7], db[centre_row], c, 0
    pool_codes = O.pack_bits_msb(O.itq_get_hash(pool, mean, rot, normalize))
    for a in (db, mean, rot, uniq, inv, off, order, pool, pool_codes):
        a.setflags(write=False)
    case = Case(db=db, mean=mean, rot=rot, normalize=normalize, bits=bits, d=d, uniq=uniq, inv=inv, off=off, order=order,
                buckets=buckets, pool=pool, pool_codes=pool_codes, zero_row=zero_row, pair_rows=pair_rows,
                centre_row=centre_row, what=what)
    # ---- the three conditions
    check_margin(pool, mean, rot, normalize, what)
    sizes = np.diff(off)
    assert uniq.shape[0] >= MIN_CODES, f"{what}: {uniq.shape[0]} unique codes"
    assert (sizes >= 2).mean() >= 0.25 and sizes.max() >= 5, f"{what}: bucket sizes {np.bincount(sizes)}"
    assert sizes[inv[zero_row]] >= 2, f"{what}: the zero row is alone in its bucket"
    case.tie_m = 20
    ids, dist = case.oracle(Q_PAIR, case.tie_m, "euclidean")
    eq = dist[1:].view(np.uint32 if dt is np.float32 else np.uint64) == dist[:-1].view(np.uint32 if dt is np.float32 else np.uint64)
    assert (eq & (ids[1:] < ids[:-1])).any(), f"{what}: no tie in descending id order in the answer for c: {ids[:4]} {dist[:4]}"
    assert set(ids[:2].tolist()) == set(pair_rows), f"{what}: the pair is not c's two nearest rows"
    return case


# The shapes of the GPU tests: (dtype, d, bits, normalize, seed, filter passes a call of 32 or more rows takes).  The
# pass count restates sq_itq.hip's rule (itq_filter_route / itq_plan): a float32 / float64 row of whole 16-byte pieces,
# normalize None or 2, up to 1024 bits -> one certified pass per 256 bits of the code; everything else float64 only.
ROUTE_CASES = [
    ("narrow", np.float32, 128, 64, None, 11, 1),
    ("narrow_norm", np.float32, 256, 128, 2, 12, 1),
    ("wide", np.float32, 512, 256, None, 13, 1),
    ("wide_f64", np.float64, 128, 64, None, 14, 1),
    ("slab_off_grid", np.float32, 100, 64, None, 15, 1),
    ("slab_100_bits", np.float64, 300, 100, 2, 16, 1),
    ("slab_1000_d", np.float32, 1000, 256, None, 17, 1),
    ("slab_320_bits", np.float32, 320, 320, None, 18, 2),
    ("slab_1024_bits", np.float32, 1024, 1024, None, 19, 4),
    ("f64_odd_row", np.float32, 130, 70, None, 20, 0),
    ("f64_norm_1", np.float32, 128, 64, 1, 21, 0),
]
ROUTE_BY_NAME = {c[0]: c for c in ROUTE_CASES}
# the four code widths of the Hamming-chain test: 1, 2, 5 and 16 words
WIDTH_CASES = {1: "narrow", 2: "slab_100_bits", 5: "slab_320_bits", 16: "slab_1024_bits"}
# the five-word case again with more than SQ_MAX_K = 16384 rows: a call that asks for every row then sorts more keys than
# the one-workgroup select holds, 64-bit keys (float32 L2) included
BIG_CENTRES = 8800


def route_case(name: str, n_centres: int = N_CENTRES) -> Case:
    _, dtype, d, bits, normalize, seed, _ = ROUTE_BY_NAME[name]
    return make_case(dtype, d, bits, normalize, seed, n_centres)
