"""
Numpy restatement and case builders for the tests of the refine stage (`sq_refine_*`): no GPU.

The restatement is the contract of include/smqtk_hip_refine.h: the store's codes and their decoding are tests/isq_cases.py's
(float32 rows are kept as they are), the refined distance is the oracle's euclidean distance over the decoded row, and a
re-rank keeps the candidate ids inside the store and orders them by (distance, id).
"""
import functools

import numpy as np

from oracle import cpu_ref as O
from smqtk_indexing_amd._lib import SQ_REFINE_F16, SQ_REFINE_F32, SQ_REFINE_SQ8
from tests import isq_cases as S
from tests import ivf_cases as C

KINDS = {"sq8": SQ_REFINE_SQ8, "f16": SQ_REFINE_F16, "f32": SQ_REFINE_F32}
# tails, 16-byte piece counts, numpy's first split, and rows of more than one 1024-byte slab: 257 floats, 1000 halves,
# 1025 bytes; 2100: three slabs of bytes, five of halves, nine of floats
WIDTHS = (1, 3, 7, 8, 9, 15, 16, 17, 33, 100, 127, 128, 129, 136, 255, 257, 300, 1000, 1025, 2100)
ROWS, NQ, KB, K = 70, 3, 37, 11
ID_BASE = 1000


def encode(x, kind, vmin=None, step=None):
    return x.copy() if kind == SQ_REFINE_F32 else S.encode(x, kind, vmin, step)


def decode(codes, kind, vmin=None, step=None):
    return codes if kind == SQ_REFINE_F32 else S.decode(codes, kind, vmin, step)


def rerank(xd, id_base, queries, cand, k):
    """(dist [nq, k], ids [nq, k]): the k nearest decoded rows among each query's candidate ids, padded as the ABI pads."""
    out = []
    for q, c in zip(queries, cand):
        ids = c[(c >= id_base) & (c < id_base + xd.shape[0])]
        dist = O.dense_distances(xd[ids - id_base], q, "euclidean") if len(ids) else np.zeros(0, np.float32)
        o = np.lexsort((ids, dist))
        out.append(C.pad(ids[o], dist[o], k))
    return np.stack([r[1] for r in out]), np.stack([r[0] for r in out])


@functools.lru_cache(maxsize=None)
def width_case(d: int):
    """(rows, vmin, step, queries, cand): 70 rows, 3 queries near rows, 37 distinct random ids per query with -1 entries,
    one id below ID_BASE and one beyond the last row."""
    rng = np.random.default_rng([11, d])
    x = (rng.standard_normal((ROWS, d)) * 3).astype(np.float32)
    vmin, step = S.train(x[:50])                       # the last 20 rows clip
    q = x[:NQ] + (rng.standard_normal((NQ, d)) * 0.5).astype(np.float32)
    cand = np.stack([ID_BASE + rng.permutation(ROWS)[:KB] for _ in range(NQ)]).astype(np.int64)
    cand[:, 5] = -1
    cand[:, 20] = -1
    cand[:, 9] = ID_BASE - 1
    cand[:, 30] = ID_BASE + ROWS
    for a in (x, vmin, step, q, cand):
        a.setflags(write=False)
    return x, vmin, step, q, cand


N_LISTS, LIST_EMPTY, LIST_SMALL = 12, 10, 11


@functools.lru_cache(maxsize=1)
def list_case():
    """(rows [600, 32], centroids [12, 32], codebooks [4, 16, 8], vmin, step, queries [33, 32]): list 10 is empty (its
    centroid is far from every row), list 11 holds the 5 rows planted at its centroid."""
    rng = np.random.default_rng(12)
    x = rng.standard_normal((600, 32)).astype(np.float32)
    cent = x[rng.choice(590, size=N_LISTS, replace=False)].copy()
    cent[LIST_EMPTY] = 100
    cent[LIST_SMALL] = 20
    x[595:] = cent[LIST_SMALL] + (rng.standard_normal((5, 32)) * 0.1).astype(np.float32)
    books = np.ascontiguousarray(x[:16].reshape(16, 4, 8).transpose(1, 0, 2))
    vmin, step = S.train(x[:400])
    q = (rng.standard_normal((33, 32)) * 1.5).astype(np.float32)
    q[1] = cent[LIST_SMALL]
    q[2] = cent[LIST_EMPTY]
    for a in (x, cent, books, vmin, step, q):
        a.setflags(write=False)
    return x, cent, books, vmin, step, q
