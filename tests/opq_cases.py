"""
Cases and numpy restatements for the tests of the OPQ transform and its training (`sq_opq_*`, hip_ivf_opq.py): no GPU.
The transform's contract (include/smqtk_hip_opq.h): within gamma_d * (|x| @ |A|.T) of the float64 product, element by
element, gamma_d = d u / (1 - d u), u = 2^-24; `reference` returns both, and nothing else is a tolerance.  `train_rotation`
is the plugin's loop with `pq_residual_cases.kmeans` for sq_pq_train and `pq_cases.encode` for the one-list index.
"""
import functools

import numpy as np

from tests.pq_cases import encode
from tests.pq_residual_cases import kmeans

TILE = 64                                   # kOpqTileRows
WIDTHS = (1, 3, 4, 5, 31, 32, 33, 35, 64, 100, 128, 130, 512, 513, 516, 1027)   # 512 | 513: the row tile resident | re-staged
ROWS = (1, TILE - 1, TILE, TILE + 1, 3 * TILE + 7)
KINDS = ("orthonormal", "general")
BLOCKS_PER_CU = 8                           # kOpqBlocksPerCu: beyond cus * 8 tiles a workgroup loops
U = 2.0 ** -24


def orthonormal(rng, d: int) -> np.ndarray:
    """The Q factor of a Gaussian matrix with the signs fixed (R's diagonal positive), float64."""
    q, r = np.linalg.qr(rng.standard_normal((d, d)))
    return q * np.where(np.diag(r) < 0, -1.0, 1.0)


@functools.lru_cache(maxsize=None)
def matrix(d: int, kind: str) -> np.ndarray:
    rng = np.random.default_rng([11, d, KINDS.index(kind)])
    a = np.ascontiguousarray(orthonormal(rng, d) if kind == "orthonormal" else rng.standard_normal((d, d)), dtype=np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def rows(n: int, d: int) -> np.ndarray:
    x = np.random.default_rng([12, n, d]).standard_normal((n, d)).astype(np.float32)
    assert (np.abs(x[x != 0]) >= np.finfo(np.float32).tiny).all()      # no subnormals
    x.setflags(write=False)
    return x


def reference(x: np.ndarray, a: np.ndarray):
    """(float64 product, the per-element bound)."""
    x64, a64, d = x.astype(np.float64), a.astype(np.float64), a.shape[0]
    return x64 @ a64.T, d * U / (1 - d * U) * (np.abs(x64) @ np.abs(a64).T)


def permutation(d: int) -> np.ndarray:
    return np.random.default_rng([13, d]).permutation(d)


def permutation_matrix(d: int) -> np.ndarray:
    """A[j][pi[j]] = 1: output column j is input column pi[j]."""
    a = np.zeros((d, d), dtype=np.float32)
    a[np.arange(d), permutation(d)] = 1
    return a


# ------------------------------------------------------------------------------------ training
T_N, T_D, T_M, T_KSUB = 4096, 32, 8, 16
T_ITERS, T_INNER = 10, 4                     # the plugin's defaults: opq_iters, OPQ_INNER_ITERS
T_BUDGET = T_INNER * (T_ITERS + 1)           # Lloyd iterations of the loop and the final training together


@functools.lru_cache(maxsize=1)
def make_training_case():
    """(X, entries): Z has product structure -- in each of m = 8 sub-spaces of 4 dimensions 16 centres with noise 0.02
    around them, a row's centre drawn independently per sub-space, sub-space j scaled by 0.6^j (uneven energy, as in the
    descriptors the index is for) -- and X = Z @ Q for a fixed rotation Q, which smears every sub-space over all columns.
    `entries`: the rows whose sub-vectors start the codebooks.  With equal scales the loop's margin over R = I is 7.61
    against 8.98; with these 0.365 against 1.102 (tests/test_host_logic_opq.py), so the case was changed."""
    rng = np.random.default_rng(14)
    centres = rng.standard_normal((T_M, T_KSUB, T_D // T_M)) * (0.6 ** np.arange(T_M))[:, None, None]
    pick = rng.integers(0, T_KSUB, size=(T_N, T_M))
    z = np.concatenate([centres[j][pick[:, j]] for j in range(T_M)], axis=1) + 0.02 * rng.standard_normal((T_N, T_D))
    x = np.ascontiguousarray(z @ orthonormal(rng, T_D), dtype=np.float32)
    x.setflags(write=False)
    return x, rng.choice(T_N, size=T_KSUB, replace=False)


def decode(books: np.ndarray, codes: np.ndarray) -> np.ndarray:
    return np.concatenate([books[j][codes[:, j]] for j in range(books.shape[0])], axis=1)


def mse(y: np.ndarray, books: np.ndarray, codes: np.ndarray) -> float:
    """Mean squared reconstruction error per row, float64."""
    return float(((y.astype(np.float64) - decode(books, codes)) ** 2).sum(axis=1).mean())


def start_books(y: np.ndarray, entries: np.ndarray, m: int) -> np.ndarray:
    """[m, ksub, dsub]: entry c of codebook j is sub-vector j of row entries[c] (the PQ classes' rule)."""
    return np.ascontiguousarray(y[entries].reshape(len(entries), m, -1).transpose(1, 0, 2))


def lloyd(y: np.ndarray, books: np.ndarray, iters: int) -> np.ndarray:
    """sq_pq_train restated: `iters` Lloyd iterations per sub-quantiser from `books`."""
    dsub = y.shape[1] // books.shape[0]
    return np.stack([kmeans(np.ascontiguousarray(y[:, j * dsub:(j + 1) * dsub]), books[j], iters) for j in range(books.shape[0])])


def rotated(x: np.ndarray, r: np.ndarray) -> np.ndarray:
    return (x.astype(np.float64) @ r.astype(np.float64).T).astype(np.float32)


def train_rotation(x: np.ndarray, entries: np.ndarray, r0: np.ndarray, m: int, iters: int) -> np.ndarray:
    """The plugin's loop: rotate, train warm-started for T_INNER iterations, code, decode, Procrustes."""
    r, books, x64 = np.array(r0, dtype=np.float32), None, x.astype(np.float64)
    for _it in range(iters):
        y = rotated(x, r)
        books = lloyd(y, start_books(y, entries, m) if books is None else books, T_INNER)
        u, _, vt = np.linalg.svd(x64.T @ decode(books, encode(books, y)).astype(np.float64))
        r = np.ascontiguousarray((u @ vt).T, dtype=np.float32)
    return r


def budget_mse(x: np.ndarray, r: np.ndarray, entries: np.ndarray, m: int) -> float:
    """The sample's error under rotation r with codebooks trained from the same start for the whole budget."""
    y = rotated(x, r)
    books = lloyd(y, start_books(y, entries, m), T_BUDGET)
    return mse(y, books, encode(books, y))
