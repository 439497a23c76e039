"""Cases and float64 references for the tests of the PCA front stage (no GPU).  The contracts are include/smqtk_hip_pca.h's:
`apply_reference` and `moments_reference` return the float64 value and the per-element bound; nothing else is a tolerance."""
import functools

import numpy as np

U = 2.0 ** -24
RUN = 1024                                   # kPcaRun
APPLY_SHAPES = ((1, 1), (3, 2), (5, 5), (35, 31), (64, 32), (100, 33), (130, 65), (516, 128), (513, 129), (1027, 256), (2052, 512), (8192, 64))
MOMENT_WIDTHS = (1, 5, 32, 33, 127, 128, 129, 260)          # 260: six tiles, three of them mirrored
MOMENT_ROWS = (2, RUN - 1, RUN, RUN + 1, 3 * RUN + 7)       # from RUN + 1 on the rows are split into chunks at every width here
MOMENT_CASES = tuple((d, n) for d in MOMENT_WIDTHS for n in MOMENT_ROWS) + ((128, 40 * RUN + 5),)


def gamma(m: int) -> float:
    return m * U / (1 - m * U)


def tile_rows(d_out: int) -> int:
    return 128 if d_out <= 32 else 64


def row_counts(d_out: int):
    t = tile_rows(d_out)
    return (1, t - 1, t, t + 1, 3 * t + 7)


@functools.lru_cache(maxsize=None)
def model(d_in: int, d_out: int):
    """(A float32 [d_out, d_in], mean float32 [d_in] with entries in 1 .. 3)."""
    rng = np.random.default_rng([21, d_in, d_out])
    a, mean = rng.standard_normal((d_out, d_in)).astype(np.float32), rng.uniform(1, 3, d_in).astype(np.float32)
    a.setflags(write=False), mean.setflags(write=False)
    return a, mean


@functools.lru_cache(maxsize=None)
def rows(n: int, d: int) -> np.ndarray:
    """N(0, 1) plus per-column offsets in [1, 3]: the column means do not cancel."""
    rng = np.random.default_rng([22, n, d])
    x = (rng.standard_normal((n, d)) + rng.uniform(1, 3, d)).astype(np.float32)
    x.setflags(write=False)
    return x


def apply_reference(x, a, mean):
    """(float64 A (x - mean), the per-element bound gamma_(d_in + 1) |A| |x - mean|)."""
    c, a64 = x.astype(np.float64) - mean.astype(np.float64), a.astype(np.float64)
    return c @ a64.T, gamma(a.shape[1] + 1) * (np.abs(c) @ np.abs(a64).T)


def moments_reference(x, mean32):
    """(float64 mean, float64 scatter about the float32 mean given, its per-element bound)."""
    c = x.astype(np.float64) - mean32.astype(np.float64)
    return x.astype(np.float64).mean(axis=0), c.T @ c, (gamma(RUN + 2) + len(x) * 2.0 ** -53) * (np.abs(c).T @ np.abs(c))


def check_moments(x, mean32, scatter, what):
    mean64, s64, bound = moments_reference(x, mean32)
    assert mean32.dtype == np.float32 and (np.abs(mean32 - mean64) <= np.spacing(np.abs(mean64).astype(np.float32))).all(), what
    err = np.abs(scatter - s64)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert (err <= bound).all(), f"{what}: element {worst} off by {err[worst]:.3e}, bound {bound[worst]:.3e}"
    assert np.array_equal(scatter, scatter.T), what


def selection(d_in: int, d_out: int):
    pi = np.random.default_rng([23, d_in]).permutation(d_in)[:d_out]
    a = np.zeros((d_out, d_in), dtype=np.float32)
    a[np.arange(d_out), pi] = 1
    return a, pi


@functools.lru_cache(maxsize=1)
def integer_case():
    """(x float32 [3400, 260] in -3 .. 3, its mean, its int64 scatter): shuffled +- pairs about an integer centre; a float32
    partial sum is at most 1024 * 4 < 2^24, so every order gives the integer."""
    rng = np.random.default_rng(24)
    half, centre = rng.integers(-2, 3, size=(1700, 260)), rng.integers(-1, 2, size=260)
    x = rng.permutation(np.vstack([centre + half, centre - half]))
    assert np.abs(x).max() <= 3 and RUN * int((half ** 2).max()) < 2 ** 24
    return x.astype(np.float32), centre, 2 * (half.T @ half)


@functools.lru_cache(maxsize=1)
def index_case():
    """(rows float32 [1200, 96] of rank-16 signal plus noise, 33 queries near rows)."""
    rng = np.random.default_rng(25)
    x = rng.standard_normal((1200, 16)) @ rng.standard_normal((16, 96)) * 2 + 0.05 * rng.standard_normal((1200, 96)) + rng.uniform(1, 3, 96)
    q = x[:33] + 0.01 * rng.standard_normal((33, 96))
    return np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(q, dtype=np.float32)


def check_training_quality(a32, x, mean32, scatter_used):
    """Ky Fan: the variance a basis captures is linear in S, so a basis optimal for S' = S + E loses at most 2 d_out |E|_2
    <= 2 d_out |B|_F against the optimum of the exact S (B: the moments bound); rounding A to float32 moves it by at most
    u sqrt(d_in) per row in norm: 2 d_out u sqrt(d_in) |S|_2 more.  Evaluated in float64 against the exact scatter."""
    _, s64, bound = moments_reference(x, mean32)
    assert (np.abs(scatter_used - s64) <= bound).all()
    d_out, d_in = a32.shape
    a = a32.astype(np.float64)
    best = np.linalg.eigvalsh(s64)[::-1][:d_out].sum()
    margin = 2 * d_out * np.linalg.norm(bound) + 2 * d_out * U * np.sqrt(d_in) * np.linalg.norm(s64, 2)
    assert np.trace(a @ s64 @ a.T) >= best - margin and margin < 1e-2 * best
