"""
Numpy restatement and case builder for the tests of the IVF-SQ index (`sq_isq_*`): no GPU.

The restatement is the contract of include/smqtk_hip_isq.h: `train`, `encode`, `decode` in float32 with every operation
rounded once (numpy never contracts), and the search is tests/ivf_cases.py's over the DECODED matrix with the lists of the
original one.  `make(case, kind)` wraps an `ivf_cases.Case`; the 8-bit ranges are trained on the first 2 000 rows only, so
later rows clip at both ends (tests/test_isq_cases_cpu.py proves it).
"""
import functools

import numpy as np

from smqtk_indexing_amd._lib import SQ_ISQ_F16, SQ_ISQ_SQ8
from tests import ivf_cases as C

KINDS = {"sq8": SQ_ISQ_SQ8, "f16": SQ_ISQ_F16}
TRAIN_ROWS = 2000
F16_WIDTHS = (1, 7, 8, 9, 16, 17, 129, 257)


def train(x):
    vmin = x.min(axis=0)
    return vmin, (x.max(axis=0) - vmin) / np.float32(255)


def encode(x, kind, vmin=None, step=None):
    """Codes of the rows of x: uint8, or the halves' bits as uint16."""
    if kind == SQ_ISQ_F16:
        with np.errstate(over="ignore"):
            return x.astype(np.float16).view(np.uint16)
    with np.errstate(all="ignore"):
        t = (x - vmin) / step
        codes = np.where(t > 0, np.minimum(np.rint(t), 255), 0).astype(np.uint8)
    codes[:, step == 0] = 0
    return codes


def decode(codes, kind, vmin=None, step=None):
    if kind == SQ_ISQ_F16:
        return codes.view(np.float16).astype(np.float32)
    return vmin + step * codes.astype(np.float32)


class SqCase:
    """`case`: the original ivf_cases.Case; `codes` in row order; `dec`: the Case over the decoded matrix with the
    original's lists, whose `answer` / `expected` are what a search must return."""


@functools.lru_cache(maxsize=8)
def make(case: C.Case, kind: int) -> SqCase:
    sc = SqCase()
    sc.case, sc.kind = case, kind
    sc.vmin, sc.step = train(case.x[:TRAIN_ROWS]) if kind == SQ_ISQ_SQ8 else (None, None)
    sc.codes = encode(case.x, kind, sc.vmin, sc.step)
    xd = decode(sc.codes, kind, sc.vmin, sc.step)
    xd.setflags(write=False)
    sc.dec = C.Case(x=xd, centroids=case.centroids, assignment=case.assignment, off=case.off, order=case.order, pool=case.pool,
                    d=case.d, n=case.n, nlist=case.nlist, what=case.what + " decoded")
    return sc
