"""
IVF-PQ ``NearestNeighborsIndex`` on MI355X behind a trained rotation: what ``FaissNearestNeighborsIndex`` reaches through the
``factory_string`` ``"OPQy,IVFx,PQy"`` (smqtk_indexing/impls/nn_index/faiss.py:190-192, :385).

A product quantiser cuts a row into ``m`` consecutive sub-vectors, so it spends its bits badly on rows whose energy is
spread unevenly over correlated dimensions.  OPQ (Ge et al.; FAISS's ``OPQMatrix``) applies an orthonormal ``R`` to every row
before it is coded and to every query before its tables are built, chosen so that the quantiser's reconstruction error on
the training sample is small; it costs no byte per row.  The rotation runs on the device (``_lib.OpqTransform``,
include/smqtk_hip_opq.h); everything behind it is one of the four IVF-PQ modes unchanged, in the rotated space: centroids,
codebooks, lists and the coded distances ``nn_many`` returns (rotated-space distances, which approximate the original ones
because ``R`` is orthonormal).  ``nn`` keeps the wrapper's last step over the original vectors (faiss.py:818-827).

Training (non-parametric OPQ), on the PQ classes' sample (``training_draws``) with one further draw of the generator for
the initial rotation -- the Q factor of a ``d x d`` Gaussian matrix with the signs fixed so that the R factor's diagonal is
positive.  Each of ``opq_iters`` iterations (default 10): ``Y = apply(R, X)`` on the device; ``sq_pq_train`` on ``Y`` for
``OPQ_INNER_ITERS`` = 4 iterations, warm-started from the previous codebooks; ``Y`` coded by a throw-away one-list
``PqIndex`` (the rule the index will use; ids ascend inside the one list, so the codes come back in sample order); decoded in
numpy; ``U, _, Vt = svd(X^T Y^)`` in float64 and ``R = (U Vt)^T`` rounded to float32 once.  The last rotation then goes in
front of the parent's training as it stands: centroids, (residuals,) and codebooks over the rotated sample.  Decode, cross
product and SVD stay on the host; ``train_profile`` holds the seconds each part took.
"""
import threading
import time
from typing import Any, Dict, Iterable, Optional, Sequence, Tuple

import numpy as np

from .. import _require_usable
from ... import _lib
from ..._compat import DescriptorElement
from .hip_ivf import training_draws
from .hip_ivf_pq import HipIvfPqNearestNeighborsIndex

PQ_MODES = {"plain": (False, False), "residual": (True, False), "packed": (False, True), "packed_residual": (True, True)}   # (residual, packed)
OPQ_INNER_ITERS = 4


def initial_rotation(rs: np.random.RandomState, d: int) -> np.ndarray:
    """float32 ``[d, d]``: the Q factor of a Gaussian matrix drawn from ``rs``, column signs fixed by the R factor's diagonal."""
    q, r = np.linalg.qr(rs.standard_normal((d, d)))
    return np.ascontiguousarray(q * np.where(np.diag(r) < 0, -1.0, 1.0), dtype=np.float32)


def decode(books: np.ndarray, codes: np.ndarray) -> np.ndarray:
    """``[n, d]``: row r is the concatenation of ``books[j][codes[r][j]]``."""
    return np.concatenate([books[j][codes[:, j]] for j in range(books.shape[0])], axis=1)


def train_rotation(x: np.ndarray, books_from: np.ndarray, m: int, r0: np.ndarray, iters: int,
                   profile: Optional[Dict[str, float]] = None) -> np.ndarray:
    """The loop of the module's docstring over the sample ``x``; the first codebooks are the sub-vectors of the rotated
    rows ``books_from``.  Returns the last ``R``."""
    n, d = x.shape
    x64 = x.astype(np.float64)
    r, books = np.ascontiguousarray(r0, dtype=np.float32), None
    spent = profile if profile is not None else {}
    for key in ("apply", "pq_train", "coding", "host"):
        spent.setdefault(key, 0.0)
    zero = np.zeros((1, d), dtype=np.float32)
    for _it in range(iters):
        t0 = time.perf_counter()
        with _lib.OpqTransform(r) as t:
            y = t.apply(x)
        t1 = time.perf_counter()
        if books is None:
            books = np.ascontiguousarray(y[books_from].reshape(len(books_from), m, d // m).transpose(1, 0, 2))
        books = _lib.pq_train(y, books, OPQ_INNER_ITERS)
        t2 = time.perf_counter()
        with _lib.PqIndex(zero, books) as coder:
            coder.add(y)
            _, ids, codes = coder.lists()
        assert np.array_equal(ids, np.arange(n))
        t3 = time.perf_counter()
        u, _, vt = np.linalg.svd(x64.T @ decode(books, codes).astype(np.float64))
        r = np.ascontiguousarray((u @ vt).T, dtype=np.float32)
        t4 = time.perf_counter()
        for key, dt in (("apply", t1 - t0), ("pq_train", t2 - t1), ("coding", t3 - t2), ("host", t4 - t3)):
            spent[key] += dt
    return r


class HipOpqIvfPqNearestNeighborsIndex(HipIvfPqNearestNeighborsIndex):
    """L2 kNN by product-quantiser codes of the rows under a trained rotation (HIP kernels)."""

    @classmethod
    def is_usable(cls) -> bool:
        return _lib.opq_usable()

    def __init__(self, nlist: Optional[int] = None, nprobe: int = 1, m: int = 8, pq_mode: str = "residual", opq_iters: int = 10,
                 train_iters: int = 10, random_seed: int = 0, read_only: bool = False):
        super().__init__(nlist=nlist, nprobe=nprobe, m=m, train_iters=train_iters, random_seed=random_seed, read_only=read_only)
        if pq_mode not in PQ_MODES:
            raise ValueError("pq_mode must be one of %s." % sorted(PQ_MODES))
        if int(opq_iters) < 0:
            raise ValueError("opq_iters must be >= 0.")
        self.pq_mode, self.opq_iters = pq_mode, int(opq_iters)
        self.residual, self.packed = PQ_MODES[pq_mode]
        if self.packed:
            self.MAX_ENTRIES = _lib.SQ_PQ_PACKED_MAX_KSUB
        self._rotation: Optional[np.ndarray] = None
        self._opq: Optional[_lib.OpqTransform] = None
        self.train_profile: Dict[str, float] = {}

    def get_config(self) -> Dict[str, Any]:
        return dict(super().get_config(), pq_mode=self.pq_mode, opq_iters=self.opq_iters)

    # the model travels with a pickle; device handles and the lock do not, and the lists are coded again on arrival
    def __getstate__(self) -> Dict[str, Any]:
        with self._lock:
            state = dict(self.__dict__)
        for key in ("_lock", "_dev", "_opq"):
            state.pop(key)
        return state

    def __setstate__(self, state: Dict[str, Any]) -> None:
        self.__dict__.update(state)
        self._lock, self._dev, self._opq = threading.RLock(), None, None
        if self._elements and self.is_usable():
            self._set_lists(self._elements, self._to_matrix(self._elements))

    # ------------------------------------------------------------------ the parent's two hooks, by mode
    def _coded_rows(self, train: np.ndarray, centroids: np.ndarray) -> np.ndarray:
        return _lib.pq_residuals(train, centroids) if self.residual else train

    def _new_device_index(self) -> Any:
        return _lib.PqIndex(self._centroids, self._codebooks, residual=self.residual, packed=self.packed)

    # ------------------------------------------------------------------ the rotation in front
    def rotate(self, rows: np.ndarray) -> np.ndarray:
        """``rows`` (float32 ``[n, d]``) under the trained rotation; as given before there is one."""
        if self._rotation is None or not rows.shape[0]:
            return rows
        if self._opq is None:
            self._opq = _lib.OpqTransform(self._rotation)
        return self._opq.apply(rows)

    def _to_matrix(self, elements: Sequence[DescriptorElement]) -> np.ndarray:
        # every row on its way to sq_pq_add passes here: build, update and the re-coding after a removal
        return self.rotate(HipIvfPqNearestNeighborsIndex._to_matrix(elements))

    def _build_index(self, descriptors: Iterable[DescriptorElement]) -> None:
        with self._lock:
            self._guard()
            descriptors = list(descriptors)
            uniq = list({d.uuid(): d for d in descriptors}.values())
            raw = HipIvfPqNearestNeighborsIndex._to_matrix(uniq)
            if raw.shape[1] % self.m:
                raise ValueError("descriptors of %d dimensions cannot be split into m = %d sub-vectors" % (raw.shape[1], self.m))
            if raw.shape[1] > _lib.SQ_OPQ_MAX_D:
                raise ValueError("descriptors of %d dimensions are beyond the transform's %d" % (raw.shape[1], _lib.SQ_OPQ_MAX_D))
            _require_usable(self)
            sample, _, rs = training_draws(raw.shape[0], self.effective_nlist(raw.shape[0]), self.random_seed)
            entries = rs.choice(len(sample), size=min(self.MAX_ENTRIES, len(sample)), replace=False)   # (the parent's further draw)
            r0 = initial_rotation(rs, raw.shape[1])
            self.train_profile = {}
            rotation = train_rotation(raw[sample], entries, self.m, r0, self.opq_iters, self.train_profile)
            old = self._rotation, self._opq
            self._rotation, self._opq = rotation, None
            try:
                super()._build_index(descriptors)
            except Exception:
                self._rotation, self._opq = old
                raise
            if old[1] is not None:
                old[1].close()

    def nn_many(self, vectors: np.ndarray, n: int = 1) -> Tuple[np.ndarray, np.ndarray]:
        """As the parent's, the queries rotated by one ``sq_opq_apply`` first; the distances are the rotated space's."""
        with self._lock:
            q = np.ascontiguousarray(np.atleast_2d(np.asarray(vectors, dtype=np.float32)))
            if self.count():
                _require_usable(self)
                q = self.rotate(q)
            return super().nn_many(q, n)
