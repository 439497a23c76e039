"""
Inverted-list ``NearestNeighborsIndex`` classes on MI355X behind a PCA projection: what ``FaissNearestNeighborsIndex``
reaches through the ``factory_string`` ``"PCAy,IVFx,Flat"`` and ``"PCAy,IVFx,PQz"`` (smqtk_indexing/impls/nn_index/faiss.py:190-192).

Wide descriptors (2048- to 4096-d CNN features) make an inverted list of full rows hardly worth building: 16 KiB per row
at 4096-d.  The projection keeps the ``pca_dims`` directions of largest variance of a training sample; every row on its
way to the lists and every query passes it (``_lib.PcaTransform``, include/smqtk_hip_pca.h), and everything behind it is
the parent class unchanged, in the reduced space: centroids, (codebooks,) lists and the distances ``nn_many`` returns.
``nn`` keeps the wrapper's last step over the original vectors (faiss.py:818-827).

Training, in ``_build_index``: ``_lib.pca_moments`` over the parent's training sample (``training_draws``) gives the float32
mean and the float64 scatter about it on the device; on the host ``numpy.linalg.eigh`` of ``scatter / (n - 1)`` in float64,
the ``pca_dims`` eigenvectors of largest eigenvalue in descending order, each flipped so that its largest-magnitude
component is positive, rounded to float32 once.  No whitening, no random rotation behind the projection.
"""
import threading
import warnings
from typing import Any, Dict, Iterable, Optional, Sequence, Tuple

import numpy as np

from .. import _require_usable
from ... import _lib
from ..._compat import DescriptorElement
from .hip_ivf import HipIvfFlatNearestNeighborsIndex, _ListIndexHostLogic, training_draws
from .hip_ivf_pq_residual import HipIvfPqResidualNearestNeighborsIndex


def principal_axes(scatter: np.ndarray, n: int, dims: int) -> np.ndarray:
    """float32 ``[dims, d]``: the eigenvectors of ``scatter / (n - 1)`` (float64, symmetric) by descending eigenvalue, signs
    fixed by the largest-magnitude component."""
    _, vecs = np.linalg.eigh(np.asarray(scatter, dtype=np.float64) / (n - 1))      # ascending eigenvalues
    a = np.ascontiguousarray(vecs[:, ::-1][:, :dims].T)
    lead = a[np.arange(dims), np.abs(a).argmax(axis=1)]
    return np.ascontiguousarray(a * np.where(lead < 0, -1.0, 1.0)[:, None], dtype=np.float32)


class _PcaFront:
    """The projection in front of an inverted-list plugin class: mixed in ahead of the parent, which supplies the lists."""

    @classmethod
    def is_usable(cls) -> bool:
        return _lib.pca_usable()

    def __init__(self, pca_dims: int = 64, **kwargs: Any):
        super().__init__(**kwargs)
        if not 1 <= int(pca_dims) <= _lib.SQ_PCA_MAX_D_OUT:
            raise ValueError("pca_dims must be between 1 and %d." % _lib.SQ_PCA_MAX_D_OUT)
        self.pca_dims = int(pca_dims)
        self._pca_matrix: Optional[np.ndarray] = None      # float32 [pca_dims, d_in]
        self._pca_mean: Optional[np.ndarray] = None        # float32 [d_in]
        self._pca: Optional[_lib.PcaTransform] = None

    def get_config(self) -> Dict[str, Any]:
        return dict(super().get_config(), pca_dims=self.pca_dims)

    # the model travels with a pickle; device handles and the lock do not, and the lists are built again on arrival
    def __getstate__(self) -> Dict[str, Any]:
        with self._lock:
            state = dict(self.__dict__)
        for key in ("_lock", "_dev", "_pca"):
            state.pop(key)
        return state

    def __setstate__(self, state: Dict[str, Any]) -> None:
        self.__dict__.update(state)
        self._lock, self._dev, self._pca = threading.RLock(), None, None
        if self._elements and self.is_usable():
            self._set_lists(self._elements, self._reduced_rows())

    def _reduced_rows(self) -> np.ndarray:
        """The reduced rows of the elements in hand."""
        return self._to_matrix(self._elements)

    # ------------------------------------------------------------------ the projection in front
    def project(self, rows: np.ndarray) -> np.ndarray:
        """``rows`` (float32 ``[n, d_in]``) centred and projected; as given before there is a model."""
        if self._pca_matrix is None:
            return rows
        if rows.ndim != 2 or rows.shape[1] != self._pca_matrix.shape[1]:
            raise ValueError("descriptors of %d dimensions cannot pass a projection of %d"
                             % (rows.shape[-1] if rows.ndim else 0, self._pca_matrix.shape[1]))
        if not rows.shape[0]:
            return np.zeros((0, self.pca_dims), dtype=np.float32)
        if self._pca is None:
            self._pca = _lib.PcaTransform(self._pca_matrix, self._pca_mean)
        return self._pca.apply(rows)

    def _to_matrix(self, elements: Sequence[DescriptorElement]) -> np.ndarray:
        # every row on its way to the lists passes here: build, update and the re-coding after a removal
        return self.project(_ListIndexHostLogic._to_matrix(elements))

    def _build_index(self, descriptors: Iterable[DescriptorElement]) -> None:
        with self._lock:
            self._guard()
            descriptors = list(descriptors)
            uniq = list({d.uuid(): d for d in descriptors}.values())
            raw = _ListIndexHostLogic._to_matrix(uniq)
            n, d = raw.shape
            if d > _lib.SQ_PCA_MAX_D_IN:
                raise ValueError("descriptors of %d dimensions are beyond the projection's %d" % (d, _lib.SQ_PCA_MAX_D_IN))
            if self.pca_dims > d:
                raise ValueError("pca_dims = %d is beyond the descriptors' %d dimensions" % (self.pca_dims, d))
            if n < 2:
                raise ValueError("a projection cannot be trained on fewer than 2 descriptors")
            _require_usable(self)
            sample, _, _ = training_draws(n, self.effective_nlist(n), self.random_seed)
            mean, scatter = _lib.pca_moments(raw[sample])
            old = self._pca_matrix, self._pca_mean, self._pca
            self._pca_matrix, self._pca_mean, self._pca = principal_axes(scatter, len(sample), self.pca_dims), mean, None
            try:
                super()._build_index(descriptors)
            except Exception:
                self._pca_matrix, self._pca_mean, self._pca = old
                raise
            if old[2] is not None:
                old[2].close()

    def nn_many(self, vectors: np.ndarray, n: int = 1) -> Tuple[np.ndarray, np.ndarray]:
        """As the parent's, the queries projected by one ``sq_pca_apply`` first; the distances are the reduced space's."""
        with self._lock:
            q = np.ascontiguousarray(np.atleast_2d(np.asarray(vectors, dtype=np.float32)))
            if self.count():
                if self._pca_matrix is not None and q.shape[1] != self._pca_matrix.shape[1]:
                    raise ValueError("queries of %d dimensions cannot pass a projection of %d" % (q.shape[1], self._pca_matrix.shape[1]))
                _require_usable(self)
                q = self.project(q)
            return super().nn_many(q, n)

    def _nn(self, d: DescriptorElement, n: int = 1) -> Tuple[Tuple[DescriptorElement, ...], Tuple[float, ...]]:
        with self._lock:
            q32 = np.asarray(d.vector()).reshape(1, -1).astype(np.float32)
            idx, _ = self.nn_many(q32, n)
            found = idx[0] >= 0
            if int(found.sum()) < n:
                warnings.warn(f"Fewer than n={n} neighbours were found in the probed lists "
                              f"(nprobe={self.nprobe}); a larger nprobe reaches more of the index.", RuntimeWarning)
            elems = self.elements_of(idx[0][found])
            if not elems:
                return elems, ()
            # faiss.py:818-827: distances from the original vectors, results ordered by them -- the reduced-space
            # distances only chose the candidates
            exact = _lib.dense_distances(q32[0], np.vstack([e.vector() for e in elems]), _lib.SQ_METRIC_L2)
            order = np.argsort(exact, kind="stable")
            return tuple(elems[i] for i in order), tuple(float(exact[i]) for i in order)


class HipPcaIvfFlatNearestNeighborsIndex(_PcaFront, HipIvfFlatNearestNeighborsIndex):
    """``"PCAy,IVFx,Flat"``: exact L2 inside the probed lists of the projected rows (HIP kernels).  The host copy of the
    rows is the reduced rows."""

    def __init__(self, pca_dims: int = 64, nlist: Optional[int] = None, nprobe: int = 1, train_iters: int = 10, random_seed: int = 0,
                 read_only: bool = False):
        super().__init__(pca_dims=pca_dims, nlist=nlist, nprobe=nprobe, train_iters=train_iters, random_seed=random_seed, read_only=read_only)

    def get_config(self) -> Dict[str, Any]:
        c = super().get_config()
        c.pop("distance_method")
        return c

    def _reduced_rows(self) -> np.ndarray:
        return self._matrix


class HipPcaIvfPqNearestNeighborsIndex(_PcaFront, HipIvfPqResidualNearestNeighborsIndex):
    """``"PCAy,IVFx,PQz"``: product-quantiser codes of the projected rows' residuals (HIP kernels); ``pca_dims`` must be a
    multiple of ``m``."""

    def __init__(self, pca_dims: int = 64, nlist: Optional[int] = None, nprobe: int = 1, m: int = 8, train_iters: int = 10,
                 random_seed: int = 0, read_only: bool = False):
        super().__init__(pca_dims=pca_dims, nlist=nlist, nprobe=nprobe, m=m, train_iters=train_iters, random_seed=random_seed,
                         read_only=read_only)
        if self.pca_dims % self.m:
            raise ValueError("pca_dims = %d cannot be split into m = %d sub-vectors" % (self.pca_dims, self.m))
