"""
IVF-SQ ``NearestNeighborsIndex`` classes on MI355X: inverted lists whose rows are kept as scalar-quantiser codes.

The contract is the one the reference's FAISS wrapper reaches through the ``factory_string``s ``"IVFx,SQ8"`` and
``"IVFx,SQfp16"`` (smqtk_indexing/impls/nn_index/faiss.py:190-192, :385): descriptors are grouped by their nearest k-means
centroid and stored as one byte per dimension (``HipIvfSq8NearestNeighborsIndex``) or as float16
(``HipIvfSqFp16NearestNeighborsIndex``); a query scans the lists of its ``nprobe`` nearest centroids and ranks their rows
by the distance to the decoded row (include/smqtk_hip_isq.h).  About a quarter and a half of IVF-Flat's device memory, and
no host copy of the matrix here.

Everything on the device goes through ``sq_isq_*`` (the extension library ``libsmqtk_hip_isq.so``).  The ``nlist`` rule, the
training sample and the initial centroids are ``HipIvfFlatNearestNeighborsIndex``'s; the 8-bit ranges are trained on the
same sample.  ``update_index`` with new uuids only is one ``add``; a replaced uuid and ``remove_from_index`` code the
remaining elements' vectors again with the same centroids and ranges -- removal in place is not implemented.  ``nn_many``
returns the decoded distances; ``nn`` keeps the wrapper's last step: the distances of the returned elements are recomputed
from their original vectors and the results ordered by those (faiss.py:818-827).
"""
import threading
import warnings
from typing import Any, Dict, Hashable, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from .. import _require_usable
from ... import _lib
from ..._compat import DescriptorElement
from ...interfaces.nearest_neighbor_index import NearestNeighborsIndex
from .hip_ivf import _ListIndexHostLogic, training_draws


class _HipIvfSqHostLogic(_ListIndexHostLogic):
    """Both classes but for ``KIND``: the state machine of ``HipIvfPqNearestNeighborsIndex`` with ranges where that class
    has codebooks."""

    KIND = _lib.SQ_ISQ_SQ8

    @classmethod
    def is_usable(cls) -> bool:
        return _lib.isq_usable()

    def __init__(self, nlist: Optional[int] = None, nprobe: int = 1, train_iters: int = 10, random_seed: int = 0,
                 read_only: bool = False):
        super().__init__()
        if int(nprobe) < 1:
            raise ValueError("nprobe must be >= 1.")
        if nlist is not None and not 1 <= int(nlist) <= _lib.SQ_IVF_MAX_LISTS:
            raise ValueError("nlist must be between 1 and %d (or None: 4 sqrt(n))." % _lib.SQ_IVF_MAX_LISTS)
        if int(train_iters) < 0:
            raise ValueError("train_iters must be >= 0.")
        self.nlist = None if nlist is None else int(nlist)
        self.nprobe = int(nprobe)
        self.train_iters = int(train_iters)
        self.random_seed = int(random_seed)
        self.read_only = read_only
        self._lock = threading.RLock()
        self._elements: List[DescriptorElement] = []       # by insertion number = the id the device returns
        self._row_of: Dict[Hashable, int] = {}
        self._centroids: Optional[np.ndarray] = None
        self._ranges: Tuple[Optional[np.ndarray], Optional[np.ndarray]] = (None, None)   # (vmin, step); F16 has none
        self._dev: Optional[_lib.IsqIndex] = None

    def get_config(self) -> Dict[str, Any]:
        return {"nlist": self.nlist, "nprobe": self.nprobe, "train_iters": self.train_iters,
                "random_seed": self.random_seed, "read_only": self.read_only}

    def training_plan(self, n: int) -> Tuple[np.ndarray, np.ndarray]:
        """(sample rows, positions of the initial centroids inside the sample): the IVF-Flat class's."""
        sample, init, _ = training_draws(n, self.effective_nlist(n), self.random_seed)
        return sample, init

    def _set_lists(self, elements: List[DescriptorElement], matrix: np.ndarray) -> None:
        """The lists over ``matrix`` with centroids and ranges in hand (the device index is built first: a failure
        leaves the old state).  The matrix is not kept."""
        dev = None
        if matrix.shape[0]:
            assert self._centroids is not None
            dev = _lib.IsqIndex(self._centroids, self.KIND, *self._ranges)
            dev.add(matrix)
        if self._dev is not None:
            self._dev.close()
        self._dev = dev
        self._elements = elements
        self._row_of = {e.uuid(): i for i, e in enumerate(elements)}

    # -------------------------------------------------------------- interface
    def count(self) -> int:
        with self._lock:
            return len(self._elements)

    def _build_index(self, descriptors: Iterable[DescriptorElement]) -> None:
        with self._lock:
            self._guard()
            uniq: Dict[Hashable, DescriptorElement] = {}
            for d in descriptors:
                uniq[d.uuid()] = d
            elements = list(uniq.values())
            matrix = self._to_matrix(elements)
            _require_usable(self)
            sample, init = self.training_plan(matrix.shape[0])
            train = matrix[sample]
            self._centroids = _lib.ivf_kmeans(train, train[init], self.train_iters)
            self._ranges = _lib.isq_train(train) if self.KIND == _lib.SQ_ISQ_SQ8 else (None, None)
            self._set_lists(elements, matrix)

    def _update_index(self, descriptors: Iterable[DescriptorElement]) -> None:
        with self._lock:
            self._guard()
            new: Dict[Hashable, DescriptorElement] = {}
            for d in descriptors:
                new[d.uuid()] = d
            add = list(new.values())
            if not self._elements or self._centroids is None:
                return self._build_index(add)
            add_m = self._to_matrix(add)
            if add_m.shape[1] != self._centroids.shape[1]:
                raise ValueError("descriptors of %d dimensions cannot join an index of %d"
                                 % (add_m.shape[1], self._centroids.shape[1]))
            _require_usable(self)
            if self._dev is not None and not any(u in self._row_of for u in new):
                # nothing replaced: the new rows join the existing lists, no retraining (faiss.py:561-640)
                self._dev.add(add_m)
                base = len(self._elements)
                self._elements.extend(add)
                self._row_of.update({e.uuid(): base + i for i, e in enumerate(add)})
                return
            kept = [e for e in self._elements if e.uuid() not in new]
            matrix = np.vstack([self._to_matrix(kept), add_m]) if kept else add_m
            self._set_lists(kept + add, np.ascontiguousarray(matrix, dtype=np.float32))

    def _remove_from_index(self, uids: Iterable[Hashable]) -> None:
        with self._lock:
            self._guard()
            uids = list(uids)
            for u in uids:
                if u not in self._row_of:
                    raise KeyError(u)          # nothing modified yet
            drop = set(uids)
            kept = [e for e in self._elements if e.uuid() not in drop]
            if kept:
                _require_usable(self)
            self._set_lists(kept, self._to_matrix(kept) if kept else np.zeros((0, 0), dtype=np.float32))

    def nn_many(self, vectors: np.ndarray, n: int = 1) -> Tuple[np.ndarray, np.ndarray]:
        """Batched search: ``[nq, d]`` -> (row ids ``[nq, k]``, decoded distances ``[nq, k]``), ``k = min(n, count)``;
        where the probed lists hold fewer than ``k`` rows the tail is ``-1`` / ``+inf``."""
        with self._lock:
            if not self.count():
                raise ValueError("No index currently set to query from!")
            _require_usable(self)
            assert self._dev is not None
            k = min(int(n), self.count())
            dist, idx = self._dev.search(np.asarray(vectors, dtype=np.float32), k, self.nprobe)
            return idx, dist

    def elements_of(self, rows: Sequence[int]) -> Tuple[DescriptorElement, ...]:
        with self._lock:
            return tuple(self._elements[int(r)] for r in rows)

    def _nn(self, d: DescriptorElement, n: int = 1
            ) -> Tuple[Tuple[DescriptorElement, ...], Tuple[float, ...]]:
        with self._lock:
            q32 = np.asarray(d.vector()).reshape(1, -1).astype(np.float32)      # faiss.py:776
            idx, _ = self.nn_many(q32, n)
            found = idx[0] >= 0                                                  # faiss.py:797-804: -1 entries are dropped
            if int(found.sum()) < n:                                            # faiss.py:805-809
                warnings.warn(f"Fewer than n={n} neighbours were found in the probed lists "
                              f"(nprobe={self.nprobe}); a larger nprobe reaches more of the index.", RuntimeWarning)
            elems = self.elements_of(idx[0][found])
            if not elems:
                return elems, ()
            # faiss.py:818-827: distances from the original vectors, results ordered by them -- the decoded distances
            # only chose the candidates
            rows = np.vstack([e.vector() for e in elems])
            exact = _lib.dense_distances(q32[0], rows, _lib.SQ_METRIC_L2)
            order = np.argsort(exact, kind="stable")
            return tuple(elems[i] for i in order), tuple(float(exact[i]) for i in order)


class HipIvfSq8NearestNeighborsIndex(_HipIvfSqHostLogic, NearestNeighborsIndex):
    """L2 kNN by 8-bit scalar-quantiser codes over the lists of the ``nprobe`` nearest k-means centroids (HIP kernels)."""
    KIND = _lib.SQ_ISQ_SQ8


class HipIvfSqFp16NearestNeighborsIndex(_HipIvfSqHostLogic, NearestNeighborsIndex):
    """L2 kNN by float16 rows over the lists of the ``nprobe`` nearest k-means centroids (HIP kernels)."""
    KIND = _lib.SQ_ISQ_F16
