"""
IVF-Flat ``NearestNeighborsIndex`` on MI355X: approximate by construction, exact inside the probed lists.

The contract is the one the reference's FAISS wrapper reaches through a ``factory_string`` with an IVF stage and its
``ivf_nprobe`` (smqtk_indexing/impls/nn_index/faiss.py:190-192, 230-236; nprobe is set before every search, :785, and
fewer than ``n`` results raise a ``RuntimeWarning`` that points at nprobe, :805-809): descriptors are grouped by their
nearest k-means centroid, a query scans the lists of its ``nprobe`` nearest centroids and returns the nearest rows
among them, by ``metrics.euclidean_distance`` (utils/metrics.py:73-86) in float32.  With ``nprobe >= nlist`` the
answers are ``HipBruteForceNearestNeighborsIndex``'s.

Everything on the device goes through ``sq_ivf_*`` (include/smqtk_hip_ivf.h, the extension library ``libsmqtk_hip_ivf.so``): k-means training, the lists, the scan.
``update_index`` adds to the existing lists without retraining (faiss.py:561-640, ``add_with_ids``); a replaced uuid
and ``remove_from_index`` rebuild the lists from the host copy of the rows with the same centroids -- removal in place
on the device is not implemented.  As in the brute-force class, when the descriptors are not float32 the distances of
the results are recomputed from the original vectors and the results ordered by those (faiss.py:818-824).
"""
import math
import threading
import warnings
from typing import Any, Dict, Hashable, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from .. import _require_usable
from ... import _lib
from ..._compat import DescriptorElement, ReadOnlyError
from ...interfaces.nearest_neighbor_index import NearestNeighborsIndex

TRAIN_ROWS_PER_LIST = 256   # the training sample is at most this many rows per list


def default_nlist(n: int) -> int:
    """Lists for ``n`` rows when none is given: ``4 sqrt(n)``, at least 1, at most ``n``."""
    return max(1, min(int(n), int(4 * math.sqrt(n))))


def training_draws(n: int, nlist: int, random_seed: int) -> Tuple[np.ndarray, np.ndarray, np.random.RandomState]:
    """(sample rows, positions of the initial centroids inside the sample, the generator after both draws) for ``n``
    rows and ``nlist`` lists: at most 256 rows per list drawn without replacement, then ``nlist`` distinct sample rows,
    both from ``RandomState(random_seed)``.  (The IVF-PQ class draws its initial codebook entries from the generator
    next.)"""
    rs = np.random.RandomState(random_seed)
    m = min(int(n), TRAIN_ROWS_PER_LIST * nlist)
    sample = np.sort(rs.choice(n, size=m, replace=False)) if m < n else np.arange(n)
    init = rs.choice(m, size=nlist, replace=False)
    return sample, init, rs


class _ListIndexHostLogic:
    """What the inverted-list plugin classes (IVF-Flat here, IVF-PQ in hip_ivf_pq.py) share on the host: the matrix of a
    set of descriptors, the read-only guard and the ``nlist`` rule.  Expects ``self.nlist`` and ``self.read_only``."""

    @staticmethod
    def _to_matrix(elements: Sequence[DescriptorElement]) -> np.ndarray:
        vecs = [e.vector() for e in elements]
        if any(v is None for v in vecs):
            raise ValueError("descriptor without a vector cannot be indexed")
        return np.ascontiguousarray(np.vstack(vecs), dtype=np.float32)

    def _guard(self) -> None:
        if self.read_only:
            raise ReadOnlyError("Cannot modify container attributes due to "
                                "being in read-only mode.")

    def effective_nlist(self, n: int) -> int:
        """The lists an index of ``n`` rows is trained with: the configured number clamped to ``n``, or ``4 sqrt(n)``."""
        nlist = default_nlist(n) if self.nlist is None else min(self.nlist, int(n))
        return max(1, min(nlist, _lib.SQ_IVF_MAX_LISTS))


class HipIvfFlatNearestNeighborsIndex(_ListIndexHostLogic, NearestNeighborsIndex):
    """L2 kNN over the lists of the ``nprobe`` nearest k-means centroids (HIP kernels)."""

    @classmethod
    def is_usable(cls) -> bool:
        return _lib.ivf_usable()

    def __init__(self, nlist: Optional[int] = None, nprobe: int = 1, train_iters: int = 10, random_seed: int = 0,
                 distance_method: str = "euclidean", read_only: bool = False):
        super().__init__()
        if distance_method != "euclidean":
            raise ValueError("Invalid distance method label. The inverted lists are 'euclidean' only.")
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
        self.distance_method = distance_method
        self.read_only = read_only
        self._lock = threading.RLock()
        self._elements: List[DescriptorElement] = []       # by insertion number = the id the device returns
        self._row_of: Dict[Hashable, int] = {}
        self._blocks: List[np.ndarray] = []                # host copy of the float32 rows, in the blocks they arrived in
        self._all_f32 = True
        self._centroids: Optional[np.ndarray] = None
        self._dev: Optional[_lib.IvfIndex] = None

    def get_config(self) -> Dict[str, Any]:
        return {"nlist": self.nlist, "nprobe": self.nprobe, "train_iters": self.train_iters,
                "random_seed": self.random_seed, "distance_method": self.distance_method, "read_only": self.read_only}

    # ------------------------------------------------------------------ state
    @property
    def _matrix(self) -> np.ndarray:
        if not self._blocks:
            return np.zeros((0, 0), dtype=np.float32)
        if len(self._blocks) > 1:
            self._blocks = [np.ascontiguousarray(np.vstack(self._blocks), dtype=np.float32)]
        return self._blocks[0]

    def training_plan(self, n: int) -> Tuple[np.ndarray, np.ndarray]:
        """(sample rows, positions of the initial centroids inside the sample) for ``n`` rows: at most 256 rows per
        list drawn without replacement, then ``nlist`` distinct sample rows, both from ``RandomState(random_seed)``."""
        sample, init, _ = training_draws(n, self.effective_nlist(n), self.random_seed)
        return sample, init

    def _set_lists(self, elements: List[DescriptorElement], matrix: np.ndarray) -> None:
        """The lists over ``matrix`` with the centroids in hand (the device index is built first: a failure leaves the
        old state)."""
        dev = None
        if matrix.shape[0]:
            assert self._centroids is not None
            dev = _lib.IvfIndex(self._centroids)
            dev.add(matrix)
        if self._dev is not None:
            self._dev.close()
        self._dev = dev
        self._elements = elements
        self._row_of = {e.uuid(): i for i, e in enumerate(elements)}
        self._blocks = [matrix] if matrix.shape[0] else []
        self._all_f32 = all(np.asarray(e.vector()).dtype == np.float32 for e in elements)

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
                self._blocks.append(add_m)
                self._all_f32 = self._all_f32 and all(np.asarray(e.vector()).dtype == np.float32 for e in add)
                return
            kept = [e for e in self._elements if e.uuid() not in new]
            rows = [self._row_of[e.uuid()] for e in kept]
            matrix = np.vstack([self._matrix[rows], add_m]) if kept else add_m
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
            rows = [self._row_of[e.uuid()] for e in kept]
            if kept:
                _require_usable(self)
            self._set_lists(kept, np.ascontiguousarray(self._matrix[rows], dtype=np.float32))

    def nn_many(self, vectors: np.ndarray, n: int = 1) -> Tuple[np.ndarray, np.ndarray]:
        """Batched search: ``[nq, d]`` -> (row ids ``[nq, k]``, distances ``[nq, k]``), ``k = min(n, count)``; where
        the probed lists hold fewer than ``k`` rows the tail is ``-1`` / ``+inf``."""
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
            idx, dist = self.nn_many(q32, n)
            found = idx[0] >= 0                                                  # faiss.py:797-804: -1 entries are dropped
            if int(found.sum()) < n:                                            # faiss.py:805-809
                warnings.warn(f"Fewer than n={n} neighbours were found in the probed lists "
                              f"(nprobe={self.nprobe}); a larger nprobe reaches more of the index.", RuntimeWarning)
            elems = self.elements_of(idx[0][found])
            if self._all_f32 or not elems:
                return elems, tuple(float(v) for v in dist[0][found])
            # faiss.py:818-824: distances from the original-dtype vectors, results ordered by them
            rows = np.vstack([e.vector() for e in elems])
            exact = _lib.dense_distances(q32[0], rows, _lib.SQ_METRIC_L2)
            order = np.argsort(exact, kind="stable")
            return tuple(elems[i] for i in order), tuple(float(exact[i]) for i in order)
