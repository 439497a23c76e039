"""
IVF-PQ ``NearestNeighborsIndex`` on MI355X: inverted lists whose rows are kept as product-quantiser codes.

The contract is the one the reference's FAISS wrapper reaches through the ``factory_string`` ``"IVFx,PQy"``
(smqtk_indexing/impls/nn_index/faiss.py:190-192, :385): descriptors are grouped by their nearest k-means centroid and
stored as ``m`` one-byte codes, a query scans the lists of its ``nprobe`` nearest centroids and ranks their rows by the
coded distance (include/smqtk_hip_pq.h).  The point is memory: ``round_up(m, 4) + 4`` bytes per row on the device and no
host copy of the matrix here.

Everything on the device goes through ``sq_pq_*`` (the extension library ``libsmqtk_hip_pq.so``).  The ``nlist`` rule, the
training sample and the initial centroids are ``HipIvfFlatNearestNeighborsIndex``'s; the initial codebook entries are the
sub-vectors of ``ksub = min(256, sample rows)`` distinct sample rows drawn next from the same generator, the same draw for
every sub-quantiser.  ``update_index`` with new uuids only is one ``add``; a replaced uuid and ``remove_from_index`` code
the remaining elements' vectors again with the same centroids and codebooks -- removal in place is not implemented.
``nn_many`` returns the coded distances; ``nn`` keeps the wrapper's last step for every dtype: the distances of the
returned elements are recomputed from their original vectors and the results ordered by those (faiss.py:818-827).
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


class HipIvfPqNearestNeighborsIndex(_ListIndexHostLogic, NearestNeighborsIndex):
    """L2 kNN by product-quantiser codes over the lists of the ``nprobe`` nearest k-means centroids (HIP kernels)."""

    @classmethod
    def is_usable(cls) -> bool:
        return _lib.pq_usable()

    def __init__(self, nlist: Optional[int] = None, nprobe: int = 1, m: int = 8, train_iters: int = 10, random_seed: int = 0,
                 read_only: bool = False):
        super().__init__()
        if int(nprobe) < 1:
            raise ValueError("nprobe must be >= 1.")
        if nlist is not None and not 1 <= int(nlist) <= _lib.SQ_IVF_MAX_LISTS:
            raise ValueError("nlist must be between 1 and %d (or None: 4 sqrt(n))." % _lib.SQ_IVF_MAX_LISTS)
        if not 1 <= int(m) <= _lib.SQ_PQ_MAX_M:
            raise ValueError("m must be between 1 and %d." % _lib.SQ_PQ_MAX_M)
        if int(train_iters) < 0:
            raise ValueError("train_iters must be >= 0.")
        self.nlist = None if nlist is None else int(nlist)
        self.nprobe = int(nprobe)
        self.m = int(m)
        self.train_iters = int(train_iters)
        self.random_seed = int(random_seed)
        self.read_only = read_only
        self._lock = threading.RLock()
        self._elements: List[DescriptorElement] = []       # by insertion number = the id the device returns
        self._row_of: Dict[Hashable, int] = {}
        self._centroids: Optional[np.ndarray] = None
        self._codebooks: Optional[np.ndarray] = None
        self._dev: Optional[_lib.PqIndex] = None

    def get_config(self) -> Dict[str, Any]:
        return {"nlist": self.nlist, "nprobe": self.nprobe, "m": self.m, "train_iters": self.train_iters,
                "random_seed": self.random_seed, "read_only": self.read_only}

    # ------------------------------------------------------------------ state (_to_matrix, _guard, effective_nlist: _ListIndexHostLogic)

    def training_plan(self, n: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(sample rows, positions of the initial centroids inside the sample, positions of the initial codebook
        entries inside the sample): the first two are the IVF-Flat class's, the third is one further draw of
        ``min(256, sample rows)`` distinct sample rows from the same generator."""
        sample, init, rs = training_draws(n, self.effective_nlist(n), self.random_seed)
        entries = rs.choice(len(sample), size=min(_lib.SQ_PQ_MAX_KSUB, len(sample)), replace=False)
        return sample, init, entries

    # The two places a subclass that codes something else than the rows themselves differs in.
    def _coded_rows(self, train: np.ndarray, centroids: np.ndarray) -> np.ndarray:
        """What the codebooks are trained on, row for row of the training sample: here the sample itself."""
        return train

    def _new_device_index(self) -> Any:
        """An empty device index over the centroids and codebooks in hand."""
        return _lib.PqIndex(self._centroids, self._codebooks)

    def _set_lists(self, elements: List[DescriptorElement], matrix: np.ndarray) -> None:
        """The lists over ``matrix`` with centroids and codebooks in hand (the device index is built first: a failure
        leaves the old state).  The matrix is not kept."""
        dev = None
        if matrix.shape[0]:
            assert self._centroids is not None and self._codebooks is not None
            dev = self._new_device_index()
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
            if matrix.shape[1] % self.m:
                raise ValueError("descriptors of %d dimensions cannot be split into m = %d sub-vectors" % (matrix.shape[1], self.m))
            _require_usable(self)
            sample, init, entries = self.training_plan(matrix.shape[0])
            train = matrix[sample]
            dsub = matrix.shape[1] // self.m
            centroids = _lib.ivf_kmeans(train, train[init], self.train_iters)
            coded = self._coded_rows(train, centroids)
            # the same rows serve every sub-quantiser: entry c of codebook j is sub-vector j of sample row entries[c]
            books0 = np.ascontiguousarray(coded[entries].reshape(len(entries), self.m, dsub).transpose(1, 0, 2))
            codebooks = _lib.pq_train(coded, books0, self.train_iters)
            self._centroids, self._codebooks = centroids, codebooks
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
        """Batched search: ``[nq, d]`` -> (row ids ``[nq, k]``, coded distances ``[nq, k]``), ``k = min(n, count)``;
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
            # faiss.py:818-827: distances from the original vectors, results ordered by them -- the coded distances only
            # chose the candidates
            rows = np.vstack([e.vector() for e in elems])
            exact = _lib.dense_distances(q32[0], rows, _lib.SQ_METRIC_L2)
            order = np.argsort(exact, kind="stable")
            return tuple(elems[i] for i in order), tuple(float(exact[i]) for i in order)
