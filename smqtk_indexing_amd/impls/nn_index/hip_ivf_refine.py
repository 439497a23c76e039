"""
IVF-PQ ``NearestNeighborsIndex`` on MI355X with a device refine stage: what ``FaissNearestNeighborsIndex`` reaches through
the ``factory_string``s ``"IVFx,PQy,RFlat"``, ``"IVFx,PQy,Refine(SQfp16)"`` and ``"IVFx,PQy,Refine(SQ8)"``
(smqtk_indexing/impls/nn_index/faiss.py:190-192, :385).

The product-quantiser codes choose ``n * k_factor`` candidates per query; a second store of all rows in id order
(``_lib.RefineStore``: float16, 8-bit codes with trained ranges, or the float32 rows) ranks them again on the device
(include/smqtk_hip_refine.h), so ``nn_many`` returns refined ids and distances.  Training plan, update and remove rules and
``nn``'s last step over the original vectors are ``HipIvfPqNearestNeighborsIndex``'s; the store is rebuilt or appended to
wherever the lists are.
"""
from typing import Any, Dict, Optional, Tuple

import numpy as np

from ... import _lib
from .hip_ivf_pq import HipIvfPqNearestNeighborsIndex

REFINE_KINDS = {"fp16": _lib.SQ_REFINE_F16, "sq8": _lib.SQ_REFINE_SQ8, "f32": _lib.SQ_REFINE_F32}


class _RefinedLists:
    """The device side of the class below: a ``PqIndex`` and the ``RefineStore`` that holds the same rows, kept in step
    (``add`` feeds both); ``search`` is the base's signature with the refined answer."""

    def __init__(self, base: Any, store: Any, k_factor: int):
        self.base, self.store, self.k_factor = base, store, k_factor

    def add(self, rows: np.ndarray) -> None:
        # the store first: its allocation is the large one, and a failed one leaves both as they were.  Should the base
        # fail behind it, the pair is out of step for good (there is no removal in place): both are closed, and the
        # owner's searches say so until the index is rebuilt.
        self.store.add(rows)
        try:
            self.base.add(rows)
        except Exception:
            self.close()
            raise

    def search(self, queries: np.ndarray, k: int, nprobe: int = 1) -> Tuple[np.ndarray, np.ndarray]:
        if not self.store.handle:
            raise RuntimeError("an add left the coded lists and the refine store out of step; rebuild the index")
        return self.store.search(self.base, queries, k, min(k * self.k_factor, self.store.n), nprobe)

    def close(self) -> None:
        self.base.close()
        self.store.close()


class HipIvfPqRefineNearestNeighborsIndex(HipIvfPqNearestNeighborsIndex):
    """L2 kNN by product-quantiser codes whose ``n * k_factor`` candidates a wider store of the rows re-ranks (HIP kernels)."""

    @classmethod
    def is_usable(cls) -> bool:
        return _lib.refine_usable()

    def __init__(self, nlist: Optional[int] = None, nprobe: int = 1, m: int = 8, residual: bool = True, packed: bool = False,
                 refine: str = "fp16", k_factor: int = 4, train_iters: int = 10, random_seed: int = 0, read_only: bool = False):
        super().__init__(nlist=nlist, nprobe=nprobe, m=m, train_iters=train_iters, random_seed=random_seed, read_only=read_only)
        if refine not in REFINE_KINDS:
            raise ValueError("refine must be one of %s." % sorted(REFINE_KINDS))
        if int(k_factor) < 1:
            raise ValueError("k_factor must be >= 1.")
        self.residual, self.packed, self.refine, self.k_factor = bool(residual), bool(packed), refine, int(k_factor)
        if self.packed:
            self.MAX_ENTRIES = _lib.SQ_PQ_PACKED_MAX_KSUB
        self._ranges: Optional[Tuple[np.ndarray, np.ndarray]] = None   # vmin, step of an 8-bit store, trained with the lists

    def get_config(self) -> Dict[str, Any]:
        return dict(super().get_config(), residual=self.residual, packed=self.packed, refine=self.refine, k_factor=self.k_factor)

    def _coded_rows(self, train: np.ndarray, centroids: np.ndarray) -> np.ndarray:
        # (called once per training, with the sample: the 8-bit store's ranges are trained on the same rows)
        self._ranges = _lib.isq_train(train) if self.refine == "sq8" else None
        return _lib.pq_residuals(train, centroids) if self.residual else train

    def _new_device_index(self) -> Any:
        base = _lib.PqIndex(self._centroids, self._codebooks, residual=self.residual, packed=self.packed)
        try:
            store = _lib.RefineStore(self._centroids.shape[1], REFINE_KINDS[self.refine], *(self._ranges or ()))
        except Exception:
            base.close()
            raise
        return _RefinedLists(base, store, self.k_factor)
