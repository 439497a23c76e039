"""
IVF-PQ ``NearestNeighborsIndex`` on MI355X with residual coding: FAISS's default for the ``factory_string``
``"IVFx,PQy"`` (smqtk_indexing/impls/nn_index/faiss.py:190-192, :385).

``HipIvfPqNearestNeighborsIndex`` with one difference: a descriptor is coded as its residual against the centroid of its
list, and a query gets one set of distance tables per probed list (include/smqtk_hip_pq.h, residual mode).  On sets with
cluster structure the codebooks then spend their entries on the spread inside a cluster instead of on the clusters'
positions.  The configuration, the ``nlist`` rule, the training sample, the centroids and the draw of the initial
codebook entries are the parent's; the codebooks are trained on the residuals of the training sample
(``pq_train(pq_residuals(train, centroids), ...)``, the initial entries the residuals of the same draw) and the device
index is created with ``residual=True``.
"""
from typing import Any

import numpy as np

from ... import _lib
from .hip_ivf_pq import HipIvfPqNearestNeighborsIndex


class HipIvfPqResidualNearestNeighborsIndex(HipIvfPqNearestNeighborsIndex):
    """L2 kNN by product-quantiser codes of the rows' residuals against their list's centroid (HIP kernels)."""

    def _coded_rows(self, train: np.ndarray, centroids: np.ndarray) -> np.ndarray:
        return _lib.pq_residuals(train, centroids)

    def _new_device_index(self) -> Any:
        return _lib.PqIndex(self._centroids, self._codebooks, residual=True)
