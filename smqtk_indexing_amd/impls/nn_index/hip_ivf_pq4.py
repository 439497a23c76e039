"""
IVF-PQ ``NearestNeighborsIndex`` classes on MI355X with 4-bit codes: what the reference's FAISS wrapper reaches through
the ``factory_string`` ``"IVFx,PQyx4"`` (smqtk_indexing/impls/nn_index/faiss.py:190-192, :385).

``HipIvfPqNearestNeighborsIndex`` and ``HipIvfPqResidualNearestNeighborsIndex`` with two differences: the codebooks have
``ksub = min(16, sample rows)`` entries -- the same further draw from the same generator, of 16 rows instead of 256 --
and the device index is created with ``packed=True`` (include/smqtk_hip_pq.h, packed mode): two codes per byte,
``round_up(ceil(m / 2), 4) + 4`` bytes per row on the device, and a scan that looks its table entries up in registers.
Everything else -- configuration, ``nlist`` rule, training, ``update_index`` / ``remove_from_index``, ``nn_many``'s coded
distances and ``nn``'s re-ranking by the original vectors -- is the parents'.
"""
from typing import Any

from ... import _lib
from .hip_ivf_pq import HipIvfPqNearestNeighborsIndex
from .hip_ivf_pq_residual import HipIvfPqResidualNearestNeighborsIndex


class HipIvfPq4NearestNeighborsIndex(HipIvfPqNearestNeighborsIndex):
    """L2 kNN by packed 4-bit product-quantiser codes over the lists of the ``nprobe`` nearest centroids (HIP kernels)."""
    MAX_ENTRIES = _lib.SQ_PQ_PACKED_MAX_KSUB

    def _new_device_index(self) -> Any:
        return _lib.PqIndex(self._centroids, self._codebooks, packed=True)


class HipIvfPq4ResidualNearestNeighborsIndex(HipIvfPqResidualNearestNeighborsIndex):
    """L2 kNN by packed 4-bit product-quantiser codes of the rows' residuals against their list's centroid (HIP kernels)."""
    MAX_ENTRIES = _lib.SQ_PQ_PACKED_MAX_KSUB

    def _new_device_index(self) -> Any:
        return _lib.PqIndex(self._centroids, self._codebooks, residual=True, packed=True)
