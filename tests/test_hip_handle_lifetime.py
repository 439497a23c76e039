"""
Device memory comes back when handles are closed: every handle kind is created, used and closed over and over, and the
free device memory after the last cycle is compared with the free memory after the first.

The buffers of a handle are owned by the structs that declare them (csrc/sq_buffers.hpp); this is the check from the
outside that none is left behind -- a leak of an index's main copies shows as 8 cycles' worth of memory, the bound is 2
(the device is shared: other tenants move the reading too, so it cannot be tight).  The footprint of a cycle is what
`DenseIndex.info()` reports for the two dense indexes plus the bytes of every other input.
"""
import numpy as np
import pytest

from smqtk_indexing_amd import _lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CYCLES = 8
K = 10


def _inputs():
    rng = np.random.default_rng(20)
    x = {}
    x["l2"] = rng.standard_normal((65536, 32)).astype(np.float32)       # large enough for the int8 copy
    x["cos"] = rng.standard_normal((4096, 40)).astype(np.float32)
    x["codes"] = rng.integers(0, 2 ** 63, size=(4096, 2), dtype=np.uint64)   # 128-bit codes
    x["rows"] = rng.standard_normal((2048, 64)).astype(np.float32)      # the LSH rows, hashed to 64 bits
    x["mean"] = x["rows"].mean(axis=0).astype(np.float64)
    x["rot"] = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((64, 64)))[0])
    x["fit"] = rng.standard_normal((2048, 32)).astype(np.float32)
    x["pc"] = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((32, 32)))[0][:, :16])
    x["r"] = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((16, 16)))[0])
    return x


def _cycle(x, dev_bufs, stream):
    """Create, use and close one handle of every kind; returns the bytes the cycle kept on the device at its peak."""
    q_dev, od, oi = dev_bufs
    # dense L2: host and asynchronous device search, one removal, one compaction
    idx = _lib.DenseIndex(x["l2"])
    info = idx.info()
    assert info["int8_copy_bytes"] > 0 and info["int8_in_use"], info
    foot = info["f32_rows_bytes"] + info["bf16_copy_bytes"] + info["int8_copy_bytes"] + info["row_stats_bytes"]
    _, i = idx.search(x["l2"][:3], K)
    assert list(i[:, 0]) == [0, 1, 2]
    idx.search_device_async(q_dev.data_ptr(), 3, K, od.data_ptr(), oi.data_ptr(), stream)
    idx.sync()
    assert oi[:, 0].tolist() == [0, 1, 2]
    idx.remove([1, 500, 65535])
    old_to_new = idx.compact()
    assert idx.count() == (65533, 65533) and old_to_new[2] == 1
    idx.close()
    # dense cosine
    idx = _lib.DenseIndex(x["cos"], metric=_lib.SQ_METRIC_COSINE)
    info = idx.info()
    foot += info["f32_rows_bytes"] + info["bf16_copy_bytes"] + info["int8_copy_bytes"] + info["row_stats_bytes"]
    _, i = idx.search(x["cos"][:2], K)
    assert list(i[:, 0]) == [0, 1]
    idx.close()
    # Hamming
    hidx = _lib.HammingIndex(x["codes"])
    hd, hi = hidx.search(x["codes"][:2], K)
    assert list(hi[:, 0]) == [0, 1] and list(hd[:, 0]) == [0, 0]
    hidx.close()
    foot += x["codes"].nbytes
    # ITQ model, rows with their bucket map, and the one-call LSH query over them
    model = _lib.ItqModel(x["mean"], x["rot"])
    codes = model.hash(x["rows"])
    uniq, inv = np.unique(codes, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    off = np.concatenate([[0], np.cumsum(np.bincount(inv, minlength=len(uniq)))]).astype(np.int64)
    lsh_codes = _lib.HammingIndex(uniq)
    rows = _lib.RowMatrix(x["rows"])
    rows.set_buckets(off, np.argsort(inv, kind="stable").astype(np.int64))
    _, got = rows.lsh_query(lsh_codes, model, x["rows"][:4], 8, _lib.SQ_METRIC_L2, K)
    assert list(got[:, 0]) == [0, 1, 2, 3]
    rows.close()
    lsh_codes.close()
    model.close()
    foot += x["rot"].nbytes + x["mean"].nbytes + x["rows"].nbytes + uniq.nbytes + off.nbytes + 8 * len(inv)
    # ITQ fit
    fit = _lib.ItqFit(x["fit"])
    assert fit.cov().shape == (32, 32)
    fit.project(x["pc"])
    assert np.isfinite(fit.iterate(x["r"])).all()
    fit.close()
    foot += x["fit"].nbytes + 2048 * 16 * 8
    return foot


def _free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_closed_handles_give_their_memory_back():
    x = _inputs()
    dev = torch.device("cuda", 0)
    # the caller's own device memory is allocated once, before the first reading
    dev_bufs = (torch.from_numpy(x["l2"][:3].copy()).to(dev), torch.empty((3, K), dtype=torch.float32, device=dev),
                torch.empty((3, K), dtype=torch.int64, device=dev))
    stream = torch.cuda.current_stream().cuda_stream
    foot = _cycle(x, dev_bufs, stream)      # warm-up: the runtime's own pools, the kernels' code objects
    free_warm = _free_bytes()
    for _ in range(CYCLES):
        assert _cycle(x, dev_bufs, stream) == foot
    free_end = _free_bytes()
    lost = free_warm - free_end
    print("cycle footprint %d bytes; free after warm-up %d, after %d cycles %d: %d lost (%.2f cycles)"
          % (foot, free_warm, CYCLES, free_end, lost, lost / foot))
    assert foot > 16 << 20, foot     # the float32 rows and the int8 copy alone (8 MiB each): what a leak is measured in
    assert lost <= 2 * foot, "free device memory fell by %d bytes over %d cycles of %d bytes each" % (lost, CYCLES, foot)
