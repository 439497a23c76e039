"""GPU tests of the PCA front stage (`sq_pca_*`, hip_ivf_pca.py): projection and moments against float64 within the derived bounds
of tests/pca_cases.py, selections and integer moments exactly, the indexes against their parent's device index over projected rows."""
import pickle

import numpy as np
import pytest
import torch

from smqtk_indexing_amd import _lib
from smqtk_indexing_amd._compat import DescriptorMemoryElement
from smqtk_indexing_amd.impls.nn_index import hip_ivf_pca as H
from tests import pca_cases as C

pytestmark = pytest.mark.gpu

GUARD = 64      # floats in front of and behind a device result
FILL = -7.5


def _within(y, x, a, mean, what):
    y64, bound = C.apply_reference(x, a, mean)
    err = np.abs(y.astype(np.float64) - y64)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert y.shape == y64.shape and (err <= bound).all(), f"{what}: element {worst} off by {err[worst]:.3e}, bound {bound[worst]:.3e}"


def _apply_device(t, x, shift):
    """x and y in device memory, `shift` floats into their allocations, y inside guards: (y, the guards)."""
    n = x.shape[0]
    xd = torch.zeros(shift + x.size, dtype=torch.float32, device="cuda")
    xd[shift:] = torch.from_numpy(np.array(x)).cuda().reshape(-1)
    yd = torch.full((GUARD + shift + n * t.d_out + GUARD,), FILL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    t.apply_device(xd.data_ptr() + 4 * shift, n, yd.data_ptr() + 4 * (GUARD + shift))
    torch.cuda.synchronize()
    out = yd.cpu().numpy()
    lo, hi = GUARD + shift, GUARD + shift + n * t.d_out
    return out[lo:hi].reshape(n, t.d_out), np.concatenate([out[:lo], out[hi:]])


@pytest.mark.parametrize("d_in,d_out", C.APPLY_SHAPES)
def test_apply_against_float64(d_in, d_out):
    a, mean = C.model(d_in, d_out)
    with _lib.PcaTransform(a, mean) as t:
        assert t.info()["tile_rows"] == C.tile_rows(d_out)
        for n in C.row_counts(d_out):
            x = C.rows(n, d_in)
            _within(t.apply(x), x, a, mean, f"{d_in}->{d_out} n={n} host")
            assert t.info()["last_rows"] == n and t.stats()["bytes_scanned"] == n * d_in * 4
        for shift in (0, 1):        # 16-byte loads where d_in allows them; a base 4 bytes into the allocation: element by element
            y, guards = _apply_device(t, x, shift)
            _within(y, x, a, mean, f"{d_in}->{d_out} n={n} device shift={shift}")
            assert (guards == FILL).all(), f"{d_in}->{d_out} shift={shift}: a write outside y"
        yd = torch.full((8,), FILL, dtype=torch.float32, device="cuda")
        t.apply_device(yd.data_ptr(), 0, yd.data_ptr() + 16)            # n = 0: nothing is written
        assert t.info()["last_rows"] == 0 and (yd.cpu().numpy() == FILL).all()


@pytest.mark.parametrize("d_in,d_out,n", [(35, 31, 391), (130, 65, 199), (516, 128, 199), (2052, 512, 65), (4, 2, None)])
def test_selection_gives_centred_columns_exactly(d_in, d_out, n):
    """y[r][j] is fl(x[r][pi[j]] - mean[pi[j]]) bit for bit.  (4, 2, None): twice a full grid's tiles: every workgroup loops."""
    a, pi = C.selection(d_in, d_out)
    mean = C.model(d_in, d_out)[1]
    with _lib.PcaTransform(a, mean) as t:
        if n is None:
            n = 2 * _lib.device_name(0)[2] * t.info()["blocks_per_cu"] * t.info()["tile_rows"] + 5
        x = C.rows(n, d_in)
        want = (x - mean)[:, pi].view(np.uint32)
        np.testing.assert_array_equal(t.apply(x).view(np.uint32), want)
        y, guards = _apply_device(t, x, 1)
        np.testing.assert_array_equal(y.view(np.uint32), want)
        assert (guards == FILL).all()


@pytest.mark.parametrize("d,n", C.MOMENT_CASES)
def test_moments_against_float64(d, n):
    x = C.rows(n, d)
    mean, scatter = _lib.pca_moments(x)
    C.check_moments(x, mean, scatter, (d, n))
    again = _lib.pca_moments(x)
    assert np.array_equal(again[0], mean) and np.array_equal(again[1], scatter)      # a fixed tree: the same bits


def test_moments_of_integers_are_exact():
    """A dropped row, a doubled chunk boundary or a swapped tile is a wrong integer."""
    x, centre, s_int = C.integer_case()
    mean, scatter = _lib.pca_moments(x)
    np.testing.assert_array_equal(mean, centre.astype(np.float32))
    np.testing.assert_array_equal(scatter, s_int.astype(np.float64))


def test_handles_of_other_kinds_and_equal_pointers_are_refused():
    a = np.eye(8, dtype=np.float32)
    x, y = np.ones((1, 8), np.float32), np.zeros((1, 8), np.float32)
    with _lib.OpqTransform(a) as opq, _lib.PcaTransform(a) as t:
        assert _lib.load_opq().sq_opq_apply(t.handle, x.ctypes.data, 1, y.ctypes.data, 0, None) == -1
        assert b"unknown handle" in _lib.load().sq_last_error()
        assert _lib.load_pca().sq_pca_apply(opq.handle, x.ctypes.data, 1, y.ctypes.data, 0, None) == -1
        assert b"unknown handle" in _lib.load().sq_last_error() and not y.any()
        with pytest.raises(_lib.HipError):
            t.apply_device(x.ctypes.data, 1, x.ctypes.data)          # equal pointers


@pytest.mark.parametrize("cls", [H.HipPcaIvfFlatNearestNeighborsIndex, H.HipPcaIvfPqNearestNeighborsIndex])
def test_index_is_the_parent_index_over_projected_rows(cls):
    """After build, update and remove `nn_many` equals, in ids and bits, the parent's device index over apply(rows) at apply(q)."""
    x, q = C.index_case()
    descr = [DescriptorMemoryElement(i) for i in range(len(x))]
    for e, v in zip(descr, x):
        e.set_vector(v)
    index = cls(pca_dims=16, nlist=8, nprobe=3, train_iters=3, random_seed=4)

    def check():
        rows = np.vstack([e.vector() for e in index._elements]).astype(np.float32)
        with _lib.PcaTransform(index._pca_matrix, index._pca_mean) as t:
            base = _lib.IvfIndex(index._centroids) if cls is H.HipPcaIvfFlatNearestNeighborsIndex else \
                _lib.PqIndex(index._centroids, index._codebooks, residual=True)
            with base:
                base.add(t.apply(rows))
                want = base.search(t.apply(q), 10, 3)
        idx, dist = index.nn_many(q, 10)
        np.testing.assert_array_equal(idx, want[1])
        np.testing.assert_array_equal(dist.view(np.uint32), want[0].view(np.uint32))

    index.build_index(descr[:1000])
    sample = x[:1000][H.training_draws(1000, 8, 4)[0]]
    C.check_training_quality(index._pca_matrix, sample, index._pca_mean, _lib.pca_moments(sample)[1])
    check()
    index.update_index(descr[1000:])
    check()
    index.remove_from_index(list(range(10, 20)))
    assert index.count() == 1190
    check()
    elems, dists = index.nn(descr[30], 5)                              # re-ranked by the original vectors
    assert elems[0].uuid() == 30 and list(dists) == sorted(dists) and dists[0] == 0
    back = pickle.loads(pickle.dumps(index))
    assert np.array_equal(back._pca_matrix, index._pca_matrix) and back.get_config() == index.get_config()
    for got, want in zip(back.nn_many(q, 10), index.nn_many(q, 10)):
        np.testing.assert_array_equal(got, want)
