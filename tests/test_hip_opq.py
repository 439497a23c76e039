"""
GPU tests of the OPQ transform and the index behind it (`sq_opq_*`, `_lib.OpqTransform`, impls/nn_index/hip_ivf_opq.py): the
transform against the float64 product within the derived bound of tests/opq_cases.py and nothing else, a permutation
matrix bit for bit; the index against a `PqIndex` over rows the transform wrote, in ids and float32 bits.
"""
import ctypes
import pickle

import numpy as np
import pytest
import torch

from smqtk_indexing_amd import _lib
from smqtk_indexing_amd._compat import DescriptorMemoryElement
from smqtk_indexing_amd.impls.nn_index import hip_ivf_opq as H
from tests import opq_cases as C
from tests import pq_cases

pytestmark = pytest.mark.gpu

GUARD = 64      # floats in front of and behind a device result
FILL = -7.5


def _within(y, x, a, what):
    y64, bound = C.reference(x, a)
    err = np.abs(y.astype(np.float64) - y64)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert (err <= bound).all(), f"{what}: element {worst} off by {err[worst]:.3e}, bound {bound[worst]:.3e}"


def _apply_device(t, x, shift):
    """The transform over rows in device memory, x and y starting `shift` floats into their allocations, y inside guards:
    (y, the guards)."""
    n, d = x.shape
    xd = torch.zeros(shift + n * d, dtype=torch.float32, device="cuda")
    xd[shift:] = torch.from_numpy(np.array(x)).cuda().reshape(-1)
    yd = torch.full((GUARD + shift + n * d + GUARD,), FILL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    t.apply_device(xd.data_ptr() + 4 * shift, n, yd.data_ptr() + 4 * (GUARD + shift))
    torch.cuda.synchronize()
    out = yd.cpu().numpy()
    lo, hi = GUARD + shift, GUARD + shift + n * d
    return out[lo:hi].reshape(n, d), np.concatenate([out[:lo], out[hi:]])


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("d", C.WIDTHS)
def test_transform_against_float64(d, kind):
    a = C.matrix(d, kind)
    with _lib.OpqTransform(a) as t:
        for n in C.ROWS:
            x = C.rows(n, d)
            _within(t.apply(x), x, a, f"d={d} {kind} n={n} host")
            assert t.info()["last_rows"] == n and t.stats()["bytes_scanned"] == n * d * 4
        for shift in (0, 1):        # 16-byte loads where d allows them; a base 4 bytes into the allocation: element by element
            y, guards = _apply_device(t, x, shift)
            _within(y, x, a, f"d={d} {kind} n={n} device shift={shift}")
            assert (guards == FILL).all(), f"d={d} shift={shift}: a write outside y"
        xd = torch.from_numpy(np.array(x)).cuda()
        t.apply_device(xd.data_ptr(), 0, 0)                            # n = 0: nothing is written, nothing is read
        assert t.info()["last_rows"] == 0


@pytest.mark.parametrize("d,n", [(35, C.ROWS[-1]), (128, C.ROWS[-1]), (516, C.ROWS[-1]), (1027, C.TILE + 1), (4, None)])
def test_permutation_moves_columns_exactly(d, n):
    """A[j][i] = (i == pi[j]): y[r][j] is x[r][pi[j]] bit for bit, so a tile, row or column mix-up is a wrong element.
    (4, None): twice the tiles of a full grid and five rows more -- every workgroup loops."""
    if n is None:
        n = 2 * _lib.device_name(0)[2] * C.BLOCKS_PER_CU * C.TILE + 5
    x = C.rows(n, d)
    with _lib.OpqTransform(C.permutation_matrix(d)) as t:
        np.testing.assert_array_equal(t.apply(x).view(np.uint32), x[:, C.permutation(d)].view(np.uint32))
        y, guards = _apply_device(t, x, 1)
        np.testing.assert_array_equal(y.view(np.uint32), x[:, C.permutation(d)].view(np.uint32))
        assert (guards == FILL).all()


def test_handles_of_other_kinds_are_refused():
    a = np.eye(8, dtype=np.float32)
    x, y = np.ones((1, 8), np.float32), np.zeros((1, 8), np.float32)
    with _lib.RefineStore(8, _lib.SQ_REFINE_F32) as store, _lib.OpqTransform(a) as t:
        assert _lib.load_opq().sq_opq_apply(store.handle, x.ctypes.data, 1, y.ctypes.data, 0, None) == -1
        assert b"unknown handle" in _lib.load().sq_last_error() and not y.any()
        assert _lib.load_refine().sq_refine_info(t.handle, (ctypes.c_int64 * 7)(), 7) == -1
        with pytest.raises(_lib.HipError):
            t.apply_device(x.ctypes.data, 1, x.ctypes.data)          # equal pointers


def _descriptors(vecs, first=0):
    out = [DescriptorMemoryElement(first + i) for i in range(len(vecs))]
    for e, v in zip(out, vecs):
        e.set_vector(v)
    return out


@pytest.mark.parametrize("nq", [1, 33])
@pytest.mark.parametrize("pq_mode", sorted(H.PQ_MODES))
def test_index_is_a_pq_index_over_transformed_rows(pq_mode, nq):
    """After build, update and remove: `nn_many` equals, in ids and distance bits, a PqIndex of the same mode, centroids and
    codebooks over Y = apply(R, X) searched with apply(R, Q).  A path that forgets the rotation, or applies it twice, differs."""
    case = pq_cases.make_case(*pq_cases.KSUB_SHAPE)
    x, q = case.x[:1200], np.ascontiguousarray(case.pool[:nq])
    descr = _descriptors(x)
    index = H.HipOpqIvfPqNearestNeighborsIndex(nlist=8, nprobe=3, m=case.m, pq_mode=pq_mode, opq_iters=2, train_iters=3, random_seed=4)

    def check():
        rows = np.vstack([e.vector() for e in index._elements]).astype(np.float32)
        residual, packed = H.PQ_MODES[pq_mode]
        with _lib.OpqTransform(index._rotation) as t, \
                _lib.PqIndex(index._centroids, index._codebooks, residual=residual, packed=packed) as base:
            base.add(t.apply(rows))
            want = base.search(t.apply(q), 10, 3)
        idx, dist = index.nn_many(q, 10)
        np.testing.assert_array_equal(idx, want[1])
        np.testing.assert_array_equal(dist.view(np.uint32), want[0].view(np.uint32))

    index.build_index(descr[:1000])
    r = index._rotation.astype(np.float64)
    assert np.abs(r @ r.T - np.eye(case.d)).max() <= case.d * 2.0 ** -23 and not np.array_equal(index._rotation, np.eye(case.d, dtype=np.float32))
    check()
    index.update_index(descr[1000:])
    check()
    index.remove_from_index(list(range(10, 20)))
    assert index.count() == 1190
    check()
    if nq == 1:
        elems, dists = index.nn(descr[30], 5)                          # re-ranked by the original vectors
        assert elems[0].uuid() == 30 and list(dists) == sorted(dists) and dists[0] == 0
        back = pickle.loads(pickle.dumps(index))
        assert np.array_equal(back._rotation, index._rotation) and back.get_config() == index.get_config()
        for got, want in zip(back.nn_many(q, 10), index.nn_many(q, 10)):
            np.testing.assert_array_equal(got, want)


def test_training_lowers_the_reconstruction_error():
    """The product-structure case of tests/opq_cases.py: after opq_iters iterations the sample's mean squared
    reconstruction error under the trained R is below that of the same training budget under R = I, and R is orthonormal.
    (The numpy restatement's two values: tests/test_host_logic_opq.py.)"""
    x, entries = C.make_training_case()

    def budget_mse(r):
        with _lib.OpqTransform(r) as t:
            y = t.apply(x)
        books = _lib.pq_train(y, C.start_books(y, entries, C.T_M), C.T_BUDGET)
        with _lib.PqIndex(np.zeros((1, C.T_D), np.float32), books) as coder:
            coder.add(y)
            codes = coder.lists()[2]
        return C.mse(y, books, codes)

    r = H.train_rotation(x, entries, C.T_M, H.initial_rotation(np.random.RandomState(0), C.T_D), C.T_ITERS)
    r64 = r.astype(np.float64)
    assert np.abs(r64 @ r64.T - np.eye(C.T_D)).max() <= C.T_D * 2.0 ** -23
    trained, plain = budget_mse(r), budget_mse(np.eye(C.T_D, dtype=np.float32))
    print(f"mse under the trained R {trained:.4f}, under R = I {plain:.4f}")
    assert trained < plain
