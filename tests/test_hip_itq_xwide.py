"""ITQ beyond 512 dimensions on the GPU: the extra-wide certified hash filter (sq_itq_xwide.hpp), the statistics of
an ITQ model handle, the device fit for 512 < d <= 8192, and the LSH pipeline over 2048-d descriptors."""
import functools

import numpy as np
import pytest

from oracle import cpu_ref as O
from smqtk_indexing_amd import _lib
from smqtk_indexing_amd.impls.lsh_functor.hip_itq import HipItqFunctor
from smqtk_indexing_amd.impls.nn_index.hip_lsh import HipLSHNearestNeighborIndex
from smqtk_indexing_amd.impls.hash_index.hip_linear import HipLinearHashIndex
from smqtk_indexing_amd._compat import DescriptorMemoryElement, MemoryDescriptorSet, MemoryKeyValueStore

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=4)
def _rotation(d, bits, seed):
    # orthonormal columns from the reduced QR of a d x bits normal matrix (a full 8192 x 8192 QR costs minutes)
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((d, bits)))
    return np.ascontiguousarray(q[:, :bits])


def _exact(x, mean, rot, ordv):
    _lib.set_option("itq_exact", 1)
    try:
        return _lib.itq_hash(x, mean, rot, ordv)
    finally:
        _lib.set_option("itq_exact", 0)


XWIDE_SHAPES = [(40_003, 1024, 256), (33, 2048, 128), (30_000, 4096, 64), (20_001, 4096, 256), (9_000, 8192, 200),
                (25_000, 1000, 100), (12_000, 4100, 33), (30_000, 576, 64)]
# (float64 rows of d % 4 == 2 are 16-byte aligned too: 514)
XWIDE_CASES = [(n, d, bits, dt) for (n, d, bits) in XWIDE_SHAPES for dt in (np.float32, np.float64)] + [(5_000, 514, 64, np.float64)]


@pytest.mark.parametrize("n,d,bits,dt", XWIDE_CASES)
def test_itq_xwide_filter_matches_float64_kernel(n, d, bits, dt):
    """The extra-wide filter (512 < d <= 8192, k blocked in slabs of 64, <= 256 bits, float32 AND float64 rows) returns
    exactly the codes of the all-float64 kernel, and both agree with the oracle: the reference's 2048-d / 4096-d CNN
    descriptors, widths that are no multiple of 64 (1000, 4100; 514 = float64 rows of d % 4 == 2), the smallest batch
    the filter takes, an all-undecided row, a zero row, a degenerate hash bit, both normalisations, both model dtypes."""
    rng = np.random.default_rng(n + d + bits)
    x = rng.standard_normal((n, d), dtype=np.float32)
    x *= rng.uniform(0.1, 30.0, (n, 1)).astype(np.float32)
    x = x.astype(dt, copy=False)
    mean = x[:2000].mean(axis=0).astype(np.float64)
    x[5] = mean.astype(dt)                  # z ~ 0 in every bit: the whole row is undecided
    x[7] = 0.0                              # zero row (norm 0 -> 1 with normalize=2)
    x[n - 1] = x[0]
    rot = _rotation(d, bits, d + bits).copy()
    rot[:, 3] = 0.0                         # a degenerate hash bit: z == -mean.R == 0 -> True everywhere
    for mean_m in (mean, mean.astype(np.float32)):
        for norm, ordv in ((None, _lib.SQ_NORM_NONE), (2, _lib.SQ_NORM_L2)):
            got = _lib.itq_hash(x, mean_m, rot, ordv)
            exact = _exact(x, mean_m, rot, ordv)
            np.testing.assert_array_equal(got, exact)
            z = O.itq_z(x, mean_m, rot, norm)
            ref = O.pack_bits_msb(z >= 0)
            bad = (got != ref).any(axis=1)
            print(f"n={n} d={d} bits={bits} {np.dtype(dt).name} norm={norm}: rows off the oracle {int(bad.sum())}")
            if bad.any():
                assert np.abs(z[bad]).min(axis=1).max() < 1e-9
            assert bad.mean() < 1e-2


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("n,d,bits", [(6_000, 2048, 128), (4_000, 4096, 256), (4_000, 1000, 100)])
def test_itq_xwide_filter_adversarial_rows(n, d, bits, dt):
    """Rows built so that many z land inside the filter's slack of 0: the mean plus tiny multiples of one rotation column
    (every other bit's z is what rounding leaves), rows of the scale 1e4 (beyond a float16 plane's range when an
    element passes 60000) and 1e-4 (float16 subnormals), zero rows under normalize=2, the mean itself.  The undecided
    path runs (the model's statistics say so) and the codes are still those of the float64 kernel, bit for bit.
    Against the oracle only the |z| < 1e-9 rule applies: by construction most rows here own such a bit."""
    rng = np.random.default_rng(d + bits)
    rot = _rotation(d, bits, d + bits)
    x = rng.standard_normal((n, d)).astype(dt)
    mean = (x[:1000].mean(axis=0) + 0.05).astype(np.float64)
    q = n // 4
    cols = rng.integers(0, bits, q)
    t = 10.0 ** rng.uniform(-7, -1, q)
    x[:q] = (mean[None, :] + t[:, None] * rot[:, cols].T).astype(dt)
    x[q:q + q // 2] *= dt(1e4)
    x[q + q // 2:2 * q] *= dt(1e-4)
    x[2 * q:2 * q + 40] = 0.0
    x[2 * q + 40] = mean.astype(dt)
    x[2 * q + 41] = 7.0e4                   # past the float16 range: the tile goes to float64 whole
    for mean_m in (mean, mean.astype(np.float32)):
        for norm, ordv in ((None, _lib.SQ_NORM_NONE), (2, _lib.SQ_NORM_L2)):
            model = _lib.ItqModel(mean_m, rot, ordv)
            got = model.hash(x)
            st = model.stats()
            model.close()
            assert st["scan_launches"] >= 1 and st["fallback_queries"] == 0 and st["candidates"] > 0
            np.testing.assert_array_equal(got, _lib.itq_hash(x, mean_m, rot, ordv))
            np.testing.assert_array_equal(got, _exact(x, mean_m, rot, ordv))
            z = O.itq_z(x, mean_m, rot, norm)
            bad = (got != O.pack_bits_msb(z >= 0)).any(axis=1)
            print(f"d={d} bits={bits} {np.dtype(dt).name} norm={norm}: undecided bits {st['candidates']} of {n * bits}, "
                  f"rows off the oracle {int(bad.sum())}")
            if bad.any():
                assert np.abs(z[bad]).min(axis=1).max() < 1e-9


def test_itq_model_stats_show_the_filter_ran():
    """sq_get_stats on an ITQ model handle: 30 000 x 4096 float32 rows stream through ONE filter kernel, no row goes to
    the float64 kernel, under 1 % of the bits stay undecided; with option itq_exact every row is a fallback row."""
    n, d, bits = 30_000, 4096, 256
    rng = np.random.default_rng(11)
    x = rng.standard_normal((n, d), dtype=np.float32)
    mean = x[:2000].mean(axis=0).astype(np.float64)
    rot = _rotation(d, bits, 5)
    model = _lib.ItqModel(mean, rot, _lib.SQ_NORM_L2)
    got = model.hash(x)
    st = model.stats()
    print("filter:", st)
    assert st["scan_launches"] >= 1 and st["fallback_queries"] == 0
    assert 0 <= st["candidates"] < 0.01 * n * bits
    assert st["bytes_scanned"] == n * d * 4
    again = model.hash(x)                   # the model's image of the rotation is reused, not rebuilt
    np.testing.assert_array_equal(again, got)
    model.set_option("itq_exact", 1)
    exact = model.hash(x)
    st = model.stats()
    print("itq_exact:", st)
    assert st["fallback_queries"] == n and st["scan_launches"] == 0 and st["candidates"] == 0
    np.testing.assert_array_equal(got, exact)
    one = model.hash(x[:1])                 # one query vector: fewer rows than any filter takes
    assert model.stats()["fallback_queries"] == 1
    np.testing.assert_array_equal(one, got[:1])
    model.close()
    with pytest.raises(RuntimeError):
        _lib.get_stats(12345)


FIT_SHAPES = [(6000, 1024, 64), (3000, 2304, 256), (2500, 4096, 128)]
# the functor comparison repeats numpy's general eigen-decomposition of the d x d covariance on both sides (tens of
# seconds at 4096): every combination at 1024, two at 2304, one at 4096
FIT_FUNCTOR_CASES = {(1024, "float32", None), (1024, "float32", 2), (1024, "float64", None), (1024, "float64", 2),
                     (2304, "float32", 2), (2304, "float64", None), (4096, "float32", 2)}


@pytest.mark.parametrize("normalize", [None, 2])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("n,d,bits", FIT_SHAPES)
def test_itq_fit_on_device_beyond_512_dimensions(n, d, bits, dt, normalize):
    """sq_itqfit_* for 512 < d <= 8192 (the projection stages its basis slice by slice: d * 8 columns stop fitting the
    LDS near d = 2300): mean / covariance / projection / per-iteration B^T V against numpy with the tolerances of
    test_itq_fit_on_device_matches_host, then the fitted model against the host fit (same seed)."""
    rng = np.random.default_rng(d + bits)
    basis = rng.standard_normal((d, d)) * np.linspace(3.0, 0.2, d)[None, :]
    x = (rng.standard_normal((n, d)) @ basis.T + rng.standard_normal(d) * 2.0).astype(dt)
    ordv = _lib.SQ_NORM_NONE if normalize is None else _lib.SQ_NORM_L2
    xn = O.itq_norm_vector(x, normalize)
    fit = _lib.ItqFit(x, ordv)
    np.testing.assert_allclose(fit.mean, xn.astype(np.float64).mean(axis=0), rtol=1e-6, atol=1e-7)
    mean = xn.mean(axis=0)
    fit.set_mean(mean)
    xc = xn.astype(np.float64) - mean.astype(np.float64)
    cov = fit.cov()
    ref_cov = np.cov(xc.T)
    np.testing.assert_allclose(cov, ref_cov, rtol=1e-5, atol=1e-6 * np.abs(cov).max())
    evals, evecs = np.linalg.eigh(ref_cov)
    pc = evecs[:, np.argsort(evals)[::-1][:bits]]
    fit.project(pc)
    v = xc @ pc
    r, _ = np.linalg.qr(rng.standard_normal((bits, bits)))
    c = fit.iterate(r)
    ref_c = np.where(v @ r >= 0, 1.0, -1.0).T @ v
    np.testing.assert_allclose(c, ref_c, rtol=1e-5, atol=1e-5 * np.abs(ref_c).max())
    fit.close()
    if (d, np.dtype(dt).name, normalize) not in FIT_FUNCTOR_CASES:
        return

    elems = [DescriptorMemoryElement(i).set_vector(row) for i, row in enumerate(x)]
    dev = HipItqFunctor(bit_length=bits, itq_iterations=15, normalize=normalize, random_seed=7)
    host = HipItqFunctor(bit_length=bits, itq_iterations=15, normalize=normalize, random_seed=7, fit_on_device=False)
    cd, ch = dev.fit(elems), host.fit(elems)
    assert dev.mean_vec.dtype == host.mean_vec.dtype
    np.testing.assert_allclose(dev.mean_vec, host.mean_vec, rtol=1e-4, atol=1e-5)

    def quant_error(f):
        z = O.itq_z(x, f.mean_vec, np.real(f.rotation), normalize)
        return np.linalg.norm(np.where(z >= 0, 1.0, -1.0) - z)

    assert abs(quant_error(dev) - quant_error(host)) <= 1e-2 * quant_error(host)
    assert cd.shape == ch.shape == (n, bits) and abs(cd.mean() - 0.5) < 0.05


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_itq_model_matches_one_shot_hash_at_2048(dt):
    """The resident model at d = 2048: single rows through the pinned path and a bulk batch give the one-shot call's
    codes."""
    rng = np.random.default_rng(3)
    n, d, bits = 5_000, 2048, 128
    x = rng.standard_normal((n, d)).astype(dt)
    mean = x[:1000].mean(axis=0)
    rot = _rotation(d, bits, 9)
    for ordv in (_lib.SQ_NORM_NONE, _lib.SQ_NORM_L2):
        want = _lib.itq_hash(x, mean, rot, ordv)
        model = _lib.ItqModel(mean, rot, ordv)
        np.testing.assert_array_equal(model.hash(x), want)
        assert model.stats()["scan_launches"] == 1
        for i in (0, 1, 4_999):
            np.testing.assert_array_equal(model.hash(x[i:i + 1]), want[i:i + 1])
        np.testing.assert_array_equal(model.hash(x[100:140]), want[100:140])
        model.close()


def test_lsh_index_over_2048_d_descriptors():
    """One HipLSHNearestNeighborIndex over 20 000 x 2048 descriptors: fitted on the device, hashed by the extra-wide
    filter, queried with device_rerank; the same index (the same model) built and queried with option itq_exact --
    every hash through the float64 kernel -- returns the same neighbours at the same distances."""
    rng = np.random.default_rng(21)
    n, d, bits = 20_000, 2048, 64
    centers = rng.standard_normal((50, d)).astype(np.float32) * 2
    x = centers[rng.integers(0, 50, n)] + rng.standard_normal((n, d), dtype=np.float32)
    elems = [DescriptorMemoryElement(i).set_vector(row) for i, row in enumerate(x)]
    f = HipItqFunctor(bit_length=bits, itq_iterations=10, normalize=2, random_seed=3)
    f.fit(elems)                            # on the device: d <= the library's limit

    def build(functor):
        idx = HipLSHNearestNeighborIndex(functor, MemoryDescriptorSet(), MemoryKeyValueStore(), HipLinearHashIndex(),
                                         distance_method="euclidean", device_rerank=True)
        idx.build_index(elems)
        return idx

    q = DescriptorMemoryElement("q")
    idx = build(f)
    got = []
    for i in range(8):
        q.set_vector(x[i * 97] + np.float32(0.01))
        r, dists = idx.nn(q, 10)
        got.append(([e.uuid() for e in r], list(dists)))
    f2 = HipItqFunctor(bit_length=bits, itq_iterations=10, normalize=2, random_seed=3)
    f2.mean_vec, f2.rotation = f.mean_vec, f.rotation
    _lib.set_option("itq_exact", 1)
    try:
        ref_idx = build(f2)
        for i in range(8):
            q.set_vector(x[i * 97] + np.float32(0.01))
            r, dists = ref_idx.nn(q, 10)
            assert ([e.uuid() for e in r], list(dists)) == got[i]
    finally:
        _lib.set_option("itq_exact", 0)
    assert all(len(u) == 10 for u, _ in got) and got[0][0][0] == 0
