"""ITQ on the GPU for descriptor widths that are no multiple of 64 (100, 200, 300, 500 ...): up to 512 elements they
are hashed by the certified slab filter (sq_itq_xwide.hpp, routed by itq_filter_route in sq_itq.hip) instead of the
all-float64 kernel.  The rule under test: a float32 / float64 row of up to 8192 elements that is a whole number of
16-byte pieces goes through a filter, and the codes are the float64 kernel's to the last bit."""
import functools

import numpy as np
import pytest

from oracle import cpu_ref as O
from smqtk_indexing_amd import _lib
from smqtk_indexing_amd.impls.lsh_functor.hip_itq import HipItqFunctor

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=16)
def _rotation(d, bits, seed):
    # orthonormal columns from the reduced QR of a d x bits normal matrix (bits <= d in every case here)
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((d, bits)))
    return np.ascontiguousarray(q[:, :bits])


def _exact(x, mean, rot, ordv):
    _lib.set_option("itq_exact", 1)
    try:
        return _lib.itq_hash(x, mean, rot, ordv)
    finally:
        _lib.set_option("itq_exact", 0)


def _whole_pieces(d, dt):
    return (d * np.dtype(dt).itemsize) % 16 == 0


def _rows(rng, n, d, dt):
    # as in test_hip_itq_xwide.py: normal rows scaled by U(0.1, 30)
    x = rng.standard_normal((n, d), dtype=np.float32)
    x *= rng.uniform(0.1, 30.0, (n, 1)).astype(np.float32)
    return x.astype(dt, copy=False)


# ---------------------------------------------------------------- a. the filter runs
@pytest.mark.parametrize("d,bits,dt", [(100, 64, np.float32), (300, 128, np.float32), (500, 256, np.float64),
                                       (36, 33, np.float32)])
def test_itq_filter_runs_at_widths_off_the_64_grid(d, bits, dt):
    """The model's statistics say which path hashed the rows: one filter launch streamed them, no row went to the
    float64 kernel.  (Before the routing took these widths: fallback_queries == n, scan_launches == 0.)"""
    n = 4129
    rng = np.random.default_rng(d + bits)
    x = _rows(rng, n, d, dt)
    mean = x[:2000].mean(axis=0).astype(np.float64)
    rot = _rotation(d, bits, d + bits)
    model = _lib.ItqModel(mean, rot, _lib.SQ_NORM_L2)
    got = model.hash(x)
    st = model.stats()
    print(f"d={d} bits={bits} {np.dtype(dt).name}:", st)
    assert st["scan_launches"] >= 1
    assert st["fallback_queries"] == 0
    assert st["bytes_scanned"] == n * d * np.dtype(dt).itemsize
    again = model.hash(x)                    # the model's cached image of the rotation serves the second call
    model.close()
    np.testing.assert_array_equal(again, got)
    np.testing.assert_array_equal(got, _exact(x, mean, rot, _lib.SQ_NORM_L2))


# ---------------------------------------------------------------- b. the codes are the float64 kernel's
ANY_SHAPES = [(4129, 4, 3), (4129, 36, 33), (4129, 100, 64), (4129, 300, 128), (2081, 260, 100), (2081, 500, 256),
              (33, 300, 64), (32, 100, 64)]
ANY_CASES = [(n, d, bits, dt) for (n, d, bits) in ANY_SHAPES for dt in (np.float32, np.float64) if _whole_pieces(d, dt)]


@pytest.mark.parametrize("n,d,bits,dt", ANY_CASES)
def test_itq_any_width_codes_match_float64_kernel(n, d, bits, dt):
    """Bit for bit the float64 kernel's codes, and the oracle's wherever z is not a rounding error away from 0.
    n = 4129 / 2081: a ragged last tile; 33 / 32: the shifted window and the smallest batch a filter takes; d = 260:
    one 16-byte piece past a whole 256-k block; d = 4: a row shorter than one k-step; bits = 33, 3, 100: padded code
    words.  Planted: the mean itself (every bit undecided), a zero row, a duplicate, a degenerate hash bit."""
    rng = np.random.default_rng(n + d + bits)
    x = _rows(rng, n, d, dt)
    mean = x[:2000].mean(axis=0).astype(np.float64)
    x[5] = mean.astype(dt)                  # z ~ 0 in every bit: the whole row is undecided
    x[7] = 0.0                              # zero row (norm 0 -> 1 with normalize=2)
    x[n - 1] = x[0]
    rot = _rotation(d, bits, d + bits).copy()
    if bits > 3:
        rot[:, 3] = 0.0                     # a degenerate hash bit: z == -mean.R == 0 -> True everywhere
    for mean_m in (mean, mean.astype(np.float32)):
        for norm, ordv in ((None, _lib.SQ_NORM_NONE), (2, _lib.SQ_NORM_L2)):
            got = _lib.itq_hash(x, mean_m, rot, ordv)
            exact = _exact(x, mean_m, rot, ordv)
            np.testing.assert_array_equal(got, exact)
            z = O.itq_z(x, mean_m, rot, norm)
            bad = (got != O.pack_bits_msb(z >= 0)).any(axis=1)
            print(f"n={n} d={d} bits={bits} {np.dtype(dt).name} norm={norm} mean {mean_m.dtype}: "
                  f"rows off the oracle {int(bad.sum())}")
            if bad.any():
                assert np.abs(z[bad]).min(axis=1).max() < 1e-9
            if n >= 2000:
                # with this data only the planted row 5 owns a bit with |z| < 1e-9: at most 1 of 2081 = 4.8e-4
                assert bad.mean() < 1e-2


# ---------------------------------------------------------------- c. the end of the buffer
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("d", [100, 300, 500])
def test_itq_any_width_rows_at_the_end_of_the_buffer(d, dt):
    """The last 16-byte pieces of a row's last slab lie beyond the row.  They must neither be read into the fragments
    nor into |x|^2 / max |x_k|: NaN and 7e4 neighbours would change the norm and trip the range rule (every bit of the
    tile to float64, visible in `candidates`), or change codes outright.  Host: the matrix is the tail slice of a
    larger array.  Device: the rows are the last bytes of a tensor, compared with the same rows placed mid-tensor
    between NaN and 7e4."""
    import torch
    n, bits = 1057, 64
    isz = np.dtype(dt).itemsize
    rng = np.random.default_rng(d)
    rot = _rotation(d, bits, d + 1)
    pre = 37
    big = np.full((pre + n, d), np.nan, dtype=dt)
    big[:pre:2] = 7.0e4
    big[pre:] = _rows(rng, n, d, dt)
    x = big[pre:]                            # ends where the array ends
    mean = x[:500].mean(axis=0).astype(np.float64)
    mid = np.concatenate([np.full((3, d), np.nan, dtype=dt), x, np.full((3, d), 7.0e4, dtype=dt)])[3:3 + n]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    code = _lib.SQ_DTYPE_F32 if dt == np.float32 else _lib.SQ_DTYPE_F64
    mean_d = torch.from_numpy(mean).to(dev)
    rot_d = torch.from_numpy(rot).to(dev)
    words = (bits + 63) // 64
    nbytes = n * d * isz
    for norm_name, ordv in (("None", _lib.SQ_NORM_NONE), ("2", _lib.SQ_NORM_L2)):
        exact = _exact(x, mean, rot, ordv)
        # host rows: the one-shot call and the resident model (its device copy is as long as the rows)
        np.testing.assert_array_equal(_lib.itq_hash(x, mean, rot, ordv), exact)
        model = _lib.ItqModel(mean, rot, ordv)
        got = model.hash(x)
        st_tail = model.stats()
        got_mid = model.hash(mid)
        st_mid = model.stats()
        model.close()
        np.testing.assert_array_equal(got, exact)
        np.testing.assert_array_equal(got_mid, exact)
        assert st_tail["fallback_queries"] == 0 and st_tail["candidates"] == st_mid["candidates"]
        assert st_tail["candidates"] < 0.01 * n * bits      # (no tile tripped the range rule)
        # device rows: the last bytes of a 20 MiB tensor (what torch's allocator hands out as one whole block) ...
        total = 20 << 20
        buf = torch.full((total // isz,), float("nan"), dtype=torch.float32 if isz == 4 else torch.float64, device=dev)
        tail = buf[total // isz - n * d:]
        tail.copy_(torch.from_numpy(np.ascontiguousarray(x)).reshape(-1))
        assert tail.data_ptr() + nbytes == buf.data_ptr() + total and tail.data_ptr() % 16 == 0
        out_tail = torch.zeros((n, words), dtype=torch.int64, device=dev)
        _lib.itq_hash_device(tail.data_ptr(), code, n, d, mean_d.data_ptr(), rot_d.data_ptr(), bits, ordv,
                             out_tail.data_ptr(), stream)
        # ... and the same rows mid-tensor: NaN before, 7e4 after
        buf2 = torch.full(((n + 64) * d,), float("nan"), dtype=buf.dtype, device=dev)
        buf2[(32 + n) * d:] = 7.0e4
        midt = buf2[32 * d:(32 + n) * d]
        midt.copy_(tail)
        out_mid = torch.zeros((n, words), dtype=torch.int64, device=dev)
        _lib.itq_hash_device(midt.data_ptr(), code, n, d, mean_d.data_ptr(), rot_d.data_ptr(), bits, ordv,
                             out_mid.data_ptr(), stream)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out_tail.cpu().numpy().view(np.uint64), exact)
        np.testing.assert_array_equal(out_mid.cpu().numpy().view(np.uint64), exact)
        assert bool(torch.isnan(buf[:16]).all()) and float(buf2[-1]) == 7.0e4   # the neighbours are untouched
        print(f"d={d} {np.dtype(dt).name} norm={norm_name}: undecided bits {st_tail['candidates']} of {n * bits}")
        del buf, buf2


# ---------------------------------------------------------------- d. adversarial rows
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("n,d,bits", [(6_000, 300, 128), (4_000, 500, 256)])
def test_itq_any_width_adversarial_rows(n, d, bits, dt):
    """test_itq_xwide_filter_adversarial_rows at 300 and 500 elements: the mean plus tiny multiples of one rotation
    column, rows of the scale 1e4 and 1e-4, zero rows, the mean itself, one row of 7e4.  The undecided path runs and
    the codes are still the float64 kernel's; against the oracle only the |z| < 1e-9 rule applies."""
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
    x[2 * q + 41] = 0.0
    x[2 * q + 41, d // 2] = 7.0e4           # one element past the float16 range: the tile goes to float64 whole
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


# ---------------------------------------------------------------- e. the shapes that had a filter keep it
@pytest.mark.parametrize("n,d,bits", [(20_000, 128, 64), (8_000, 512, 256), (8_000, 1000, 64)])
def test_itq_routing_of_filtered_shapes_is_unchanged(n, d, bits):
    """The narrow (128 -> 64 bits), wide (512 -> 256 bits) and extra-wide (1000 -> 64 bits) float32 shapes: one filter
    launch, no fallback row, the float64 kernel's codes -- as before the routing changed."""
    rng = np.random.default_rng(d + bits)
    x = _rows(rng, n, d, np.float32)
    mean = x[:2000].mean(axis=0).astype(np.float64)
    rot = _rotation(d, bits, d + bits)
    for ordv in (_lib.SQ_NORM_NONE, _lib.SQ_NORM_L2):
        model = _lib.ItqModel(mean, rot, ordv)
        got = model.hash(x)
        st = model.stats()
        model.close()
        print(f"d={d} bits={bits}:", st)
        assert st["scan_launches"] == 1 and st["fallback_queries"] == 0
        assert 0 <= st["candidates"] < 0.01 * n * bits
        np.testing.assert_array_equal(got, _exact(x, mean, rot, ordv))


def test_itq_rows_off_the_16_byte_grid_keep_the_float64_kernel():
    """What stays outside the rule: 50 float32 elements are 200 bytes, no whole number of 16-byte pieces; fewer than
    32 rows; option itq_exact.  All of it is hashed by the float64 kernel, as before."""
    n, bits = 4129, 64
    rng = np.random.default_rng(50)
    for d, dt in ((50, np.float32), (101, np.float64)):
        x = _rows(rng, n, d, dt)
        mean = x[:2000].mean(axis=0).astype(np.float64)
        rot = _rotation(d, min(bits, d), d)
        model = _lib.ItqModel(mean, rot, _lib.SQ_NORM_L2)
        got = model.hash(x)
        st = model.stats()
        model.close()
        assert st["scan_launches"] == 0 and st["fallback_queries"] == n
        np.testing.assert_array_equal(got, _exact(x, mean, rot, _lib.SQ_NORM_L2))
    x = _rows(rng, n, 100, np.float32)
    mean = x[:2000].mean(axis=0).astype(np.float64)
    rot = _rotation(100, bits, 100)
    model = _lib.ItqModel(mean, rot, _lib.SQ_NORM_NONE)
    full = model.hash(x)
    np.testing.assert_array_equal(model.hash(x[:31]), full[:31])
    assert model.stats()["fallback_queries"] == 31 and model.stats()["scan_launches"] == 0
    model.set_option("itq_exact", 1)
    np.testing.assert_array_equal(model.hash(x), full)
    assert model.stats()["fallback_queries"] == n and model.stats()["scan_launches"] == 0
    model.close()


def test_itq_model_second_call_and_misaligned_device_rows():
    """Two per-call decisions at the smallest slab shape (4129 x 100 -> 64 bits).  A second call on one model runs on
    the image of the rotation the first call left on the handle: the same codes AND the same statistics (the count of
    undecided bits moves with any change of that image or of the error bound).  Device rows whose pointer is advanced
    by one element are not 16-byte aligned: the float64 kernel hashes them, to the same codes."""
    import torch
    n, d, bits = 4129, 100, 64
    rng = np.random.default_rng(d + bits + 1)
    x = _rows(rng, n, d, np.float32)
    mean = x[:2000].mean(axis=0).astype(np.float64)
    rot = _rotation(d, bits, d + bits)
    model = _lib.ItqModel(mean, rot, _lib.SQ_NORM_L2)
    first, st_first = model.hash(x), model.stats()
    second, st_second = model.hash(x), model.stats()
    print("first:", st_first, "second:", st_second)
    assert st_first["scan_launches"] == 1 and st_first["fallback_queries"] == 0 and st_first["candidates"] > 0
    assert st_second == st_first
    np.testing.assert_array_equal(second, first)
    np.testing.assert_array_equal(first, _exact(x, mean, rot, _lib.SQ_NORM_L2))
    dev = torch.device("cuda", 0)
    flat = torch.zeros(n * d + 1, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    for shift, launches, fallback in ((0, 1, 0), (1, 0, n)):
        rows = flat[shift:shift + n * d]
        rows.copy_(torch.from_numpy(x.reshape(-1)))
        assert rows.data_ptr() % 16 == 4 * shift
        out = torch.zeros((n, 1), dtype=torch.int64, device=dev)
        model.hash_device(rows.data_ptr(), _lib.SQ_DTYPE_F32, n, out.data_ptr(), stream)
        torch.cuda.synchronize()
        st = model.stats()
        assert st["scan_launches"] == launches and st["fallback_queries"] == fallback, (shift, st)
        np.testing.assert_array_equal(out.cpu().numpy().view(np.uint64), first)
    model.close()


# ---------------------------------------------------------------- f. through the plugin
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_itq_functor_hashes_300_d_descriptors(dt):
    """HipItqFunctor.get_hash_packed over 3000 x 300 rows, normalize=2, against the oracle's get_hash one vector at a
    time: a row may differ only where it owns a bit with |z| < 1e-9."""
    n, d, bits = 3000, 300, 64
    rng = np.random.default_rng(300)
    x = _rows(rng, n, d, dt)
    f = HipItqFunctor(bit_length=bits, normalize=2)
    f.mean_vec = O.itq_norm_vector(x[:1000], 2).mean(axis=0).astype(np.float64)
    f.rotation = _rotation(d, bits, 17)
    got = f.get_hash_packed(x)
    st = f._device_model().stats()
    assert st["scan_launches"] >= 1 and st["fallback_queries"] == 0
    ref = np.stack([O.itq_get_hash(x[i], f.mean_vec, f.rotation, 2) for i in range(n)])
    bad = (got != O.pack_bits_msb(ref)).any(axis=1)
    print(f"{np.dtype(dt).name}: rows off the oracle {int(bad.sum())}")
    if bad.any():
        z = O.itq_z(x[bad], f.mean_vec, f.rotation, 2)
        assert np.abs(z).min(axis=1).max() < 1e-9
    assert bad.mean() < 1e-2
    np.testing.assert_array_equal(O.unpack_bits_msb(got[:5], bits), np.stack([f.get_hash(x[i]) for i in range(5)]))
