"""ITQ codes of 257 to 1024 bits (5 to 16 words) on the GPU: the certified slab filter (sq_itq_xwide.hpp) hashes them in
column groups of 256 bits, one pass over the rows per group, instead of the all-float64 kernel (itq_filter_route in
sq_itq.hip).  The codes are the float64 kernel's to the last bit; codes up to 256 bits and beyond 1024 bits route as
before."""
import functools

import numpy as np
import pytest

from oracle import cpu_ref as O
from smqtk_indexing_amd import _lib
from smqtk_indexing_amd.impls.lsh_functor.hip_itq import HipItqFunctor

pytestmark = pytest.mark.gpu

N = 4129          # no multiple of 32: a partial last tile


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


def _rows(rng, n, d, dt):
    # as in test_hip_itq_any_width.py: normal rows scaled by U(0.1, 30)
    x = rng.standard_normal((n, d), dtype=np.float32)
    x *= rng.uniform(0.1, 30.0, (n, 1)).astype(np.float32)
    return x.astype(dt, copy=False)


def _groups(bits):
    return ((bits + 63) // 64 + 3) // 4     # passes over the rows: one per 4 code words


@functools.lru_cache(maxsize=4)
def _data(d, bits, dtname):
    x = _rows(np.random.default_rng(d + bits), N, d, np.dtype(dtname))
    x.setflags(write=False)
    return x, x[:2000].mean(axis=0).astype(np.float64), _rotation(d, bits, d + bits)


@functools.lru_cache(maxsize=64)
def _hashed(d, bits, dtname, ordv, mean32):
    """One shape through the resident model (twice), the float64 kernel and the one-shot call; shared by the tests."""
    x, mean, rot = _data(d, bits, dtname)
    if mean32:
        mean = mean.astype(np.float32)
    model = _lib.ItqModel(mean, rot, ordv)
    got = model.hash(x)
    st = model.stats()
    again = model.hash(x)                    # the model's cached image of the rotation serves the second call
    model.close()
    return got, st, again, _exact(x, mean, rot, ordv), _lib.itq_hash(x, mean, rot, ordv)


# (d, bits, dtype): every group count, every last-group CT, a non-zero pad
WIDE_CODE_SHAPES = [(512, 512, "float32"),      # 2 groups; a width that was the wide kernel's
                    (320, 300, "float32"),      # 5 words, pad 20, last group CT 2
                    (300, 257, "float64"),      # pad 63, off the 64 grid
                    (768, 448, "float64"),      # 7 words, last group CT 6
                    (4100, 640, "float32"),     # 3 groups, last CT 4, d beyond 512 and off the grid
                    (1000, 1000, "float32"),    # 16 words, pad 24
                    (2048, 1024, "float32")]    # 4 full groups
NORMS = [_lib.SQ_NORM_NONE, _lib.SQ_NORM_L2]
WIDE_CODE_CASES = [(d, bits, dt, ordv, False) for (d, bits, dt) in WIDE_CODE_SHAPES for ordv in NORMS] + \
                  [(512, 512, "float32", ordv, True) for ordv in NORMS] + [(320, 300, "float32", _lib.SQ_NORM_L2, True)]


# ---------------------------------------------------------------- 1. the filter runs
@pytest.mark.parametrize("d,bits,dtname,ordv,mean32", WIDE_CODE_CASES)
def test_itq_filter_hashes_codes_of_257_to_1024_bits(d, bits, dtname, ordv, mean32):
    """The model's statistics say which path hashed the rows: one filter pass per 256 bits of the code streamed them,
    no row went to the float64 kernel, and the codes are the float64 kernel's and the one-shot call's bit for bit.
    (Before the routing took these codes: scan_launches == 0, fallback_queries == n.)  mean32: a float32 model mean on
    float32 rows, the subtraction in the promoted dtype."""
    got, st, again, exact, oneshot = _hashed(d, bits, dtname, ordv, mean32)
    print(f"d={d} bits={bits} {dtname} norm={ordv} mean32={mean32}:", st)
    assert got.shape == (N, (bits + 63) // 64)
    np.testing.assert_array_equal(got, exact)
    np.testing.assert_array_equal(got, oneshot)
    np.testing.assert_array_equal(again, got)
    assert st["scan_launches"] >= 1
    assert st["scan_launches"] == _groups(bits)          # one launch per column group
    assert st["fallback_queries"] == 0
    assert st["bytes_scanned"] == N * d * np.dtype(dtname).itemsize * _groups(bits)


# ---------------------------------------------------------------- 2. the undecided share
@pytest.mark.parametrize("d,bits,dtname,ordv,mean32", [c for c in WIDE_CODE_CASES if c[2] == "float32"])
def test_itq_wide_codes_undecided_share(d, bits, dtname, ordv, mean32):
    """The cap the slab filter's tests hold on this generator at up to 256 bits.  The bound is per column and unchanged,
    so a larger share means a group read another group's error terms (the float64 kernel alone: candidates == 0)."""
    _, st, _, _, _ = _hashed(d, bits, dtname, ordv, mean32)
    print(f"d={d} bits={bits} norm={ordv} mean32={mean32}: undecided bits {st['candidates']} of {N * bits}")
    assert 0 <= st["candidates"] < 0.01 * N * bits


# ---------------------------------------------------------------- 3. the oracle
@pytest.mark.parametrize("d,bits,dtname", [(320, 300, "float32"), (768, 448, "float64")])
def test_itq_wide_codes_against_the_oracle(d, bits, dtname):
    """The first 200 rows against the oracle's get_hash one vector at a time (normalize=2): a row may differ only where
    it owns a bit with |z| < 1e-9."""
    x, mean, rot = _data(d, bits, dtname)
    got = _hashed(d, bits, dtname, _lib.SQ_NORM_L2, False)[0][:200]
    ref = np.stack([O.itq_get_hash(x[i], mean, rot, 2) for i in range(200)])
    bad = (got != O.pack_bits_msb(ref)).any(axis=1)
    print(f"d={d} bits={bits} {dtname}: rows off the oracle {int(bad.sum())}")
    if bad.any():
        z = O.itq_z(x[:200][bad], mean, rot, 2)
        assert np.abs(z).min(axis=1).max() < 1e-9
    assert bad.mean() < 1e-2


# ---------------------------------------------------------------- 4. edges inside groups
def test_itq_wide_codes_edge_rows():
    """512 -> 512 bits, float32: a zero row (norm replaced by 1), a row with an element of 7e4 (the range rule sends its
    tile's bits to float64 in every group), a NaN and an inf, and rows that are exact multiples of one rotation column
    of the second group -- under a zero mean the z of every other column is what rounding leaves, so those bits are
    the float64 kernel's order of summation or nothing."""
    d = bits = 512
    x, mean, rot = _data(d, bits, "float32")
    x = x.copy()
    rng = np.random.default_rng(7)
    x[3] = 0.0
    x[40, 100] = 7.0e4
    x[77, 5] = np.nan
    x[78, 300] = np.inf
    cols = rng.integers(256, 512, 64)
    t = (10.0 ** rng.uniform(-3, 3, 64)) * rng.choice([-1.0, 1.0], 64)
    x[1000:1064] = (t[:, None] * rot[:, cols].T).astype(np.float32)
    for mean_m in (mean, np.zeros(d)):
        for ordv in NORMS:
            model = _lib.ItqModel(mean_m, rot, ordv)
            with np.errstate(all="ignore"):
                got = model.hash(x)
            st = model.stats()
            model.close()
            print(f"zero mean={not mean_m.any()} norm={ordv}:", st)
            assert st["scan_launches"] >= 1 and st["fallback_queries"] == 0
            # the 7e4, NaN and inf rows' tiles (rows 32..63, 64..95): all 512 bits of 64 rows undecided
            assert st["candidates"] >= 64 * bits
            np.testing.assert_array_equal(got, _exact(x, mean_m, rot, ordv))


# ---------------------------------------------------------------- 5. small and device-resident
def test_itq_wide_codes_small_batches_and_device_rows():
    """33 and 32 rows take the filter (the window of the last tile moves back), 31 the float64 kernel.  The same rows
    as a device tensor on a torch stream: equal codes, and candidates == -1 (the call is asynchronous)."""
    import torch
    d = bits = 512
    x, mean, rot = _data(d, bits, "float32")
    full = _hashed(d, bits, "float32", _lib.SQ_NORM_L2, False)[0]
    model = _lib.ItqModel(mean, rot, _lib.SQ_NORM_L2)
    for n in (33, 32):
        np.testing.assert_array_equal(model.hash(x[:n]), full[:n])
        st = model.stats()
        assert st["scan_launches"] == _groups(bits) and st["fallback_queries"] == 0
    np.testing.assert_array_equal(model.hash(x[:31]), full[:31])
    st = model.stats()
    assert st["scan_launches"] == 0 and st["fallback_queries"] == 31
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        xd = torch.from_numpy(x.copy()).to(dev)
        out = torch.zeros((N, bits // 64), dtype=torch.int64, device=dev)
        assert xd.data_ptr() % 16 == 0
        model.hash_device(xd.data_ptr(), _lib.SQ_DTYPE_F32, N, out.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    st = model.stats()
    model.close()
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint64), full)
    assert st["candidates"] == -1
    assert st["scan_launches"] == _groups(bits) and st["fallback_queries"] == 0
    assert st["bytes_scanned"] == N * d * 4 * _groups(bits)


# ---------------------------------------------------------------- 6. what stays
def test_itq_codes_beyond_1024_bits_keep_the_float64_kernel():
    """17 words: the float64 kernel, as before."""
    n, d, bits = 2000, 2048, 1088
    x = _rows(np.random.default_rng(d + bits), n, d, np.float32)
    mean = x.mean(axis=0).astype(np.float64)
    rot = _rotation(d, bits, d + bits)
    model = _lib.ItqModel(mean, rot, _lib.SQ_NORM_L2)
    got = model.hash(x)
    st = model.stats()
    model.close()
    assert st["scan_launches"] == 0 and st["fallback_queries"] == n
    assert st["bytes_scanned"] == n * d * 4
    np.testing.assert_array_equal(got, _exact(x, mean, rot, _lib.SQ_NORM_L2))


def test_itq_256_bit_codes_keep_one_pass():
    """2048 -> 256 bits: one filter launch over the rows, as the existing test of that shape has it."""
    n, d, bits = 2000, 2048, 256
    x = _rows(np.random.default_rng(d + bits), n, d, np.float32)
    mean = x.mean(axis=0).astype(np.float64)
    rot = _rotation(d, bits, d + bits)
    model = _lib.ItqModel(mean, rot, _lib.SQ_NORM_L2)
    got = model.hash(x)
    st = model.stats()
    model.close()
    assert st["scan_launches"] == 1 and st["fallback_queries"] == 0
    assert st["bytes_scanned"] == n * d * 4
    np.testing.assert_array_equal(got, _exact(x, mean, rot, _lib.SQ_NORM_L2))


# ---------------------------------------------------------------- 7. through the plugin
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_itq_functor_hashes_512_bit_codes(dt):
    """HipItqFunctor(bit_length=512, normalize=2) over 3000 x 1024 rows: the filter ran, get_hash_packed against the
    oracle's get_hash one vector at a time on the first 300 rows (a row may differ only where it owns a bit with
    |z| < 1e-9), get_hash of one row is that row's 512 booleans."""
    n, d, bits, ncmp = 3000, 1024, 512, 300
    rng = np.random.default_rng(1024)
    x = _rows(rng, n, d, dt)
    f = HipItqFunctor(bit_length=bits, normalize=2)
    f.mean_vec = O.itq_norm_vector(x[:1000], 2).mean(axis=0).astype(np.float64)
    f.rotation = _rotation(d, bits, 17)
    got = f.get_hash_packed(x)
    st = f._device_model().stats()
    print(f"{np.dtype(dt).name}:", st)
    assert got.shape == (n, bits // 64)
    assert st["scan_launches"] >= 1 and st["fallback_queries"] == 0
    ref = np.stack([O.itq_get_hash(x[i], f.mean_vec, f.rotation, 2) for i in range(ncmp)])
    bad = (got[:ncmp] != O.pack_bits_msb(ref)).any(axis=1)
    print(f"{np.dtype(dt).name}: rows off the oracle {int(bad.sum())}")
    if bad.any():
        z = O.itq_z(x[:ncmp][bad], f.mean_vec, f.rotation, 2)
        assert np.abs(z).min(axis=1).max() < 1e-9
    assert bad.mean() < 1e-2
    one = f.get_hash(x[11])
    assert one.dtype == bool and one.shape == (bits,)
    np.testing.assert_array_equal(one, O.unpack_bits_msb(got[11:12], bits)[0])
