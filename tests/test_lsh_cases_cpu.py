"""
CPU tests of tests/lsh_cases.py, the case builder of tests/test_hip_lsh_composite.py: every parametrisation the GPU
tests use is built here, so the builder's conditions (bit margin of every pool query, bucket sizes, the descending-id
tie of the planted pair) are proven without a GPU and with no query left out; and the vectorised oracle is the
oracle's own `lsh_nn`, ids and distance bits.
"""
import numpy as np
import pytest

from oracle import cpu_ref as O
from tests import lsh_cases as L


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("name", [c[0] for c in L.ROUTE_CASES] + ["slab_320_bits/big"])
def test_builder_conditions_hold(name):
    big = name.endswith("/big")
    case = L.route_case(name.split("/")[0], L.BIG_CENTRES if big else L.N_CENTRES)    # asserts conditions 1 - 3
    n = case.db.shape[0]
    assert case.uniq.shape == (len(case.buckets), case.words) and case.pool.shape == (L.POOL, case.d)
    assert n > 16384 + 600 if big else 11_000 <= n <= 15_000
    # the map lists every row once, buckets in row order, codes ascending and unique
    assert np.array_equal(np.sort(case.order), np.arange(n)) and case.off[0] == 0 and case.off[-1] == n
    assert all(b == sorted(b) for b in case.buckets)
    # the specials: db[7] and a centre with copies are rows of the matrix, the zero row has company, the zero query
    # hashes into the zero row's bucket
    assert np.array_equal(case.pool[L.Q_ROW7], case.db[7]) and np.array_equal(case.pool[L.Q_CENTRE], case.db[case.centre_row])
    assert not case.db[case.zero_row].any() and not case.pool[L.Q_ZERO].any()
    assert np.array_equal(case.pool_codes[L.Q_ZERO], case.uniq[case.inv[case.zero_row]])
    assert len(case.buckets[case.inv[case.zero_row]]) >= 2
    # the pair: same distance bits from c, the later candidate has the lower id
    ids, dist = case.oracle(L.Q_PAIR, case.tie_m, "euclidean")
    assert _bits(dist)[0] == _bits(dist)[1] and ids[0] > ids[1] and set(ids[:2].tolist()) == set(case.pair_rows)
    # exact copies exist: the centre's answer starts with two or more zero distances, ascending ids (one bucket)
    ids, dist = case.oracle(L.Q_CENTRE, 1, "euclidean", k=3)
    assert dist[0] == 0 and ids[0] == min(case.buckets[case.inv[case.centre_row]])


@pytest.mark.parametrize("name", ["slab_100_bits", "narrow"])
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_fast_oracle_is_the_oracle(name, metric):
    case = L.route_case(name)
    for qi, m in ((L.Q_ROW7, 7), (L.Q_PAIR, 20), (9, 60)):
        ids, dist = O.lsh_nn(case.pool[qi], m, case.mean, case.rot, case.normalize, case.uniq, case.buckets, case.db, metric)
        fi, fd = L.lsh_nn_fast(case.pool[qi], m, case.mean, case.rot, case.normalize, case.uniq, case.buckets, case.db, metric)
        assert fd.dtype == dist.dtype
        np.testing.assert_array_equal(fi, ids)
        np.testing.assert_array_equal(_bits(fd), _bits(dist))
        ci, cd = case.oracle(qi, m, metric)                                 # the cached form, sliced
        np.testing.assert_array_equal(ci, ids)
        np.testing.assert_array_equal(_bits(cd), _bits(dist))
