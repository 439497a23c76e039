"""
GPU tests of the Hamming search at every code width up to 1024 bits: the register kernels for 3 and 5 .. 16 words, the
three-launch call and the LDS-DMA ring for 3, 5, 6 and 7 words, and `HammingIndex.plan`, the read-only view of what a
call would do.  Everything goes through `_lib.HammingIndex` (or the plugins on top of it) and is compared with
`oracle.cpu_ref.hamming_topk` / `lsh_nn`: distances are integers, so equality is the only tolerance.
"""
import bisect
import functools

import numpy as np
import pytest

from oracle import cpu_ref as O
from smqtk_indexing_amd import _lib
from smqtk_indexing_amd._compat import DescriptorMemoryElement, MemoryDescriptorSet, MemoryKeyValueStore
from smqtk_indexing_amd.impls.hash_index.hip_linear import HipLinearHashIndex
from smqtk_indexing_amd.impls.lsh_functor.hip_itq import HipItqFunctor
from smqtk_indexing_amd.impls.nn_index.hip_lsh import HipLSHNearestNeighborIndex
from tests.golden import inputs as GI

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

STREAM_NONE, STREAM_REGISTER, STREAM_RING = 0, 1, 2
CHAIN_ALL_KEYS, CHAIN_GENERAL, CHAIN_THREE_LAUNCH = 0, 1, 2


@functools.lru_cache(maxsize=4)
def _case(w, n, nq_max, seed):
    """Unique random codes (sorted: row id = rank) and a pool of queries; queries[0] is a stored code."""
    rng = np.random.default_rng(seed)
    codes = np.unique(rng.integers(0, 2 ** 64, size=(n, w), dtype=np.uint64), axis=0)
    pool = rng.integers(0, 2 ** 64, size=(nq_max, w), dtype=np.uint64)
    pool[0] = codes[len(codes) // 3]
    codes.setflags(write=False)
    pool.setflags(write=False)
    return codes, pool


def _queries(codes, pool, nq):
    q = pool[:nq].copy()
    q[-1] = codes[-1]                   # the last code: the guarded tail of every kernel
    if nq > 1:
        q[0] = pool[0]
    return q


@functools.lru_cache(maxsize=64)
def _oracle_cached(w, n, nq_max, seed, nq, k):
    codes, pool = _case(w, n, nq_max, seed)
    q = _queries(codes, pool, nq)
    out = [O.hamming_topk(codes, row, k) for row in q]
    return np.stack([d for d, _ in out]), np.stack([i for _, i in out])


def _oracle(codes, queries, k):
    out = [O.hamming_topk(codes, row, k) for row in queries]
    return np.stack([d for d, _ in out]), np.stack([i for _, i in out])


def _insert_positions(codes, new):
    keys = [tuple(r) for r in codes.tolist()]
    return np.array([bisect.bisect_left(keys, tuple(r)) for r in new.tolist()], dtype=np.int64)


def _fresh(rng, codes, m, w):
    """m sorted unique codes none of which is in `codes`."""
    new = np.unique(rng.integers(0, 2 ** 64, size=(m, w), dtype=np.uint64), axis=0)
    have = {tuple(r) for r in codes.tolist()}
    return new[[tuple(r) not in have for r in new.tolist()]]


# ------------------------------------------------------------------------------------ 1. every width, every chain
_WIDTH_CASES = [(w, nq) for w in (3, 5, 6, 7, 9, 12, 15) for nq in (1, 9, 33, 70)] + [(8, 70), (16, 70)]


@pytest.mark.parametrize("w,nq", _WIDTH_CASES)
def test_every_width_every_chain_matches_oracle(w, nq):
    """Ring automatic / off / forced times three-launch off / on, k = 1 and 100: the oracle's distances and ids, no
    query on the exact path, and a mini-list stream (register or ring) behind every one of them -- never the atomic
    scan with global counters, which is what these widths took before."""
    n, seed = 70_001, 4000 + w
    codes, pool = _case(w, n, 70, seed)
    queries = _queries(codes, pool, nq)
    idx = _lib.HammingIndex(codes, id_base=7)
    try:
        for k in (1, 100):
            rd, ri = _oracle_cached(w, n, 70, seed, nq, k)
            for ring in (-1, 0, 1):
                for fused in (0, 1):
                    idx.set_option("hamming_ring", ring)
                    idx.set_option("hamming_fused", fused)
                    plan = idx.plan(nq, k)
                    d, i = idx.search(queries, k)
                    what = f"W={w} nq={nq} k={k} ring={ring} fused={fused} plan={plan}"
                    np.testing.assert_array_equal(d, rd, err_msg=what)
                    np.testing.assert_array_equal(i, ri + 7, err_msg=what)
                    assert idx.stats()["fallback_queries"] == 0, what
                    assert plan["stream"] != STREAM_NONE, what
                    assert plan["chain"] != CHAIN_ALL_KEYS, what
    finally:
        idx.close()


def test_plan_reports_the_routing_rules():
    """The plan of a few shapes whose routing the rules fix: three launches up to 7 words only, the ring for 3, 5, 6, 7
    when forced, 8 words beyond one ring launch's 64 queries on the register stream, the all-keys chain of a small
    array, and the same answer for a pipelined call."""
    rng = np.random.default_rng(12)
    for w, nq, ring, want_chain, want_stream in [(3, 4, -1, CHAIN_THREE_LAUNCH, STREAM_REGISTER), (7, 4, 1, CHAIN_THREE_LAUNCH, STREAM_RING),
                                                 (6, 100, 1, CHAIN_GENERAL, STREAM_RING), (8, 4, -1, CHAIN_GENERAL, STREAM_RING),
                                                 (8, 65, -1, CHAIN_GENERAL, STREAM_REGISTER), (8, 4, 0, CHAIN_GENERAL, STREAM_REGISTER),
                                                 (12, 4, 1, CHAIN_GENERAL, STREAM_REGISTER), (16, 64, -1, CHAIN_GENERAL, STREAM_RING)]:
        codes = np.unique(rng.integers(0, 2 ** 64, size=(70_001, w), dtype=np.uint64), axis=0)
        idx = _lib.HammingIndex(codes)
        idx.set_option("hamming_ring", ring)
        p = idx.plan(nq, 10)
        assert (p["chain"], p["stream"]) == (want_chain, want_stream), (w, nq, ring, p)
        assert p["workgroups"] > 0 and p["slots"] >= 32 and p["sample_step"] >= 1 and p["candidate_cap"] == 65536
        assert p["queries_per_launch"] == (64 if want_stream == STREAM_RING else 2048 // w if w > 5 else 384)
        assert p["thresholds_in_stream"] == (1 if want_chain == CHAIN_THREE_LAUNCH and want_stream == STREAM_REGISTER else 0)
        assert idx.plan(nq, 10, async_=True)["chain"] == want_chain
        assert idx.plan(3, 70_001)["chain"] == CHAIN_ALL_KEYS        # cap = 2 k >= n
        idx.close()


# ------------------------------------------------------------------------------------ 2. the bet, at the new widths
@pytest.mark.parametrize("w,nq", [(w, nq) for w in (3, 5, 6, 7) for nq in (1, 17, 32)])
def test_tightened_threshold_at_the_new_widths(w, nq):
    """The sequence of test_hamming_fused_small_batch_matches_oracle on 192 .. 448-bit codes: three identical calls, the
    tightened threshold admits strictly fewer candidates than the safe one, a lost bet (hamming_tighten = 2) redoes the
    call and counts every query, and the general chain answers the same.  k = 2048 is the three-launch call's limit:
    its sample is the whole array (sample step 1), the rank rule r = k / step + 7 sqrt(k / step) + 6 is then beyond k
    and the bet is not taken -- both settings admit exactly the same candidates there (the test below takes the bet at
    k = 2048 over a larger array).  k = 2049 is not fused."""
    n, seed = 150_017, 5000 + w
    codes, pool = _case(w, n, 32, seed)
    queries = _queries(codes, pool, nq)
    idx = _lib.HammingIndex(codes, id_base=7)
    try:
        for k in (100, 2048, 2049):
            idx.set_option("hamming_fused", 1)
            idx.set_option("hamming_tighten", 1)
            rd, ri = _oracle_cached(w, n, 32, seed, nq, k)
            plan = idx.plan(nq, k)
            assert plan["chain"] == (CHAIN_THREE_LAUNCH if k <= 2048 else CHAIN_GENERAL), plan
            for rep in range(3):
                d, i = idx.search(queries, k)
                assert idx.stats()["fallback_queries"] == 0
                np.testing.assert_array_equal(d, rd)
                np.testing.assert_array_equal(i, ri + 7)
            cands_bet = idx.stats()["candidates"]
            idx.set_option("hamming_tighten", 0)
            d1, i1 = idx.search(queries, k)
            np.testing.assert_array_equal(d1, rd)
            np.testing.assert_array_equal(i1, ri + 7)
            cands_safe = idx.stats()["candidates"]
            print(f"W={w} nq={nq} k={k}: candidates tightened {cands_bet}, safe {cands_safe}, plan {plan}")
            if k == 100:
                assert cands_bet < cands_safe
            else:
                assert plan["sample_step"] == 1 and cands_bet == cands_safe
            idx.set_option("hamming_tighten", 2)
            d2, i2 = idx.search(queries, k)
            np.testing.assert_array_equal(d2, rd)
            np.testing.assert_array_equal(i2, ri + 7)
            assert idx.stats()["fallback_queries"] == (nq if k <= 2048 else 0)
            idx.set_option("hamming_tighten", 1)
            idx.set_option("hamming_fused", 0)
            d3, i3 = idx.search(queries, k)
            np.testing.assert_array_equal(d3, rd)
            np.testing.assert_array_equal(i3, ri + 7)
            assert idx.stats()["candidates"] == cands_safe      # the general chain: the safe threshold's mini-lists
    finally:
        idx.close()


@pytest.mark.parametrize("w,nq", [(w, nq) for w in (3, 5, 6, 7) for nq in (1, 32)])
def test_tightened_threshold_at_k_2048_over_a_larger_array(w, nq):
    """k = 2048 with the bet taken: at n = 300 001 the sample is every second block (step 2), the rank rule gives
    r = 1024 + 7 sqrt(1024) + 6 = 1254 < k, and the tightened threshold admits strictly fewer candidates than the safe
    one; the lost bet (hamming_tighten = 2) redoes the call and counts every query."""
    n, seed, k = 300_001, 5100 + w, 2048
    codes, pool = _case(w, n, 32, seed)
    queries = _queries(codes, pool, nq)
    rd, ri = _oracle_cached(w, n, 32, seed, nq, k)
    idx = _lib.HammingIndex(codes, id_base=7)
    try:
        plan = idx.plan(nq, k)
        assert plan["chain"] == CHAIN_THREE_LAUNCH and plan["sample_step"] == 2, plan
        cands = {}
        for tighten in (1, 0, 2):
            idx.set_option("hamming_tighten", tighten)
            d, i = idx.search(queries, k)
            np.testing.assert_array_equal(d, rd)
            np.testing.assert_array_equal(i, ri + 7)
            cands[tighten] = idx.stats()["candidates"]
            assert idx.stats()["fallback_queries"] == (nq if tighten == 2 else 0)
        print(f"W={w} nq={nq} k={k}: candidates tightened {cands[1]}, safe {cands[0]}, plan {plan}")
        assert cands[1] < cands[0]
    finally:
        idx.close()


@pytest.mark.parametrize("w,nq", [(16, 150), (7, 300)])
def test_more_queries_than_one_register_stream_launch(w, nq):
    """The register stream takes 2048 / W queries per launch beyond 5 words (128 at 16 words, 292 at 7): a batch beyond
    that is streamed in several launches, each with its own compaction, and answers like the oracle."""
    n, seed, k = 70_001, 4000 + w, 10
    codes, pool = _case(w, n, nq, seed)
    queries = _queries(codes, pool, nq)
    rd, ri = _oracle(codes, queries, k)
    idx = _lib.HammingIndex(codes)
    try:
        idx.set_option("hamming_ring", 0)
        for fused in (0, 1):
            idx.set_option("hamming_fused", fused)
            plan = idx.plan(nq, k)
            assert plan["stream"] == STREAM_REGISTER and plan["chain"] == CHAIN_GENERAL and plan["queries_per_launch"] == 2048 // w < nq, plan
            d, i = idx.search(queries, k)
            np.testing.assert_array_equal(d, rd)
            np.testing.assert_array_equal(i, ri)
            assert idx.stats()["fallback_queries"] == 0
    finally:
        idx.close()


# ------------------------------------------------------------------------------------ 3. ring units
@pytest.mark.parametrize("w", [3, 5, 6, 7])
@pytest.mark.parametrize("n_kind", ["inside", "whole", "whole_plus_one"])
def test_ring_units_of_w_kib(w, n_kind):
    """The ring with units of W KiB (128 codes): an array that ends inside a unit, one of whole units and one code
    more; 2 queries and 65 (two launches of at most 64); the explicit rank table after an append."""
    k = 50
    rng = np.random.default_rng(6000 + w)
    base, _ = _case(w, 100_003, 65, 6000 + w)
    n = {"inside": len(base), "whole": 128 * 700, "whole_plus_one": 128 * 700 + 1}[n_kind]
    assert n <= len(base) and n % 128 == {"inside": 35, "whole": 0, "whole_plus_one": 1}[n_kind]
    codes = base[:n]
    pool = rng.integers(0, 2 ** 64, size=(65, w), dtype=np.uint64)
    pool[0] = codes[n // 3]
    idx = _lib.HammingIndex(codes)
    try:
        idx.set_option("hamming_ring", 1)
        for nq in (2, 65):
            queries = _queries(codes, pool, nq)
            assert idx.plan(nq, k)["stream"] == STREAM_RING
            d, i = idx.search(queries, k)
            assert idx.stats()["fallback_queries"] == 0
            rd, ri = _oracle(codes, queries, k)
            np.testing.assert_array_equal(d, rd)
            np.testing.assert_array_equal(i, ri)
        new = _fresh(rng, codes, 300, w)
        idx.append(new, _insert_positions(codes, new))
        merged = np.unique(np.concatenate([codes, new]), axis=0)
        assert idx.plan(2, k)["stream"] == STREAM_RING
        queries = _queries(merged, pool, 3)
        d, i = idx.search(queries, k)
        rd, ri = _oracle(merged, queries, k)
        np.testing.assert_array_equal(d, rd)
        np.testing.assert_array_equal(i, ri)
    finally:
        idx.close()


@pytest.mark.parametrize("w", [3, 5, 7])
def test_ring_declines_a_misaligned_borrowed_array(w):
    """A borrowed device array that starts one odd-width code into an allocation is 8-byte but not 16-byte aligned:
    the ring (16-byte DMA pieces) is not taken even when forced, the register stream answers."""
    k = 50
    base, pool = _case(w, 100_003, 65, 6000 + w)
    dev = torch.device("cuda", 0)
    held = torch.from_numpy(base.view(np.int64).copy()).to(dev)
    codes = base[1:]
    _lib.set_option("hamming_no_permute", 1)             # (a permuted copy would be the library's own, aligned allocation)
    try:
        idx = _lib.HammingIndex(held.data_ptr() + 8 * w, n=len(codes), words=w, device_ptr=True, keepalive=held)
    finally:
        _lib.set_option("hamming_no_permute", 0)
    try:
        assert (held.data_ptr() + 8 * w) % 16 == 8
        idx.set_option("hamming_ring", 1)
        queries = _queries(codes, pool, 2)
        assert idx.plan(2, k)["stream"] == STREAM_REGISTER
        d, i = idx.search(queries, k)
        rd, ri = _oracle(codes, queries, k)
        np.testing.assert_array_equal(d, rd)
        np.testing.assert_array_equal(i, ri)
    finally:
        idx.close()


# ------------------------------------------------------------------------------------ 4. mutation and pipelining
@pytest.mark.parametrize("w", [3, 5])
def test_append_and_remove_equal_a_fresh_index(w):
    k = 40
    rng = np.random.default_rng(7000 + w)
    codes, pool = _case(w, 80_001, 9, 7000 + w)
    idx = _lib.HammingIndex(codes)
    fresh = None
    try:
        new = _fresh(rng, codes, 500, w)
        idx.append(new, _insert_positions(codes, new))
        merged = np.unique(np.concatenate([codes, new]), axis=0)
        gone = np.sort(rng.choice(len(merged), size=700, replace=False)).astype(np.int64)
        idx.remove(gone)
        left = np.delete(merged, gone, axis=0)
        fresh = _lib.HammingIndex(left)
        queries = pool[:9].copy()
        queries[1] = merged[gone[0]]                    # a removed code: not found at distance 0
        queries[-1] = left[-1]
        rd, ri = _oracle(left, queries, k)
        for ring in (0, 1):
            for h in (idx, fresh):
                h.set_option("hamming_ring", ring)
                d, i = h.search(queries, k)
                np.testing.assert_array_equal(d, rd)
                np.testing.assert_array_equal(i, ri)
        assert rd[1, 0] > 0
    finally:
        idx.close()
        if fresh is not None:
            fresh.close()


@pytest.mark.parametrize("depth", [2, 3])
def test_pipelined_calls_equal_blocking_calls(depth):
    w, k = 3, 30
    codes, pool = _case(w, 80_001, 80, 7100)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    idx = _lib.HammingIndex(codes, id_base=5)
    try:
        sizes = [4, 40, 1, 70, 4]
        qs = [_queries(codes, pool[j:], b) for j, b in enumerate(sizes)]
        want = [idx.search(q, k) for q in qs]
        rd, ri = _oracle(codes, qs[1], k)
        np.testing.assert_array_equal(want[1][0], rd)
        np.testing.assert_array_equal(want[1][1], ri + 5)
        qd = [torch.from_numpy(q.view(np.int64)).to(dev) for q in qs]
        od = [torch.empty((b, k), dtype=torch.int32, device=dev) for b in sizes]
        oi = [torch.empty((b, k), dtype=torch.int64, device=dev) for b in sizes]
        idx.set_option("hamming_async_depth", depth)
        for j, q in enumerate(qd):
            idx.search_device_async(q.data_ptr(), sizes[j], k, od[j].data_ptr(), oi[j].data_ptr(), stream)
            f = j - (depth - 1)
            if f >= 0:
                np.testing.assert_array_equal(od[f].cpu().numpy(), want[f][0])
                np.testing.assert_array_equal(oi[f].cpu().numpy(), want[f][1])
        idx.sync()
        for f in range(len(sizes)):
            np.testing.assert_array_equal(od[f].cpu().numpy(), want[f][0])
            np.testing.assert_array_equal(oi[f].cpu().numpy(), want[f][1])
    finally:
        idx.close()


# ------------------------------------------------------------------------------------ 5. overflow
def test_low_entropy_codes_overflow_to_the_exact_path():
    codes, queries = GI.hamming_inputs(150_000, 192, 77, "lowent")
    assert codes.shape[1] == 3
    _lib.set_option("candidate_cap", 2048)
    try:
        idx = _lib.HammingIndex(codes)
        d, i = idx.search(queries, 50)
        assert idx.stats()["fallback_queries"] > 0
        rd, ri = _oracle(codes, queries, 50)
        np.testing.assert_array_equal(d, rd)
        np.testing.assert_array_equal(i, ri)
        idx.close()
    finally:
        _lib.set_option("candidate_cap", 0)


# ------------------------------------------------------------------------------------ 6. through the plugins
@pytest.mark.parametrize("bits", [192, 320])
def test_linear_hash_index_nn_over_wide_hash_vectors(bits):
    rng = np.random.default_rng(bits)
    v = rng.random((70_001, bits)) > 0.5
    packed = np.unique(O.pack_bits_msb(v), axis=0)
    idx = HipLinearHashIndex()
    idx.build_index(v)
    assert idx.count() == len(packed)
    for q in (v[11], rng.random(bits) > 0.5):
        rows, dists = idx.nn(q, 25)
        rd, ri = O.hamming_topk(packed, O.pack_bits_msb(q[None])[0], 25)
        np.testing.assert_array_equal(O.pack_bits_msb(rows), packed[ri])
        np.testing.assert_allclose(dists, rd / float(bits), rtol=0, atol=1e-15)


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_lsh_index_with_320_bit_itq_codes(metric):
    """HipLSHNearestNeighborIndex over 12 000 descriptors of 320 dimensions hashed to 320 bits (five words), the model
    set directly.  candidate_cap = 2048 keeps 12 000 codes off the all-keys chain, so the nearest codes come from the
    five-word stream kernels."""
    rng = np.random.default_rng(320)
    n, d, bits, nn = 12_000, 320, 320, 20
    db = rng.standard_normal((n, d)).astype(np.float32)
    q_, _ = np.linalg.qr(rng.standard_normal((d, d)))
    rot = np.ascontiguousarray(q_[:, :bits])
    mean = np.zeros(d, dtype=np.float64)
    f = HipItqFunctor(bit_length=bits)
    f.mean_vec, f.rotation = mean, rot
    packed = O.pack_bits_msb(O.itq_get_hash(db, mean, rot))
    uniq, inv = np.unique(packed, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    buckets = [[] for _ in range(len(uniq))]
    for r, u in enumerate(inv.tolist()):
        buckets[u].append(r)
    _lib.set_option("candidate_cap", 2048)
    try:
        index = HipLSHNearestNeighborIndex(f, MemoryDescriptorSet(), MemoryKeyValueStore(), HipLinearHashIndex(),
                                           distance_method=metric)
        index.build_index([DescriptorMemoryElement(i).set_vector(row) for i, row in enumerate(db)])
        qs = rng.standard_normal((8, d)).astype(np.float32)
        qs[0] = db[7]
        for q in qs:
            r, dists = index.nn(DescriptorMemoryElement("q").set_vector(q), nn)
            ids, rd = O.lsh_nn(q, nn, mean, rot, None, uniq, buckets, db, metric)
            assert [e.uuid() for e in r] == ids.tolist()
            if metric == "euclidean":
                np.testing.assert_array_equal(np.asarray(dists, dtype=rd.dtype), rd)
            else:
                np.testing.assert_allclose(dists, rd, rtol=1e-12, atol=1e-15)
    finally:
        _lib.set_option("candidate_cap", 0)
