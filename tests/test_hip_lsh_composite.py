"""
GPU tests of `sq_lsh_query`, the LSH pipeline in one device call (hash -> nearest codes -> bucket expansion -> exact
re-rank), on every route its three stages take: each certified ITQ filter and the float64 kernel INSIDE the composite
(calls of 31, 32 and 70 queries: the filters engage at 32 rows), the Hamming chains fed with device-resident codes of
1, 2, 5 and 16 words, device-memory mode on a caller's stream, partial and empty buckets, scratch buffers shared with
`sq_rows_rerank` across calls of changing shape, and the tie rule.

The cases come from tests/lsh_cases.py, which proves on the CPU (tests/test_lsh_cases_cpu.py) that every pool query
keeps every bit 1e-9 |x - mean||R_j| away from zero, that multi-row buckets exist and that the planted pair's tie is
one that row-id order would get wrong.

Comparison rule, every test: ids equal `lsh_nn_fast`'s (the oracle's lsh_nn, vectorised), -1 / +inf behind the last
candidate; L2 distances equal bits (float32 or float64 as the rows are); cosine distances rtol 1e-12, atol 1e-15, and
where an id differs `O.assert_topk_equivalent(rtol=1e-12)` decides (the project's convention for cosine near-ties;
every such query is recorded in NEAR_TIES and printed).  A NaN of the oracle (the zero row under cosine; numpy's stable
argsort puts it last) must be a NaN at the same position.  The zero QUERY is checked under L2 only.

Tie rule of the composite: equal distances are ordered by candidate position -- codes in (Hamming distance, code id)
order, rows of a bucket in row order -- not by row id.
"""
import numpy as np
import pytest

from oracle import cpu_ref as O
from smqtk_indexing_amd import _lib
from tests import lsh_cases as L

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CHAIN_ALL_KEYS, CHAIN_GENERAL, CHAIN_THREE_LAUNCH = 0, 1, 2
METRIC = {"euclidean": _lib.SQ_METRIC_L2, "cosine": _lib.SQ_METRIC_COSINE}
CAP = 2048
# sq_hamming_fused.hpp / sq_hamming.hip: the three-launch call takes codes of up to HF_MAX_WORDS words, sorts up to
# HF_SORT_CAP keys (2 k of them) and up to stream_qbatch(W) queries when the ring is not the stream
HF_MAX_WORDS, HF_SORT_CAP = 7, 4096
NEAR_TIES = []      # (case, query, m, metric) whose ids were accepted through assert_topk_equivalent


def _stream_qbatch(w):
    return 1024 if w <= 2 else 384 if w <= 5 else 2048 // w


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


class Rig:
    """One set of handles over a case: rows + bucket map, the codes' Hamming index, the model."""

    def __init__(self, case, cap=CAP, csr=None):
        off, order = (case.off, case.order) if csr is None else csr
        self.case = case
        self.hidx = _lib.HammingIndex(case.uniq)
        if cap:
            self.hidx.set_option("candidate_cap", cap)      # this handle only
        self.rows = _lib.RowMatrix(case.db)
        self.rows.set_buckets(off, order)
        norm = _lib.SQ_NORM_NONE if case.normalize is None else int(case.normalize)
        self.model = _lib.ItqModel(case.mean, case.rot, norm)

    def query(self, q, m, metric, k):
        return self.rows.lsh_query(self.hidx, self.model, q, m, METRIC[metric], k)

    def close(self):
        self.rows.close()
        self.hidx.close()
        self.model.close()


def _compare_one(what, ids, rd, dist_row, got_row, metric):
    """One query's output row against the oracle's (ids, distances) already cut to k."""
    kk = len(ids)
    assert (got_row[kk:] == -1).all() and np.isposinf(dist_row[kk:]).all(), f"{what}: padding behind {kk} candidates"
    g_ids, g_d = got_row[:kk], dist_row[:kk]
    if metric == "euclidean":
        assert g_d.dtype == rd.dtype, what
        np.testing.assert_array_equal(g_ids, ids, err_msg=what)
        np.testing.assert_array_equal(_bits(g_d), _bits(rd), err_msg=what)
        return
    nan = np.isnan(rd)
    np.testing.assert_array_equal(np.isnan(g_d), nan, err_msg=what + ": NaN positions")
    np.testing.assert_allclose(g_d[~nan], rd[~nan], rtol=1e-12, atol=1e-15, err_msg=what)
    if not np.array_equal(g_ids, ids):
        np.testing.assert_array_equal(g_ids[nan], ids[nan], err_msg=what)
        O.assert_topk_equivalent(rd[~nan], ids[~nan], g_d[~nan], g_ids[~nan], rtol=1e-12)
        NEAR_TIES.append(what)
        print("cosine near-tie accepted:", what)


def _check(case, qidx, m, k, metric, dist, got, buckets=None, tag=None):
    assert dist.shape == got.shape == (len(qidx), k)
    for row, qi in enumerate(qidx):
        if metric == "cosine" and qi == L.Q_ZERO:
            continue
        ids, rd = case.oracle(qi, m, metric, k=k, buckets=buckets, tag=tag)
        _compare_one(f"{case.what} query {qi} nq={len(qidx)} m={m} k={k} {metric}", ids, rd, dist[row], got[row], metric)


def _call(rig, qidx, m, k, metric, **kw):
    qidx = list(range(qidx)) if isinstance(qidx, int) else list(qidx)
    dist, got = rig.query(rig.case.pool[qidx], m, metric, k)
    _check(rig.case, qidx, m, k, metric, dist, got, **kw)
    return dist, got


# ------------------------------------------------------------------------------------ 1. every hash route
@pytest.mark.parametrize("name", [c[0] for c in L.ROUTE_CASES])
def test_composite_on_every_hash_route(name):
    """Calls of 31, 32 and 70 queries (m = k = 20; at 32 also m = 1 and 300), both metrics, on a shape for every
    branch of itq_filter_route / itq_plan: the model's statistics show no filter pass at 31 rows and the route's pass
    count from 32 on, the Hamming handle (candidate_cap = 2048 on the handle) is off the all-keys chain, and every row
    and distance is the oracle's.  One case also runs a handle with the default cap: the all-keys chain."""
    passes = L.ROUTE_BY_NAME[name][6]
    case = L.route_case(name)
    rig = Rig(case)
    try:
        for metric in ("euclidean", "cosine"):
            for nq, m in ((31, 20), (32, 20), (70, 20), (32, 1), (32, 300)):
                plan = rig.hidx.plan(nq, m)
                assert plan["chain"] != CHAIN_ALL_KEYS and plan["candidate_cap"] == CAP, (name, nq, m, plan)
                assert plan["stream"] != 0, (name, nq, m, plan)         # a mini-list stream (register or ring) reads the codes
                _call(rig, nq, m, 20, metric)
                st = rig.model.stats()
                assert st["scan_launches"] == (0 if nq < 32 else passes), (name, nq, m, st)
                assert st["fallback_queries"] == (nq if nq < 32 or passes == 0 else 0), (name, nq, m, st)
        if name == "narrow":
            other = _lib.HammingIndex(case.uniq)                    # default cap: every code is a candidate
            try:
                assert other.plan(32, 20)["chain"] == CHAIN_ALL_KEYS
                dist, got = rig.rows.lsh_query(other, rig.model, case.pool[:32], 20, METRIC["euclidean"], 20)
                _check(case, list(range(32)), 20, 20, "euclidean", dist, got)
            finally:
                other.close()
    finally:
        rig.close()


# ------------------------------------------------------------------------------------ 2. the Hamming chains
@pytest.mark.parametrize("w", sorted(L.WIDTH_CASES))
def test_composite_hamming_chains(w):
    """Codes of 1, 2, 5 and 16 words from the hash stage into each chain of the search, the chain asserted from
    plan(): 4 queries (three launches up to 7 words, the general chain beyond), 70 queries (past the 32 whose
    thresholds the stream's prologue computes; 16 words: general), 2 m beyond the pick kernel's sort (general at every
    width, the candidate cap rises to 2 m) and m beyond the number of codes (clamped: all keys, every row a candidate,
    k = n + 5 so that padding is written)."""
    case = L.route_case(L.WIDTH_CASES[w])
    assert case.words == w
    n, u = case.db.shape[0], case.uniq.shape[0]
    fused_w = w <= HF_MAX_WORDS
    big_m = HF_SORT_CAP // 2 + 52
    assert 2 * big_m > HF_SORT_CAP and big_m < u // 2
    rig = Rig(case)
    try:
        for nq, m, k, chain, cap in ((4, 20, 20, CHAIN_THREE_LAUNCH if fused_w else CHAIN_GENERAL, CAP),
                                     (70, 20, 20, CHAIN_THREE_LAUNCH if fused_w and 70 <= _stream_qbatch(w) else CHAIN_GENERAL, CAP),
                                     (8, big_m, 50, CHAIN_GENERAL, 2 * big_m),
                                     (4, u + 10, n + 5, CHAIN_ALL_KEYS, 2 * u)):
            plan = rig.hidx.plan(nq, m)
            assert (plan["chain"], plan["candidate_cap"]) == (chain, cap), (w, nq, m, plan)
            for metric in ("euclidean", "cosine"):
                _call(rig, nq, m, k, metric)
    finally:
        rig.close()


# ------------------------------------------------------------------------------------ 3. device memory
@pytest.mark.parametrize("name,metric", [("narrow", "euclidean"), ("narrow", "cosine"), ("wide_f64", "euclidean")])
def test_composite_in_device_memory_equals_host_memory(name, metric):
    """SQ_MEM_DEVICE as the benchmark runs it: rows borrowed from a torch tensor, the CSR map on the device, queries
    and both outputs on the device, a non-default stream.  32 and 33 queries (the filter runs), outputs pre-filled with
    a sentinel, k beyond some queries' candidate count: after the stream is synchronised the bits are the host-mode
    call's, the oracle's as above, and no sentinel is left, the padded tail included."""
    case = L.route_case(name)
    passes = L.ROUTE_BY_NAME[name][6]
    dev = torch.device("cuda:0")
    m, k = 20, 64
    host = Rig(case)
    db_t = torch.from_numpy(np.array(case.db)).to(dev)
    off_t = torch.from_numpy(np.array(case.off)).to(dev)
    order_t = torch.from_numpy(np.array(case.order)).to(dev)
    rows = _lib.RowMatrix(db_t.data_ptr(), n=case.db.shape[0], d=case.d, dtype=case.db.dtype, device_ptr=True, keepalive=db_t)
    rows.set_buckets(off_t.data_ptr(), order_t.data_ptr(), n_codes=case.uniq.shape[0], device_ptr=True, keepalive=(off_t, order_t))
    stream = torch.cuda.Stream(device=dev)
    f32_out = case.db.dtype == np.float32 and metric == "euclidean"
    try:
        for nq in (32, 33):
            hd, hr = _call(host, nq, m, k, metric)
            assert (hr == -1).any(), "k was meant to exceed some query's candidate count"
            q_t = torch.from_numpy(np.array(case.pool[:nq])).to(dev)
            od = torch.full((nq, k), -3.0, dtype=torch.float32 if f32_out else torch.float64, device=dev)
            orow = torch.full((nq, k), -77, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            rows.lsh_query_device(host.hidx, host.model, q_t.data_ptr(), nq, m, METRIC[metric], k, od.data_ptr(), orow.data_ptr(),
                                  stream.cuda_stream)
            stream.synchronize()
            assert host.model.stats()["scan_launches"] == passes
            dd, dr = od.cpu().numpy(), orow.cpu().numpy()
            assert not (dr == -77).any() and not (dd == -3.0).any(), "a sentinel survived"
            np.testing.assert_array_equal(dr, hr)
            np.testing.assert_array_equal(_bits(dd), _bits(hd))
            _check(case, list(range(nq)), m, k, metric, dd, dr)
    finally:
        rows.close()
        host.close()


# ------------------------------------------------------------------------------------ 4. partial and empty buckets
def test_composite_partial_and_empty_buckets():
    """The two-word case with a bucket map that lists 90 % of the rows (removed descriptors keep their slot in the
    matrix), so some codes keep an empty bucket.  Queries equal to unlisted rows never get those rows back; a query
    whose one nearest code has an empty bucket is all -1 / +inf next to queries that have candidates; three such queries
    alone (no candidate in the whole call: one padded key per query through keys, select and finalize) are all padding
    and the call succeeds."""
    case = L.route_case(L.WIDTH_CASES[2])
    n, u = case.db.shape[0], case.uniq.shape[0]
    rng = np.random.default_rng(5)
    gone = np.sort(rng.choice(n, size=n // 10, replace=False))
    live = np.setdiff1d(np.arange(n), gone)
    off, order, buckets = L.csr_of(case.inv, u, live)
    sizes = np.diff(off)
    assert off[-1] == len(live) and (sizes == 0).sum() >= 3
    empty = [int(r) for r in gone if sizes[case.inv[r]] == 0][:3]            # unlisted rows whose bucket is now empty
    shared = [int(r) for r in gone if sizes[case.inv[r]] >= 2][:3]           # unlisted rows whose bucket still has rows
    assert len(empty) == 3 and len(shared) == 3
    listed = [int(r) for r in live[:3]]
    qrows = empty + shared + listed
    L.check_margin(case.db[qrows], case.mean, case.rot, case.normalize, "partial-map queries")
    codes = O.pack_bits_msb(O.itq_get_hash(case.db[qrows], case.mean, case.rot, case.normalize))
    np.testing.assert_array_equal(codes, case.uniq[case.inv[qrows]])

    def expect(rows_of_q, m, metric, k):
        return [L.lsh_nn_fast(case.db[r], m, case.mean, case.rot, case.normalize, case.uniq, buckets, case.db, metric, k=k)
                for r in rows_of_q]

    def run(rig, rows_of_q, m, metric, k):
        dist, got = rig.query(case.db[rows_of_q], m, metric, k)
        for j, (ids, rd) in enumerate(expect(rows_of_q, m, metric, k)):
            _compare_one(f"partial map, row {rows_of_q[j]} as query, m={m} {metric}", ids, rd, dist[j], got[j], metric)
        return dist, got

    rig = Rig(case, csr=(off, order))
    try:
        for metric in ("euclidean", "cosine"):
            dist, got = run(rig, qrows, 20, metric, 20)
            assert not np.isin(got, gone).any(), "an unlisted row came back"
            assert (got[:, 0] >= 0).all()
            # one query without candidates among queries that have some
            dist, got = run(rig, [empty[0]] + listed, 1, metric, 5)
            assert (got[0] == -1).all() and np.isposinf(dist[0]).all() and (got[1:, 0] == np.array(listed)).all()
            # no candidate in the whole call
            dist, got = run(rig, empty, 1, metric, 5)
            assert (got == -1).all() and np.isposinf(dist).all()
    finally:
        rig.close()


# ------------------------------------------------------------------------------------ 5. shared scratch
def test_composite_scratch_survives_changing_shapes():
    """One set of handles over the five-word case built with more than SQ_MAX_K rows (about 18 000, so that a call for
    every row sorts more keys than the one-workgroup select holds in either key width), a sequence of calls whose
    scratch (candidates, offsets, counts, keys, sort buffers) is shared and changes size and key type from call to call,
    `sq_rows_rerank` on the same matrix among them; every call is checked against the oracle and the first call, run
    again at the end, reproduces its bits."""
    case = L.route_case("slab_320_bits", L.BIG_CENTRES)
    n, u = case.db.shape[0], case.uniq.shape[0]
    assert n > _lib.SQ_MAX_K
    rig = Rig(case)
    try:
        first = {metric: _call(rig, 70, 300, 300, metric) for metric in ("euclidean", "cosine")}
        _call(rig, 1, 1, 1, "euclidean")
        for metric in ("euclidean", "cosine"):          # 64-bit keys, then 128-bit keys: k_sel = n, k_out = n + 5
            assert rig.hidx.plan(32, u)["chain"] == CHAIN_ALL_KEYS
            dist, got = _call(rig, 32, u, n + 5, metric)
            assert (got[:, n:] == -1).all() and (got[:, :n] >= 0).all()
            assert all(np.array_equal(np.sort(got[j, :n]), np.arange(n)) for j in (0, 31))
        # sq_rows_rerank with hand-made lists: an empty one, a repeated row, lists of very different lengths
        rng = np.random.default_rng(8)
        lists = [rng.integers(0, n, size=c) for c in (700, 0, 3, 2500, 41)]
        lists[2][:] = lists[0][0]
        qs = case.pool[:5]
        cand = np.concatenate(lists).astype(np.int64)
        offs = np.r_[0, np.cumsum([len(x) for x in lists])].astype(np.int64)
        for metric in ("euclidean", "cosine"):
            dist, pos = rig.rows.rerank(qs, METRIC[metric], cand, offs, 50)
            for j, lst in enumerate(lists):
                if metric == "cosine" and j == L.Q_ZERO:
                    continue
                rd = O.dense_distances(case.db[lst], qs[j], metric) if len(lst) else np.zeros(0, dist.dtype)
                o = np.argsort(rd, kind="stable")[:50]
                _compare_one(f"rerank list {j} {metric}", o, rd[o], dist[j], pos[j], metric)
        _call(rig, 33, 7, 50, "cosine")
        _call(rig, 33, 7, 50, "euclidean")
        for metric in ("euclidean", "cosine"):
            dist, got = _call(rig, 70, 300, 300, metric)
            np.testing.assert_array_equal(got, first[metric][1])
            np.testing.assert_array_equal(_bits(dist), _bits(first[metric][0]))
    finally:
        rig.close()


# ------------------------------------------------------------------------------------ 6. ties
@pytest.mark.parametrize("name", ["narrow", "slab_100_bits", "slab_320_bits"])
def test_composite_ties_follow_candidate_order(name):
    """The planted pair c + e, c - e (bit-equal L2 distances from the query c, the two rows in different buckets, the
    row of the nearer code holding the HIGHER id) comes back in candidate order, ids descending; the exact copies of a
    centre (one bucket, row order) ascending.  Alone (nq = 1: the float64 hash) and inside a call of 32."""
    case = L.route_case(name)
    m = case.tie_m
    hi, lo = max(case.pair_rows), min(case.pair_rows)
    copies = [r for r in case.buckets[case.inv[case.centre_row]] if np.array_equal(case.db[r], case.db[case.centre_row])]
    assert len(copies) >= 1
    rig = Rig(case)
    try:
        for qidx in ([L.Q_PAIR], [L.Q_CENTRE], list(range(32))):
            dist, got = _call(rig, qidx, m, m, "euclidean")
            if L.Q_PAIR in qidx:
                j = qidx.index(L.Q_PAIR)
                assert got[j, :2].tolist() == [hi, lo] and _bits(dist[j])[0] == _bits(dist[j])[1], (got[j, :4], dist[j, :4])
            if L.Q_CENTRE in qidx:
                j = qidx.index(L.Q_CENTRE)
                assert got[j, :len(copies)].tolist() == copies and (dist[j, :len(copies)] == 0).all()
            _call(rig, qidx, m, m, "cosine")
    finally:
        rig.close()
