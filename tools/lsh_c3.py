"""
bench.py --workload lsh_c3: BASELINE.json config 3 end to end on one MI355X --
10 M x 128 float32 descriptors -> 64-bit ITQ codes -> Hamming top-n over the unique codes -> bucket expansion ->
exact re-rank -> top-k, i.e. LSHNearestNeighborIndex.nn (impls/nn_index/lsh.py:452-519) for batches of queries.

A step is ONE sq_lsh_query call (include/smqtk_hip.h) on `--queries` query descriptors resident in HBM: hash, nearest
codes, bucket expansion and re-rank all run on the device.  Reported: queries/s and recall@k against the exact
brute-force ground truth (sq_dense_search over the same matrix), for the reference's own setting (n nearest codes =
the n results asked for) and for wider code searches (`other_code_counts`): recall < 1 is the LSH algorithm's, not
the kernels' -- every stage is bit-exact against the oracle (tests/).  The index (codes, unique codes, CSR bucket map)
is built on the device outside the timed region.  CPU leg: the oracle's lsh_nn (reference-faithful: per-row Python
distance calls) on a sub-sample, scaled.
"""
import os
import time

import numpy as np

HBM_PEAK_GBS = 8000.0


def run(args, torch, dist, _lib, world, rank, dev, use_dist, emit, make_rows):
    if world != 1:
        raise SystemExit("--workload lsh_c3 is a one-GPU workload (BASELINE config 3)")
    n, d, k, bits = args.rows, args.dim, args.k, 64
    nq = args.queries
    stream = torch.cuda.current_stream().cuda_stream
    t_build = time.perf_counter()
    db = make_rows(torch, args.data, n, d, dev, 3)
    qs_all = make_rows(torch, args.data, max(nq, 256), d, dev, 1234)
    # ITQ model as SURVEY 8(d) C3: orthonormal R (QR of a seeded Gaussian, first 64 columns), mean of a 100 k sample
    rot_np, _ = np.linalg.qr(np.random.default_rng(5).standard_normal((d, d)))
    rot_np = np.ascontiguousarray(rot_np[:, :bits])
    mean_t = db[:100_000].to(torch.float64).mean(dim=0).contiguous()
    model_note = "fixed: orthonormal R (QR of a seeded Gaussian, first 64 columns), mean of a 100 k sample (SURVEY 8d, C3)"
    if getattr(args, "fit", False):
        # a TRAINED model: ItqFunctor.fit (impls/lsh_functor/itq.py:291-387) on a 1 M-row sample, its O(n) products on the
        # device (HipItqFunctor._fit_device: mean, covariance, PCA projection, 50 ITQ iterations), outside the timed region
        from smqtk_indexing_amd.impls.lsh_functor.hip_itq import HipItqFunctor
        t_fit = time.perf_counter()
        sample = db[:: max(1, n // 1_000_000)][:1_000_000].cpu().numpy()
        f = HipItqFunctor(bit_length=bits, itq_iterations=50, random_seed=0)
        mean_h, rot_h = f._fit_device(sample)
        rot_np = np.ascontiguousarray(np.real(rot_h)).astype(np.float64)
        mean_t = torch.from_numpy(np.asarray(mean_h, dtype=np.float64)).to(dev).contiguous()
        model_note = (f"fitted: HipItqFunctor.fit products on the device over a {sample.shape[0]}-row sample, 50 ITQ iterations, "
                      f"{time.perf_counter() - t_fit:.2f} s")
        del sample
    rot_t = torch.from_numpy(rot_np).to(dev)
    codes = torch.empty((n, 1), dtype=torch.int64, device=dev)
    _lib.itq_hash_device(db.data_ptr(), 0, n, d, mean_t.data_ptr(), rot_t.data_ptr(), bits, _lib.SQ_NORM_NONE,
                         codes.data_ptr(), stream)
    torch.cuda.synchronize()
    # unique codes ascending AS UNSIGNED integers (row id of the hash index = rank of the code): flipping the top bit
    # makes int64 order equal uint64 order
    top = torch.tensor(-0x8000000000000000, dtype=torch.int64, device=dev)
    flipped = codes.view(-1) ^ top
    uniq_f, inverse = torch.unique(flipped, sorted=True, return_inverse=True)
    ucodes = (uniq_f ^ top).contiguous()
    n_codes = int(ucodes.numel())
    order = torch.argsort(inverse, stable=True).contiguous()                 # rows bucket by bucket, row order inside
    counts = torch.bincount(inverse, minlength=n_codes)
    csr_off = torch.zeros(n_codes + 1, dtype=torch.int64, device=dev)
    csr_off[1:] = torch.cumsum(counts, 0)
    del flipped, uniq_f, inverse, counts
    torch.cuda.synchronize()
    _lib.set_option("profile", 1)
    hidx = _lib.HammingIndex(ucodes.data_ptr(), n=n_codes, words=1, device_ptr=True, keepalive=ucodes)
    rows = _lib.RowMatrix(db.data_ptr(), n=n, d=d, dtype=np.float32, device_ptr=True, keepalive=db)
    rows.set_buckets(csr_off.data_ptr(), order.data_ptr(), n_codes=n_codes, device_ptr=True, keepalive=(csr_off, order))
    model = _lib.ItqModel(mean_t.cpu().numpy(), rot_np, _lib.SQ_NORM_NONE)
    dense = _lib.DenseIndex(db.data_ptr(), n=n, d=d, device_ptr=True, keepalive=db)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t_build

    def measure(nq_, n_codes_wanted, steps, warmup):
        q = qs_all[:nq_].contiguous()
        od = torch.empty((nq_, k), dtype=torch.float32, device=dev)
        orow = torch.empty((nq_, k), dtype=torch.int64, device=dev)
        ham_ms = []
        for _ in range(warmup):
            rows.lsh_query_device(hidx, model, q.data_ptr(), nq_, n_codes_wanted, _lib.SQ_METRIC_L2, k, od.data_ptr(),
                                  orow.data_ptr(), stream)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            rows.lsh_query_device(hidx, model, q.data_ptr(), nq_, n_codes_wanted, _lib.SQ_METRIC_L2, k, od.data_ptr(),
                                  orow.data_ptr(), stream)
            ham_ms.append(hidx.stats()["scan_ms"])
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        # recall@k against the exact brute-force answer (same matrix, same queries)
        gd = torch.empty((nq_, k), dtype=torch.float32, device=dev)
        gi = torch.empty((nq_, k), dtype=torch.int64, device=dev)
        dense.search_device(q.data_ptr(), nq_, k, gd.data_ptr(), gi.data_ptr(), stream)
        torch.cuda.synchronize()
        got, want = orow.cpu().numpy(), gi.cpu().numpy()
        hits = sum(len(set(got[j][got[j] >= 0].tolist()) & set(want[j].tolist())) for j in range(nq_))
        found = float((got >= 0).sum()) / nq_
        # the LSH answer must be the exact order of ITS candidates: returned distances ascending and those of the rows
        dd = od.cpu().numpy()
        assert all((np.diff(dd[j][got[j] >= 0]) >= 0).all() for j in range(nq_))
        return {"queries_per_s": nq_ / dt, "ms_per_step": dt * 1e3, "recall_at_k": hits / float(nq_ * k),
                "results_per_query": found, "hamming_scan_ms": float(np.mean(ham_ms))}

    head = measure(nq, args.lsh_n or k, args.steps, args.warmup)
    others = {}
    for nc in ((1000, 10000) if args.full else ()):
        if nc != (args.lsh_n or k):
            others[f"n_codes_{nc}"] = measure(nq, nc, max(3, args.steps // 4), 1)
    if args.full:
        others["batch_256_n_codes_%d" % (args.lsh_n or k)] = measure(256, args.lsh_n or k, max(3, args.steps // 4), 1)

    line = {
        "metric": "queries/sec + recall@k=100, LSH pipeline (10Mx128 -> 64-bit ITQ codes -> Hamming top-n -> bucket expansion -> exact re-rank)",
        "value": head["queries_per_s"], "unit": "queries/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": head["ms_per_step"], "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "u64 codes (xor + popcount) for the scan; f32 exact re-rank (bit-identical to numpy); ITQ sign bits = float64 evaluation",
        "data": f"synthetic {args.data} float32 descriptors generated on device; queries from the same distribution",
        "config": {"workload": f"lsh_c3_{n}x{d}_bits{bits}_k{k}", "db_rows_total": n, "dim": d, "bits": bits, "k": k,
                   "unique_codes": n_codes, "itq_model": model_note, "queries_per_step": nq, "nearest_codes_per_query": args.lsh_n or k,
                   "index_build_s_on_device": build_s,
                   "recall_at_k_vs_exact_L2": head["recall_at_k"], "results_per_query": head["results_per_query"],
                   "recall_note": "the reference's algorithm expands the n nearest CODES (lsh.py:480-501); with 64-bit codes over "
                                  "10 M descriptors nearly every code is its own bucket, so n = k = 100 codes yield ~100 candidates: "
                                  "low recall is the algorithm's; other_code_counts widens the code search"},
        "roofline": {"bound": "hbm", "kernel": "hamming_stream_kernel (one pass over the unique codes)",
                     "kernel_ms": head["hamming_scan_ms"], "algorithmic_bytes_per_launch": n_codes * 8,
                     "achieved": n_codes * 8 / (head["hamming_scan_ms"] * 1e-3) / 1e9 if head["hamming_scan_ms"] > 0 else None,
                     "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": n_codes * 8 / (head["hamming_scan_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS if head["hamming_scan_ms"] > 0 else None,
                     "traffic": None,
                     "note": "80 MB per pass: a 10 us floor; the step is launch / latency bound (hash, histogram, threshold, stream, "
                             "compaction, select, expansion, re-rank, select), which is why queries are batched"},
        "other_code_counts": others,
    }
    if args.full and not args.no_cpu_baseline:
        from oracle import cpu_ref as O
        sub = 200_000
        dbh = db[:sub].cpu().numpy().astype(np.float64)           # the reference works on float64 descriptors by default
        mean_h = mean_t.cpu().numpy()
        t1 = time.perf_counter()
        bits_h = O.itq_get_hash(dbh, mean_h, rot_np)                # (vectorised here; the reference hashes row by row)
        packed = O.pack_bits_msb(bits_h)
        uniq, inv = np.unique(packed, axis=0, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        buckets = [[] for _ in range(uniq.shape[0])]
        for r, u in enumerate(inv.tolist()):
            buckets[u].append(r)
        t_index = time.perf_counter() - t1
        qh = qs_all[:4].cpu().numpy().astype(np.float64)
        t1 = time.perf_counter()
        for qv in qh:
            O.lsh_nn(qv, k, mean_h, rot_np, None, uniq, buckets, dbh, "euclidean")
        dtq = (time.perf_counter() - t1) / len(qh)
        line["cpu_baseline"] = {
            "value": 1.0 / (dtq * n / sub), "unit": "queries/s", "cores": 1, "kind": "port",
            "sample": f"oracle/cpu_ref.lsh_nn (hash query, popcount scan of the unique codes, bucket expansion, per-row distance "
                      f"calls + stable sort as lsh.py:452-519) on {sub} descriptors: {dtq * 1e3:.1f} ms per query (index build "
                      f"{t_index:.1f} s), scaled linearly in rows to {n}; host has {len(os.sched_getaffinity(0))} cores",
        }
    emit(line)
    dense.close()
    hidx.close()
    rows.close()
    model.close()
