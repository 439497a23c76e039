#!/usr/bin/env python3
"""
IVF-SQ (8-bit and float16) beside IVF-Flat, residual IVF-PQ and the exact index on one GPU, one session
(profiles/ivf_sq.txt is this script's output, once per data set).

Rows and queries come from bench.py's generators (make_rows "normal", seeds 3 and 1234: the headline set; --data
clustered: its clustered set).  Centroids are trained as tools/ivf_bench.py trains them (a sample of 256 rows per list,
RandomState(0)); the 8-bit ranges (sq_isq_train) and the residual codebooks (m = --m, 256 entries, as tools/pq_bench.py
--residual) on the same sample.  All rows are added from device memory in blocks of --add-block rows.  For every batch size
the blocking calls of every index at every nprobe are timed in alternating windows: a window is `--calls` calls over 8
rotating query batches, timed with the host clock (every call returns when its results are final); the figure is the
median window with the fastest and slowest beside it.  recall@k is of the ids as returned (decoded or coded distances, no
re-ranking) against the exact call's ids on the same queries.  The scan kernels' own time comes from a separate pass with
option "profile" = 1 (hipEvents around the scan kernel), over the bytes the scan reads (candidates x row stride), given
against --hbm-peak.  Under each table: the SQ8 and F16 scans as a ratio to ivf_scan_kernel at equal nprobe.

    python tools/isq_bench.py --out profiles/ivf_sq.txt
    python tools/isq_bench.py --only 32,64 --calls 200 --windows 1 --no-pq --no-exact    # one shape, e.g. under a counter run
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--m", type=int, default=32, help="sub-quantisers of the residual IVF-PQ index")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--nprobes", default="1,4,16,64")
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--calls", type=int, default=200, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--add-block", type=int, default=2_000_000)
    ap.add_argument("--data", choices=["normal", "clustered"], default="normal")
    ap.add_argument("--only", default="", help="nq,nprobe: time this shape alone")
    ap.add_argument("--no-pq", action="store_true")
    ap.add_argument("--no-exact", action="store_true", help="no exact index: no recall")
    ap.add_argument("--hbm-peak", type=float, default=8000.0, help="GB/s the scan's byte rate is given against")
    ap.add_argument("--out", default="", help="append the report here")
    args = ap.parse_args()

    import torch
    import bench
    from smqtk_indexing_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("isq_bench needs a GPU")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    n, d, k, nlist = args.rows, args.dim, args.k, args.nlist
    nprobes = [int(v) for v in args.nprobes.split(",")]
    batches = [int(v) for v in args.batches.split(",")]
    if args.only:
        only = tuple(int(v) for v in args.only.split(","))
        batches, nprobes = [only[0]], [only[1]]
    db = bench.make_rows(torch, args.data, n, d, dev, 3)
    nbatch = 8
    all_q = bench.make_rows(torch, args.data, max(batches) * nbatch, d, dev, 1234)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    say(f"# IVF-SQ vs IVF-Flat vs residual IVF-PQ vs exact, {_lib.device_name(0)[0]}: {n} x {d} float32 rows ({args.data}), nlist {nlist}, k {k}")

    rs = np.random.RandomState(0)
    sm = min(n, 256 * nlist)
    sample_rows = np.sort(rs.choice(n, size=sm, replace=False))
    sample = db[torch.from_numpy(sample_rows).to(dev)].cpu().numpy()
    init = sample[rs.choice(sm, size=nlist, replace=False)]
    entry_rows = rs.choice(sm, size=min(256, sm), replace=False)
    t0 = time.perf_counter()
    centroids = _lib.ivf_kmeans(sample, init, args.iters)
    t1 = time.perf_counter()
    vmin, step = _lib.isq_train(sample)
    say(f"train: {sm} sample rows; centroids ({args.iters} iterations) {t1 - t0:.2f} s, 8-bit ranges {time.perf_counter() - t1:.3f} s")
    matrix_bytes = n * d * 4
    summary = {"rows": n, "dim": d, "nlist": nlist, "k": k, "data": args.data, "indexes": {}}

    def add_all(index):
        t = time.perf_counter()
        for s in range(0, n, args.add_block):
            e = min(n, s + args.add_block)
            index.add(db.data_ptr() + s * d * 4, n=e - s, device_ptr=True)
        return time.perf_counter() - t

    def made(name, index, fields):
        add_s = add_all(index)
        info = index.info()
        res = sum(info[f] for f in fields)
        say(f"{name}: add {add_s:.2f} s; resident {' + '.join(f'{f} {info[f]}' for f in fields)} = {res} bytes = {res / matrix_bytes:.4f} x the matrix "
            f"({(info[fields[0]] + 4 * n) / n:.0f} bytes per row)")
        indexes[name] = index
        summary["indexes"][name] = {"add_s": add_s, "resident_bytes": res}

    indexes = {}
    made("sq8", _lib.IsqIndex(centroids, _lib.SQ_ISQ_SQ8, vmin, step), ("codes_bytes", "ids_offsets_bytes", "coarse_params_bytes"))
    made("f16", _lib.IsqIndex(centroids, _lib.SQ_ISQ_F16), ("codes_bytes", "ids_offsets_bytes", "coarse_params_bytes"))
    made("flat", _lib.IvfIndex(centroids), ("rows_bytes", "ids_offsets_bytes", "coarse_bytes"))
    if not args.no_pq:
        m = args.m
        sample_res = _lib.pq_residuals(sample, centroids)
        books0 = np.ascontiguousarray(sample_res[entry_rows].reshape(len(entry_rows), m, d // m).transpose(1, 0, 2))
        t0 = time.perf_counter()
        books = _lib.pq_train(sample_res, books0, args.iters)
        say(f"rpq{m}: codebooks {time.perf_counter() - t0:.2f} s")
        made(f"rpq{m}", _lib.PqIndex(centroids, books, residual=True), ("codes_bytes", "ids_offsets_bytes", "books_coarse_bytes"))
    dense = None
    if not args.no_exact:
        dense = _lib.DenseIndex(db.data_ptr(), n=n, d=d, device_ptr=True, keepalive=db)

    def window(call, qs, od, oi, calls):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for c in range(calls):
            call(qs[c % nbatch], od, oi)
        return (time.perf_counter() - t) / calls * 1e3

    report = []
    for nq in batches:
        qs = [all_q[j * nq:(j + 1) * nq].contiguous() for j in range(nbatch)]
        od = torch.empty((nq, k), dtype=torch.float32, device=dev)
        oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        shapes = {}
        if dense is not None:
            shapes["exact"] = lambda q, od_, oi_: dense.search_device(q.data_ptr(), nq, k, od_.data_ptr(), oi_.data_ptr(), stream)
        for name, index in indexes.items():
            for p in nprobes:
                shapes[(name, p)] = (lambda ix, p_: lambda q, od_, oi_: ix.search_device(q.data_ptr(), nq, k, p_, od_.data_ptr(), oi_.data_ptr(),
                                                                                        stream))(index, p)
        # answers once: recall against the exact ids, and the warm-up of every shape
        truth, recall = [], {}
        for name, call in shapes.items():
            hits = 0
            for j in range(nbatch):
                call(qs[j], od, oi)
                got = oi.cpu().numpy()
                if name == "exact":
                    truth.append(got)
                elif truth:
                    hits += sum(len(np.intersect1d(got[i], truth[j][i])) for i in range(nq))
            if name != "exact":
                recall[name] = hits / (nbatch * nq * k) if truth else float("nan")
        times = {name: [] for name in shapes}
        for _ in range(args.windows):
            for name, call in shapes.items():
                times[name].append(window(call, qs, od, oi, args.calls))
        scan = {}       # the scan kernels' own time: hipEvents inside the library, a pass of its own
        for name, index in indexes.items():
            index.set_option("profile", 1)
            for p in nprobes:
                v, by, cands = [], 0, 0
                for c in range(min(args.calls, 64)):
                    shapes[(name, p)](qs[c % nbatch], od, oi)
                    st = index.stats()
                    v.append(st["scan_ms"])
                    by, cands = st["bytes_scanned"], st["candidates"]
                scan[(name, p)] = (statistics.median(v), by, cands)
            index.reset_options()
        say()
        say(f"## {nq} quer{'y' if nq == 1 else 'ies'} per blocking call ({args.windows} windows of {args.calls} calls; median [fastest .. slowest] ms per call)")
        if "exact" in times:
            say(f"exact              {statistics.median(times['exact']):8.3f} [{min(times['exact']):.3f} .. {max(times['exact']):.3f}] ms")
        for p in nprobes:
            for name in indexes:
                key = (name, p)
                t = statistics.median(times[key])
                sms, by, cands = scan[key]
                gbs = by / (sms * 1e-3) / 1e9 if sms > 0 else float("nan")
                say(f"nprobe {p:<3d} {name:<5s} {t:8.3f} [{min(times[key]):.3f} .. {max(times[key]):.3f}] ms   recall@{k} {recall[key]:.3f}   "
                    f"scan kernel {sms * 1e3:8.1f} us, {cands / nq:9.0f} rows per query, {by / 1e6:8.2f} MB, {gbs:7.1f} GB/s = {gbs / args.hbm_peak:5.3f} of "
                    f"{args.hbm_peak:.0f}, {cands / (sms * 1e-3) / 1e9 if sms > 0 else float('nan'):6.2f} G rows/s")
                report.append({"queries": nq, "nprobe": p, "index": name, "ms_per_call": t, "ms_fastest": min(times[key]), "ms_slowest": max(times[key]),
                               "recall": recall[key], "scan_kernel_ms": sms, "scan_bytes": by, "candidates": cands})
        say(f"# against ivf_scan_kernel at equal nprobe, {nq} quer{'y' if nq == 1 else 'ies'}: scan-kernel time flat / sq (above 1: the decoding scan is faster), call-time ratio")
        for p in nprobes:
            fl = scan[("flat", p)][0]
            say(f"nprobe {p:<3d} " + "   ".join(f"{name}: scan {fl / scan[(name, p)][0]:5.2f} x ({scan[(name, p)][0] * 1e3:7.1f} vs {fl * 1e3:7.1f} us), "
                                                f"call {statistics.median(times[('flat', p)]) / statistics.median(times[(name, p)]):5.2f} x"
                                                for name in ("sq8", "f16") if scan[(name, p)][0] > 0))
    summary["shapes"] = report
    say()
    say(json.dumps(summary))
    say()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    for index in indexes.values():
        index.close()
    if dense is not None:
        dense.close()


if __name__ == "__main__":
    main()
