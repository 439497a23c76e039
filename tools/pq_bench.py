#!/usr/bin/env python3
"""
IVF-PQ beside IVF-Flat and the exact index on one GPU, one session (profiles/ivf_pq.txt is this script's output).

Rows and queries come from bench.py's generators (make_rows "normal", seeds 3 and 1234: the headline set; --data
clustered: its clustered set).  Centroids are trained as tools/ivf_bench.py trains them (a sample of 256 rows per list,
RandomState(0)); the codebooks of every `m` are trained on the same sample from `ksub` distinct sample rows drawn next.
All rows are added from device memory in blocks of --add-block rows.  For every batch size the blocking calls of the exact
index, of IVF-Flat and of IVF-PQ (every m) at every nprobe are timed in alternating windows: a window is `--calls` calls
over 8 rotating query batches, timed with the host clock (every call returns when its results are final); the figure is
the median window with the fastest and slowest beside it.  recall@k is against the exact call's ids on the same queries.
The scan kernels' own time comes from a separate pass with option "profile" = 1 (hipEvents around the scan kernel, and
for IVF-PQ a second pair around pq_tables_kernel), over the bytes the scan reads: candidates x code stride.  A further
pass with "profile" = 2 times a launch of pq_scan_kernel on the same grid that only stages the tables and stores one
word per lane: its share of the scan's time is the share spent staging tables (launch overhead included).  --no-flat / --no-exact
leave those indexes out (their float32 rows are what limits the row count that fits beside each other).
--residual adds, for every m, the index in residual mode (sq_pq_create_residual; "rpq<m>" in the table): its codebooks are
trained on sq_pq_residuals of the same sample from the residuals of the same entry rows, it is timed in the same
alternating windows, and under each table its call time is given as a ratio to plain PQ and to IVF-Flat at equal nprobe
(profiles/ivf_pq_residual.txt is the output with this flag).  For a residual index "tables kernel" is
pq_tables_res_kernel summed over the launches of a call; option "profile" = 2 means 1 there, so no staging-only figure.

    python tools/pq_bench.py                      # the full table
    python tools/pq_bench.py --only 32,16 --ms 32 --calls 200 --windows 1 --no-flat --no-exact   # one shape, e.g. under a counter run
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
    ap.add_argument("--ms", default="8,32", help="sub-quantisers: one IVF-PQ index each")
    ap.add_argument("--ksub", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--nprobes", default="1,4,16,64")
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--calls", type=int, default=200, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--add-block", type=int, default=2_000_000)
    ap.add_argument("--train-rows-per-list", type=int, default=256)
    ap.add_argument("--data", choices=["normal", "clustered"], default="normal")
    ap.add_argument("--only", default="", help="nq,nprobe: time this shape alone")
    ap.add_argument("--no-flat", action="store_true")
    ap.add_argument("--no-exact", action="store_true")
    ap.add_argument("--residual", action="store_true", help="also the residual-mode index of every m")
    ap.add_argument("--out", default="", help="also write the report here")
    args = ap.parse_args()

    import torch
    import bench
    from smqtk_indexing_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("pq_bench needs a GPU")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    n, d, k, nlist, ksub = args.rows, args.dim, args.k, args.nlist, args.ksub
    ms_ = [int(v) for v in args.ms.split(",")]
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
    say(f"# IVF-PQ vs IVF-Flat vs exact, {_lib.device_name(0)[0]}: {n} x {d} float32 rows ({args.data}), nlist {nlist}, ksub {ksub}, k {k}")

    # ---- train on a sample
    rs = np.random.RandomState(0)
    sm = min(n, args.train_rows_per_list * nlist)
    sample_rows = np.sort(rs.choice(n, size=sm, replace=False))
    sample = db[torch.from_numpy(sample_rows).to(dev)].cpu().numpy()
    init = sample[rs.choice(sm, size=nlist, replace=False)]
    entry_rows = rs.choice(sm, size=ksub, replace=False)
    entries = sample[entry_rows]
    t0 = time.perf_counter()
    centroids = _lib.ivf_kmeans(sample, init, args.iters)
    say(f"train: {sm} sample rows, {args.iters} iterations; centroids {time.perf_counter() - t0:.2f} s")
    matrix_bytes = n * d * 4
    summary = {"rows": n, "dim": d, "nlist": nlist, "ksub": ksub, "k": k, "data": args.data, "indexes": {}}

    def add_all(index):
        t = time.perf_counter()
        for s in range(0, n, args.add_block):
            e = min(n, s + args.add_block)
            index.add(db.data_ptr() + s * d * 4, n=e - s, device_ptr=True)
        return time.perf_counter() - t

    indexes = {}
    for m in ms_:
        dsub = d // m
        books0 = np.ascontiguousarray(entries.reshape(ksub, m, dsub).transpose(1, 0, 2))
        t0 = time.perf_counter()
        books = _lib.pq_train(sample, books0, args.iters)
        train_s = time.perf_counter() - t0
        pq = _lib.PqIndex(centroids, books)
        add_s = add_all(pq)
        info = pq.info()
        res = info["codes_bytes"] + info["ids_offsets_bytes"] + info["books_coarse_bytes"]
        say(f"pq m={m}: codebooks {train_s:.2f} s, add {add_s:.2f} s in blocks of {args.add_block}; resident (sq_pq_info): codes {info['codes_bytes']}, "
            f"ids + offsets {info['ids_offsets_bytes']}, codebooks + coarse index {info['books_coarse_bytes']} = {res} bytes = "
            f"{res / matrix_bytes:.4f} x the matrix ({(info['codes_bytes'] + 4 * n) / n:.0f} bytes per row)")
        indexes[f"pq{m}"] = pq
        summary["indexes"][f"pq{m}"] = {"train_s": train_s, "add_s": add_s, "resident_bytes": res}
    if args.residual:
        t0 = time.perf_counter()
        sample_res = _lib.pq_residuals(sample, centroids)
        say(f"residuals of the sample (sq_pq_residuals, host memory): {time.perf_counter() - t0:.2f} s")
        for m in ms_:
            books0 = np.ascontiguousarray(sample_res[entry_rows].reshape(ksub, m, d // m).transpose(1, 0, 2))
            t0 = time.perf_counter()
            books = _lib.pq_train(sample_res, books0, args.iters)
            train_s = time.perf_counter() - t0
            rpq = _lib.PqIndex(centroids, books, residual=True)
            add_s = add_all(rpq)
            info = rpq.info()
            res = info["codes_bytes"] + info["ids_offsets_bytes"] + info["books_coarse_bytes"]
            say(f"rpq m={m}: codebooks {train_s:.2f} s, add {add_s:.2f} s; resident (sq_pq_info): codes {info['codes_bytes']}, ids + offsets "
                f"{info['ids_offsets_bytes']}, codebooks + coarse index + centroids {info['books_coarse_bytes']} = {res} bytes = {res / matrix_bytes:.4f} x the matrix")
            indexes[f"rpq{m}"] = rpq
            summary["indexes"][f"rpq{m}"] = {"train_s": train_s, "add_s": add_s, "resident_bytes": res}
    if not args.no_flat:
        flat = _lib.IvfIndex(centroids)
        add_s = add_all(flat)
        fi = flat.info()
        res = fi["rows_bytes"] + fi["ids_offsets_bytes"] + fi["coarse_bytes"]
        say(f"flat: add {add_s:.2f} s; resident (sq_ivf_info) {res} bytes = {res / matrix_bytes:.4f} x the matrix")
        indexes["flat"] = flat
        summary["indexes"]["flat"] = {"add_s": add_s, "resident_bytes": res}
    dense = None
    if not args.no_exact:
        dense = _lib.DenseIndex(db.data_ptr(), n=n, d=d, device_ptr=True, keepalive=db)
        di = dense.info()
        res = di["f32_rows_bytes"] + di["bf16_copy_bytes"] + di["int8_copy_bytes"] + di["row_stats_bytes"]
        say(f"exact: resident (sq_dense_info) {res} bytes = {res / matrix_bytes:.4f} x the matrix")

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
        # the scan kernels' own time: hipEvents inside the library, a pass of its own
        scan = {}
        for name, index in indexes.items():
            for p in nprobes:
                med = {}
                for mode in (1, 2) if name.startswith("pq") else (1,):
                    index.set_option("profile", mode)
                    v, tv, by, cands = [], [], 0, 0
                    for c in range(min(args.calls, 64)):
                        shapes[(name, p)](qs[c % nbatch], od, oi)
                        st = index.stats()
                        v.append(st["scan_ms"])
                        tv.append(st["rerank_ms"])
                        by, cands = st["bytes_scanned"], st["candidates"]
                    med[mode] = (statistics.median(v), statistics.median(tv))
                # (mode 1: the scan kernel and, for IVF-PQ, pq_tables_kernel; mode 2: a scan launch that only stages the tables)
                scan[(name, p)] = (med[1][0], by, cands, med[1][1], med[2][0] if 2 in med else float("nan"))
            index.reset_options()
        say()
        say(f"## {nq} quer{'y' if nq == 1 else 'ies'} per blocking call ({args.windows} windows of {args.calls} calls; median [fastest .. slowest] ms per call)")
        if "exact" in times:
            ex = statistics.median(times["exact"])
            say(f"exact              {ex:8.3f} [{min(times['exact']):.3f} .. {max(times['exact']):.3f}] ms")
        for p in nprobes:
            for name in indexes:
                key = (name, p)
                t = statistics.median(times[key])
                sms, by, cands, tms, stage_ms = scan[key]
                gbs = by / (sms * 1e-3) / 1e9 if sms > 0 else float("nan")
                say(f"nprobe {p:<3d} {name:<5s} {t:8.3f} [{min(times[key]):.3f} .. {max(times[key]):.3f}] ms   recall@{k} {recall[key]:.3f}   "
                    f"scan kernel {sms * 1e3:8.1f} us, {cands / nq:9.0f} rows per query, {by / 1e6:8.2f} MB, {gbs:7.1f} GB/s, "
                    f"{cands / (sms * 1e-3) / 1e9 if sms > 0 else float('nan'):6.2f} G rows/s"
                    + (f"   tables kernel {tms * 1e3:6.1f} us, staging-only scan launch {stage_ms * 1e3:6.1f} us = {100 * stage_ms / sms:4.1f} % of the scan"
                       if name.startswith("pq") and sms > 0 else
                       f"   tables kernel {tms * 1e3:6.1f} us" if name.startswith("rpq") else ""))
                report.append({"queries": nq, "nprobe": p, "index": name, "ms_per_call": t, "ms_fastest": min(times[key]), "ms_slowest": max(times[key]),
                               "recall": recall[key], "scan_kernel_ms": sms, "scan_bytes": by, "candidates": cands,
                               "tables_kernel_ms": tms, "staging_only_ms": stage_ms})
        if args.residual:
            say(f"# residual against plain PQ and IVF-Flat at equal nprobe, {nq} quer{'y' if nq == 1 else 'ies'}: call-time ratios, recall, kernel time")
            for p in nprobes:
                for m in ms_:
                    tr, tp = statistics.median(times[(f"rpq{m}", p)]), statistics.median(times[(f"pq{m}", p)])
                    tf = statistics.median(times[("flat", p)]) if "flat" in indexes else float("nan")
                    rs_, rp_ = scan[(f"rpq{m}", p)], scan[(f"pq{m}", p)]
                    say(f"nprobe {p:<3d} m={m:<2d}  rpq / pq {tr / tp:5.2f}   rpq / flat {tr / tf:5.2f}   recall@{k} rpq {recall[(f'rpq{m}', p)]:.3f} pq {recall[(f'pq{m}', p)]:.3f}"
                        f"   tables + scan kernels: rpq {rs_[3] * 1e3:7.1f} + {rs_[0] * 1e3:7.1f} us, pq {rp_[3] * 1e3:7.1f} + {rp_[0] * 1e3:7.1f} us")
    summary["shapes"] = report
    say()
    say(json.dumps(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for index in indexes.values():
        index.close()
    if dense is not None:
        dense.close()


if __name__ == "__main__":
    main()
