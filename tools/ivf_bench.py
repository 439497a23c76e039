#!/usr/bin/env python3
"""
IVF-Flat against the exact index on one GPU, one session (profiles/ivf_flat.txt is this script's output).

Rows and queries come from bench.py's headline generator (make_rows "normal", seeds 3 and 1234; --data clustered: its
clustered set).  The index is trained
on a sample of 256 rows per list (numpy RandomState(0), without replacement) from `nlist` distinct sample rows, then
all rows are added from device memory.  For every batch size the blocking exact call (sq_dense_search, SQ_MEM_DEVICE)
and the blocking IVF call (sq_ivf_search, SQ_MEM_DEVICE) of every nprobe are timed in alternating windows: a window is
`--calls` calls over 8 rotating query batches, timed with the host clock (both calls return when their results are
final); the figure is the median window, with the fastest and slowest beside it.  Recall@k is against the exact
call's ids on the same queries.  The scan kernel's own time comes from a separate pass with option "profile" (hipEvents
around ivf_scan_kernel), over the bytes the scan reads: candidates x row stride x 4.

    python tools/ivf_bench.py                      # the full table
    python tools/ivf_bench.py --only 1,16 --calls 200 --windows 1     # one shape, e.g. under rocprofv3 --kernel-trace --stats
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

HBM_PEAK_TBS = 8.0          # MI355X HBM3E specification peak
HBM_COPY_TBS = 6.29         # what a float4 copy kernel reaches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--nprobes", default="1,4,16,64")
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--calls", type=int, default=200, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--data", choices=["normal", "clustered"], default="normal",
                    help="bench.py's generators: normal = the headline set (no cluster structure: the hardest case for "
                         "inverted lists); clustered = 1024 Gaussian centres, rows = centre + 0.25 N(0,1)")
    ap.add_argument("--only", default="", help="nq,nprobe: time this IVF shape alone (no exact index, no recall)")
    ap.add_argument("--out", default="", help="also write the report here")
    args = ap.parse_args()

    import torch
    import bench
    from smqtk_indexing_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("ivf_bench needs a GPU")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    n, d, k, nlist = args.rows, args.dim, args.k, args.nlist
    nprobes = [int(v) for v in args.nprobes.split(",")]
    batches = [int(v) for v in args.batches.split(",")]
    only = tuple(int(v) for v in args.only.split(",")) if args.only else None
    if only:
        batches, nprobes = [only[0]], [only[1]]
    db = bench.make_rows(torch, args.data, n, d, dev, 3)
    nbatch = 8
    all_q = bench.make_rows(torch, args.data, max(batches) * nbatch, d, dev, 1234)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    say(f"# IVF-Flat vs exact, {_lib.device_name(0)[0]}: {n} x {d} float32 rows ({args.data}), nlist {nlist}, k {k}")

    # ---- train on a sample, add everything
    rs = np.random.RandomState(0)
    m = min(n, 256 * nlist)
    sample_rows = np.sort(rs.choice(n, size=m, replace=False))
    sample = db[torch.from_numpy(sample_rows).to(dev)].cpu().numpy()
    init = sample[rs.choice(m, size=nlist, replace=False)]
    t0 = time.perf_counter()
    centroids = _lib.ivf_kmeans(sample, init, args.iters)
    train_s = time.perf_counter() - t0
    ivf = _lib.IvfIndex(centroids)
    t0 = time.perf_counter()
    ivf.add(db.data_ptr(), n=n, device_ptr=True)
    add_s = time.perf_counter() - t0
    info = ivf.info()
    sizes = np.diff(ivf.lists()[0])
    say(f"train: {m} sample rows, {args.iters} iterations, {train_s:.2f} s (host arrays in and out)   add: {add_s:.2f} s "
        f"({info['add_us'] / 1e6:.2f} s inside sq_ivf_add)")
    say(f"lists: longest {info['longest_list']}, median {int(np.median(sizes))}, shortest {int(sizes.min())}, empty {info['empty_lists']}")
    res_ivf = info["rows_bytes"] + info["ids_offsets_bytes"] + info["coarse_bytes"]
    say(f"resident (sq_ivf_info): rows {info['rows_bytes']}, ids + offsets {info['ids_offsets_bytes']}, coarse index {info['coarse_bytes']}"
        f" = {res_ivf} bytes = {res_ivf / (n * d * 4):.3f} x the matrix")

    dense = None
    if not only:
        dense = _lib.DenseIndex(db.data_ptr(), n=n, d=d, device_ptr=True, keepalive=db)
        di = dense.info()
        res_dense = di["f32_rows_bytes"] + di["bf16_copy_bytes"] + di["int8_copy_bytes"] + di["row_stats_bytes"]
        say(f"resident (sq_dense_info): rows {di['f32_rows_bytes']} (borrowed), bf16 copy {di['bf16_copy_bytes']}, int8 copy {di['int8_copy_bytes']},"
            f" statistics {di['row_stats_bytes']} = {res_dense} bytes = {res_dense / (n * d * 4):.3f} x the matrix; build {di['build_ms'] / 1e3:.2f} s")

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
        for p in nprobes:
            shapes[p] = (lambda p_: lambda q, od_, oi_: ivf.search_device(q.data_ptr(), nq, k, p_, od_.data_ptr(), oi_.data_ptr(), stream))(p)
        # answers once: recall against the exact ids, rows scanned, and the warm-up of every shape
        truth, recall, scanned = [], {}, {}
        for name, call in shapes.items():
            hits = cands = 0
            for j in range(nbatch):
                call(qs[j], od, oi)
                got = oi.cpu().numpy()
                if name == "exact":
                    truth.append(got)
                elif truth:
                    hits += sum(len(np.intersect1d(got[i], truth[j][i])) for i in range(nq))
                if name != "exact":
                    cands += ivf.stats()["candidates"]
            if name != "exact":
                recall[name] = hits / (nbatch * nq * k) if truth else float("nan")
                scanned[name] = cands / (nbatch * nq)
        # timed windows, alternating over the shapes
        times = {name: [] for name in shapes}
        for _ in range(args.windows):
            for name, call in shapes.items():
                times[name].append(window(call, qs, od, oi, args.calls))
        # the scan kernel's own time: hipEvents inside the library, a pass of its own
        scan = {}
        ivf.set_option("profile", 1)
        for p in nprobes:
            ms, by = [], 0
            for c in range(args.calls):
                shapes[p](qs[c % nbatch], od, oi)
                st = ivf.stats()
                ms.append(st["scan_ms"])
                by = st["bytes_scanned"]
            scan[p] = (statistics.median(ms), by)
        ivf.reset_options()
        say()
        say(f"## {nq} quer{'y' if nq == 1 else 'ies'} per blocking call ({args.windows} windows of {args.calls} calls; median [fastest .. slowest] ms per call)")
        ex = statistics.median(times["exact"]) if "exact" in times else float("nan")
        if "exact" in times:
            say(f"exact        {ex:8.3f} [{min(times['exact']):.3f} .. {max(times['exact']):.3f}] ms  {nq / ex * 1e3:10.0f} queries/s   reads the scan copy of all {n} rows")
        for p in nprobes:
            t = statistics.median(times[p])
            sms, by = scan[p]
            tbs = by / (sms * 1e-3) / 1e12 if sms > 0 else float("nan")
            say(f"nprobe {p:<5d} {t:8.3f} [{min(times[p]):.3f} .. {max(times[p]):.3f}] ms  {nq / t * 1e3:10.0f} queries/s   {ex / t:6.2f} x exact   "
                f"recall@{k} {recall[p]:.3f}   rows scanned per query {scanned[p]:9.0f}   scan kernel {sms * 1e3:7.1f} us, "
                f"{by / 1e6:8.2f} MB, {tbs:5.2f} TB/s = {100 * tbs / HBM_PEAK_TBS:4.1f} % of {HBM_PEAK_TBS} TB/s ({100 * tbs / HBM_COPY_TBS:4.1f} % of a copy's {HBM_COPY_TBS})")
            report.append({"queries": nq, "nprobe": p, "ms_per_call": t, "ms_fastest": min(times[p]), "ms_slowest": max(times[p]),
                           "exact_ms_per_call": ex, "recall": recall[p], "rows_scanned_per_query": scanned[p], "scan_kernel_ms": sms,
                           "scan_bytes": by})
    say()
    say(json.dumps({"rows": n, "dim": d, "nlist": nlist, "k": k, "data": args.data, "train_s": train_s, "add_s": add_s, "resident_ivf_bytes": res_ivf,
                    "shapes": report}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    ivf.close()
    if dense is not None:
        dense.close()


if __name__ == "__main__":
    main()
