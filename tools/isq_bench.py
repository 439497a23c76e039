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

--shared: the two scans of the IVF-SQ index against each other (profiles/ivf_sq_shared_scan.txt): handle option
"isq_scan" = 0 (isq_scan_kernel: a probed code row is read and decoded once per query) and 1 (isq_scan_shared_kernel: a
row decoded once per group of 8 queries of its list) for both kinds, batches of 1 / 32 / 256 / 1024 queries at nprobe 16
and 64, with IVF-Flat's list-major call ("ivf_scan" = 1) on the same batch beside them.  The options alternate window by
window in one process (a window is this much time of the slowest option, 3 .. 100 blocking device calls over 8 rotating
query batches, on the host clock; median of --windows windows with the fastest and slowest beside it); the scan kernel's
own time is a pass of its own under option "profile" (the list-major path's sort and grouping are outside those events and
inside the call's time).  The answers of the two options are compared bit for bit before anything is timed.  Last, per
kind, the R of the automatic rule: the smallest of 1, 2, 4, 8 pairs per list at which option 1 is no slower than option 0
on every measured batch with at least that many.

    python tools/isq_bench.py --shared --out profiles/ivf_sq_shared_scan.txt
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
    ap.add_argument("--nprobes", default="", help="default 1,4,16,64; with --shared 16,64")
    ap.add_argument("--batches", default="", help="default 1,32; with --shared 1,32,256,1024")
    ap.add_argument("--shared", action="store_true", help="the per-query scan against the list-major scan (option \"isq_scan\" 0 / 1)")
    ap.add_argument("--window-ms", type=float, default=60.0, help="--shared: a window is this much time of the slowest option, 3 .. 100 calls")
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
    nprobes = [int(v) for v in (args.nprobes or ("16,64" if args.shared else "1,4,16,64")).split(",")]
    batches = [int(v) for v in (args.batches or ("1,32,256,1024" if args.shared else "1,32")).split(",")]
    if args.only:
        only = tuple(int(v) for v in args.only.split(","))
        batches, nprobes = [only[0]], [only[1]]
    db = bench.make_rows(torch, args.data, n, d, dev, 3)
    nbatch = 8
    all_q = bench.make_rows(torch, args.data, max(batches) * nbatch, d, dev, 1234)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    say(f"# {'IVF-SQ scans: per query (isq_scan 0) vs list-major (isq_scan 1), beside IVF-Flat list-major' if args.shared else 'IVF-SQ vs IVF-Flat vs residual IVF-PQ vs exact'}, {_lib.device_name(0)[0]}: {n} x {d} float32 rows ({args.data}), nlist {nlist}, k {k}")

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
    if args.shared:
        shared_scans(args, torch, _lib, indexes, all_q, batches, nprobes, nbatch, stream, say)
        finish(args, lines, indexes.values())
        return
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
    finish(args, lines, list(indexes.values()) + ([dense] if dense is not None else []))


def finish(args, lines, indexes):
    print(flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")
    for index in indexes:
        index.close()


def shared_scans(args, torch, _lib, indexes, all_q, batches, nprobes, nbatch, stream, say):
    """--shared: see the module's docstring."""
    k, nlist, dev = args.k, args.nlist, all_q.device
    flat = indexes["flat"]
    flat.set_option("ivf_scan", 1)
    say("ms per blocking call, median [fastest .. slowest] of %d alternating windows; scan = the scan kernel alone, us" % args.windows)
    say("kind queries nprobe pairs/nlist |  option 0 ms              scan us |  option 1 ms              scan us  served |  call 0/1  scan 0/1 | flat list-major ms   scan us")

    def window(call, qs, calls):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for c in range(calls):
            call(qs[c % nbatch])
        return (time.perf_counter() - t) / calls * 1e3

    def scan_us(index, call, qs, calls):
        index.set_option("profile", 1)
        ms = []
        for c in range(calls):
            call(qs[c % nbatch])
            ms.append(index.stats()["scan_ms"])
        index.set_option("profile", 0)
        return statistics.median(ms) * 1e3

    ratio = {"sq8": [], "f16": []}      # (pairs per list, option 0 ms / option 1 ms)
    for nq in batches:
        qs = [all_q[j * nq:(j + 1) * nq].contiguous() for j in range(nbatch)]
        od = torch.empty((nq, k), dtype=torch.float32, device=dev)
        oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
        for p in nprobes:
            calls_of = {name: (lambda ix: lambda q: ix.search_device(q.data_ptr(), nq, k, p, od.data_ptr(), oi.data_ptr(), stream))(ix)
                        for name, ix in indexes.items()}
            # warm-up, the answers' equality, the calls per window
            first, served = [], {}
            for name in ("sq8", "f16"):
                answers = {}
                for opt in (0, 1):
                    indexes[name].set_option("isq_scan", opt)
                    calls_of[name](qs[0])
                    t = time.perf_counter()
                    calls_of[name](qs[0])
                    first.append((time.perf_counter() - t) * 1e3)
                    if opt:
                        served[name] = indexes[name].stats()["mid_tier_queries"]
                    answers[opt] = (od.cpu().numpy().view(np.uint32).copy(), oi.cpu().numpy().copy())
                assert np.array_equal(answers[1][0], answers[0][0]) and np.array_equal(answers[1][1], answers[0][1]), "the scans disagree"
            calls_of["flat"](qs[0])
            calls = int(min(100, max(3, args.window_ms / max(first))))
            times = {key: [] for key in (("sq8", 0), ("sq8", 1), ("f16", 0), ("f16", 1), "flat")}
            for _ in range(args.windows):
                for key in times:
                    if key != "flat":
                        indexes[key[0]].set_option("isq_scan", key[1])
                    times[key].append(window(calls_of["flat" if key == "flat" else key[0]], qs, calls))
            scan = {"flat": scan_us(flat, calls_of["flat"], qs, calls)}
            for name in ("sq8", "f16"):
                for opt in (0, 1):
                    indexes[name].set_option("isq_scan", opt)
                    scan[(name, opt)] = scan_us(indexes[name], calls_of[name], qs, calls)

            def fig(key):
                return f"{statistics.median(times[key]):8.3f} [{min(times[key]):7.3f} .. {max(times[key]):7.3f}]"

            for name in ("sq8", "f16"):
                t0, t1 = statistics.median(times[(name, 0)]), statistics.median(times[(name, 1)])
                ratio[name].append((nq * min(p, nlist) / nlist, t0 / t1))
                say(f"{name:4s} {nq:7d} {p:6d} {nq * min(p, nlist) / nlist:11.2f} | {fig((name, 0))} {scan[(name, 0)]:9.1f} | {fig((name, 1))} {scan[(name, 1)]:9.1f} "
                    f"{served[name]:7d} | {t0 / t1:7.2f} x {scan[(name, 0)] / scan[(name, 1)]:7.2f} x | {statistics.median(times['flat']):8.3f} "
                    f"{scan['flat']:14.1f}   ({calls} calls per window)")
    say()
    for name, rows in ratio.items():
        fits = [R for R in (1, 2, 4, 8) if any(ppl >= R for ppl, _ in rows) and all(gain >= 1.0 for ppl, gain in rows if ppl >= R)]
        say(f"# {name}: R = {fits[0] if fits else 0} (option 1 no slower than option 0 on every measured batch of at least R pairs per list; 0 = never)")


if __name__ == "__main__":
    main()
