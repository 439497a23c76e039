#!/usr/bin/env python3
"""
The two scans of the IVF-Flat index against each other, one GPU, one session (profiles/ivf_shared_scan.txt is this
script's output): handle option "ivf_scan" = 0 (ivf_scan_kernel: a probed list is read once per query), 1
(ivf_scan_shared_kernel: the pairs sorted by list, a list read once per group of 8 queries) and -1 (the default rule).

Rows, queries, training and the add are those of tools/ivf_bench.py.  For every batch size and nprobe the three options
and the blocking exact call of the same batch are timed in alternating windows: a window is `calls` blocking device
calls over 8 rotating query batches on the host clock; the figure is the median window with the fastest and slowest
beside it.  The scan kernel's own time is a pass of its own under option "profile" (hipEvents around the scan kernel;
the list-major path's sort and grouping are outside them and inside the call's time).  `pairs / distinct` is the
sharing the list-major scan lives on: (query, list) pairs of a call over the distinct lists it probes.

    python tools/ivf_shared_bench.py --out profiles/ivf_shared_scan.txt                       # 10 M x 128, nlist 4096, N(0,1)
    python tools/ivf_shared_bench.py --data clustered
    python tools/ivf_shared_bench.py --rows 1000000 --nlist 0 --batches 1024 --nprobes 16     # BASELINE config 2; 0 = default_nlist
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPTIONS = (0, 1, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=4096, help="0 = the plugin's default_nlist(rows)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--nprobes", default="1,4,16,64")
    ap.add_argument("--batches", default="1,32,256,1024")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=60.0, help="calls per window: this much time of the slowest option, 3 .. 100 calls")
    ap.add_argument("--data", choices=["normal", "clustered"], default="normal")
    ap.add_argument("--out", default="", help="append the report here")
    args = ap.parse_args()

    import torch
    import bench
    from smqtk_indexing_amd import _lib
    from smqtk_indexing_amd.impls.nn_index.hip_ivf import default_nlist
    if _lib.device_count() < 1:
        raise SystemExit("ivf_shared_bench needs a GPU")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    n, d, k = args.rows, args.dim, args.k
    nlist = args.nlist if args.nlist > 0 else default_nlist(n)
    nprobes = [int(v) for v in args.nprobes.split(",")]
    batches = [int(v) for v in args.batches.split(",")]
    nbatch = 8
    db = bench.make_rows(torch, args.data, n, d, dev, 3)
    all_q = bench.make_rows(torch, args.data, max(batches) * nbatch, d, dev, 1234)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    say(f"# IVF-Flat scans, {_lib.device_name(0)[0]}: {n} x {d} float32 rows ({args.data}), nlist {nlist}"
        f"{' (default_nlist)' if args.nlist <= 0 else ''}, k {k}")
    rs = np.random.RandomState(0)
    m = min(n, 256 * nlist)
    sample = db[torch.from_numpy(np.sort(rs.choice(n, size=m, replace=False))).to(dev)].cpu().numpy()
    centroids = _lib.ivf_kmeans(sample, sample[rs.choice(m, size=nlist, replace=False)], args.iters)
    ivf = _lib.IvfIndex(centroids)
    ivf.add(db.data_ptr(), n=n, device_ptr=True)
    sizes = np.diff(ivf.lists()[0])
    say(f"lists: longest {sizes.max()}, median {int(np.median(sizes))}, shortest {sizes.min()}, empty {(sizes == 0).sum()}")
    dense = _lib.DenseIndex(db.data_ptr(), n=n, d=d, device_ptr=True, keepalive=db)
    coarse = _lib.DenseIndex(centroids)
    say("ms per blocking call, median [fastest .. slowest] of %d alternating windows; scan = the scan kernel alone, us" % args.windows)
    say("queries nprobe  pairs/nlist pairs/distinct |   exact ms |  option 0 ms              scan us |  option 1 ms              scan us  served |"
        "  default ms              served |  1 vs 0")

    def window(call, qs, calls):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for c in range(calls):
            call(qs[c % nbatch])
        return (time.perf_counter() - t) / calls * 1e3

    for nq in batches:
        qs = [all_q[j * nq:(j + 1) * nq].contiguous() for j in range(nbatch)]
        od = torch.empty((nq, k), dtype=torch.float32, device=dev)
        oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
        exact = lambda q: dense.search_device(q.data_ptr(), nq, k, od.data_ptr(), oi.data_ptr(), stream)
        for p in nprobes:
            call = lambda q: ivf.search_device(q.data_ptr(), nq, k, p, od.data_ptr(), oi.data_ptr(), stream)
            probed = coarse.search(qs[0].cpu().numpy(), min(p, nlist))[1]
            distinct = len(np.unique(probed))
            # warm-up, the answers' equality, the calls per window and the path each option took
            answers, served, first = {}, {}, {}
            exact(qs[0])
            for opt in OPTIONS:
                ivf.set_option("ivf_scan", opt)
                call(qs[0])
                t = time.perf_counter()
                call(qs[0])
                first[opt] = (time.perf_counter() - t) * 1e3
                served[opt] = ivf.stats()["mid_tier_queries"]
                answers[opt] = (od.cpu().numpy().view(np.uint32).copy(), oi.cpu().numpy().copy())
            for opt in OPTIONS[1:]:
                assert np.array_equal(answers[opt][0], answers[0][0]) and np.array_equal(answers[opt][1], answers[0][1]), "the scans disagree"
            calls = int(min(100, max(3, args.window_ms / max(first.values()))))
            times = {name: [] for name in ("exact",) + OPTIONS}
            for _ in range(args.windows):
                times["exact"].append(window(exact, qs, calls))
                for opt in OPTIONS:
                    ivf.set_option("ivf_scan", opt)
                    times[opt].append(window(call, qs, calls))
            scan = {}
            ivf.set_option("profile", 1)
            for opt in OPTIONS[:2]:
                ivf.set_option("ivf_scan", opt)
                ms = []
                for c in range(calls):
                    call(qs[c % nbatch])
                    ms.append(ivf.stats()["scan_ms"])
                scan[opt] = statistics.median(ms) * 1e3
            ivf.set_option("profile", 0)

            def fig(name):
                return f"{statistics.median(times[name]):8.3f} [{min(times[name]):7.3f} .. {max(times[name]):7.3f}]"

            t0, t1 = statistics.median(times[0]), statistics.median(times[1])
            say(f"{nq:7d} {p:6d} {nq * min(p, nlist) / nlist:12.2f} {nq * min(p, nlist) / distinct:14.2f} | {statistics.median(times['exact']):10.3f} | "
                f"{fig(0)} {scan[0]:9.1f} | {fig(1)} {scan[1]:9.1f} {served[1]:7d} | {fig(-1)} {served[-1]:7d} | {t0 / t1:6.2f} x   ({calls} calls per window)")
    say()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    for index in (ivf, dense, coarse):
        index.close()


if __name__ == "__main__":
    main()
