#!/usr/bin/env python3
"""
The refine stage on one GPU, one session (profiles/ivf_refine.txt is this script's output, once per data set).

Rows, queries, centroids, 8-bit ranges and residual codebooks are tools/isq_bench.py's (bench.py's generators, a sample of
256 rows per list, RandomState(0)); the codebooks are trained on the first --book-sample residuals of that sample, and the
packed index gets 16-entry codebooks from the same draw.

Part 1, recall and call time: residual IVF-PQ (m = --m; one-byte and packed 4-bit codes) behind an F16 and an SQ8 store at
k_factor 1 .. 16, beside the unrefined bases, IVF-SQfp16 and IVF-Flat.  Blocking device calls in alternating windows of
--calls calls over 8 rotating query batches, host clock, median [fastest .. slowest]; recall@k of the ids as returned
against the exact index on the same queries; resident bytes of every index and store.

Part 2, the kernel alone: refine_rerank_kernel with the LDS-staged gather (option "refine_direct" = 0) against the
direct-load variant (= 1) at 32 queries x kb 400 and 1600.  A window is one launch over each of --lists distinct
candidate lists (scattered distinct rows; together several hundred MB of code rows, beyond the 256 MB MALL, so a launch
finds none of its rows cached from the window before); the figure is the sum of the launches' hipEvent times (option
"profile") per launch, windows alternate between the variants, median and spread (max - min) / median over --windows.
For the F32 store the same lists go through sq_rows_rerank (rows_rerank_keys_kernel, which has no event timing) and
through sq_refine_rerank as host-memory calls: whole-call time, host clock.

    python tools/refine_bench.py --out profiles/ivf_refine.txt [--data clustered]
"""
import argparse
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
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--nprobes", default="16,64")
    ap.add_argument("--batches", default="32,1")
    ap.add_argument("--factors", default="1,2,4,8,16")
    ap.add_argument("--calls", type=int, default=40, help="calls per timed window (part 1)")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--lists", type=int, default=200, help="distinct candidate lists per window at kb 400 (part 2; kb 1600: a quarter)")
    ap.add_argument("--book-sample", type=int, default=65_536, help="residuals the codebooks are trained on (as profiles/ivf_pq_packed.txt)")
    ap.add_argument("--add-block", type=int, default=2_000_000)
    ap.add_argument("--data", choices=["normal", "clustered"], default="normal")
    ap.add_argument("--no-kernel", action="store_true", help="part 1 only")
    ap.add_argument("--hbm-peak", type=float, default=8000.0, help="GB/s the gathered byte rate is given against")
    ap.add_argument("--out", default="", help="append the report here")
    args = ap.parse_args()

    import torch
    import bench
    from smqtk_indexing_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("refine_bench needs a GPU")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    n, d, k, nlist, m = args.rows, args.dim, args.k, args.nlist, args.m
    nprobes = [int(v) for v in args.nprobes.split(",")]
    batches = [int(v) for v in args.batches.split(",")]
    factors = [int(v) for v in args.factors.split(",")]
    db = bench.make_rows(torch, args.data, n, d, dev, 3)
    nbatch = 8
    all_q = bench.make_rows(torch, args.data, max(batches) * nbatch, d, dev, 1234)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    say(f"# refine stage, {_lib.device_name(0)[0]}: {n} x {d} float32 rows ({args.data}), nlist {nlist}, k {k}, residual PQ m {m}")

    rs = np.random.RandomState(0)
    sm = min(n, 256 * nlist)
    sample = db[torch.from_numpy(np.sort(rs.choice(n, size=sm, replace=False))).to(dev)].cpu().numpy()
    init = sample[rs.choice(sm, size=nlist, replace=False)]
    entry_rows = rs.choice(sm, size=min(256, sm), replace=False)
    centroids = _lib.ivf_kmeans(sample, init, args.iters)
    vmin, step = _lib.isq_train(sample)
    sample_res = _lib.pq_residuals(sample, centroids)
    books = {}
    for name, entries in (("rpq", entry_rows), ("rpq4", entry_rows[:16])):
        books0 = np.ascontiguousarray(sample_res[entries].reshape(len(entries), m, d // m).transpose(1, 0, 2))
        books[name] = _lib.pq_train(sample_res[:args.book_sample], books0, args.iters)
    matrix_bytes = n * d * 4

    def made(name, index, fields):
        for s in range(0, n, args.add_block):
            index.add(db.data_ptr() + s * d * 4, n=min(n, s + args.add_block) - s, device_ptr=True)
        info = index.info()
        res = sum(info[f] for f in fields)
        say(f"resident {name:<10s} {res:>12d} bytes = {res / matrix_bytes:.4f} x the matrix")
        return index, res

    pq_fields = ("codes_bytes", "ids_offsets_bytes", "books_coarse_bytes")
    isq_fields = ("codes_bytes", "ids_offsets_bytes", "coarse_params_bytes")
    store_fields = ("codes_bytes", "params_bytes")
    bases = {"rpq": made("rpq", _lib.PqIndex(centroids, books["rpq"], residual=True), pq_fields),
             "rpq4": made("rpq4", _lib.PqIndex(centroids, books["rpq4"], residual=True, packed=True), pq_fields)}
    others = {"isq-f16": made("isq-f16", _lib.IsqIndex(centroids, _lib.SQ_ISQ_F16), isq_fields),
              "flat": made("flat", _lib.IvfIndex(centroids), ("rows_bytes", "ids_offsets_bytes", "coarse_bytes"))}
    stores = {"f16": made("store-f16", _lib.RefineStore(d, _lib.SQ_REFINE_F16), store_fields),
              "sq8": made("store-sq8", _lib.RefineStore(d, _lib.SQ_REFINE_SQ8, vmin, step), store_fields)}
    for b, (_, bres) in bases.items():
        for s, (_, sres) in stores.items():
            say(f"resident {b + '+' + s:<10s} {bres + sres:>12d} bytes = {(bres + sres) / matrix_bytes:.4f} x the matrix")
    dense = _lib.DenseIndex(db.data_ptr(), n=n, d=d, device_ptr=True, keepalive=db)

    # ------------------------------------------------------------------ part 1
    for nq in batches:
        qs = [all_q[j * nq:(j + 1) * nq].contiguous() for j in range(nbatch)]
        od = torch.empty((nq, k), dtype=torch.float32, device=dev)
        oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        out = (od.data_ptr(), oi.data_ptr(), stream)
        truth = []
        for j in range(nbatch):
            dense.search_device(qs[j].data_ptr(), nq, k, *out)
            truth.append(oi.cpu().numpy())
        for p in nprobes:
            shapes = {}
            for name, (ix, _) in list(bases.items()) + list(others.items()):
                shapes[name] = (lambda ix_: lambda q: ix_.search_device(q.data_ptr(), nq, k, p, *out))(ix)
            for b, (bix, _) in bases.items():
                for s, (six, _) in stores.items():
                    for f in factors:
                        shapes[f"{b}+{s} x{f}"] = (lambda bix_, six_, f_: lambda q: six_.search_device(bix_, q.data_ptr(), nq, k, k * f_, p, *out))(bix, six, f)
            recall = {}
            for name, call in shapes.items():           # answers once: recall, and the warm-up of every shape
                hits = 0
                for j in range(nbatch):
                    call(qs[j])
                    got = oi.cpu().numpy()
                    hits += sum(len(np.intersect1d(got[i], truth[j][i])) for i in range(nq))
                recall[name] = hits / (nbatch * nq * k)
            times = {name: [] for name in shapes}
            for _ in range(args.windows):
                for name, call in shapes.items():
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    for c in range(args.calls):
                        call(qs[c % nbatch])
                    times[name].append((time.perf_counter() - t) / args.calls * 1e3)
            say()
            say(f"## {nq} quer{'y' if nq == 1 else 'ies'} per blocking call, nprobe {p} ({args.windows} windows of {args.calls} calls; median [fastest .. slowest] ms per call)")
            for name in shapes:
                t = times[name]
                say(f"{name:<14s} recall@{k} {recall[name]:.3f}   {statistics.median(t):7.3f} [{min(t):.3f} .. {max(t):.3f}] ms")

    # ------------------------------------------------------------------ part 2
    if not args.no_kernel:
        for ix, _ in list(bases.values()) + list(others.values()):
            ix.close()
        nq = 32
        q = all_q[:nq].contiguous()
        od = torch.empty((nq, k), dtype=torch.float32, device=dev)
        oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
        stores["f32"] = made("store-f32", _lib.RefineStore(d, _lib.SQ_REFINE_F32), store_fields)
        rng = np.random.default_rng(0)

        def scattered(kb):   # kb distinct rows far apart: a random start and a stride coprime to the row count
            while True:
                s = int(rng.integers(n // 16, n)) | 1
                if np.gcd(s, n) == 1:
                    return (int(rng.integers(n)) + np.arange(kb, dtype=np.int64) * s) % n

        say()
        say(f"## refine_rerank_kernel alone, {nq} queries: LDS-staged gather against direct loads, us per launch (sum of hipEvent times over a window of")
        say(f"## distinct candidate lists / launches; median of {args.windows} alternating windows, spread = (max - min) / median)")
        say("kind  kb    lists  window_MB  staged_us spread  direct_us spread  staged/direct  direct_GB/s  of_peak")
        for kb in (400, 1600):
            nl = max(8, args.lists * 400 // kb)
            cand_host = np.stack([np.stack([scattered(kb) for _ in range(nq)]) for _ in range(nl)])
            cand = torch.from_numpy(cand_host).to(dev)
            torch.cuda.synchronize()
            for name in ("sq8", "f16", "f32"):
                store = stores[name][0]
                store.set_option("profile", 1)
                stride = store.info()["row_stride_bytes"]
                us = {0: [], 1: []}
                for w in range(args.windows + 1):
                    for direct in (0, 1):
                        store.set_option("refine_direct", direct)
                        tot = 0.0
                        for li in range(nl):
                            store.rerank_device(q.data_ptr(), nq, cand[li].data_ptr(), kb, k, od.data_ptr(), oi.data_ptr(), stream)
                            tot += store.stats()["scan_ms"]
                        if w:                                          # the first window warms up
                            us[direct].append(tot / nl * 1e3)
                store.reset_options()
                med = {v: statistics.median(us[v]) for v in us}
                spread = {v: (max(us[v]) - min(us[v])) / med[v] for v in us}
                gbs = nq * kb * stride / (med[1] * 1e-6) / 1e9
                say(f"{name:<4s}  {kb:<4d}  {nl:<5d}  {nl * nq * kb * stride / 1e6:9.0f}  {med[0]:9.1f} {spread[0]:6.2f}  {med[1]:9.1f} {spread[1]:6.2f}  "
                    f"{med[0] / med[1]:13.2f}  {gbs:11.1f}  {gbs / args.hbm_peak:7.3f}")
            # F32 rows: the LSH tail's re-rank (sq_rows_rerank) against sq_refine_rerank, host-memory calls on the same lists
            rows = _lib.RowMatrix(db.data_ptr(), n=n, d=d, dtype=np.float32, device_ptr=True, keepalive=db)
            qh = q.cpu().numpy()
            off = np.arange(nq + 1, dtype=np.int64) * kb
            store = stores["f32"][0]
            calls = {"sq_rows_rerank": lambda li: rows.rerank(qh, _lib.SQ_METRIC_L2, cand_host[li].reshape(-1), off, k),
                     "sq_refine_rerank": lambda li: store.rerank(qh, cand_host[li], k)}
            ms = {name: [] for name in calls}
            for w in range(args.windows + 1):
                for name, call in calls.items():
                    t = time.perf_counter()
                    for li in range(nl):
                        call(li)
                    if w:
                        ms[name].append((time.perf_counter() - t) / nl * 1e3)
            say(f"f32   {kb:<4d}  whole host-memory call, ms: " + "   ".join(
                f"{name} {statistics.median(v):.3f} [{min(v):.3f} .. {max(v):.3f}]" for name, v in ms.items()))
            rows.close()
    say()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
