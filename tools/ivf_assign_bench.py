#!/usr/bin/env python3
"""
Inverted-list builds with the MFMA assignment kernel (option "ivf_assign" = 1) against the sliced exact dense search (= 0),
one GPU, one session (profiles/ivf_assign.txt is this script's output, once per data set).

Four build steps on bench.py's row generator, each timed --repeats times per option, the options alternating (0, 1, 0, 1 ...),
host clock around the blocking calls named below and nothing else (an index is created before the window and read back
through lists() after it, in the last run of each option only), median [fastest .. slowest]:

    k-means        sq_ivf_kmeans over the sample (--sample rows, --iters iterations)
    flat add       sq_ivf_add of all rows, device memory, blocks of --add-block
    pq train       sq_pq_train, m = --m, 256 entries, over the sample (rows and codebooks in device memory)
    pq add         sq_pq_add of all rows, device memory, blocks of --add-block

The results of the two options are compared (centroids, codebooks, lists and codes must be equal).  For the two adds one
more index is filled with option "profile" = 1 on the handle: the stats then hold ivf_assign_kernel's own time (hipEvent
pairs around each launch, summed over the adds; no warm-up launch of its own -- the timed steps before it have run the
kernel), from which the FLOP rate 2 n (nlist d + m ksub dsub) / time is computed, and the undecided share.

    python tools/ivf_assign_bench.py --out profiles/ivf_assign.txt [--data clustered]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPQ_TFLOPS = 57.7   # opq_apply_kernel at d = 128, profiles/ivf_opq.txt: the yardstick


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--sample", type=int, default=1 << 20)
    ap.add_argument("--add-block", type=int, default=2_000_000)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--data", choices=["normal", "clustered"], default="normal")
    ap.add_argument("--out", default="", help="append the report here")
    args = ap.parse_args()

    import torch
    import bench
    from smqtk_indexing_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("ivf_assign_bench needs a GPU")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    n, d, nlist, m = args.rows, args.dim, args.nlist, args.m
    ksub, dsub = 256, d // m
    db = bench.make_rows(torch, args.data, n, d, dev, 3)
    torch.cuda.synchronize()
    rs = np.random.RandomState(0)
    sm = min(n, args.sample)
    sample = db[torch.from_numpy(np.sort(rs.choice(n, size=sm, replace=False))).to(dev)].cpu().numpy()
    init = sample[rs.choice(sm, size=nlist, replace=False)]
    books0 = np.ascontiguousarray(sample[rs.choice(sm, size=ksub, replace=False)].reshape(ksub, m, dsub).transpose(1, 0, 2))
    say(f"# ivf_assign, {_lib.device_name(0)[0]}: {n} x {d} float32 rows ({args.data}), nlist {nlist}, sample {sm}, {args.iters} iterations, PQ m {m} x {ksub}")

    def add_all(index, profile=0):
        index.set_option("profile", profile)
        launches = decided = fallback = 0
        ms = 0.0
        for s in range(0, n, args.add_block):
            index.add(db.data_ptr() + s * d * 4, n=min(n, s + args.add_block) - s, device_ptr=True)
            st = index.stats()
            launches, decided, fallback, ms = launches + st["scan_launches"], decided + st["candidates"], fallback + st["fallback_queries"], ms + st["scan_ms"]
        return launches, decided, fallback, ms

    state = {}
    sample_dev = torch.from_numpy(sample).to(dev)
    c_void = ctypes.c_void_p

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    # a step returns (seconds of the timed calls alone, result or None); `check`: the run whose result is compared --
    # creating the index, reading it back through lists() and closing it are outside the timed window
    def kmeans(check):
        return timed(lambda: _lib.ivf_kmeans(sample, init, args.iters))

    def pq_train(check):
        # rows and codebooks in device memory: a host-memory call's strided copy per sub-quantiser is the same under both options
        books = torch.from_numpy(books0).to(dev)
        sec, rc = timed(lambda: _lib.load_pq().sq_pq_train(c_void(sample_dev.data_ptr()), sm, d, m, ksub, c_void(books.data_ptr()), args.iters,
                                                           _lib.SQ_MEM_DEVICE))
        if rc != 0:
            raise SystemExit(f"sq_pq_train failed: {rc}")
        return sec, books.cpu().numpy()

    def add_step(make, label):
        def step(check):
            with make() as idx:
                sec, _ = timed(lambda: add_all(idx))
                if not check:
                    return sec, None
                read_s, got = timed(idx.lists)
                print(f"  ({label}: lists() of the finished index, outside the window: {read_s:.3f} s)", flush=True)
                return sec, got
        return step

    flat_add = add_step(lambda: _lib.IvfIndex(state["centroids"]), "flat add")
    pq_add = add_step(lambda: _lib.PqIndex(state["centroids"], state["books"]), "pq add")

    def same(a, b):
        a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
        return all(np.array_equal(u, v) for u, v in zip(a, b))

    wins = 0
    for name, fn, keep in (("k-means", kmeans, "centroids"), ("flat add", flat_add, None), ("pq train", pq_train, "books"), ("pq add", pq_add, None)):
        times, result = {0: [], 1: []}, {}
        for rep in range(args.repeats):
            for mode in (0, 1):
                _lib.set_option("ivf_assign", mode)
                try:
                    sec, got = fn(rep == args.repeats - 1)
                finally:
                    _lib.set_option("ivf_assign", 1)
                times[mode].append(sec)
                result[mode] = got
                print(f"  ({name} option {mode}: {sec:.3f} s)", flush=True)
        med = {k: statistics.median(v) for k, v in times.items()}
        wins += med[1] < med[0]
        say(f"{name:<9s} option 0: {med[0]:8.3f} s [{min(times[0]):.3f} .. {max(times[0]):.3f}]   option 1: {med[1]:8.3f} s "
            f"[{min(times[1]):.3f} .. {max(times[1]):.3f}]   {med[0] / med[1]:6.2f} x   results equal: {same(result[0], result[1])}")
        if keep:
            state[keep] = result[1]

    # the kernel alone: one more add per index kind with event timing (the kernels are warm from the steps above)
    for name, make, flop_row in (("flat add", lambda: _lib.IvfIndex(state["centroids"]), 2.0 * nlist * d),
                                 ("pq add", lambda: _lib.PqIndex(state["centroids"], state["books"]), 2.0 * (nlist * d + m * ksub * dsub))):
        with make() as idx:
            idx.set_option("ivf_assign", 1)
            launches, decided, fallback, ms = add_all(idx, profile=1)
        tf = flop_row * n / (ms * 1e-3) / 1e12 if ms > 0 else float("nan")
        say(f"{name:<9s} ivf_assign_kernel: {launches} launches, {ms:9.2f} ms, {tf:6.1f} TFLOP/s = {tf / OPQ_TFLOPS:.2f} x opq_apply_kernel's {OPQ_TFLOPS}; "
            f"undecided {fallback} of {decided + fallback} rows = {fallback / max(1, decided + fallback):.5f}")
    say(f"option 1 is the faster one in {wins} of 4 steps")
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
