#!/usr/bin/env python3
"""
The OPQ transform and the index behind it on one GPU, one session (profiles/ivf_opq.txt is this script's output).

Part 1, the kernel: sq_opq_apply from device memory at --apply-shapes (rows x d), beside a device-to-device copy of the same
bytes (the floor: the kernel reads and writes n d 4 bytes each).  Windows of --calls enqueued calls ended by a synchronise,
host clock, alternating between the two, median [fastest .. slowest] over --windows; the executed float32 MFMA rate is
2 n d^2 over the median (the flops of the padded tiles are not counted).
Part 2, recall and call overhead, per data set ("clustered": bench.py's generator; "correlated": the same rows times a fixed
random matrix with a decaying spectrum, `correlated` below): IVF-PQ plain and residual with and without the rotation, same
sample, same codebook budget (the loop's inner iterations are OPQ's own).  Training time split into apply, sq_pq_train,
coding and host (decode + cross product + SVD); recall@k of the coded answer against the exact index; the 32-query blocking
device call at each nprobe, with the rotation (one sq_opq_apply of 32 rows, then sq_pq_search) and without, alternating
windows.

    python tools/opq_bench.py --out profiles/ivf_opq.txt
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def correlated(torch, rows, seed=77, decay=0.97):
    """rows @ M, M = U diag(decay^i) V^T for seeded orthonormal U, V: correlated columns, energy spread unevenly."""
    d = rows.shape[1]
    rs = np.random.RandomState(seed)
    u, v = (np.linalg.qr(rs.standard_normal((d, d)))[0] for _ in range(2))
    mat = (u * decay ** np.arange(d)) @ v.T
    return rows @ torch.from_numpy(mat.astype(np.float32)).to(rows.device)


def windows(shapes, calls, n_windows, sync):
    """{name: sorted seconds per call}: windows alternate between the shapes."""
    out = {name: [] for name in shapes}
    for _ in range(n_windows):
        for name, fn in shapes.items():
            sync()
            t0 = time.perf_counter()
            for c in range(calls):
                fn(c)
            sync()
            out[name].append((time.perf_counter() - t0) / calls)
    return {name: sorted(v) for name, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--apply-shapes", default="10000000x128,1000000x1024")
    ap.add_argument("--rows", type=int, default=10_000_000, help="rows of the indexes of part 2")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--nq", type=int, default=32)
    ap.add_argument("--nprobes", default="1,4,16,64")
    ap.add_argument("--recall-nprobe", type=int, default=16)
    ap.add_argument("--sample", type=int, default=65_536, help="rows the rotation and the codebooks are trained on")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--add-block", type=int, default=2_000_000)
    ap.add_argument("--sets", default="clustered,correlated")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import bench
    from smqtk_indexing_amd import _lib
    from smqtk_indexing_amd.impls.nn_index import hip_ivf_opq as H
    if _lib.device_count() < 1:
        raise SystemExit("opq_bench needs a GPU")
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    stream = torch.cuda.current_stream().cuda_stream
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def fmt(v):
        return f"{statistics.median(v) * 1e3:8.3f} ms [{v[0] * 1e3:.3f} .. {v[-1] * 1e3:.3f}]"

    say(f"# OPQ transform and index, {_lib.device_name(0)[0]}")
    # ------------------------------------------------------------------ part 1
    for shape in args.apply_shapes.split(","):
        n, d = (int(v) for v in shape.split("x"))
        x = torch.randn((n, d), dtype=torch.float32, device=dev)
        y = torch.empty_like(x)
        rot = np.linalg.qr(np.random.RandomState(1).standard_normal((d, d)))[0].astype(np.float32)
        with _lib.OpqTransform(rot) as t:
            shapes = {"apply": lambda c: t.apply_device(x.data_ptr(), n, y.data_ptr(), stream), "copy": lambda c: y.copy_(x)}
            for fn in shapes.values():
                fn(0)
            res = windows(shapes, args.calls, args.windows, sync)
        med = statistics.median(res["apply"])
        say(f"apply {n} x {d}: {fmt(res['apply'])}   d2d copy of the same bytes {fmt(res['copy'])}   "
            f"{2 * n * d * 4 / med / 1e9:.0f} GB/s read + written, {2.0 * n * d * d / med / 1e12:.1f} TFLOP/s float32 MFMA executed")
        del x, y
    # ------------------------------------------------------------------ part 2
    n, d, k, nq, m, nlist = args.rows, args.dim, args.k, args.nq, args.m, args.nlist
    nprobes = [int(v) for v in args.nprobes.split(",")]
    for name in args.sets.split(","):
        db = bench.make_rows(torch, "clustered", n, d, dev, 3)
        qs = bench.make_rows(torch, "clustered", nq, d, dev, 1234)
        if name == "correlated":
            db, qs = correlated(torch, db), correlated(torch, qs)
        sync()
        say(f"## {name}: {n} x {d}, nlist {nlist}, m {m}, k {k}, {nq} queries, sample {args.sample}")
        rs = np.random.RandomState(0)
        sample = db[torch.from_numpy(np.sort(rs.choice(n, size=min(n, args.sample), replace=False))).to(dev)].cpu().numpy()
        init = rs.choice(len(sample), size=nlist, replace=False)
        entries = rs.choice(len(sample), size=256, replace=False)
        prof = {}
        t0 = time.perf_counter()
        rot = H.train_rotation(sample, entries, m, H.initial_rotation(rs, d), 10, prof)
        total = time.perf_counter() - t0
        say("training the rotation, 10 iterations: %.2f s = apply %.2f + sq_pq_train %.2f + coding %.2f + host (decode, cross product, SVD) %.2f"
            % (total, prof["apply"], prof["pq_train"], prof["coding"], prof["host"]))
        dense = _lib.DenseIndex(db.data_ptr(), n=n, d=d, device_ptr=True, keepalive=db)
        od = torch.empty((nq, k), dtype=torch.float32, device=dev)
        oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
        qr = torch.empty_like(qs)
        blk = torch.empty((min(n, args.add_block), d), dtype=torch.float32, device=dev)
        sync()
        dense.search_device(qs.data_ptr(), nq, k, od.data_ptr(), oi.data_ptr(), stream)
        truth = oi.cpu().numpy()
        calls = {}
        with _lib.OpqTransform(rot) as t:
            for label, r in (("no rotation", None), ("OPQ", t)):
                smp = sample if r is None else r.apply(sample)
                cent = _lib.ivf_kmeans(smp, smp[init], 10)
                for residual in (False, True):
                    coded = _lib.pq_residuals(smp, cent) if residual else smp
                    books = _lib.pq_train(coded, np.ascontiguousarray(coded[entries].reshape(256, m, d // m).transpose(1, 0, 2)), 10)
                    index = _lib.PqIndex(cent, books, residual=residual)
                    for s in range(0, n, args.add_block):
                        r_n = min(n, s + args.add_block) - s
                        src = db.data_ptr() + s * d * 4
                        if r is not None:
                            r.apply_device(src, r_n, blk.data_ptr(), stream)
                            sync()
                            src = blk.data_ptr()
                        index.add(src, n=r_n, device_ptr=True)

                    def call(p, r=r, index=index):
                        q = qs.data_ptr()
                        if r is not None:
                            r.apply_device(q, nq, qr.data_ptr(), stream)
                            q = qr.data_ptr()
                        index.search_device(q, nq, k, p, od.data_ptr(), oi.data_ptr(), stream)

                    call(args.recall_nprobe)
                    found = oi.cpu().numpy()
                    recall = np.mean([len(set(f.tolist()) & set(e.tolist())) / k for f, e in zip(found, truth)])
                    say(f"recall@{k} at nprobe {args.recall_nprobe}: {'residual' if residual else 'plain':<8s} {label:<11s} {recall:.3f}")
                    calls[(label, residual)] = (call, index)
            for p in nprobes:
                shapes = {f"{'residual' if res else 'plain'} {label}": (lambda c, fn=fn: fn(p)) for (label, res), (fn, _) in calls.items()}
                for fn in shapes.values():
                    fn(0)
                got = windows(shapes, args.calls, args.windows, sync)
                say(f"{nq}-query call at nprobe {p}: " + "   ".join(f"{nm} {fmt(v)}" for nm, v in got.items()))
            for _, index in calls.values():
                index.close()
        dense.close()
        del db, dense
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
