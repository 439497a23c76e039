#!/usr/bin/env python3
"""
The PCA front stage on one GPU, one session (profiles/pca.txt is this script's output).

Part 1, the projection: sq_pca_apply from device memory at --apply-shapes (rows x d_in x d_out), beside (a) a device-to-device
copy of the input's bytes and (b) the only route there was before: sq_opq_apply with the projection zero padded to
d_in x d_in.  Each variant is timed by device events around windows of --calls enqueued calls, the windows alternating
between the variants, median [fastest .. slowest] over --windows.  FLOP and bytes are computed from the shapes:
2 n d_in d_out and 4 n (d_in + d_out).
Part 2, the moments: sq_pca_moments at --moment-shapes from device memory (host clock around the blocking call) and from
host memory, beside numpy's float64 X.T @ X on the host in the same run.
Part 3, the index: a clustered set of --rows x --dim, IVF-Flat at full width against IVF-Flat behind a projection to
--pca-dims: build seconds, resident bytes, the --nq-query device call at each nprobe (alternating windows), recall@k against
the exact index.

    python tools/pca_bench.py --out profiles/pca.txt
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_windows(torch, variants, calls, n_windows):
    """{name: sorted seconds per call}, by device events; windows alternate between the variants."""
    out = {name: [] for name in variants}
    for _ in range(n_windows):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _c in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) * 1e-3 / calls)
    return {name: sorted(v) for name, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--apply-shapes", default="2000000x2048x256,2000000x2048x64,1000000x4096x256")
    ap.add_argument("--moment-shapes", default="262144x2048,1048576x128")
    ap.add_argument("--rows", type=int, default=2_000_000, help="rows of the indexes of part 3 (0: skip the part)")
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--pca-dims", type=int, default=256)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--nq", type=int, default=32)
    ap.add_argument("--nprobes", default="1,4,16,64")
    ap.add_argument("--sample", type=int, default=262_144, help="rows the projection and the centroids are trained on")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--add-block", type=int, default=500_000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import bench
    from smqtk_indexing_amd import _lib
    from smqtk_indexing_amd.impls.nn_index.hip_ivf_pca import principal_axes
    if _lib.device_count() < 1:
        raise SystemExit("pca_bench needs a GPU")
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    stream = torch.cuda.current_stream().cuda_stream
    def say(s=""):
        print(s, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(s + "\n")

    def fmt(v):
        return f"{statistics.median(v) * 1e3:8.3f} ms [{v[0] * 1e3:.3f} .. {v[-1] * 1e3:.3f}]"

    say(f"# PCA front stage, {_lib.device_name(0)[0]}")
    # ------------------------------------------------------------------ part 1
    for shape in filter(None, args.apply_shapes.split(",")):
        n, d_in, d_out = (int(v) for v in shape.split("x"))
        x = torch.randn((n, d_in), dtype=torch.float32, device=dev)
        y = torch.empty((n, d_out), dtype=torch.float32, device=dev)
        wide = torch.empty_like(x)            # the copy's and the padded OPQ route's destination
        rs = np.random.RandomState(1)
        a = np.linalg.qr(rs.standard_normal((d_in, d_out)))[0].T.astype(np.float32)
        padded = np.zeros((d_in, d_in), dtype=np.float32)
        padded[:d_out] = a
        with _lib.PcaTransform(a, rs.standard_normal(d_in).astype(np.float32)) as t, _lib.OpqTransform(padded) as o:
            variants = {"pca": lambda: t.apply_device(x.data_ptr(), n, y.data_ptr(), stream), "copy": lambda: wide.copy_(x),
                        "opq padded": lambda: o.apply_device(x.data_ptr(), n, wide.data_ptr(), stream)}
            for fn in variants.values():
                fn()
            res = event_windows(torch, variants, args.calls, args.windows)
        med = {name: statistics.median(v) for name, v in res.items()}
        say(f"apply {n} x {d_in} -> {d_out}: pca {fmt(res['pca'])}   d2d copy of the input {fmt(res['copy'])}   "
            f"opq padded to {d_in} x {d_in} {fmt(res['opq padded'])}")
        say(f"    pca: {2.0 * n * d_in * d_out / med['pca'] / 1e12:.1f} TFLOP/s float32 MFMA from shapes, "
            f"{4.0 * n * (d_in + d_out) / med['pca'] / 1e9:.0f} GB/s read + written; opq padded / pca = {med['opq padded'] / med['pca']:.2f} "
            f"(FLOP ratio {d_in / d_out:.0f}); pca / copy = {med['pca'] / med['copy']:.2f}")
        del x, y, wide
    # ------------------------------------------------------------------ part 2
    for shape in filter(None, args.moment_shapes.split(",")):
        n, d = (int(v) for v in shape.split("x"))
        xd = torch.randn((n, d), dtype=torch.float32, device=dev) + 2
        md = torch.empty(d, dtype=torch.float32, device=dev)
        sd = torch.empty((d, d), dtype=torch.float64, device=dev)
        lib = _lib.load_pca()

        def on_device():
            _lib._check(lib.sq_pca_moments(xd.data_ptr(), n, d, md.data_ptr(), sd.data_ptr(), _lib.SQ_MEM_DEVICE), "sq_pca_moments")

        on_device()
        times = []
        for _ in range(args.windows):
            sync()
            t0 = time.perf_counter()
            on_device()
            times.append(time.perf_counter() - t0)
        xh = xd.cpu().numpy()
        t0 = time.perf_counter()
        _lib.pca_moments(xh)
        t_host_call = time.perf_counter() - t0
        t0 = time.perf_counter()
        x64 = xh.astype(np.float64)
        x64 -= x64.mean(axis=0)
        x64.T @ x64
        t_numpy = time.perf_counter() - t0
        times.sort()
        say(f"moments {n} x {d}: device memory {fmt(times)} ({1.0 * n * d * d / statistics.median(times) / 1e12:.1f} TFLOP/s of the "
            f"triangle's n d^2)   host memory, copies included {t_host_call:.3f} s   numpy float64 centre + X.T @ X {t_numpy:.3f} s")
        del xd, sd
    # ------------------------------------------------------------------ part 3
    n, d, k, nq, nlist = args.rows, args.dim, args.k, args.nq, args.nlist
    if n:
        nprobes = [int(v) for v in args.nprobes.split(",")]
        db = bench.make_rows(torch, "clustered", n, d, dev, 3)
        qs = bench.make_rows(torch, "clustered", nq, d, dev, 1234)
        sync()
        say(f"## index: clustered {n} x {d}, nlist {nlist}, pca_dims {args.pca_dims}, k {k}, {nq} queries, sample {args.sample}")
        rs = np.random.RandomState(0)
        sample = db[torch.from_numpy(np.sort(rs.choice(n, size=min(n, args.sample), replace=False))).to(dev)].cpu().numpy()
        init = rs.choice(len(sample), size=nlist, replace=False)
        od = torch.empty((nq, k), dtype=torch.float32, device=dev)
        oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
        dense = _lib.DenseIndex(db.data_ptr(), n=n, d=d, device_ptr=True, keepalive=db)
        dense.search_device(qs.data_ptr(), nq, k, od.data_ptr(), oi.data_ptr(), stream)
        sync()
        truth = oi.cpu().numpy()
        dense.close()
        calls = {}
        for label in ("full width", "PCA"):
            t0 = time.perf_counter()
            t = None
            if label == "PCA":
                mean, scatter = _lib.pca_moments(sample)
                t = _lib.PcaTransform(principal_axes(scatter, len(sample), args.pca_dims), mean)
            smp = sample if t is None else t.apply(sample)
            t_train = time.perf_counter() - t0
            cent = _lib.ivf_kmeans(smp, smp[init], 10)
            index = _lib.IvfIndex(cent)
            blk = torch.empty((min(n, args.add_block), smp.shape[1]), dtype=torch.float32, device=dev)
            for s in range(0, n, args.add_block):
                r_n = min(n, s + args.add_block) - s
                src = db.data_ptr() + s * d * 4
                if t is not None:
                    t.apply_device(src, r_n, blk.data_ptr(), stream)
                    sync()
                    src = blk.data_ptr()
                index.add(src, n=r_n, device_ptr=True)
            sync()
            say(f"{label}: build {time.perf_counter() - t0:.2f} s (of it moments + eigh + projecting the sample {t_train:.2f} s), "
                f"resident bytes {sum(v for key, v in index.info().items() if key.endswith('_bytes'))}")
            qr = torch.empty((nq, smp.shape[1]), dtype=torch.float32, device=dev)

            def call(p, t=t, index=index, qr=qr):
                q = qs.data_ptr()
                if t is not None:
                    t.apply_device(q, nq, qr.data_ptr(), stream)
                    q = qr.data_ptr()
                index.search_device(q, nq, k, p, od.data_ptr(), oi.data_ptr(), stream)

            calls[label] = (call, index, t)
        for p in nprobes:
            recalls = {}
            for label, (fn, _, _) in calls.items():
                fn(p)
                sync()
                found = oi.cpu().numpy()
                recalls[label] = np.mean([len(set(f.tolist()) & set(e.tolist())) / k for f, e in zip(found, truth)])
            got = {label: [] for label in calls}
            for _ in range(args.windows):
                for label, (fn, _, _) in calls.items():
                    sync()
                    t0 = time.perf_counter()
                    for _c in range(args.calls):
                        fn(p)
                    sync()
                    got[label].append((time.perf_counter() - t0) / args.calls)
            say(f"nprobe {p}: " + "   ".join(f"{label} {fmt(sorted(v))} recall@{k} {recalls[label]:.3f}" for label, v in got.items()))
        for _, index, t in calls.values():
            index.close()
            if t is not None:
                t.close()


if __name__ == "__main__":
    main()
