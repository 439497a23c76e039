#!/usr/bin/env python
"""
What sq_dense_remove / sq_dense_compact cost and what they save (profiles/r06_dense_remove.txt).

    python tools/dense_remove_bench.py step    [--remove-frac 0.01]   pipelined 32-query steps as bench.py runs them
    python tools/dense_remove_bench.py hostway [--remove-frac 0.01]   the host's way round: search(k + dead) + np.isin
    python tools/dense_remove_bench.py mutate                         remove 1 k / 100 k ids, compact at 25 % removed,
                                                                      against sq_dense_create of the survivors from host memory

`--lib PATH` loads another build of libsmqtk_hip.so (a library built from the parent commit knows `step` without
removal, `hostway`, and the create half of `mutate`).  One JSON line per run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["step", "hostway", "mutate"])
    ap.add_argument("--lib", default="")
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--queries", type=int, default=32)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--remove-frac", type=float, default=0.0)
    args = ap.parse_args()
    if args.lib:
        os.environ["SMQTK_HIP_LIBRARY"] = os.path.abspath(args.lib)
    import torch
    from smqtk_indexing_amd import _lib

    dev = torch.device("cuda", 0)
    n, d, k, nq = args.rows, args.dim, args.k, args.queries
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    db = torch.empty((n, d), dtype=torch.float32, device=dev)
    for s in range(0, n, 1 << 21):
        db[s:s + (1 << 21)].normal_(generator=g)
    qs = [torch.empty((nq, d), dtype=torch.float32, device=dev).normal_(generator=g) for _ in range(8)]
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(2)
    out = {"mode": args.mode, "lib": args.lib or "tree", "rows": n, "dim": d, "k": k, "queries": nq}

    if args.mode in ("step", "hostway"):
        index = _lib.DenseIndex(db.data_ptr(), n=n, d=d, device_ptr=True, keepalive=db)
        dead = np.sort(rng.choice(n, int(n * args.remove_frac), replace=False)) if args.remove_frac > 0 else np.zeros(0, np.int64)
        out["removed"] = int(len(dead))
    if args.mode == "step":
        if len(dead):
            t0 = time.perf_counter()
            index.remove(dead)
            out["remove_ms"] = (time.perf_counter() - t0) * 1e3
        od = [torch.empty((nq, k), dtype=torch.float32, device=dev) for _ in range(2)]
        oi = [torch.empty((nq, k), dtype=torch.int64, device=dev) for _ in range(2)]
        ms = []
        for _ in range(args.runs):
            for phase, steps in (("warm", args.warmup), ("timed", args.steps)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(steps):
                    index.search_device_async(qs[i % 8].data_ptr(), nq, k, od[i & 1].data_ptr(), oi[i & 1].data_ptr(), stream)
                index.sync()
                torch.cuda.synchronize()
                if phase == "timed":
                    ms.append((time.perf_counter() - t0) * 1e3 / steps)
        out["step_ms"] = [round(v, 4) for v in ms]
        out["stats"] = {k_: v for k_, v in index.stats().items() if k_ in ("fallback_queries", "mid_tier_queries", "bytes_scanned", "scan_launches")}
        if len(dead):
            got = oi[(args.steps - 1) & 1].cpu().numpy()
            assert not np.isin(got, dead).any(), "a removed row was returned"
    elif args.mode == "hostway":
        # what the plugin did before: ask for k + dead neighbours, drop the dead ones on the host
        kk = k + len(dead)
        od = torch.empty((nq, kk), dtype=torch.float32, device=dev)
        oi = torch.empty((nq, kk), dtype=torch.int64, device=dev)
        ms = []
        for r in range(args.runs + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            index.search_device(qs[r % 8].data_ptr(), nq, kk, od.data_ptr(), oi.data_ptr(), stream)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            idx, dist = oi.cpu().numpy(), od.cpu().numpy()
            live = ~np.isin(idx, dead)
            pos = np.argsort(~live, axis=1, kind="stable")[:, :k]
            np.take_along_axis(idx, pos, axis=1), np.take_along_axis(dist, pos, axis=1)
            t2 = time.perf_counter()
            if r:   # (the first call sizes the workspace)
                ms.append([round((t1 - t0) * 1e3, 3), round((t2 - t1) * 1e3, 3)])
        out["search_ms_then_host_filter_ms"] = ms
    else:
        dbh = db.cpu().numpy()
        res = {"remove_1k_ms": [], "remove_100k_ms": [], "compact_25pct_ms": [], "create_survivors_from_host_ms": []}
        have_remove = hasattr(_lib.load(), "sq_dense_remove")
        dead25 = np.sort(rng.choice(n, n // 4, replace=False))
        keep = np.ones(n, dtype=bool)
        keep[dead25] = False
        survivors = np.ascontiguousarray(dbh[keep])
        for _ in range(args.runs):
            t0 = time.perf_counter()
            fresh = _lib.DenseIndex(survivors)
            res["create_survivors_from_host_ms"].append(round((time.perf_counter() - t0) * 1e3, 2))
            out["create_build_ms_from_info"] = fresh.info()["build_ms"]
            fresh.close()
            if not have_remove:
                continue
            index = _lib.DenseIndex(dbh)
            a, b, c = dead25[:1000], dead25[1000:101_000], dead25[101_000:]
            for name, ids in (("remove_1k_ms", a), ("remove_100k_ms", b), (None, c)):
                t0 = time.perf_counter()
                index.remove(ids)
                if name:
                    res[name].append(round((time.perf_counter() - t0) * 1e3, 3))
            t0 = time.perf_counter()
            o2n = index.compact()
            res["compact_25pct_ms"].append(round((time.perf_counter() - t0) * 1e3, 2))
            assert index.count() == (len(survivors), len(survivors)) and (o2n[dead25] == -1).all()
            index.close()
        out.update(res)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
