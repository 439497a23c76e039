#!/usr/bin/env python3
"""Measurement helper: the int8 first stage for rows of 513 .. 8192 dimensions (sq_dense_i8_wide.hpp, option
"dense_int8_wide") against the bfloat16 chain on the SAME index in the same process ("dense_int8" = 0 on the handle is
the call an index without the copy makes).  32 queries per step over a device-resident matrix; per metric and filter:
the pipelined step (SQ_MEM_DEVICE_ASYNC, depth 2, wall time over --steps calls after --warmup), the full pass's own
duration from profiled blocking calls (sq_stats_t.scan_ms, median) and its fraction of the HBM peak, the rows re-ranked
per query, fallback queries, and the index's build time and resident bytes (sq_dense_info).

    python tools/int8_wide_bench.py                       # the two shapes of profiles/int8_wide.txt
    python tools/int8_wide_bench.py --shapes 200000x1000  # any n x d
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from smqtk_indexing_amd import _lib  # noqa: E402

HBM_PEAK = 8.0e12
SHAPES = "1000000x4096,2000000x2048"


def run(n, d, metric, name, k, steps, warmup):
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x = torch.empty((n, d), dtype=torch.float32, device=dev)
    step = max(1, (1 << 28) // d)
    for s in range(0, n, step):
        x[s:s + step].normal_(generator=g)
    idx = _lib.DenseIndex(x.data_ptr(), n=n, d=d, metric=metric, device_ptr=True, keepalive=x, options={"dense_int8_wide": 1})
    info = idx.info()
    print(f"n={n} d={d} {name}: build {info['build_ms']:.1f} ms (int8 copy {info['build_int8_ms']:.1f} ms); resident: float32 rows "
          f"{info['f32_rows_bytes']} B, bfloat16 copy {info['bf16_copy_bytes']} B, int8 copy {info['int8_copy_bytes']} B; "
          f"int8 in use: {info['int8_in_use']}", flush=True)
    rows = torch.randint(0, n, (4, 32), generator=torch.Generator().manual_seed(2))
    qs = [(x[r.to(dev)] + 0.05 * torch.randn((32, d), device=dev, generator=g)).contiguous() for r in rows]
    ddt = torch.float64 if metric == _lib.SQ_METRIC_COSINE else torch.float32
    od = [torch.empty((32, k), dtype=ddt, device=dev) for _ in range(2)]
    oi = [torch.empty((32, k), dtype=torch.int64, device=dev) for _ in range(2)]
    keep = {}
    for tag, int8 in (("bfloat16", 0), ("int8", 1)):
        if int8 and not info["int8_in_use"]:
            print("   the build declined the int8 copy for this data", flush=True)
            continue
        idx.set_option("dense_int8", int8)
        idx.set_option("profile", 1)
        scan, cand, fb, nbytes = [], [], 0, 0
        for j in range(2 + 5):                       # two warm-up calls
            idx.search_device(qs[j % 4].data_ptr(), 32, k, od[0].data_ptr(), oi[0].data_ptr(), st)
            s = idx.stats()
            if j >= 2:
                scan.append(s["scan_ms"])
                cand.append(s["candidates"] / 32.0)
                fb += s["fallback_queries"] + s["mid_tier_queries"]
                nbytes = s["bytes_scanned"]
        keep[tag] = (od[0].clone(), oi[0].clone())
        idx.set_option("profile", 0)
        torch.cuda.synchronize()
        t0 = 0.0
        for j in range(warmup + steps):
            if j == warmup:
                idx.sync()
                t0 = time.perf_counter()
            idx.search_device_async(qs[j % 4].data_ptr(), 32, k, od[j % 2].data_ptr(), oi[j % 2].data_ptr(), st)
        idx.sync()
        per_step = (time.perf_counter() - t0) / steps
        pass_ms = float(np.median(scan))
        print(f"   {tag:8s}: step {per_step * 1e3:.3f} ms; full pass {pass_ms:.3f} ms for {nbytes / 1e9:.2f} GB = "
              f"{nbytes / (pass_ms * 1e-3) / HBM_PEAK:.3f} of the HBM peak; {np.mean(cand):.0f} rows re-ranked per query; "
              f"{fb} queries handed on in 5 calls", flush=True)
    if len(keep) == 2:
        same = torch.equal(keep["int8"][1], keep["bfloat16"][1]) and torch.equal(keep["int8"][0], keep["bfloat16"][0])
        print(f"   identical answers: {bool(same)}", flush=True)
    idx.close()
    del x
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated n x d")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    a = ap.parse_args()
    print("library:", _lib.LIB_PATH, flush=True)
    for shape in a.shapes.split(","):
        n, d = (int(v) for v in shape.lower().split("x"))
        for metric, name in ((_lib.SQ_METRIC_L2, "euclidean"), (_lib.SQ_METRIC_COSINE, "cosine")):
            run(n, d, metric, name, a.k, a.steps, a.warmup)


if __name__ == "__main__":
    main()
