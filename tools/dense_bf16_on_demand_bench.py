#!/usr/bin/env python3
"""Measurement helper: what option "dense_bf16"  costs and saves.  Per shape and mode -- 1: the bfloat16
scan copy built at create (the default), -1: built by the first search that streams it, 0: never -- over one
device-resident matrix:

  * resident bytes per copy (sq_dense_info) after create, and after the first large batch;
  * sq_dense_create wall time;
  * the first 256-query call, blocking (under -1 it includes the build of the copy; under 0 it is answered by the middle
    tier / the exact path), and the same call again;
  * the steady pipelined 32-query step (SQ_MEM_DEVICE_ASYNC, depth 2, wall time over --steps calls after --warmup);
  * whether the answers of the modes are the same bits.

A library that does not know the option (a commit before it) reports the default mode only.

    python tools/dense_bf16_on_demand_bench.py            # the three shapes of profiles/dense_bf16_on_demand.txt
    python tools/dense_bf16_on_demand_bench.py --shapes 1000000x128:l2 --modes 1,-1
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from smqtk_indexing_amd import _lib  # noqa: E402

SHAPES = "10000000x128:l2,12500000x512:cosine,2000000x2048:l2:wide"
BIG = 256


def knows_the_option():
    return _lib.load().sq_set_option(b"dense_bf16", 1) == 0


def gb(b):
    return "%.3f GB" % (b / 1e9)


def run(n, d, metric, name, wide, modes, k, steps, warmup):
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x = torch.empty((n, d), dtype=torch.float32, device=dev)
    step = max(1, (1 << 28) // d)
    for s in range(0, n, step):
        x[s:s + step].normal_(generator=g)
    rows = torch.randint(0, n, (4, 32), generator=torch.Generator().manual_seed(2))
    qs = [(x[r.to(dev)] + 0.05 * torch.randn((32, d), device=dev, generator=g)).contiguous() for r in rows]
    big = (x[torch.randint(0, n, (BIG,), generator=torch.Generator().manual_seed(3)).to(dev)] +
           0.05 * torch.randn((BIG, d), device=dev, generator=g)).contiguous()
    ddt = torch.float64 if metric == _lib.SQ_METRIC_COSINE else torch.float32
    od = [torch.empty((32, k), dtype=ddt, device=dev) for _ in range(2)]
    oi = [torch.empty((32, k), dtype=torch.int64, device=dev) for _ in range(2)]
    bd = torch.empty((BIG, k), dtype=ddt, device=dev)
    bi = torch.empty((BIG, k), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    print(f"n={n} d={d} {name}{' dense_int8_wide=1' if wide else ''}: float32 rows {gb(n * d * 4)}", flush=True)
    keep = {}
    for mode in modes:
        opts = {"dense_int8_wide": 1} if wide else {}
        if mode != 1:
            opts["dense_bf16"] = mode
        t0 = time.perf_counter()
        idx = _lib.DenseIndex(x.data_ptr(), n=n, d=d, metric=metric, device_ptr=True, keepalive=x, options=opts or None)
        create_ms = (time.perf_counter() - t0) * 1e3
        info = idx.info()

        def big_call():
            torch.cuda.synchronize()
            t = time.perf_counter()
            idx.search_device(big.data_ptr(), BIG, k, bd.data_ptr(), bi.data_ptr(), st)
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3, idx.stats()

        def steady():
            t = 0.0
            for j in range(warmup + steps):
                if j == warmup:
                    idx.sync()
                    t = time.perf_counter()
                idx.search_device_async(qs[j % 4].data_ptr(), 32, k, od[j % 2].data_ptr(), oi[j % 2].data_ptr(), st)
            idx.sync()
            return (time.perf_counter() - t) / steps * 1e3

        step_before = steady()       # (before any large batch: under -1 the copy does not exist yet)
        small = (od[(warmup + steps - 1) % 2].clone(), oi[(warmup + steps - 1) % 2].clone())
        first_ms, s1 = big_call()
        after = idx.info()
        second_ms, s2 = big_call()
        step_after = steady()
        keep[mode] = (bd.clone(), bi.clone(), small)
        resident = info["bf16_copy_bytes"] + info["int8_copy_bytes"] + info["row_stats_bytes"]
        resident_after = after["bf16_copy_bytes"] + after["int8_copy_bytes"] + after["row_stats_bytes"]
        print(f"   dense_bf16 = {mode:2d}: create {create_ms:8.1f} ms (library {info['build_ms']:.1f}, int8 copy {info['build_int8_ms']:.1f}); "
              f"after create: bfloat16 {gb(info['bf16_copy_bytes'])}, int8 {gb(info['int8_copy_bytes'])}, statistics "
              f"{gb(info['row_stats_bytes'])} = {1 + resident / (n * d * 4):.3f} x the matrix; int8 in use: {info['int8_in_use']}", flush=True)
        print(f"                    32-query step {step_before:.3f} ms; first {BIG}-query call {first_ms:.2f} ms "
              f"({s1['mid_tier_queries']} queries on the middle tier, {s1['fallback_queries']} on the exact path), second {second_ms:.2f} ms; "
              f"then bfloat16 {gb(after['bf16_copy_bytes'])} = {1 + resident_after / (n * d * 4):.3f} x the matrix, "
              f"32-query step {step_after:.3f} ms", flush=True)
        idx.close()
        del idx
        torch.cuda.empty_cache()
    base = keep[modes[0]]
    for mode in modes[1:]:
        same = all(torch.equal(a, b) for a, b in zip(keep[mode][:2] + keep[mode][2], base[:2] + base[2]))
        print(f"   dense_bf16 = {mode}: answers identical to dense_bf16 = {modes[0]}: {bool(same)}", flush=True)
    del x
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated n x d:metric[:wide]")
    ap.add_argument("--modes", default="1,-1,0")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    print("library:", os.path.relpath(_lib.LIB_PATH), "| device:", _lib.device_name(0)[0], flush=True)
    modes = [int(m) for m in a.modes.split(",")]
    if not knows_the_option():
        print('this library has no option "dense_bf16": the default mode only', flush=True)
        modes = [1]
    for shape in a.shapes.split(","):
        parts = shape.lower().split(":")
        n, d = (int(v) for v in parts[0].split("x"))
        metric = _lib.SQ_METRIC_COSINE if len(parts) > 1 and parts[1] == "cosine" else _lib.SQ_METRIC_L2
        run(n, d, metric, "cosine" if metric == _lib.SQ_METRIC_COSINE else "euclidean", "wide" in parts[2:], modes, a.k, a.steps, a.warmup)


if __name__ == "__main__":
    main()
