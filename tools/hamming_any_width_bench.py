#!/usr/bin/env python3
"""Time the Hamming search over codes of 3 .. 16 words: blocking calls of 1, 32 and 256 queries and pipelined
one-query calls, 10 M unique random codes, k = 100.

Only calls every commit of the library has (create, search on device pointers, the pipelined form, sync), so the same
script, copied into a checkout of the parent commit, measures that one -- as it is, or over the same codes zero-padded
to the next width it has kernels for (--pad: 3 -> 4, 5 .. 7 -> 8, 9 .. 15 -> 16 words; the distances do not change).
Every shape is timed in --rounds rounds of calls, each call a host clock around work that ends in a device wait.  One
JSON line per (width, shape): the median of all timed calls, their 5th and 95th percentile and maximum, and the
median of each round.  The spread of a shape is the range of its round medians, max - min: what is compared between
two builds is a median, so its noise is how far the median moves when the same measurement is repeated.  Percentiles
of single calls are no measure of that: one call in a hundred waits for somebody else's work on a shared box, and the
calls of the atomic scan fall into two groups by themselves (768 bits, 32 queries: near 11.5 and near 26 ms).

    python parent/tools/hamming_any_width_bench.py --label parent > a.jsonl
    python parent/tools/hamming_any_width_bench.py --label parent-padded --pad > b.jsonl
    python tools/hamming_any_width_bench.py --label tree > c.jsonl
    python tools/hamming_any_width_bench.py --combine a.jsonl b.jsonl c.jsonl > profiles/hamming_any_width.txt
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIDTHS = (3, 5, 6, 7, 8, 12, 16)
SHAPES = (("block", 1), ("block", 32), ("block", 256), ("pipelined", 1))


def padded_width(w: int) -> int:
    return 1 if w <= 1 else 2 if w == 2 else 4 if w <= 4 else 8 if w <= 8 else 16


def make_codes(n: int, w: int, seed: int):
    """n unique random codes in ascending order (first words distinct, so the order is decided there) and 256 queries,
    every eighth a stored code."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 2 ** 64, size=(n, w), dtype=np.uint64)
    codes = codes[np.argsort(codes[:, 0], kind="stable")]
    assert (codes[1:, 0] > codes[:-1, 0]).all(), "first words collide: another seed"
    queries = rng.integers(0, 2 ** 64, size=(256, w), dtype=np.uint64)
    queries[::8] = codes[rng.integers(0, n, size=32)]
    return codes, queries


def measure(args) -> None:
    import torch
    from smqtk_indexing_amd import _lib
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    for w in args.widths:
        codes, queries = make_codes(args.n, w, 100 + w)
        wp = padded_width(w) if args.pad else w
        if wp != w:                                   # zero words in front: same distances, same order
            codes = np.concatenate([np.zeros((args.n, wp - w), dtype=np.uint64), codes], axis=1)
            queries = np.concatenate([np.zeros((256, wp - w), dtype=np.uint64), queries], axis=1)
        idx = _lib.HammingIndex(codes)
        del codes
        qd = torch.from_numpy(queries.view(np.int64)).to(dev)
        checksum = None
        for mode, nq in SHAPES:
            od = [torch.empty((nq, args.k), dtype=torch.int32, device=dev) for _ in range(4)]
            oi = [torch.empty((nq, args.k), dtype=torch.int64, device=dev) for _ in range(4)]

            def one_block():
                t0 = time.perf_counter()
                idx.search_device(qd.data_ptr(), nq, args.k, od[0].data_ptr(), oi[0].data_ptr(), stream)   # returns when the results are final
                return time.perf_counter() - t0

            def one_train(calls=16):
                t0 = time.perf_counter()
                for j in range(calls):
                    idx.search_device_async(qd.data_ptr(), nq, args.k, od[j % 4].data_ptr(), oi[j % 4].data_ptr(), stream)
                idx.sync()
                return (time.perf_counter() - t0) / calls

            one = one_block if mode == "block" else one_train
            for _ in range(args.warmup):
                one()
            times, round_medians = [], []
            for _ in range(args.rounds):
                rt = []
                t_end = time.perf_counter() + args.seconds / args.rounds
                while len(rt) < args.min_reps or (time.perf_counter() < t_end and len(rt) < args.max_reps):
                    rt.append(one())
                round_medians.append(statistics.median(rt))
                times += rt
            torch.cuda.synchronize()
            st = idx.stats()
            if mode == "block" and nq == 32:
                checksum = int(od[0].to(torch.int64).sum().item()), int(oi[0].sum().item())
            print(json.dumps({"label": args.label, "words": w, "stored_words": wp, "n": args.n, "k": args.k, "mode": mode, "nq": nq,
                              "median_ms": 1e3 * statistics.median(times), "min_ms": 1e3 * min(times), "max_ms": 1e3 * max(times),
                              "p05_ms": 1e3 * float(np.percentile(times, 5)), "p95_ms": 1e3 * float(np.percentile(times, 95)),
                              "round_medians_ms": [1e3 * m for m in round_medians],
                              "spread_ms": 1e3 * (max(round_medians) - min(round_medians)), "reps": len(times), "fallback_queries": st["fallback_queries"],
                              "candidates": st["candidates"], "checksum_q32": checksum}), flush=True)
        idx.close()


def combine(paths) -> None:
    cols = []
    for p in paths:
        rows = [json.loads(line) for line in open(p) if line.startswith("{")]
        cols.append({(r["words"], r["mode"], r["nq"]): r for r in rows})
    labels = [next(iter(c.values()))["label"] if c else "?" for c in cols]
    first = next(iter(cols[0].values()))
    print(f"# Hamming search, {first['n']} unique random codes, k = {first['k']}: ms per call, median [range of the round medians] (p5 .. p95; max of the timed calls), stored words")
    print(f"# columns: {' | '.join(labels)};  last column: first / last medians, whether last < first - spread(first) with spread = range of the")
    print(f"# {len(first['round_medians_ms'])} round medians, and whether the two bands of single calls are apart (p95 of the last < p5 of the first)")
    print("# checksums (sum of distances, sum of ids of the 32-query call) must agree across the columns of a width")
    for key in sorted(cols[0]):
        w, mode, nq = key
        cells, sums = [], set()
        for c in cols:
            r = c.get(key)
            if r is None:
                cells.append("-")
                continue
            cells.append(f"{r['median_ms']:9.3f} [{min(r['round_medians_ms']):.3f} .. {max(r['round_medians_ms']):.3f}] ({r['p05_ms']:.3f} .. {r['p95_ms']:.3f}; {r['max_ms']:.3f}) W{r['stored_words']}")
            if r["checksum_q32"]:
                sums.add(tuple(r["checksum_q32"]))
        a, c = cols[0].get(key), cols[-1].get(key)
        verdict = ""
        if a and c:
            verdict = (f"x{a['median_ms'] / c['median_ms']:.2f} {'faster' if c['median_ms'] < a['median_ms'] - a['spread_ms'] else 'NOT beyond the spread'}"
                       f", bands {'apart' if c['p95_ms'] < a['p05_ms'] else 'OVERLAP'}")
        print(f"W={w:2d} {mode:9s} nq={nq:3d} | " + " | ".join(cells) + f" | {verdict}" + ("" if len(sums) <= 1 else "  CHECKSUMS DIFFER"))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--label", default="tree")
    ap.add_argument("--pad", action="store_true", help="store the codes zero-padded to the next of 4, 8, 16 words")
    ap.add_argument("--widths", default=",".join(map(str, WIDTHS)))
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5, help="rounds per shape: the spread is the range of their medians")
    ap.add_argument("--seconds", type=float, default=1.0, help="timed window per shape, shared by the rounds")
    ap.add_argument("--min-reps", type=int, default=5, help="calls per round at least")
    ap.add_argument("--max-reps", type=int, default=60, help="calls per round at most")
    ap.add_argument("--combine", nargs="+", metavar="JSONL", help="print the table of these result files (first = baseline, last = this tree)")
    args = ap.parse_args()
    if args.combine:
        combine(args.combine)
        return
    args.widths = [int(w) for w in args.widths.split(",") if w]
    measure(args)


if __name__ == "__main__":
    main()
