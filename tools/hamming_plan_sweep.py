#!/usr/bin/env python3
"""Sweep the decisions of the Hamming search driver and print what each case did.

One index per code width (1, 2, 3, 4, 5, 6, 7, 8, 12, 16 words at n = 300 001) plus one small index (n = 5 000: n <= cap,
the all-keys chain), fixed seeds, unique random codes.  Every edge of the driver's nq and k rules, both stream kernels
forced and automatic, the fused and the general chain, blocking and DEVICE_ASYNC calls.  A line per (index, nq, k): a
hash of the distances and indices (one per case where the cases differ) and, for each of the twelve cases,
hamming_ring,hamming_fused,mode=candidates/scan launches/fallback queries, followed by the plan of the call
(HammingIndex.plan: chain.stream.thresholds-in-stream.workgroups.slots.step.cap.queries-per-launch).  Two builds that
plan alike print the same bytes on the same machine (the stream's grid depends on the CU count); --no-plan leaves
the plans out, which is the format of a build without the plan view:

    python tools/hamming_plan_sweep.py > sweep.txt
"""
import argparse
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from smqtk_indexing_amd import _lib  # noqa: E402

NQS = (1, 8, 9, 24, 25, 32, 33, 64, 65, 385, 1025)      # the edges of every nq rule of hamming_plan
KS = (1, 100, 2048, 2049)                               # the fused limit is 2 k <= HF_SORT_CAP
INDEXES = [(1, 300_001), (2, 300_001), (3, 300_001), (4, 300_001), (5, 300_001), (6, 300_001), (7, 300_001), (8, 300_001), (12, 300_001),
           (16, 300_001), (1, 5_000)]


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--widths", default="", help="comma-separated subset of the code widths (default: all)")
    ap.add_argument("--no-plan", action="store_true", help="do not print the plans")
    args = ap.parse_args()
    import torch
    only = {int(w) for w in args.widths.split(",") if w}
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    for w, n in INDEXES:
        if only and w not in only:
            continue
        rng = np.random.default_rng(1000 * w + n % 1000)
        codes = np.unique(rng.integers(0, 2 ** 64, size=(n, w), dtype=np.uint64), axis=0)
        pool = rng.integers(0, 2 ** 64, size=(max(NQS), w), dtype=np.uint64)
        pool[::7] = codes[rng.integers(0, len(codes), size=len(pool[::7]))]   # some queries are stored codes
        pool_dev = torch.from_numpy(pool.view(np.int64)).to(dev)
        idx = _lib.HammingIndex(codes)
        for nq in NQS:
            for k in KS:
                od = torch.empty((nq, k), dtype=torch.int32, device=dev)
                oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
                cases, hashes = [], []
                for ring in (-1, 0, 1):
                    for fused in (0, 1):
                        idx.set_option("hamming_ring", ring)
                        idx.set_option("hamming_fused", fused)
                        for mode in ("block", "async"):
                            if mode == "block":
                                d, i = idx.search(pool[:nq], k)
                            else:
                                idx.search_device_async(pool_dev.data_ptr(), nq, k, od.data_ptr(), oi.data_ptr(), stream)
                                idx.sync()
                                d, i = od.cpu().numpy(), oi.cpu().numpy()
                            st = idx.stats()
                            hashes.append(hashlib.sha1(np.ascontiguousarray(d).tobytes() + np.ascontiguousarray(i).tobytes()).hexdigest()[:16])
                            plan = "" if args.no_plan else ":" + ".".join(str(v) for v in idx.plan(nq, k, async_=mode == "async").values())
                            cases.append(f"{ring},{fused},{mode}={st['candidates']}/{st['scan_launches']}/{st['fallback_queries']}{plan}")
                if len(set(hashes)) == 1:        # (every chain answers alike: the hash once)
                    hashes = hashes[:1]
                print(f"W={w} n={len(codes)} nq={nq} k={k} sha1={','.join(hashes)} {' '.join(cases)}", flush=True)
        idx.close()


if __name__ == "__main__":
    main()
