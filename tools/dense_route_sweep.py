#!/usr/bin/env python3
"""Sweep the routes of the dense search driver and print what each call answered and did.

Fixed seeds.  One line per (index, options, mode, nq, k): a sha1 of distances + ids and
candidates / scan launches / fallback queries / middle-tier queries / bytes scanned from stats().  Two builds that decide
alike print the same bytes on the same machine (grids depend on the CU count), except inside the fused int8 call (up to
32 queries, int8 copy in use, dense_fused = 1): its `candidates` vary from run to run, with dense_tighten = 0 as well,
and where the lists are at their cap the later tiers' counts follow (profiles/dense_driver_before_after.txt):

    python tools/dense_route_sweep.py > sweep.txt

Indexes, both metrics: 5 000 x 128 (the all-rows path), 70 001 x d for d in 100, 128, 256, 400, 512, and 70 001 x 600 with
"dense_int8_wide" 0 and 1.  Every option set runs on a fresh index with dense_blocks = 8: all of them on 70 001 x 128,
the defaults, dense_int8 = 0 and candidate_cap = 4 k (lists overflow: the later tiers run) on the others.  Every nq with
k = 10, every k (one beyond the one-workgroup select) with nq = 1 and 33; asynchronous modes (depth 3: streams 1,
streams 2, streams 2 without the call graph) at nq = 17, 33, 130, ten calls each so that every slot launches its graph.
Uses only the Python API of smqtk_indexing_amd._lib.
"""
import argparse
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from smqtk_indexing_amd import _lib  # noqa: E402

NQS = (1, 17, 32, 33, 64, 65, 97, 128, 130, 257)
KS = (1, 10, 100)
K_BEYOND = {"l2": 16385, "cos": 7169}     # one past the one-workgroup select (kSelectLdsKeys64 / kSelectLdsKeys128)
ASYNC_NQS = (17, 33, 130)
ASYNC_MODES = (("a3s1", dict(dense_async_streams=1, dense_graph=1)), ("a3s2", dict(dense_async_streams=2, dense_graph=1)),
               ("a3g0", dict(dense_async_streams=2, dense_graph=0)))
ASYNC_CALLS = 10
CAP4K = "cap4k"
OPTION_SETS = [("defaults", {}), ("int8=0", dict(dense_int8=0)), (CAP4K, {}), ("fused=0", dict(dense_fused=0)),
               ("tighten=0", dict(dense_tighten=0)), ("fused_prep=0", dict(dense_fused_prep=0)), ("qt=1", dict(dense_qt=1)),
               ("qt=2", dict(dense_qt=2)), ("qt=4", dict(dense_qt=4)), ("qplanes=1", dict(dense_qplanes=1)),
               ("qplanes=2", dict(dense_qplanes=2)), ("bf16=0", dict(dense_bf16=0)), ("mid_tier=0", dict(dense_mid_tier=0)),
               ("force_fallback=1", dict(force_fallback=1)), ("segments=1", dict(dense_rerank_segments=1)),
               ("segments=4", dict(dense_rerank_segments=4)), ("segments=8", dict(dense_rerank_segments=8))]
# (name, n, d, create options, how many of OPTION_SETS)
INDEXES = [("small", 5_000, 128, {}, 2), ("d100", 70_001, 100, {}, 3), ("d128", 70_001, 128, {}, len(OPTION_SETS)), ("d256", 70_001, 256, {}, 3),
           ("d400", 70_001, 400, {}, 3), ("d512", 70_001, 512, {}, 3), ("d600", 70_001, 600, dict(dense_int8_wide=0), 3),
           ("d600w", 70_001, 600, dict(dense_int8_wide=1), 3)]


def _sha(d, i):
    return hashlib.sha1(np.ascontiguousarray(d).tobytes() + np.ascontiguousarray(i).tobytes()).hexdigest()[:16]


def _line(tag, mode, nq, k, sha, st):
    print("%s mode=%s nq=%d k=%d sha1=%s stats=%d/%d/%d/%d/%d" % (tag, mode, nq, k, sha, st["candidates"], st["scan_launches"],
                                                                  st["fallback_queries"], st["mid_tier_queries"], st["bytes_scanned"]), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--indexes", default="", help="comma-separated subset of the index names (default: all)")
    args = ap.parse_args()
    import torch
    only = {w for w in args.indexes.split(",") if w}
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    for mname, metric in (("l2", _lib.SQ_METRIC_L2), ("cos", _lib.SQ_METRIC_COSINE)):
        for iname, n, d, create, n_sets in INDEXES:
            if only and iname not in only:
                continue
            rng = np.random.default_rng(1000 * d + n % 1000 + (7 if mname == "cos" else 0))
            db = rng.standard_normal((n, d)).astype(np.float32)
            pool = rng.standard_normal((max(NQS), d)).astype(np.float32)
            pool[::5] = db[rng.integers(0, n, size=len(pool[::5]))] + np.float32(1e-3) * rng.standard_normal((len(pool[::5]), d)).astype(np.float32)
            pool_dev = torch.from_numpy(pool).to(dev)
            pairs = [(nq, 10) for nq in NQS] + [(nq, k) for nq in (1, 33) for k in KS if k != 10]
            if n > 65536:
                pairs += [(nq, K_BEYOND[mname]) for nq in (1, 33)]
            for oname, opts in OPTION_SETS[:n_sets]:
                tag = "%s-%s opts=%s" % (mname, iname, oname)
                idx = _lib.DenseIndex(db, metric=metric, options=dict(create, dense_blocks=8, **opts))
                for nq, k in pairs:
                    if oname == CAP4K:
                        idx.set_option("candidate_cap", 4 * k)
                    dist, ids = idx.search(pool[:nq], k)
                    _line(tag, "block", nq, k, _sha(dist, ids), idx.stats())
                idx.set_option("dense_async_depth", 3)
                if oname == CAP4K:
                    idx.set_option("candidate_cap", 40)
                dt = torch.float64 if mname == "cos" else torch.float32
                for mode, mopts in ASYNC_MODES:
                    for name, value in mopts.items():
                        idx.set_option(name, value)
                    for nq in ASYNC_NQS:
                        od = torch.zeros((ASYNC_CALLS, nq, 10), dtype=dt, device=dev)
                        oi = torch.zeros((ASYNC_CALLS, nq, 10), dtype=torch.int64, device=dev)
                        torch.cuda.synchronize()
                        for c in range(ASYNC_CALLS):
                            idx.search_device_async(pool_dev.data_ptr(), nq, 10, od[c].data_ptr(), oi[c].data_ptr(), stream)
                        idx.sync()
                        torch.cuda.synchronize()
                        _line(tag, mode, nq, 10, _sha(od.cpu().numpy(), oi.cpu().numpy()), idx.stats())
                idx.close()


if __name__ == "__main__":
    main()
