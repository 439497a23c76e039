#!/usr/bin/env python3
"""Sweep the maintenance half of the dense index -- create, append, remove + compact, the copies it keeps -- and print what
the index held and answered after every step.

Fixed seeds.  One line per step: info() without its two times (rows, d, bytes of the float32 rows / bfloat16 copy / int8
copy / row statistics, owned, int8 in use), then for 9 fixed queries at k = 10 a sha1 of distances + ids and candidates /
scan launches / fallback queries / middle-tier queries / bytes scanned from stats().  Every index is created with
dense_fused = 0 (outside the fused int8 call `candidates` is deterministic: profiles/dense_driver_before_after.txt) and
dense_blocks = 8.  Two builds that keep and decide alike print the same bytes on the same machine; with the int8 build's
report on stderr merged in, also what each build of the copy chose:

    SQ_INT8_REPORT=1 python tools/dense_index_sweep.py > sweep.txt 2>&1

Scenarios, both metrics, 70 001 rows unless stated: create at d = 100, 128, 256, 512 and at 600 with dense_int8_wide = 1;
60 000 rows + 10 000 appended (born below the int8 copy's minimum); 70 001 x 128 + 3 + 1 000 + enough to pass twice the
built size (the clamp is chosen again); + 1 100 rows scaled x 100 (too many always-candidates: chosen again); dense_int8 = 0;
dense_bf16 = -1 with a first 64-query search; 5 000 rows removed, compacted (below the minimum: no copy), 500 appended.
Uses only the Python API of smqtk_indexing_amd._lib.
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from smqtk_indexing_amd import _lib  # noqa: E402

N = 70_001
NQ, K = 9, 10
INFO = ("rows", "d", "f32_rows_bytes", "f32_rows_owned", "bf16_copy_bytes", "int8_copy_bytes", "row_stats_bytes", "int8_in_use")
STATS = ("candidates", "scan_launches", "fallback_queries", "mid_tier_queries", "bytes_scanned")


class Scenario:
    def __init__(self, mname, metric, name, d, seed, **options):
        self.tag = "%s-%s" % (mname, name)
        self.metric, self.d, self.options = metric, d, dict(options, dense_fused=0, dense_blocks=8)
        self.rng = np.random.default_rng(seed + (7 if mname == "cos" else 0))
        self.qs = self.rng.standard_normal((64, d)).astype(np.float32)
        self.idx = None

    def rows(self, n, scale=1.0):
        return (np.float32(scale) * self.rng.standard_normal((n, self.d))).astype(np.float32)

    def step(self, what, nq=NQ):
        sys.stderr.flush()
        dist, ids = self.idx.search(self.qs[:nq], K)
        sha = hashlib.sha1(np.ascontiguousarray(dist).tobytes() + np.ascontiguousarray(ids).tobytes()).hexdigest()[:16]
        info, st = self.idx.info(), self.idx.stats()
        print("%s %s info=%s nq=%d sha1=%s stats=%s" % (self.tag, what, "/".join(str(int(info[f])) for f in INFO), nq, sha,
                                                       "/".join(str(st[f]) for f in STATS)), flush=True)

    def create(self, n=N):
        self.idx = _lib.DenseIndex(self.rows(n), metric=self.metric, options=self.options)
        self.step("create(%d)" % n)
        return self

    def append(self, n, scale=1.0):
        self.idx.append(self.rows(n, scale))
        self.step("append(%d%s)" % (n, "" if scale == 1.0 else " x%g" % scale))
        return self

    def close(self):
        self.idx.close()


def main() -> None:
    for mname, metric in (("l2", _lib.SQ_METRIC_L2), ("cos", _lib.SQ_METRIC_COSINE)):
        for d in (100, 128, 256, 512):
            Scenario(mname, metric, "d%d" % d, d, 10 * d).create().close()
        Scenario(mname, metric, "d600w", 600, 6000, dense_int8_wide=1).create().close()
        Scenario(mname, metric, "born_small", 128, 1).create(60_000).append(10_000).close()
        Scenario(mname, metric, "grows", 128, 2).create().append(3).append(1_000).append(2 * N + 1 - (N + 1_003)).close()
        Scenario(mname, metric, "outliers", 128, 3).create().append(1_100, scale=100.0).close()
        Scenario(mname, metric, "int8=0", 128, 4, dense_int8=0).create().append(1_000).close()
        s = Scenario(mname, metric, "bf16=-1", 128, 5, dense_bf16=-1).create()
        s.step("first-64", nq=64)
        s.step("again")
        s.close()
        s = Scenario(mname, metric, "compact", 128, 6).create()
        s.idx.remove(np.random.default_rng(60).choice(N, size=5_000, replace=False))
        s.step("remove(5000)")
        s.idx.compact()
        s.step("compact")
        s.append(500).close()


if __name__ == "__main__":
    main()
