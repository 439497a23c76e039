#!/usr/bin/env python3
"""Measurement helper: a resident ITQ model hashing device-resident rows to codes of 512 and 1024 bits -- the slab
filter of sq_itq_xwide.hpp in column groups of 256 bits, one pass over the rows per group -- against the all-float64
kernel (the model's option itq_exact = what hashed these codes before the filter took them), in the same process.
hipEvent times after warm-up, median and spread of the timed calls, the two paths alternating; each filter time
against its two roofs: the row bytes of every pass at the HBM peak (8 TB/s) and the three float16 products
3 x 2 n d bits at the dense f16 MFMA peak (2.5 PFLOP/s).  The undecided share comes from one host-memory call on the
first rows (a device call is asynchronous and does not read the counter back).

    python tools/itq_wide_codes_bench.py                  # the shapes of profiles/itq_wide_codes.txt
    python tools/itq_wide_codes_bench.py --scale 0.25     # every n times 0.25
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from smqtk_indexing_amd import _lib  # noqa: E402

HBM_PEAK = 8.0e12
F16_PEAK = 2.5e15
SHAPES = ((2_000_000, 4096, 512, "float32"), (2_000_000, 4096, 1024, "float32"), (2_000_000, 2048, 512, "float32"),
          (4_000_000, 2048, 512, "float64"), (2_000_000, 1000, 512, "float32"), (2_000_000, 512, 512, "float32"))
SHARE_ROWS = 20_000     # rows of the host call that reads the undecided share


def run(n, d, bits, dtname, norm, calls):
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    dt = getattr(torch, dtname)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x = torch.empty((n, d), dtype=dt, device=dev)
    step = max(1, (1 << 28) // d)
    for s in range(0, n, step):
        x[s:s + step].normal_(generator=g)
    rot_np, _ = np.linalg.qr(np.random.default_rng(5).standard_normal((d, bits)))
    rot_np = np.ascontiguousarray(rot_np[:, :bits])
    mean_np = x[:100_000].double().mean(dim=0).cpu().numpy()
    words = (bits + 63) // 64
    groups = (words + 3) // 4
    code = _lib.SQ_DTYPE_F32 if dt == torch.float32 else _lib.SQ_DTYPE_F64
    model = _lib.ItqModel(mean_np, rot_np, norm)
    outs = {0: torch.empty((n, words), dtype=torch.int64, device=dev), 1: torch.empty((n, words), dtype=torch.int64, device=dev)}
    ts = {0: [], 1: []}
    stats = {}
    for i in range(2 + calls):                            # two warm-up rounds; the two paths alternate
        for exact in (0, 1):
            model.set_option("itq_exact", exact)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            model.hash_device(x.data_ptr(), code, n, outs[exact].data_ptr(), st)
            e1.record()
            torch.cuda.synchronize()
            stats[exact] = model.stats()
            if i >= 2:
                ts[exact].append(e0.elapsed_time(e1) * 1e-3)
    model.set_option("itq_exact", 0)
    assert stats[0]["scan_launches"] == groups and stats[0]["fallback_queries"] == 0, stats[0]
    assert stats[1]["scan_launches"] == 0 and stats[1]["fallback_queries"] == n, stats[1]
    m = min(n, SHARE_ROWS)
    model.hash(x[:m].cpu().numpy())
    cand = model.stats()["candidates"]
    model.close()
    t, t64 = float(np.median(ts[0])), float(np.median(ts[1]))
    row_bytes = groups * n * d * x.element_size()
    flop = 3.0 * 2.0 * n * d * bits
    t_hbm, t_mfma = row_bytes / HBM_PEAK, flop / F16_PEAK
    bound = "HBM" if t_hbm >= t_mfma else "f16 MFMA"
    print(f"n={n} d={d} bits={bits} {dtname} norm={norm}: filter ({groups} passes) {t * 1e3:.3f} ms "
          f"[{min(ts[0]) * 1e3:.3f} .. {max(ts[0]) * 1e3:.3f}]; float64 kernel {t64 * 1e3:.3f} ms "
          f"[{min(ts[1]) * 1e3:.3f} .. {max(ts[1]) * 1e3:.3f}] ({t64 / t:.2f} x); roofs: {groups} x rows at HBM peak "
          f"{t_hbm * 1e3:.3f} ms, 3 products at f16 peak {t_mfma * 1e3:.3f} ms -> {bound} binds, "
          f"{max(t_hbm, t_mfma) / t:.3f} of that roof; undecided {cand} of {m * bits} bits ({cand / (m * bits):.5f}); "
          f"identical codes: {bool(torch.equal(outs[0], outs[1]))}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every n (smaller boxes)")
    ap.add_argument("--only", type=int, default=-1, help="index of the one shape to run")
    a = ap.parse_args()
    print("library:", _lib.LIB_PATH, flush=True)
    print("one launch of the filter per column group of 256 bits (the group as a grid dimension: not tried)", flush=True)
    for i, (n, d, bits, dtname) in enumerate(SHAPES):
        if a.only >= 0 and i != a.only:
            continue
        for norm in (_lib.SQ_NORM_NONE, _lib.SQ_NORM_L2):
            run(int(n * a.scale), d, bits, dtname, norm, a.calls)


if __name__ == "__main__":
    main()
