#!/usr/bin/env python3
"""Measurement helper: sq_itq_hash on device-resident rows of 513 .. 8192 elements (sq_itq_xwide.hpp) against the
all-float64 kernel (option itq_exact = what hashed these shapes before the extra-wide filter existed).  hipEvent
times after warm-up, median of the timed calls, and each result against its two roofs: the row bytes at the HBM peak
(8 TB/s) and the three float16 products 3 x 2 n d bits at the dense f16 MFMA peak (2.5 PFLOP/s).

    python tools/itq_xwide_bench.py                  # the four shapes of profiles/r05_itq_xwide.txt
    python tools/itq_xwide_bench.py --no-float64     # filter only (e.g. with SMQTK_HIP_LIBRARY pointing at another build)
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
SHAPES = ((2_000_000, 4096, 256, "float32"), (2_000_000, 4096, 64, "float32"), (4_000_000, 2048, 128, "float64"),
          (2_000_000, 1000, 64, "float32"))


def run(n, d, bits, dtname, norm, with_float64, calls):
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
    rot = torch.from_numpy(np.ascontiguousarray(rot_np[:, :bits])).to(dev)
    mean = x[:100_000].double().mean(dim=0).contiguous()
    words = (bits + 63) // 64
    out = torch.empty((n, words), dtype=torch.int64, device=dev)
    code = _lib.SQ_DTYPE_F32 if dt == torch.float32 else _lib.SQ_DTYPE_F64
    res, keep = {}, None
    for tag, exact in (("filter", 0), ("float64", 1)):
        if exact and not with_float64:
            continue
        _lib.set_option("itq_exact", exact)
        ts = []
        for i in range(2 + (2 if exact else calls)):     # two warm-up calls
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.itq_hash_device(x.data_ptr(), code, n, d, mean.data_ptr(), rot.data_ptr(), bits, norm, out.data_ptr(), st)
            e1.record()
            torch.cuda.synchronize()
            if i >= 2:
                ts.append(e0.elapsed_time(e1) * 1e-3)
        res[tag] = float(np.median(ts))
        if not exact:
            keep = out.clone()
    _lib.set_option("itq_exact", 0)
    t = res["filter"]
    row_bytes = n * d * x.element_size()
    flop = 3.0 * 2.0 * n * d * bits
    t_hbm, t_mfma = row_bytes / HBM_PEAK, flop / F16_PEAK
    bound = "HBM" if t_hbm >= t_mfma else "f16 MFMA"
    line = (f"n={n} d={d} bits={bits} {dtname} norm={norm}: default path {t * 1e3:.3f} ms; roofs: rows at HBM peak "
            f"{t_hbm * 1e3:.3f} ms, 3 products at f16 peak {t_mfma * 1e3:.3f} ms -> {bound} binds, "
            f"{max(t_hbm, t_mfma) / t:.3f} of that roof")
    if "float64" in res:
        line += (f"; float64 kernel {res['float64'] * 1e3:.3f} ms ({res['float64'] / t:.1f} x); identical codes: "
                 f"{bool(torch.equal(keep, out))}")
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-float64", action="store_true", help="skip the itq_exact run")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every n (smaller boxes)")
    a = ap.parse_args()
    print("library:", _lib.LIB_PATH, flush=True)
    for (n, d, bits, dtname) in SHAPES:
        for norm in (_lib.SQ_NORM_NONE, _lib.SQ_NORM_L2):
            run(int(n * a.scale), d, bits, dtname, norm, not a.no_float64, a.calls)


if __name__ == "__main__":
    main()
