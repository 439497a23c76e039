#!/usr/bin/env python3
"""Measurement helper: sq_itq_model_hash on device-resident rows whose width is no multiple of 64 (100, 300, 500: the
slab filter of sq_itq_xwide.hpp, routed by itq_filter_route in sq_itq.hip), three ways per shape --

  1. the all-float64 kernel (option itq_exact on the model handle: what hashed these widths before),
  2. the default path,
  3. the default path at the next multiple of 64 (128, 320, 512) on zero-padded copies of the same rows, the rotation
     padded with zero rows: the same codes from the kernels that move whole 256-byte row units (sq_itq_fast.hpp /
     sq_itq_wide.hpp), i.e. what the guarded 16-byte pieces cost against a padded layout.

hipEvent times after two warm-up calls, median [min .. max] of the timed calls, and the default path against the
row bytes at the HBM peak (8 TB/s).  The codes of (1) and (2) are compared, and those of (3) with (2).

    python tools/itq_any_width_bench.py                 # the four shapes of profiles/itq_any_width.txt
    python tools/itq_any_width_bench.py --scale 0.1     # a tenth of the rows
"""
import argparse
import ctypes
import os
import socket
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from smqtk_indexing_amd import _lib  # noqa: E402

HBM_PEAK = 8.0e12
SHAPES = ((10_000_000, 100, 64, "float32"), (2_000_000, 300, 128, "float32"), (2_000_000, 300, 128, "float64"),
          (2_000_000, 500, 256, "float32"))


class Timing(float):
    """The median of the timed calls, with their spread for the report."""
    def __new__(cls, ts):
        self = super().__new__(cls, float(np.median(ts)))
        self.lo, self.hi = float(min(ts)), float(max(ts))
        return self

    def ms(self):
        return f"{self * 1e3:.3f} ms [{self.lo * 1e3:.3f} .. {self.hi * 1e3:.3f}]"


def timed_hash(model, x, out, calls):
    n, d = x.shape
    code = _lib.SQ_DTYPE_F32 if x.dtype == torch.float32 else _lib.SQ_DTYPE_F64
    st = torch.cuda.current_stream().cuda_stream
    ts = []
    for i in range(2 + calls):                           # two warm-up calls
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = _lib.load().sq_itq_model_hash(model.handle, ctypes.c_void_p(x.data_ptr()), code, n,
                                           ctypes.c_void_p(out.data_ptr()), _lib.SQ_MEM_DEVICE, ctypes.c_void_p(st or None))
        e1.record()
        torch.cuda.synchronize()
        if rc != _lib.SQ_OK:
            raise RuntimeError(f"sq_itq_model_hash failed (code {rc})")
        if i >= 2:
            ts.append(e0.elapsed_time(e1) * 1e-3)
    return Timing(ts), model.stats()


def run(n, d, bits, dtname, norm, calls):
    dev = torch.device("cuda", 0)
    dt = getattr(torch, dtname)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x = torch.empty((n, d), dtype=dt, device=dev)
    step = max(1, (1 << 28) // d)
    for s in range(0, n, step):
        x[s:s + step].normal_(generator=g)
    rot, _ = np.linalg.qr(np.random.default_rng(5).standard_normal((d, bits)))
    rot = np.ascontiguousarray(rot[:, :bits])
    mean = x[:100_000].double().mean(dim=0).cpu().numpy()
    words = (bits + 63) // 64
    out = torch.empty((n, words), dtype=torch.int64, device=dev)

    model = _lib.ItqModel(mean, rot, norm)
    t_new, st_new = timed_hash(model, x, out, calls)
    codes_new = out.clone()
    model.set_option("itq_exact", 1)
    t_f64, st_f64 = timed_hash(model, x, out, min(calls, 3))
    same_f64 = bool(torch.equal(codes_new, out))
    model.close()

    dpad = (d + 63) // 64 * 64
    xp = torch.zeros((n, dpad), dtype=dt, device=dev)
    xp[:, :d] = x
    del x
    rot_p = np.zeros((dpad, bits))
    rot_p[:d] = rot
    mean_p = np.zeros(dpad)
    mean_p[:d] = mean
    model = _lib.ItqModel(mean_p, rot_p, norm)
    t_pad, st_pad = timed_hash(model, xp, out, calls)
    # (the padded rows have the same norms, means and products, up to the order of the float32 sums: the filter's
    # verdicts may differ, the float64 signs of the bits it leaves may not -- except where z is a rounding error from 0)
    diff_pad = int((codes_new != out).any(dim=1).sum())
    model.close()

    row_bytes = n * d * xp.element_size()
    t_hbm = row_bytes / HBM_PEAK
    print(f"n={n} d={d} bits={bits} {dtname} norm={norm}: float64 kernel {t_f64.ms()} | default path "
          f"{t_new.ms()} ({t_f64 / t_new:.2f} x, launches {st_new['scan_launches']}, fallback rows "
          f"{st_new['fallback_queries']}, identical codes: {same_f64}; {t_hbm / t_new:.3f} of the HBM peak) | "
          f"padded to d={dpad} {t_pad.ms()} (default / padded {t_new / t_pad:.2f}, launches "
          f"{st_pad['scan_launches']}, rows that differ {diff_pad}); float64 run: fallback rows {st_f64['fallback_queries']}",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every n (smaller boxes)")
    a = ap.parse_args()
    print("library:", _lib.LIB_PATH, "| device:", torch.cuda.get_device_name(0), "| box:", socket.gethostname(), flush=True)
    for (n, d, bits, dtname) in SHAPES:
        for norm in (_lib.SQ_NORM_NONE, _lib.SQ_NORM_L2):
            run(int(n * a.scale), d, bits, dtname, norm, a.calls)


if __name__ == "__main__":
    main()
