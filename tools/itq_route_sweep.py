#!/usr/bin/env python3
"""Sweep the decisions of the ITQ hash driver and print what each case did.

Two grids, fixed seeds, normal rows:

  shapes   every (element type, d, bits) at n = 4129 host rows -- the narrow, wide and slab filters, the float64 kernel
           (rows that are no whole number of 16-byte pieces, d or bits beyond the limits) -- as the one-shot itq_hash, a
           first ItqModel.hash and a second one on the same model (the slab filter's cached image), normalize None, and
           one ItqModel.hash with normalize 2.  (d >= 1000 takes a subset of the widths: its models are the large ones.)
  calls    one shape per route and kernel instantiation, every per-call rule: n = 31 / 32 / 33 / 4129, normalize
           None / 2 / 1, option itq_exact 0 / 1 on the handle, host rows, device rows and device rows whose pointer is
           advanced by one element (misaligned).

A line per case: the case, a sha1 of the codes and scan_launches/candidates/fallback_queries/bytes_scanned of the model
handle (candidates is -1 after a device call; `-` for the one-shot call, which has no handle).  The rotation is
orthonormal (QR) for bits <= d <= 1000 and a scaled normal matrix otherwise: the kernels do not need orthogonality.
Two builds that route and bound alike print the same bytes on the same machine (`candidates` moves with the filter's
error bound and with its image of R):

    python tools/itq_route_sweep.py > sweep.txt
"""
import argparse
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from smqtk_indexing_amd import _lib  # noqa: E402

N = 4129
DS = {"f32": (64, 128, 192, 256, 320, 512, 100, 300, 520, 1000, 8192, 50, 8196),
      "f64": (64, 128, 192, 256, 320, 512, 100, 300, 520, 1000, 8192, 101, 8196)}
BITS = (60, 64, 128, 200, 256, 257, 512, 1000, 1024, 1025)
BITS_LARGE_D = (64, 200, 256, 257, 1024, 1025)          # d >= 1000
CALL_SHAPES = (("f32", 128, 64), ("f32", 64, 128), ("f32", 256, 256), ("f32", 512, 256), ("f64", 128, 64), ("f32", 100, 64),
               ("f64", 300, 257), ("f32", 1000, 200), ("f32", 50, 64), ("f64", 101, 64))
NORMS = (("none", _lib.SQ_NORM_NONE), ("2", _lib.SQ_NORM_L2), ("1", _lib.SQ_NORM_L1))


def model_of(d: int, bits: int):
    rng = np.random.default_rng(100_000 * d + bits)
    if bits <= d <= 1000:
        rot = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((d, d)))[0][:, :bits])
    else:
        rot = rng.standard_normal((d, bits)) / np.sqrt(d)
    return 0.05 * rng.standard_normal(d), rot


def rows_of(dtype: str, d: int) -> np.ndarray:
    x = np.random.default_rng(7 * d + 1).standard_normal((N, d))
    return x.astype(np.float32) if dtype == "f32" else x


def line(case: str, codes: np.ndarray, st) -> None:
    stats = "-" if st is None else f"{st['scan_launches']}/{st['candidates']}/{st['fallback_queries']}/{st['bytes_scanned']}"
    print(f"{case} sha1={hashlib.sha1(np.ascontiguousarray(codes).tobytes()).hexdigest()[:16]} {stats}", flush=True)


def sweep_shapes(only_d) -> None:
    for dtype, ds in DS.items():
        for d in ds:
            if only_d and d not in only_d:
                continue
            x = rows_of(dtype, d)
            for bits in (BITS if d < 1000 else BITS_LARGE_D):
                mean, rot = model_of(d, bits)
                case = f"shape {dtype} d={d} bits={bits} n={N}"
                line(f"{case} norm=none one-shot", _lib.itq_hash(x, mean, rot), None)
                model = _lib.ItqModel(mean, rot)
                for call in ("first", "second"):
                    line(f"{case} norm=none {call}", model.hash(x), model.stats())
                model.close()
                model = _lib.ItqModel(mean, rot, _lib.SQ_NORM_L2)
                line(f"{case} norm=2 first", model.hash(x), model.stats())
                model.close()


def sweep_calls() -> None:
    import torch
    dev = torch.device("cuda", 0)
    for dtype, d, bits in CALL_SHAPES:
        x = rows_of(dtype, d)
        dt = _lib.SQ_DTYPE_F32 if dtype == "f32" else _lib.SQ_DTYPE_F64
        flat = torch.zeros(N * d + 1, dtype=torch.float32 if dtype == "f32" else torch.float64, device=dev)
        mean, rot = model_of(d, bits)
        words = (bits + 63) // 64
        for norm_name, norm in NORMS:
            model = _lib.ItqModel(mean, rot, norm)
            for exact in (0, 1):
                model.set_option("itq_exact", exact)
                for n in (31, 32, 33, N):
                    case = f"call {dtype} d={d} bits={bits} n={n} norm={norm_name} exact={exact}"
                    line(f"{case} host", model.hash(x[:n]), model.stats())
                    for mem, shift in (("device", 0), ("device+1", 1)):
                        rows = flat[shift:shift + n * d]
                        rows.copy_(torch.from_numpy(x[:n].reshape(-1)))
                        out = torch.zeros((n, words), dtype=torch.int64, device=dev)
                        model.hash_device(rows.data_ptr(), dt, n, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
                        torch.cuda.synchronize()
                        line(f"{case} {mem}", out.cpu().numpy().view(np.uint64), model.stats())
            model.close()


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--d", default="", help="comma-separated subset of the widths of the shape grid (default: all)")
    ap.add_argument("--grid", default="shapes,calls", help="which grids to run (default: shapes,calls)")
    args = ap.parse_args()
    if "shapes" in args.grid:
        sweep_shapes({int(v) for v in args.d.split(",") if v})
    if "calls" in args.grid:
        sweep_calls()


if __name__ == "__main__":
    main()
