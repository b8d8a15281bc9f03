"""The integer (scaled-DCT) transform kernel beside the production float kernel, one process, one frame, identical warm / iters:

    python tools/scaled_timing.py [--dim 4096] [--setting med] [--quality 50] [--warm 20] [--iters 200] [--rounds 3]

prints the replayed per-launch time of tic_dctq_scaled_dev_timed_warm and of tic_dctq_dev_timed_warm (TIC_KERNEL_HYBRID), alternating,
the best and median round of each, and the whole-codec time of tic_compress_scaled_dev beside tic_compress_dev (resident image and
stream, wall clock around the synchronous call)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import tinyimgcodec_amd as T  # noqa: E402
from tinyimgcodec_amd import _native as N  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--dim", type=int, default=4096)
ap.add_argument("--setting", default="med", choices=("best", "high", "med", "low"))
ap.add_argument("--quality", type=int, default=50)
ap.add_argument("--warm", type=int, default=20)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()

L = N.load()
ctx = T.Context(0)
dim, qf = args.dim, ("best", "high", "med", "low").index(args.setting)
img = np.random.default_rng(1234).integers(0, 256, (dim, dim), dtype=np.uint8)
d_img, d_zz, d_out = C.c_void_p(), C.c_void_p(), C.c_void_p()
cap = L.tic_compress_scaled_bound(dim, dim)
ctx.check(L.tic_dev_alloc(ctx.handle, img.size, C.byref(d_img)))
ctx.check(L.tic_dev_alloc(ctx.handle, img.size * 2, C.byref(d_zz)))
ctx.check(L.tic_dev_alloc(ctx.handle, cap, C.byref(d_out)))
ctx.check(L.tic_memcpy_h2d(ctx.handle, d_img, img.ctypes.data, img.size))
ms = C.c_float()
res = {"scaled": [], "hybrid": []}
for r in range(args.rounds):
    ctx.check(L.tic_dctq_scaled_dev_timed_warm(ctx.handle, d_img, dim, dim, dim, qf, d_zz, args.warm, args.iters, C.byref(ms), None))
    res["scaled"].append(ms.value / args.iters * 1e3)
    ctx.check(L.tic_dctq_dev_timed_warm(ctx.handle, d_img, dim, dim, dim, args.quality, d_zz, N.KERNEL_HYBRID, args.warm, args.iters, C.byref(ms), None))
    res["hybrid"].append(ms.value / args.iters * 1e3)
print("%s  %dx%d  warm %d iters %d rounds %d" % (ctx.arch, dim, dim, args.warm, args.iters, args.rounds))
for name, label in (("scaled", "tic_dctq_scaled_dev (%s)" % args.setting), ("hybrid", "tic_dctq_dev HYBRID (q = %d)" % args.quality)):
    v = res[name]
    print("%-34s per launch: best %.2f us, median %.2f us  (%.0f GB/s at 3 B/px)  rounds %s" %
          (label, min(v), statistics.median(v), 3 * dim * dim / (min(v) * 1e-6) / 1e9, " ".join("%.2f" % x for x in v)))
print("scaled / hybrid (best rounds): %.3f" % (min(res["scaled"]) / min(res["hybrid"])))
n = C.c_size_t()
for label, fn, q in (("tic_compress_scaled_dev (%s)" % args.setting, L.tic_compress_scaled_dev, qf), ("tic_compress_dev (q = %d)" % args.quality, L.tic_compress_dev, args.quality)):
    ts = []
    for k in range(12):
        t = time.perf_counter()
        ctx.check(fn(ctx.handle, d_img, dim, dim, dim, q, d_out, cap, C.byref(n)))
        ts.append((time.perf_counter() - t) * 1e6)
    print("%-34s whole codec, resident: best %.1f us, median %.1f us of 10 (2 warm-up), %d bytes" % (label, min(ts[2:]), statistics.median(ts[2:]), n.value))
for p in (d_img, d_zz, d_out):
    L.tic_dev_free(ctx.handle, p)
ctx.close()
