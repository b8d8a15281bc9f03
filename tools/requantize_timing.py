"""Timing of requantisation (include/tinyimgcodec_hip_requantize.h), written to profiles/requantize.txt.  Figures are recorded, none is asserted.

(1) Stream -> stream, host to host: requantize() and requantize_to_size() of THIS build against the route a caller had before - ANOTHER build
    of the library (--other, required: the parent commit's, built into tools/bin/ and loaded side by side by ctypes, the way tools/ab_libs.py
    binds builds) running tic_decompress followed by tic_compress (fixed quality) or tic_compress_to_size (budget) - the two alternating, over
    the 49 benchmark streams at q = 90 with half their size as the budget, and one 4096 x 4096 stream.  The loop's own run-to-run spread
    stands beside every ratio.
(2) Kernels on resident coefficients (tic_requant_kernels_timed): the store kernel alone, the measuring kernel at 1, 7 and 64 qualities per
    launch, and the composition it replaces (store kernel + the size kernel's descriptor form) at the same counts, 512 x 512 and 4096 x 4096;
    bytes moved against the 8 TB/s the project reckons with.

Usage: python tools/requantize_timing.py --other tools/bin/libparent.so [--rounds 7] [--out profiles/requantize.txt]"""
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
ap.add_argument("--other", required=True, help="the library whose tic_decompress + tic_compress_to_size make the loop: the parent commit's build")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=None)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def bind(path, names):
    L = C.CDLL(path)
    for name in names:
        res, a = N.SIGNATURES[name]
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, a
    return L


P = bind(args.other, ("tic_create", "tic_destroy", "tic_decompress", "tic_compress", "tic_compress_to_size", "tic_compress_bound"))
assert not hasattr(P, "tic_requantize"), "--other already has the new calls: it is not the parent's build"
pctx = P.tic_create(0)
assert pctx
ctx = T.Context(0)
L = N.load()


def parent_loop(s, h, w, q=None, budget=None):
    """decompress, then compress at q or to the budget, with the parent's library -> bytes"""
    px = np.empty((h, w), np.uint8)
    buf = np.frombuffer(s, np.uint8)
    out = np.empty(P.tic_compress_bound(h, w), np.uint8)
    n, qq = C.c_size_t(0), C.c_int(0)
    assert P.tic_decompress(pctx, buf.ctypes.data, buf.size, px.ctypes.data, px.size) == 0
    if q is not None:
        assert P.tic_compress(pctx, px.ctypes.data, h, w, w, q, out.ctypes.data, out.size, C.byref(n)) == 0
    else:
        assert P.tic_compress_to_size(pctx, px.ctypes.data, h, w, w, budget, 1, 99, out.ctypes.data, out.size, C.byref(n), C.byref(qq)) == 0
    return n.value, qq.value


def timed(fn, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e6


def ab(label, new, old, reps):
    new(), old()
    a, b = [], []
    for _ in range(args.rounds):
        a.append(timed(new, reps))
        b.append(timed(old, reps))
    ma, mb = statistics.median(a), statistics.median(b)
    say("  %-44s new %9.1f us   loop %9.1f us   loop / new %5.2f   (loop's own spread %.1f %%, new's %.1f %%)"
        % (label, ma, mb, mb / ma, 100 * (max(b) - min(b)) / mb, 100 * (max(a) - min(a)) / ma))


say("requantize_timing: %s, other = %s, %d rounds" % (ctx.arch, os.path.basename(args.other), args.rounds))
say("(1) stream -> stream, host to host")
pixels = np.load(os.path.join(ROOT, "tests", "golden", "benchmark_set.npz"))["pixels"]
streams = [T.compress(pixels[i], 90, ctx=ctx) for i in range(49)]
say("  the 49 benchmark streams at q = 90 (512 x 512, %d bytes in all), per stream:" % sum(map(len, streams)))
ab("requantize(s, 50) | decompress + compress(50)", lambda: [T.requantize(s, 50, ctx=ctx) for s in streams],
   lambda: [parent_loop(s, 512, 512, q=50) for s in streams], 3)
ab("requantize_to_size(s, len / 2) | + compress_to_size", lambda: [T.requantize_to_size(s, len(s) // 2, ctx=ctx) for s in streams],
   lambda: [parent_loop(s, 512, 512, budget=len(s) // 2) for s in streams], 3)
same = sum(len(T.requantize_to_size(s, len(s) // 2, ctx=ctx)[0]) for s in streams), sum(parent_loop(s, 512, 512, budget=len(s) // 2)[0] for s in streams)
say("  (per-stream times are the figures above / 49; bytes within the budgets: requantised %d, through pixels %d)" % same)
big = np.random.default_rng(4096).integers(0, 256, (4096, 4096), dtype=np.uint8)
s_big = T.compress(big, 90, ctx=ctx)
say("  one 4096 x 4096 stream at q = 90 (%d bytes):" % len(s_big))
ab("requantize(s, 50) | decompress + compress(50)", lambda: T.requantize(s_big, 50, ctx=ctx), lambda: parent_loop(s_big, 4096, 4096, q=50), 3)
ab("requantize_to_size(s, len / 2) | + compress_to_size", lambda: T.requantize_to_size(s_big, len(s_big) // 2, ctx=ctx),
   lambda: parent_loop(s_big, 4096, 4096, budget=len(s_big) // 2), 3)
say("  last search: %r" % (T.last_requantize(ctx),))

say("(2) kernels on resident coefficients, us per launch (median of %d rounds; min .. max)" % args.rounds)
ms = C.c_float()
for dim in (512, 4096):
    img = pixels[0] if dim == 512 else big
    zz, hdr = T.entropy_decode_zz(T.compress(img, 90, ctx=ctx), ctx=ctx)
    n = zz.shape[0]
    d = C.c_void_p()
    ctx.check(L.tic_dev_alloc(ctx.handle, zz.nbytes, C.byref(d)))
    ctx.check(L.tic_memcpy_h2d(ctx.handle, d, zz.ctypes.data, zz.nbytes))
    say("  %d x %d at q = 90, %d blocks, %.1f MB of coefficients (%.2f us at 8 TB/s), %.1f %% of them zero"
        % (dim, dim, n, zz.nbytes / 1e6, zz.nbytes / 8e6, 100.0 * np.count_nonzero(zz == 0) / zz.size))
    for nq in (1, 7, 64):
        if dim == 4096 and nq == 64:
            qs = np.linspace(1, 90, 16).astype(np.intc)  # (64 frames of 32 MB are more workspace than the composition is given)
        else:
            qs = np.unique(np.linspace(1, 90, nq).astype(np.intc)) if nq > 1 else np.array([50], np.intc)
        qs = np.ascontiguousarray(qs, np.intc)
        iters = max(20, int(2e9 // (n * 64 * len(qs))))
        res = {}
        sizes = {}
        for mode, name in ((0, "store"), (1, "measuring"), (2, "store + size")):
            v = []
            got = np.zeros(len(qs), np.int64)
            for _ in range(args.rounds):
                ctx.check(L.tic_requant_kernels_timed(ctx.handle, d, n, 90, qs.ctypes.data, len(qs), mode, 3, iters, C.byref(ms), got.ctypes.data))
                v.append(ms.value * 1e3 / iters)
            res[name], sizes[name] = v, got.copy()
        assert np.array_equal(sizes["measuring"], sizes["store + size"]), (sizes["measuring"], sizes["store + size"])
        moved = {"store": zz.nbytes * (1 + len(qs)), "measuring": zz.nbytes, "store + size": zz.nbytes * (1 + 2 * len(qs))}
        for name, v in res.items():
            m = statistics.median(v)
            say("    %2d qualities  %-13s %9.2f us  (%.2f .. %.2f)   %7.1f MB moved, %5.2f TB/s" % (len(qs), name, m, min(v), max(v), moved[name] / 1e6, moved[name] / m / 1e6))
        say("    %2d qualities  composition / measuring kernel: %.2f" % (len(qs), statistics.median(res["store + size"]) / statistics.median(res["measuring"])))
    ctx.check(L.tic_dev_free(ctx.handle, d))
P.tic_destroy(pctx)
ctx.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
