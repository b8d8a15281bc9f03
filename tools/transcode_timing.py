"""The coefficient reader and lossless re-tabling beside what they stand next to, one process, the sides alternating round by round:

    python tools/transcode_timing.py [--dim 4096] [--warm 10] [--iters 100] [--rounds 7] [--part a|b|all]

(a) the new reader against the existing decoder on the same resident streams (noise --dim^2 at q = 10 / 50 / 90, a 512^2 image of the
    benchmark set at q = 50): tic_entropy_decode_dev against tic_decompress_dev with the header guess off - both synchronous, both read
    the 16-byte header first, wall clock around `iters` calls - and the reader's two launches alone between two events
    (tic_entropy_decode_dev_timed).  Kernel times come from a separate run under rocprofv3 --kernel-trace --stats with --part a.
(b) retable_adaptive host to host on 512^2, 1080p and --dim^2 (Lenna, tiled) at q = 10 and 50 against the same call with
    TIC_DECODE_HOST=1 (the host reader in front of the device encoder: what a caller could build from internals before) and against
    compress_adaptive(decompress(s), q) - which is NOT equivalent: a second quantisation, other bytes; it is the only public route
    there was.  retable_default the same way against TIC_DECODE_HOST=1.
Best, median and the spread (max - min over the rounds, as a share of the median) of every side are printed."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("TIC_TEST_HOOKS", "1")  # (b) switches the host reader on inside the process
import numpy as np  # noqa: E402

import tinyimgcodec_amd as T  # noqa: E402
from tinyimgcodec_amd import _native as N  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--dim", type=int, default=4096)
ap.add_argument("--warm", type=int, default=10)
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--part", choices=("a", "b", "all"), default="all")
args = ap.parse_args()

L = N.load()
ctx = T.Context(0)
GOLDEN = os.path.join(ROOT, "tests", "golden")
lenna = np.load(os.path.join(GOLDEN, "lenna.npz"))["img"]
bench1 = np.load(os.path.join(GOLDEN, "benchmark_set.npz"))["pixels"][0]


def tiled(h, w):
    return np.ascontiguousarray(np.tile(lenna, ((h + 511) // 512, (w + 511) // 512))[:h, :w])


def show(label, v):
    med = statistics.median(v)
    print("  %-66s best %9.1f us, median %9.1f us, spread %4.1f %%" % (label, min(v), med, 100.0 * (max(v) - min(v)) / med))


def wall_per_call(fn, iters):
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    return (time.perf_counter() - t) * 1e6 / iters


print("%s  warm %d iters %d rounds %d" % (ctx.arch, args.warm, args.iters, args.rounds))
if args.part in ("a", "all"):
    dim = args.dim
    noise = np.random.default_rng(1234).integers(0, 256, (dim, dim), dtype=np.uint8)
    jobs = [("noise %dx%d q=%d" % (dim, dim, q), noise, q) for q in (10, 50, 90)] + [("benchmark image 1, 512x512 q=50", bench1, 50)]
    ctx.check(L.tic_set_decode_guess(ctx.handle, 0))
    print("(a) the coefficient reader against the decoder, stream and output resident:")
    for name, img, q in jobs:
        h, w = img.shape
        s = np.frombuffer(T.compress(img, q, ctx=ctx), np.uint8)
        n = L.tic_num_blocks(h, w)
        d_s, d_zz, d_px = C.c_void_p(), C.c_void_p(), C.c_void_p()
        ctx.check(L.tic_dev_alloc(ctx.handle, s.size + 64, C.byref(d_s)))
        ctx.check(L.tic_dev_alloc(ctx.handle, n * 128, C.byref(d_zz)))
        ctx.check(L.tic_dev_alloc(ctx.handle, h * w, C.byref(d_px)))
        ctx.check(L.tic_memcpy_h2d(ctx.handle, d_s, s.ctypes.data, s.size))

        def reader():
            ctx.check(L.tic_entropy_decode_dev(ctx.handle, d_s, s.size, d_zz, n, None, None, None, None))

        def decoder():
            ctx.check(L.tic_decompress_dev(ctx.handle, d_s, s.size, d_px, w, h * w, None, None))

        ms = C.c_float()
        v = {"reader": [], "decoder": [], "events": []}
        for r in range(args.rounds + 1):  # (round 0 warms both sides)
            v["reader"].append(wall_per_call(reader, args.iters))
            assert (L.tic_last_decode_path(ctx.handle), L.tic_last_decode_giveup(ctx.handle)) == (1, 0)
            v["decoder"].append(wall_per_call(decoder, args.iters))
            assert (L.tic_last_decode_path(ctx.handle), L.tic_last_decode_giveup(ctx.handle)) == (1, 0)
            ctx.check(L.tic_entropy_decode_dev_timed(ctx.handle, d_s, s.size, d_zz, n, args.warm, args.iters, C.byref(ms)))
            v["events"].append(ms.value / args.iters * 1e3)
        # the rows are the stream's coefficients
        zz = np.empty((n, 64), np.int16)
        ctx.check(L.tic_memcpy_d2h(ctx.handle, zz.ctypes.data, d_zz, zz.nbytes))
        assert T.entropy_encode(zz, h, w, q) == s.tobytes()
        print(" %s, %d bytes, %.0f bits per block:" % (name, s.size, s.size * 8.0 / n))
        show("tic_entropy_decode_dev (synchronous call)", v["reader"][1:])
        show("tic_decompress_dev, guess off (synchronous call)", v["decoder"][1:])
        show("the reader's two launches between events", v["events"][1:])
        print("      reader / decoder (median): %.3f" % (statistics.median(v["reader"][1:]) / statistics.median(v["decoder"][1:])))
        for p in (d_s, d_zz, d_px):
            L.tic_dev_free(ctx.handle, p)
    ctx.check(L.tic_set_decode_guess(ctx.handle, 1))

if args.part in ("b", "all"):
    assert L.tic_build_has_test_hooks() == 1, "part (b) needs the hooks build (TIC_TEST_HOOKS=1)"
    print("(b) re-tabling, host to host:")
    iters = max(3, args.iters // 10)
    for label, img in (("512x512", bench1), ("1080x1920", tiled(1080, 1920)), ("%dx%d" % (args.dim, args.dim), tiled(args.dim, args.dim))):
        for q in (10, 50):
            s = T.compress(img, q, ctx=ctx)
            ra = T.retable_adaptive(s, ctx=ctx)
            path_ra = L.tic_last_decode_path(ctx.handle)
            assert ra == T.compress_adaptive(img, q, ctx=ctx) and T.retable_default(ra, ctx=ctx) == s
            path_rd = L.tic_last_decode_path(ctx.handle)

            def hosted(fn, arg):
                os.environ["TIC_DECODE_HOST"] = "1"
                try:
                    return wall_per_call(lambda: fn(arg, ctx=ctx), iters)
                finally:
                    del os.environ["TIC_DECODE_HOST"]

            v = {k: [] for k in ("ra", "ra_host", "requant", "rd", "rd_host")}
            for r in range(args.rounds + 1):
                v["ra"].append(wall_per_call(lambda: T.retable_adaptive(s, ctx=ctx), iters))
                v["ra_host"].append(hosted(T.retable_adaptive, s))
                v["requant"].append(wall_per_call(lambda: T.compress_adaptive(T.decompress(s, ctx=ctx), q, ctx=ctx), iters))
                v["rd"].append(wall_per_call(lambda: T.retable_default(ra, ctx=ctx), iters))
                v["rd_host"].append(hosted(T.retable_default, ra))
            print(" %s q=%d: %d -> %d bytes (%.1f %% saved); reader of retable_adaptive: %s, of retable_default: %s (1 device, 2 host):"
                  % (label, q, len(s), len(ra), 100.0 * (len(s) - len(ra)) / len(s), path_ra, path_rd))
            show("retable_adaptive", v["ra"][1:])
            show("retable_adaptive, TIC_DECODE_HOST=1", v["ra_host"][1:])
            show("compress_adaptive(decompress(s)) - not equivalent: a second quantisation", v["requant"][1:])
            show("retable_default", v["rd"][1:])
            show("retable_default, TIC_DECODE_HOST=1", v["rd_host"][1:])
ctx.close()
