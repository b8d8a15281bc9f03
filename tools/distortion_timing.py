"""Rate-distortion control beside what it replaces, one process, resident frames (Lenna as it is, and noise and Lenna tiled to --dim):

    python tools/distortion_timing.py [--dim 4096] [--warm 20] [--iters 200] [--rounds 5]

(a) the measuring kernel alone (tic_distortion_dev_timed: events around back-to-back launches) beside idct_kernel on the same
    coefficients of quality 50 (tic_idct_dev_timed), and the other two launches of a rate-distortion probe timed the same way: the
    transform (tic_dctq_dev_timed_warm) and the size kernel (tic_entropy_size_dev_timed);
(b) one probe - tic_rd_points_dev with one quality, and per probe with 16 in one submission - beside what a caller had before:
    tic_compress_dev + tic_decompress_dev + a download of the frame + the squared error in numpy (wall clock around the synchronous calls);
(c) tic_compress_to_psnr_dev over 1..97 at three targets beside the same bisection written with those three per probe, with the probes
    and host waits of every search.
The two sides of (b) and (c) alternate round by round; best and median of the rounds are printed."""
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
ap.add_argument("--warm", type=int, default=20)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()

L = N.load()
ctx = T.Context(0)
lenna = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "lenna.npz"))["img"]
big = args.dim
frames = [("lenna 512x512", lenna),
          ("noise %dx%d" % (big, big), np.random.default_rng(1234).integers(0, 256, (big, big), dtype=np.uint8)),
          ("lenna tiled %dx%d" % (big, big), np.ascontiguousarray(np.tile(lenna, ((big + 511) // 512, (big + 511) // 512))[:big, :big]))]
QMAX = 97  # (98 and 99 have a coefficient without a Huffman code on these frames)


def wall(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e6


def show(label, v):
    print("  %-64s best %8.1f us, median %8.1f us" % (label, min(v), statistics.median(v)))


print("%s  warm %d iters %d rounds %d" % (ctx.arch, args.warm, args.iters, args.rounds))
for name, img in frames:
    dim = img.shape[0]
    assert img.shape == (dim, dim)
    cap = L.tic_compress_bound(dim, dim)
    d_img, d_zz, d_out, d_dec = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    ctx.check(L.tic_dev_alloc(ctx.handle, dim * dim, C.byref(d_img)))
    ctx.check(L.tic_dev_alloc(ctx.handle, L.tic_num_blocks(dim, dim) * 128 + 16, C.byref(d_zz)))
    ctx.check(L.tic_dev_alloc(ctx.handle, cap, C.byref(d_out)))
    ctx.check(L.tic_dev_alloc(ctx.handle, dim * dim, C.byref(d_dec)))
    n, q_out, sse_out = C.c_size_t(), C.c_int(), C.c_uint64()
    hh, ww = C.c_int(), C.c_int()
    dec = np.empty((dim, dim), np.uint8)
    wide = img.astype(np.int32)

    def old_probe(q):
        """compress, decompress, download, square: -> (stream length or None, squared error)."""
        rc = L.tic_compress_dev(ctx.handle, d_img, dim, dim, dim, q, d_out, cap, C.byref(n))
        if rc == N.TIC_E_RANGE:
            return None, None
        ctx.check(rc)
        ctx.check(L.tic_decompress_dev(ctx.handle, d_out, n.value, d_dec, dim, dim * dim, C.byref(hh), C.byref(ww)))
        ctx.check(L.tic_memcpy_d2h(ctx.handle, dec.ctypes.data, d_dec, dim * dim))
        d = wide - dec
        return n.value, int(np.einsum("ij,ij->", d, d, dtype=np.int64))

    def old_search(max_sse, qmin=1, qmax=QMAX):
        calls = 1
        size, sse = old_probe(qmax)
        if size is None or sse > max_sse:
            return None, calls
        lo, hi, last = qmin, qmax, qmax
        while lo < hi:
            mid = (lo + hi) // 2
            calls += 1
            size, sse = old_probe(mid)
            last = mid
            if size is not None and sse <= max_sse:
                hi = mid
            else:
                lo = mid + 1
        if last != lo:  # the stream in d_out is not the chosen quality's
            calls += 1
            ctx.check(L.tic_compress_dev(ctx.handle, d_img, dim, dim, dim, lo, d_out, cap, C.byref(n)))
        return lo, calls

    print("%s:" % name)
    ctx.check(L.tic_memcpy_h2d(ctx.handle, d_img, img.ctypes.data, img.size))
    # (a) the measuring kernel, idct_kernel and the other two launches of a probe, each alone between two events, quality 50
    ms, v = C.c_float(), {"transform": [], "size kernel": [], "measuring kernel": [], "idct_kernel": []}
    for r in range(args.rounds):
        ctx.check(L.tic_dctq_dev_timed_warm(ctx.handle, d_img, dim, dim, dim, 50, d_zz, N.KERNEL_AUTO, args.warm, args.iters, C.byref(ms), None))
        v["transform"].append(ms.value / args.iters * 1e3)
        ctx.check(L.tic_entropy_size_dev_timed(ctx.handle, d_zz, dim, dim, args.warm, args.iters, C.byref(ms)))
        v["size kernel"].append(ms.value / args.iters * 1e3)
        ctx.check(L.tic_distortion_dev_timed(ctx.handle, d_zz, d_img, dim, dim, dim, 50, -1, args.warm, args.iters, C.byref(ms)))
        v["measuring kernel"].append(ms.value / args.iters * 1e3)
        ctx.check(L.tic_idct_dev_timed(ctx.handle, d_zz, d_dec, dim, dim, dim, 50, -1, args.warm, args.iters, C.byref(ms)))
        v["idct_kernel"].append(ms.value / args.iters * 1e3)
    for k, t in v.items():
        print("  (a) %-17s alone, q = 50: best %8.2f us, median %8.2f us per frame" % (k, min(t), statistics.median(t)))
    print("      measuring kernel: %.2f TB/s at 3 B per pixel (2 B coefficients + 1 B original); measuring / idct_kernel (best): %.3f"
          % (3 * dim * dim / (min(v["measuring kernel"]) * 1e-6) / 1e12, min(v["measuring kernel"]) / min(v["idct_kernel"])))
    # (b) one probe beside compress + decompress + download + host squared error
    q1, q16 = (C.c_int * 1)(50), (C.c_int * 16)(*range(5, 96, 6))
    s1, a1, b1 = (C.c_longlong * 1)(), (C.c_uint64 * 1)(), (C.c_uint64 * 1)()
    s16, a16, b16 = (C.c_longlong * 16)(), (C.c_uint64 * 16)(), (C.c_uint64 * 16)()
    res = {"probe": [], "probe16": [], "old": []}
    old = None
    for r in range(args.rounds + 2):
        res["probe"].append(wall(lambda: ctx.check(L.tic_rd_points_dev(ctx.handle, d_img, dim, dim, dim, q1, 1, s1, a1, b1))))
        t = time.perf_counter()
        old = old_probe(50)
        res["old"].append((time.perf_counter() - t) * 1e6)
        res["probe16"].append(wall(lambda: ctx.check(L.tic_rd_points_dev(ctx.handle, d_img, dim, dim, dim, q16, 16, s16, a16, b16))) / 16)
    assert (s1[0], a1[0]) == old, ((s1[0], a1[0]), old)
    show("(b) one probe (tic_rd_points_dev, 1 quality)", res["probe"][2:])
    show("    per probe, 16 qualities in one submission", res["probe16"][2:])
    show("    compress_dev + decompress_dev + download + numpy (q = 50)", res["old"][2:])
    print("      probe / old (best): %.3f     q = 50: %d bytes, PSNR %.2f dB (the reference's arithmetic: %.2f dB)"
          % (min(res["probe"][2:]) / min(res["old"][2:]), s1[0], T.psnr_from_sse(a1[0], dim * dim), T.psnr_from_sse(b1[0], dim * dim)))
    # (c) the search beside the same bisection with the three calls per probe
    qs = (C.c_int * 3)(20, 50, 90)
    s3, a3, b3 = (C.c_longlong * 3)(), (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
    ctx.check(L.tic_rd_points_dev(ctx.handle, d_img, dim, dim, dim, qs, 3, s3, a3, b3))
    for max_sse in list(a3):
        new, oldt = [], []
        for r in range(args.rounds + 1):
            new.append(wall(lambda: ctx.check(L.tic_compress_to_psnr_dev(ctx.handle, d_img, dim, dim, dim, max_sse, 1, QMAX, d_out, cap, C.byref(n),
                                                                          C.byref(q_out), C.byref(sse_out)))))
            got = (q_out.value, n.value)
            t = time.perf_counter()
            q_old, calls = old_search(max_sse)
            oldt.append((time.perf_counter() - t) * 1e6)
            assert (q_old, n.value) == got, (q_old, n.value, got)
        probes, waits = C.c_int(), C.c_int()
        ctx.check(L.tic_compress_to_psnr_dev(ctx.handle, d_img, dim, dim, dim, max_sse, 1, QMAX, d_out, cap, C.byref(n), C.byref(q_out), C.byref(sse_out)))
        ctx.check(L.tic_last_rate_search(ctx.handle, C.byref(probes), C.byref(waits)))
        print("  (c) at least %.2f dB -> quality %d, %d bytes" % (T.psnr_from_sse(max_sse, dim * dim), got[0], got[1]))
        show("    tic_compress_to_psnr_dev (%d probes, %d host waits)" % (probes.value, waits.value), new[1:])
        show("    bisection with compress + decompress + download + numpy (%d calls)" % calls, oldt[1:])
        print("      new / old (best): %.3f" % (min(new[1:]) / min(oldt[1:])))
    for p in (d_img, d_zz, d_out, d_dec):
        L.tic_dev_free(ctx.handle, p)
ctx.close()
