"""Rate control beside what it replaces, one process, resident frames (4096^2 noise and Lenna tiled to 4096^2):

    python tools/rate_control_timing.py [--dim 4096] [--warm 20] [--iters 200] [--rounds 5]

(a) the size kernel alone (tic_entropy_size_dev_timed: events around back-to-back launches) and its fraction of 8 TB/s at the 2 bytes
    per coefficient it reads;
(b) one probe - transform + size kernel, tic_stream_sizes_dev with one quality, and per probe with 16 in one submission - beside one
    tic_compress_dev call (wall clock around the synchronous calls);
(c) tic_compress_to_size_dev over 1..99 at three budgets beside the same bisection written with tic_compress_dev per probe (what a
    caller had before: a stream per probe, its out_len read back), with the probes and host waits of every search.
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
dim = args.dim
lenna = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "lenna.npz"))["img"]
frames = {"noise": np.random.default_rng(1234).integers(0, 256, (dim, dim), dtype=np.uint8),
          "lenna tiled": np.ascontiguousarray(np.tile(lenna, ((dim + 511) // 512, (dim + 511) // 512))[:dim, :dim])}
cap = L.tic_compress_bound(dim, dim)
d_img, d_zz, d_out = C.c_void_p(), C.c_void_p(), C.c_void_p()
ctx.check(L.tic_dev_alloc(ctx.handle, dim * dim, C.byref(d_img)))
ctx.check(L.tic_dev_alloc(ctx.handle, L.tic_num_blocks(dim, dim) * 128 + 16, C.byref(d_zz)))
ctx.check(L.tic_dev_alloc(ctx.handle, cap, C.byref(d_out)))
n, q_out = C.c_size_t(), C.c_int()


def wall(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e6


def show(label, v):
    print("  %-58s best %8.1f us, median %8.1f us" % (label, min(v), statistics.median(v)))


def old_search(budget, qmin=1, qmax=99):
    """The bisection with the entry points the library had before: a whole tic_compress_dev per probe."""
    calls = 0

    def fits(q):
        nonlocal calls
        calls += 1
        rc = L.tic_compress_dev(ctx.handle, d_img, dim, dim, dim, q, d_out, cap, C.byref(n))
        if rc == N.TIC_E_RANGE:
            return False
        ctx.check(rc)
        return n.value <= budget

    if not fits(qmin):
        return None, calls
    lo, hi = qmin, qmax
    last = qmin
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if fits(mid):
            lo = last = mid
        else:
            hi = mid - 1
            last = None
    if last != lo:  # the stream in d_out is not the chosen quality's
        fits(lo)
    return lo, calls


print("%s  %dx%d  warm %d iters %d rounds %d" % (ctx.arch, dim, dim, args.warm, args.iters, args.rounds))
for name, img in frames.items():
    print("%s:" % name)
    ctx.check(L.tic_memcpy_h2d(ctx.handle, d_img, img.ctypes.data, img.size))
    # (a) the size kernel alone, on the coefficients of quality 50
    ctx.check(L.tic_dctq_dev(ctx.handle, d_img, dim, dim, dim, 50, d_zz, N.KERNEL_AUTO))
    ms, v = C.c_float(), []
    for r in range(args.rounds):
        ctx.check(L.tic_entropy_size_dev_timed(ctx.handle, d_zz, dim, dim, args.warm, args.iters, C.byref(ms)))
        v.append(ms.value / args.iters * 1e3)
    print("  (a) size kernel alone, q = 50 coefficients: best %.2f us, median %.2f us per frame = %.2f TB/s = %.0f %% of 8 TB/s at 2 B per coefficient"
          % (min(v), statistics.median(v), 2 * dim * dim / (min(v) * 1e-6) / 1e12, 100 * 2 * dim * dim / (min(v) * 1e-6) / 8e12))
    # (b) one probe beside one tic_compress_dev
    q1, s1 = (C.c_int * 1)(50), (C.c_longlong * 1)()
    q16, s16 = (C.c_int * 16)(*range(5, 96, 6)), (C.c_longlong * 16)()
    res = {"probe": [], "probe16": [], "compress": []}
    for r in range(args.rounds + 2):
        res["probe"].append(wall(lambda: ctx.check(L.tic_stream_sizes_dev(ctx.handle, d_img, dim, dim, dim, q1, 1, s1))))
        res["compress"].append(wall(lambda: ctx.check(L.tic_compress_dev(ctx.handle, d_img, dim, dim, dim, 50, d_out, cap, C.byref(n)))))
        res["probe16"].append(wall(lambda: ctx.check(L.tic_stream_sizes_dev(ctx.handle, d_img, dim, dim, dim, q16, 16, s16))) / 16)
    assert s1[0] == n.value
    show("(b) one probe (tic_stream_sizes_dev, 1 quality)", res["probe"][2:])
    show("    per probe, 16 qualities in one submission", res["probe16"][2:])
    show("    one tic_compress_dev (q = 50, %d bytes)" % n.value, res["compress"][2:])
    print("      probe / compress (best): %.3f" % (min(res["probe"][2:]) / min(res["compress"][2:])))
    # (c) the search beside the same bisection with tic_compress_dev per probe
    qs, sz = (C.c_int * 3)(20, 50, 90), (C.c_longlong * 3)()
    ctx.check(L.tic_stream_sizes_dev(ctx.handle, d_img, dim, dim, dim, qs, 3, sz))
    for budget in list(sz):
        new, old = [], []
        for r in range(args.rounds + 1):
            new.append(wall(lambda: ctx.check(L.tic_compress_to_size_dev(ctx.handle, d_img, dim, dim, dim, budget, 1, 99, d_out, cap, C.byref(n), C.byref(q_out)))))
            got = (q_out.value, n.value)
            t = time.perf_counter()
            q_old, calls = old_search(budget)
            old.append((time.perf_counter() - t) * 1e6)
            assert (q_old, n.value) == got, (q_old, n.value, got)
        probes, waits = C.c_int(), C.c_int()
        ctx.check(L.tic_last_rate_search(ctx.handle, C.byref(probes), C.byref(waits)))
        print("  (c) budget %d bytes -> quality %d" % (budget, got[0]))
        show("    tic_compress_to_size_dev (%d probes, %d host waits)" % (probes.value, waits.value), new[1:])
        show("    bisection with tic_compress_dev (%d calls, as many waits)" % calls, old[1:])
        print("      new / old (best): %.3f" % (min(new[1:]) / min(old[1:])))
for p in (d_img, d_zz, d_out):
    L.tic_dev_free(ctx.handle, p)
ctx.close()
