"""Rate control of the adaptive family beside what it replaces, one process, writes profiles/adaptive_rate.txt:

    python tools/adaptive_rate_timing.py [--warm 20] [--iters 200] [--rounds 7] [--out profiles/adaptive_rate.txt]

1. The statistics kernels alone on the same resident coefficients (tic_adaptive_stats_v_dev_timed: events around back-to-back rounds of
   reset + launch): adaptive_stats_probe_kernel_v (kernel 0, at several workgroup caps) against adaptive_stats_v_kernel (kernel 1, the
   yardstick, timed twice per round for its own spread), the size kernel (tic_entropy_size_dev_timed) on the same buffer beside them.
   Shapes: seven probes of bench01 (the middles of the first round of a search over 1..99 at depth 3) in one launch; one probe of
   4096^2 noise at q = 50.
2. compress_adaptive_to_size over 1..99 on bench01 and on 4096^2 noise against the same bisection with one tic_compress_adaptive per
   step (what a caller had before), and the 49 x 6 benchmark table in one compressed_sizes_adaptive_batch call against the loop of
   len(compress_adaptive(...)).
The sides of every comparison alternate round by round; medians with min-max of the rounds are printed."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import tinyimgcodec_amd as T  # noqa: E402
from tinyimgcodec_amd import _native as N  # noqa: E402

# hipcc -Rpass-analysis=kernel-resource-usage on tic_adaptive_stats_gpu.hip (gfx950), recorded when the kernel last changed
RESOURCES = "adaptive_stats_probe_kernel_v: 60 VGPRs, 0 AGPRs, 80 SGPRs, LDS 10920 bytes per workgroup, scratch 0 bytes per lane, no spills, occupancy 8 waves per SIMD"

ap = argparse.ArgumentParser()
ap.add_argument("--warm", type=int, default=20)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_rate.txt"))
args = ap.parse_args()

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def spread(v):
    return "median %9.2f  (min %9.2f, max %9.2f)" % (statistics.median(v), min(v), max(v))


L = N.load()
ctx = T.Context(0)
golden = os.path.join(ROOT, "tests", "golden")
bench = np.load(os.path.join(golden, "benchmark_set.npz"))["pixels"]
bench01 = bench[0]
noise = np.random.default_rng(1234).integers(0, 256, (4096, 4096), dtype=np.uint8)
FIRST_ROUND = (50, 75, 87, 62, 25, 37, 13)  # rate_candidates(1, 99, depth 3)

say("adaptive rate control: tools/adaptive_rate_timing.py --warm %d --iters %d --rounds %d on %s" % (args.warm, args.iters, args.rounds, ctx.arch))
say(RESOURCES)
say()
say("1. statistics kernels, us per round of reset + launch (%d timed rounds per figure, %d figures)" % (args.iters, args.rounds))


def kernel_shape(label, zz, nblocks, h, w):
    zz = np.ascontiguousarray(zz, np.int16)
    d = C.c_void_p()
    ctx.check(L.tic_dev_alloc(ctx.handle, zz.nbytes + 16, C.byref(d)))
    ctx.check(L.tic_memcpy_h2d(ctx.handle, d, zz.ctypes.data, zz.nbytes))
    nb = (C.c_size_t * len(nblocks))(*nblocks)
    ms = C.c_float(0)

    def stats(kernel, cap):
        ctx.check(L.tic_adaptive_stats_v_dev_timed(ctx.handle, d, len(nblocks), nb, kernel, cap, args.warm, args.iters, C.byref(ms)))
        return ms.value * 1e3 / args.iters

    def size():
        ctx.check(L.tic_entropy_size_dev_timed(ctx.handle, d, h, w, args.warm, args.iters, C.byref(ms)))
        return ms.value * 1e3 / args.iters

    sides = [("adaptive_stats_v_kernel (yardstick)", lambda: stats(1, 0)), ("adaptive_stats_v_kernel (again)", lambda: stats(1, 0)),
             ("probe kernel, plan's groups", lambda: stats(0, 0)), ("probe kernel, at most 512 groups", lambda: stats(0, 512)),
             ("probe kernel, at most 256 groups", lambda: stats(0, 256)), ("size kernel, one launch (no reset)", size)]
    got = {name: [] for name, _ in sides}
    for _ in range(args.rounds):
        for name, fn in sides:
            got[name].append(fn())
    say("  %s: %d probes, %d blocks, %.1f MB of coefficients" % (label, len(nblocks), sum(nblocks), zz.nbytes / 1e6))
    for name, _ in sides:
        say("    %-38s %s" % (name, spread(got[name])))
    ctx.check(L.tic_dev_free(ctx.handle, d))
    return {k: statistics.median(v) for k, v in got.items()}, abs(statistics.median(got[sides[0][0]]) - statistics.median(got[sides[1][0]]))


zz7 = np.concatenate([T.dctq(bench01, q, ctx=ctx) for q in FIRST_ROUND])
nb01 = L.tic_num_blocks(*bench01.shape)
m7, s7 = kernel_shape("bench01 at q = %s" % (FIRST_ROUND,), zz7, [nb01] * 7, bench01.shape[0] * 7, bench01.shape[1])
m1, s1 = kernel_shape("4096^2 noise at q = 50", T.dctq(noise, 50, ctx=ctx), [L.tic_num_blocks(4096, 4096)], 4096, 4096)
old7, new7, old1, new1 = (m7["adaptive_stats_v_kernel (yardstick)"], m7["probe kernel, plan's groups"], m1["adaptive_stats_v_kernel (yardstick)"],
                          m1["probe kernel, plan's groups"])
slower_both = new7 > old7 + s7 and new1 > old1 + s1
say("  decision: the probe kernel is %s at seven probes (%.2f against %.2f us, yardstick spread %.2f) and %s at 4096^2 (%.2f against %.2f us, spread"
    " %.2f): %s" % ("slower" if new7 > old7 else "faster", new7, old7, s7, "slower" if new1 > old1 else "faster", new1, old1, s1,
                    "slower at both shapes by more than the spread - the search routes must use adaptive_stats_v_kernel" if slower_both
                    else "not slower at both shapes - the search routes use it"))
say()
say("2. search and table, us per call (wall clock around synchronous calls, %d rounds, sides alternating)" % args.rounds)


def wall(fn):
    t = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t) * 1e6, r


def loop_search(img, budget, qmin=1, qmax=99):
    """The bisection with what the library had before: a whole tic_compress_adaptive per step, its length read back."""
    h, w = img.shape
    cap = L.tic_compress_bound(h, w) + 4096
    out = getattr(ctx, "_timing_buf", None)
    if out is None or out.size < cap:
        out = ctx._timing_buf = np.empty(cap, np.uint8)
    n = C.c_size_t(0)
    calls = last = 0

    def fits(q):
        nonlocal calls, last
        calls, last = calls + 1, q
        rc = L.tic_compress_adaptive(ctx.handle, img.ctypes.data, h, w, w, q, out.ctypes.data, cap, C.byref(n))
        return rc == 0 and n.value <= budget

    assert fits(qmin)
    lo, hi = qmin, qmax
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if fits(mid):
            lo = mid
        else:
            hi = mid - 1
    if last != lo:  # the buffer holds the last probe's stream: another quality's as often as not
        fits(lo)
    return out[: n.value].tobytes(), lo, calls


for label, img in (("bench01", bench01), ("4096^2 noise", noise)):
    budget = int(T.compressed_size_adaptive(img, 50, ctx=ctx))
    a, b = [], []
    for _ in range(args.rounds + 1):
        ta, (bs_new, q_new) = wall(lambda: T.compress_adaptive_to_size(img, budget, ctx=ctx))
        p, w_, s_ = C.c_int(), C.c_int(), C.c_int()
        L.tic_last_adaptive_rate(ctx.handle, C.byref(p), C.byref(w_), C.byref(s_))
        tb, (bs_old, q_old, calls) = wall(lambda: loop_search(img, budget))
        assert (bs_new, q_new) == (bs_old, q_old)
        a.append(ta)
        b.append(tb)
    a, b = a[1:], b[1:]  # (the first round warms both)
    say("  %s, budget = its size at q = 50 (%d bytes) -> q = %d" % (label, budget, q_new))
    say("    %-52s %s" % ("compress_adaptive_to_size (%d probes, %d waits, %d launches)" % (p.value, w_.value, s_.value), spread(a)))
    say("    %-52s %s" % ("bisection, tic_compress_adaptive per step (%d calls)" % calls, spread(b)))

frames = list(bench)
qs = (90, 80, 50, 20, 10, 5)
a, b = [], []
for _ in range(max(3, args.rounds // 2) + 1):
    ta, table = wall(lambda: T.compressed_sizes_adaptive_batch(frames, qs, ctx=ctx))
    tb, loop = wall(lambda: [[len(T.compress_adaptive(im, q, ctx=ctx)) for q in qs] for im in frames])
    assert table.tolist() == loop
    a.append(ta)
    b.append(tb)
a, b = a[1:], b[1:]
say("  the 49 x 6 benchmark table")
say("    %-52s %s" % ("compressed_sizes_adaptive_batch, one call", spread(a)))
say("    %-52s %s" % ("loop of len(compress_adaptive(image, q))", spread(b)))
ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
