"""The adaptive encoder over a list of frames, three ways, in one process on one GPU (it fails without one): host clock around the Python
calls - every one returns its streams, so the device has finished -, after warm-up, the lines interleaved and the order rotated:
  (a) loop         compress_adaptive() per frame: the yardstick, which the batch route leaves untouched.  It is timed as TWO lines,
                   (a) and (a'), so that their medians' difference measures the yardstick against itself;
  (b) one call     ONE compress_batch_adaptive() over the list;
  (c) default      ONE mixed compress_batch() over the list: the default-table floor (no statistics, no table build).
Workloads: the reference's benchmark loop (49 images x qualities 90, 80, 50, 20, 10, 5: 294 frames of 512 x 512), bytes checked against
tests/golden/adaptive_streams.json once; and 16 frames of 1080p noise at q = 50, (b) checked against (a).
The bar (294-frame set): (b) faster than (a) by more than |median (a) - median (a')|.
  python tools/adaptive_batch_timing.py [--rounds 30]
  python tools/adaptive_batch_timing.py --kernels N     only N one-call runs per workload after one warm call (for a kernel trace)"""
import argparse, hashlib, json, os, statistics, sys, time
sys.path.insert(0, '.')
import numpy as np
import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--kernels", type=int, default=0)
args = ap.parse_args()
assert args.rounds >= 30 or args.kernels
ctx = T.Context(0)  # (raises without a GPU)
QS = (90, 80, 50, 20, 10, 5)
px = np.load(os.path.join("tests", "golden", "benchmark_set.npz"))["pixels"]
gold = {(e["image"], e["quality"]): e["sha256"] for e in json.load(open(os.path.join("tests", "golden", "adaptive_streams.json")))["benchmark"]}
pairs = [(i, q) for i in range(px.shape[0]) for q in QS]
bench = ([np.ascontiguousarray(px[i]) for i, _ in pairs], [q for _, q in pairs])
noise = ([np.random.default_rng(3000 + k).integers(0, 256, (1080, 1920), dtype=np.uint8) for k in range(16)], [50] * 16)


def loop(frames, qs):
    return [T.compress_adaptive(f, q, ctx=ctx) for f, q in zip(frames, qs)]


def one_call(frames, qs):
    return T.compress_batch_adaptive(frames, qs, ctx=ctx)


def default_tables(frames, qs):
    return T.compress_batch(frames, qs, ctx=ctx)


def figures():
    import ctypes as C
    v = [C.c_int() for _ in range(3)]
    N.load().tic_last_compress_batch_adaptive(ctx.handle, *[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def measure(title, work):
    frames, qs = work
    lines = [("(a)  loop of compress_adaptive", loop), ("(a') the same loop again", loop), ("(b)  one compress_batch_adaptive", one_call),
             ("(c)  one mixed compress_batch", default_tables)]
    for _ in range(3):  # warm: slots, pools, tables
        want, got = loop(frames, qs), one_call(frames, qs)
        default_tables(frames, qs)
    assert got == want, title
    if work is bench:
        assert all(hashlib.sha256(s).hexdigest() == gold[(i + 1, q)] for s, (i, q) in zip(got, pairs))
    print("%s: %d frames, %d adaptive bytes (default tables: %d); every stream of (b) equals (a)%s; batch_frames %d, single_frames %d, chunks %d"
          % ((title, len(frames), sum(map(len, got)), sum(map(len, default_tables(frames, qs))), " and the reference's" if work is bench else "")
             + (one_call(frames, qs) and figures())))
    res = {name: [] for name, _ in lines}
    for r in range(args.rounds):
        for name, fn in lines[r % len(lines):] + lines[:r % len(lines)]:
            t = time.perf_counter()
            fn(frames, qs)
            res[name].append((time.perf_counter() - t) * 1e3)
    med = {k: statistics.median(x) for k, x in res.items()}
    for name, _ in lines:
        x = res[name]
        print("  %-34s median %8.3f ms  min %8.3f  max %8.3f  (%d rounds; %7.2f us per frame)" % (name, med[name], min(x), max(x), len(x), med[name] * 1e3 / len(frames)))
    a, a2, b, c = (med[name] for name, _ in lines)
    spread = abs(a - a2)
    print("  yardstick against itself: %.3f ms; (b) against (a): %+.3f ms (%.2f x); (b) against (c): %+.3f ms (%.2f x)  ->  %s"
          % (spread, b - min(a, a2), b / min(a, a2), b - c, b / c,
             "one call FASTER than the loop by more than the spread" if min(a, a2) - b > spread else "one call NOT faster than the loop beyond the spread"))


if args.kernels:
    for work in (bench, noise):
        one_call(*work)
        for _ in range(args.kernels):
            one_call(*work)
        print("one-call runs done:", len(work[0]), "frames, figures", figures())
else:
    measure("benchmark set", bench)
    measure("1080p noise", noise)
ctx.close()
