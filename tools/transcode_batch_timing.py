"""Batch transcoding against the loop of single calls, host to host, in one process: tic_retable_adaptive_batch / tic_retable_default_batch
of THIS build against a loop of tic_retable_adaptive / tic_retable_default of ANOTHER build of the library (--other, required: the parent
commit's, built into tools/bin/ and loaded side by side by ctypes - the way tools/ab_libs.py, a script, binds builds), the two alternating,
medians of --rounds rounds.  Beside every ratio the loop's own run-to-run spread ((max - min) / median over the rounds): a ratio inside it
says nothing.

  - the 294 streams of the reference's benchmark set in one call, both directions;
  - the 49 streams at q = 5 alone (the stated use case: an archive of low-quality streams), both directions;
  - 16 frames of 1080p noise at q = 50, both directions.

Usage: python tools/transcode_batch_timing.py --other tools/bin/libparent.so [--rounds 9] [--out FILE]   (the output is profiles/transcode_batch.txt (2))"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tinyimgcodec_amd import _native as N  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--other", required=True, help="the library whose single calls make the loop: the parent commit's build")
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.rounds >= 7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bind(path, tables):
    L = C.CDLL(path)
    for t in tables:
        for name, (res, a) in t.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, a
    return L


new = bind(N.LIB_PATH, (N.SIGNATURES, N.TRANSCODE_SIGNATURES, N.TRANSCODE_BATCH_SIGNATURES))
old = bind(args.other, (N.SIGNATURES, N.TRANSCODE_SIGNATURES))
ctx_new = new.tic_create(0)
ctx_old = old.tic_create(0)
assert ctx_new and ctx_old
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def compress(img, q):
    out = np.empty(new.tic_compress_bound(*img.shape), np.uint8)
    n = C.c_size_t(0)
    assert new.tic_compress(ctx_new, img.ctypes.data, img.shape[0], img.shape[1], img.strides[0], q, out.ctypes.data, out.size, C.byref(n)) == 0
    return out[: n.value].copy()


def loop(L, ctx, fn_name, streams, outs):
    fn, n = getattr(L, fn_name), C.c_size_t(0)
    t0 = time.perf_counter()
    for s, o in zip(streams, outs):
        rc = fn(ctx, s.ctypes.data, s.size, o.ctypes.data, o.size, C.byref(n))
        assert rc == 0, (fn_name, rc)
    return time.perf_counter() - t0, n.value


def batch(fn_name, streams, outs):
    k = len(streams)
    sp = (C.c_void_p * k)(*[s.ctypes.data for s in streams])
    op = (C.c_void_p * k)(*[o.ctypes.data for o in outs])
    ln = (C.c_size_t * k)(*[s.size for s in streams])
    cp = (C.c_size_t * k)(*[o.size for o in outs])
    ol = (C.c_size_t * k)()
    t0 = time.perf_counter()
    rc = getattr(new, fn_name)(ctx_new, sp, ln, k, op, cp, ol, None)
    dt = time.perf_counter() - t0
    assert rc == 0, (fn_name, rc, new.tic_last_error(ctx_new).decode())
    return dt, list(ol)


def counters():
    v = [C.c_int(-1) for _ in range(3)]
    assert new.tic_last_transcode_batch(ctx_new, *[C.byref(x) for x in v]) == 0
    return tuple(x.value for x in v)


def measure(what, defaults):
    """defaults: default-table streams (uint8 arrays).  Both directions, the batch of this build against the loop of the other."""
    k = len(defaults)
    outs_a = [np.empty(s.size + 8192, np.uint8) for s in defaults]
    _, lens = batch("tic_retable_adaptive_batch", defaults, outs_a)
    adaptives = [o[:n].copy() for o, n in zip(outs_a, lens)]
    outs_d = [np.empty(s.size + 8192, np.uint8) for s in defaults]
    _, lens = batch("tic_retable_default_batch", adaptives, outs_d)
    assert all(bytes(o[:n]) == bytes(s) for o, n, s in zip(outs_d, lens, defaults)), "there and back is not the identity"
    for direction, src, outs, single in (("-> adaptive", defaults, outs_a, "tic_retable_adaptive"), ("-> default ", adaptives, outs_d, "tic_retable_default")):
        bname = single + "_batch"
        for _ in range(2):  # warm: buffers grown, tables uploaded
            loop(old, ctx_old, single, src, outs)
            batch(bname, src, outs)
        c = counters()
        tl, tb = [], []
        for _ in range(args.rounds):
            tl.append(loop(old, ctx_old, single, src, outs)[0])
            tb.append(batch(bname, src, outs)[0])
        ml, mb = statistics.median(tl), statistics.median(tb)
        say("%-28s %s  %3d frames: loop %8.3f ms (%6.1f us/frame, spread %4.1f %%)  batch %8.3f ms (%6.1f us/frame, spread %4.1f %%)  loop / batch = %5.2f  "
            "(batch_frames, single_frames, chunks) = %s" % (what, direction, k, ml * 1e3, ml * 1e6 / k, 100 * (max(tl) - min(tl)) / ml, mb * 1e3, mb * 1e6 / k,
                                                              100 * (max(tb) - min(tb)) / mb, ml / mb, c))


say("batch transcoding: this build's batch calls against the loop of single calls of %s; %d rounds, alternating, medians" % (args.other, args.rounds))
pixels = np.load(os.path.join(ROOT, "tests", "golden", "benchmark_set.npz"))["pixels"]
qualities = (5, 10, 20, 50, 80, 90)
bench = {q: [compress(np.ascontiguousarray(p), q) for p in pixels] for q in qualities}
assert len(pixels) == 49
measure("benchmark set, 294 streams", [s for q in qualities for s in bench[q]])
measure("benchmark set, q = 5", bench[5])
rng = np.random.default_rng(1080)
measure("1080p noise, q = 50", [compress(rng.integers(0, 256, (1080, 1920), dtype=np.uint8), 50) for _ in range(16)])
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
new.tic_destroy(ctx_new)
old.tic_destroy(ctx_old)
