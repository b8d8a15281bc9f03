"""The adaptive decoder over a list of streams, three ways, in one process on one GPU (it fails without one): host clock around the calls - every
one returns its pixels, so the device has finished -, the median of --rounds interleaved repetitions after three warm ones, the order rotated (the lines keep their cyclic order):
  (a) one call     ONE decompress_batch_adaptive() over the list (this build);
  (b) loop         tic_decompress_adaptive per stream against ANOTHER build of the library - the parent commit's, which has no batch call -
                   loaded side by side (the way of tools/ab_libs.py and tools/ab_adaptive_dec.py), an output array per stream as in (b');
  (b') the loop    of decompress_adaptive() on this build (the single call is untouched by the batch: the two loops should agree);
  (c) default      ONE decompress_batch() of the default-table streams of the same frames, for orientation.
Workloads: the reference's benchmark loop (49 images x qualities 90, 80, 50, 20, 10, 5: 294 streams of 512 x 512, built with ONE
compress_batch_adaptive, bytes checked against tests/golden/adaptive_streams.json, pixels of (a) against benchmark_set.json); 16 frames of 1080p
noise at q = 50, (a) checked against (b) and (b').  After the timed rounds: the figures of (c), and the phases (tic_last_batch_phases) of the
median of seven more calls of (a).
  python tools/adaptive_decode_batch_timing.py path/to/libparent.so [--rounds 30]"""
import argparse, ctypes as C, hashlib, json, os, statistics, sys, time
sys.path.insert(0, '.')
import numpy as np
import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

ap = argparse.ArgumentParser()
ap.add_argument("other")
ap.add_argument("--rounds", type=int, default=30)
args = ap.parse_args()
assert args.rounds >= 30
print("command line: python tools/adaptive_decode_batch_timing.py %s --rounds %d" % (args.other, args.rounds))
L = N.load()
old = C.CDLL(args.other)
for name in ("tic_create", "tic_destroy", "tic_decompress_adaptive"):
    res, a = N.SIGNATURES[name]
    fn = getattr(old, name); fn.restype = res; fn.argtypes = a
assert not hasattr(old, "tic_decompress_batch_adaptive"), "the other library is to be the parent's: it has no batch call"
ctx = T.Context(0)  # (raises without a GPU)
octx = old.tic_create(0)
assert octx
QS = (90, 80, 50, 20, 10, 5)
golden = os.path.join("tests", "golden")
px = np.load(os.path.join(golden, "benchmark_set.npz"))["pixels"]
gold = {(e["image"], e["quality"]): e["sha256"] for e in json.load(open(os.path.join(golden, "adaptive_streams.json")))["benchmark"]}
decoded = {(e["image"], e["quality"]): e["decoded_sha256"] for e in json.load(open(os.path.join(golden, "benchmark_set.json")))["entries"]}
pairs = [(i, q) for i in range(px.shape[0]) for q in QS]
bench = ([np.ascontiguousarray(px[i]) for i, _ in pairs], [q for _, q in pairs])
noise = ([np.random.default_rng(3000 + k).integers(0, 256, (1080, 1920), dtype=np.uint8) for k in range(16)], [50] * 16)


def sha(b):
    return hashlib.sha256(b).hexdigest()


def measure(title, work):
    frames, qs = work
    streams = T.compress_batch_adaptive(frames, qs, ctx=ctx)
    plain = T.compress_batch(frames, qs, ctx=ctx)
    bufs = [np.frombuffer(s, np.uint8) for s in streams]
    shapes = [f.shape for f in frames]

    def one_call():
        return T.decompress_batch_adaptive(streams, ctx=ctx)

    def parent_loop():  # (what decompress_adaptive() does per stream, on the other library: an output array each)
        outs = []
        for b, (h, w) in zip(bufs, shapes):
            o = np.zeros((h, w), np.uint8)
            assert old.tic_decompress_adaptive(octx, b.ctypes.data, b.size, o.ctypes.data, o.size) == 0
            outs.append(o)
        return outs

    def this_loop():
        return [T.decompress_adaptive(s, ctx=ctx) for s in streams]

    def default_tables():
        return T.decompress_batch(plain, ctx=ctx)

    lines = [("(a)  one decompress_batch_adaptive", one_call), ("(b)  loop, the other build", parent_loop), ("(b') loop, this build", this_loop),
             ("(c)  one decompress_batch, default tables", default_tables)]
    for _ in range(3):  # warm: buffers, tables
        got, want, mine = one_call(), parent_loop(), this_loop()
        default_tables()
    assert all(np.array_equal(g, w) and np.array_equal(g, m) for g, w, m in zip(got, want, mine)), title
    if work is bench:
        assert all(sha(s) == gold[(i + 1, q)] for s, (i, q) in zip(streams, pairs))
        assert all(sha(np.ascontiguousarray(g).tobytes()) == decoded[(i + 1, q)] for g, (i, q) in zip(got, pairs))
    v = [C.c_int() for _ in range(3)]
    one_call()
    L.tic_last_decompress_batch_adaptive(ctx.handle, *[C.byref(x) for x in v])
    print("%s: %d streams, %d adaptive bytes (default tables: %d); the pixels of (a), (b) and (b') are equal%s; batch_frames %d, single_frames %d, chunks %d, direct %d"
          % (title, len(streams), sum(map(len, streams)), sum(map(len, plain)), " and the reference's" if work is bench else "", v[0].value, v[1].value, v[2].value,
             L.tic_last_decompress_batch_adaptive_direct(ctx.handle)))
    res = {name: [] for name, _ in lines}
    for r in range(args.rounds):
        for name, fn in lines[r % len(lines):] + lines[:r % len(lines)]:
            t = time.perf_counter()
            fn()
            res[name].append((time.perf_counter() - t) * 1e3)
    med = {k: statistics.median(x) for k, x in res.items()}
    for name, _ in lines:
        x = res[name]
        print("  %-42s median %9.3f ms  min %9.3f  max %9.3f  (%d rounds; %8.2f us per frame)" % (name, med[name], min(x), max(x), len(x), med[name] * 1e3 / len(streams)))
    a, b, b2, c = (med[name] for name, _ in lines)
    print("  (a) against (b): %+.3f ms (%.3f x)  ->  one call %s than the parent's loop at the median; (a) against (b'): %.3f x; (a) against (c): %+.3f ms (%.2f x)"
          % (a - b, a / b, "FASTER" if a < b else "NOT faster", a / b2, a - c, a / c))
    v4 = [C.c_int() for _ in range(4)]
    default_tables()
    L.tic_last_decompress_batch(ctx.handle, *[C.byref(x) for x in v4])
    print("  (c): batch_frames %d, single_frames %d, chunks %d, direct %d" % tuple(x.value for x in v4))
    runs = []
    for _ in range(7):  # the phases of seven more calls of (a): the call with the median total is shown
        ph = (C.c_double * 8)()
        t = time.perf_counter()
        one_call()
        dt = (time.perf_counter() - t) * 1e3
        L.tic_last_batch_phases(ctx.handle, ph)
        runs.append((dt, list(ph)))
    dt, ph = sorted(runs)[len(runs) // 2]
    print("  phases of a call of (a) that took %.3f ms: pack the upload buffer %.3f | upload, kernels, status %.3f | download %.3f | hand-out %.3f | single calls %.3f"
          % (dt, ph[0], ph[1], ph[2], ph[4], ph[5]))


measure("benchmark set", bench)
measure("1080p noise", noise)
old.tic_destroy(octx)
ctx.close()
