"""A byte budget per frame for a whole list of frames, three ways, in one process on one GPU (it fails without one): a host clock around
calls that return their streams - so the device has finished -, --rounds interleaved repetitions after two warm ones, the order rotated:
  (a) one call     ONE tic_compress_batch_to_size over the list (this build);
  (b) loop         tic_compress_to_size per frame against ANOTHER build of the library - the parent commit's, which has no batch call -
                   loaded side by side (the way of tools/ab_libs.py and tools/adaptive_decode_batch_timing.py);
  (b') the loop    of tic_compress_to_size on this build (the single call is untouched by the batch: the two loops should agree; their
                   difference is the loop's own spread).
Workloads: (1) the 49 benchmark images, each at six budgets (4, 8, 16, 32, 64, 128 KiB): 294 frames of 512 x 512 in one call;
(2) 16 frames of 1080p noise, each with its own q = 50 size as the budget.  Every side's streams and qualities are checked against the
others'.  Criterion, on (1): the one call is faster than the parent's loop at the median by more than the loop's own spread - the tool says
in plain words whether it is.  Also printed: probes, host waits and size-kernel launches per side.
  python tools/rate_batch_timing.py path/to/libparent.so [--rounds 7]"""
import argparse, ctypes as C, os, statistics, sys, time
sys.path.insert(0, '.')
import numpy as np
import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

ap = argparse.ArgumentParser()
ap.add_argument("other")
ap.add_argument("--rounds", type=int, default=7)
args = ap.parse_args()
assert args.rounds >= 7
print("command line: python tools/rate_batch_timing.py %s --rounds %d" % (args.other, args.rounds))
L = N.load()
old = C.CDLL(args.other)
for name in ("tic_create", "tic_destroy", "tic_compress_to_size", "tic_last_rate_search", "tic_compress_bound"):
    res, a = N.SIGNATURES[name]
    fn = getattr(old, name); fn.restype = res; fn.argtypes = a
assert not hasattr(old, "tic_compress_batch_to_size"), "the other library is to be the parent's: it has no batch call"
ctx = T.Context(0)  # (raises without a GPU)
octx = old.tic_create(0)
assert octx
px = np.load(os.path.join("tests", "golden", "benchmark_set.npz"))["pixels"]
KIB = (4, 8, 16, 32, 64, 128)
bench = ([np.ascontiguousarray(px[i]) for i in range(px.shape[0]) for _ in KIB], [k << 10 for _ in range(px.shape[0]) for k in KIB])
noise_frames = [np.random.default_rng(3000 + k).integers(0, 256, (1080, 1920), dtype=np.uint8) for k in range(16)]
noise = (noise_frames, [int(v) for v in T.compressed_sizes_batch(noise_frames, [50], ctx=ctx)[:, 0]])


def measure(title, work):
    frames, budgets = work
    n = len(frames)
    caps_l = [L.tic_compress_bound(f.shape[0], f.shape[1]) for f in frames]
    bufs = [np.empty(c, np.uint8) for c in caps_l]
    inp = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
    hs = (C.c_int * n)(*[f.shape[0] for f in frames])
    ws = (C.c_int * n)(*[f.shape[1] for f in frames])
    strides = (C.c_ssize_t * n)(*[f.shape[1] for f in frames])
    outp = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    caps = (C.c_size_t * n)(*caps_l)
    budg = (C.c_size_t * n)(*budgets)
    lens, quals, status = (C.c_size_t * n)(), (C.c_int * n)(), (C.c_int * n)()
    counts = {}

    def result():
        return [(bufs[i][: lens[i]].tobytes(), quals[i]) if status[i] == 0 else (None, status[i], lens[i]) for i in range(n)]

    def one_call():
        L.tic_compress_batch_to_size(ctx.handle, inp, n, hs, ws, strides, budg, 1, 99, outp, caps, lens, quals, status)

    def loop_on(lib, handle):
        def run():
            ln, q = C.c_size_t(), C.c_int()
            probes = waits = 0
            p, w = C.c_int(), C.c_int()
            for i in range(n):
                status[i] = lib.tic_compress_to_size(handle, inp[i], hs[i], ws[i], strides[i], budg[i], 1, 99, outp[i], caps[i], C.byref(ln), C.byref(q))
                lens[i], quals[i] = ln.value, q.value
                lib.tic_last_rate_search(handle, C.byref(p), C.byref(w))
                probes, waits = probes + p.value, waits + w.value
            counts[run] = (probes, waits)
        return run

    parent_loop, this_loop = loop_on(old, octx), loop_on(L, ctx.handle)
    lines = [("(a)  one tic_compress_batch_to_size", one_call), ("(b)  loop, the other build", parent_loop), ("(b') loop, this build", this_loop)]
    results = []
    for _ in range(2):  # warm, and the check: the three sides agree in every stream, quality and failure
        results = []
        for _, fn in lines:
            fn()
            results.append(result())
    assert results[0] == results[1] == results[2], "the sides disagree"
    ok = sum(r[0] is not None for r in results[0])
    times = {label: [] for label, _ in lines}
    for r in range(args.rounds):
        for k in range(len(lines)):
            label, fn = lines[(k + r) % len(lines)]
            t = time.perf_counter()
            fn()
            times[label].append((time.perf_counter() - t) * 1e3)
    one_call()
    v = [C.c_int() for _ in range(6)]
    L.tic_last_rate_batch(ctx.handle, *[C.byref(x) for x in v])
    bf, sf, ch, pr, wa, la = [x.value for x in v]
    print("%s: %d frames, %d within budget, %.1f MB of pixels" % (title, n, ok, sum(f.size for f in frames) / 1e6))
    for label, _ in lines:
        t = times[label]
        print("  %-38s median %9.3f ms  min %9.3f  max %9.3f" % (label, statistics.median(t), min(t), max(t)))
    print("  (a): %d batch frames, %d behind the batch, %d chunks, %d probes, %d search waits (+ the mixed batch's), %d size launches (one per <= 64 probes)"
          % (bf, sf, ch, pr, wa, la))
    for label, fn in (("(b) ", parent_loop), ("(b')", this_loop)):
        print("  %s: %d probes, %d host waits, as many size launches as probes" % (label, counts[fn][0], counts[fn][1]))
    a, b, b2 = (statistics.median(times[label]) for label, _ in lines)
    spread = max(abs(b - b2), max(times[lines[1][0]]) - min(times[lines[1][0]]))
    print("  the loop against itself: (b) - (b') = %+.3f ms at the median; (b)'s own range %.3f ms -> spread %.3f ms" % (b - b2, max(times[lines[1][0]]) - min(times[lines[1][0]]), spread))
    verdict = "FASTER than" if b - a > spread else ("SLOWER than" if a - b > spread else "NOT DISTINGUISHABLE from")
    print("  (a) against (b): %+.3f ms (%.2f x)  ->  the one call is %s the parent's loop at the median (difference %s the loop's own spread)"
          % (a - b, b / a, verdict, "beyond" if abs(a - b) > spread else "within"))


print(ctx.arch, "rounds", args.rounds)
measure("(1) benchmark images x six budgets", bench)
measure("(2) 16 frames of 1080p noise, budget = own q = 50 size", noise)
old.tic_destroy(octx)
ctx.close()
