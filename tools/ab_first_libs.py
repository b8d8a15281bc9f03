"""A/B of a context's FIRST calls between builds of the library in one process: per round and library a fresh context - tic_create, the
first tic_compress_batch of the 49 frames of tests/golden/benchmark_set.npz (allocates every batch slot), the first of 16 seeded 1080p
frames (releases the slots and allocates them again, larger), tic_destroy - rounds interleaved and the order rotated, one untimed round
first; every library's bytes are compared.  Median, minimum and maximum per line and library, and for the product the verdict of
tools/ab_batch_libs.py against two parent builds.  Milliseconds.
Usage: python tools/ab_first_libs.py tools/bin/libparent_a.so tools/bin/libparent_b.so"""
import ctypes as C, os, statistics, sys, time
sys.path.insert(0, '.')
import numpy as np
from tinyimgcodec_amd import _native as N
names = ("tic_create", "tic_destroy", "tic_compress_batch", "tic_compress_bound", "tic_last_error")
def bind(path):
    L = C.CDLL(path)
    for name in names:
        res, a = N.SIGNATURES[name]
        fn = getattr(L, name); fn.restype = res; fn.argtypes = a
    return L
libs = {"product": bind(N.LIB_PATH)}
for pth in sys.argv[1:]:
    libs[os.path.basename(pth).replace("lib", "").replace(".so", "")] = bind(pth)
px = np.load(os.path.join("tests", "golden", "benchmark_set.npz"))["pixels"]
bset = [np.ascontiguousarray(px[i]) for i in range(px.shape[0])]
hd = [np.random.default_rng(1234 + i).integers(0, 256, (1080, 1920), dtype=np.uint8) for i in range(16)]
def batch(L, ctx, frames, q):
    n, (h, w) = len(frames), frames[0].shape
    cap = L.tic_compress_bound(h, w)
    pool = np.zeros((n, cap), dtype=np.uint8)
    inp = (C.c_void_p * n)(*[f.ctypes.data for f in frames]); outp = (C.c_void_p * n)(*[pool[i].ctypes.data for i in range(n)])
    caps = (C.c_size_t * n)(*([cap] * n)); lens = (C.c_size_t * n)()
    t = time.perf_counter()
    rc = L.tic_compress_batch(ctx, inp, n, h, w, w, q, outp, caps, lens, 0)
    t = (time.perf_counter() - t) * 1e3
    assert rc == 0, L.tic_last_error(ctx)
    return t, [pool[i, : lens[i]].tobytes() for i in range(n)]
lines = ("tic_create", "first batch 49x512^2", "first batch 16x1080p", "tic_destroy")
res = {(l, n): [] for l in lines for n in libs}
order, ref = list(libs), None
for r in range(1 + 9):  # (round 0 untimed: the process's first use of every library)
    for name in order[r % len(order):] + order[:r % len(order)]:
        L = libs[name]
        t = time.perf_counter(); ctx = L.tic_create(0); t0 = (time.perf_counter() - t) * 1e3
        assert ctx
        t1, s1 = batch(L, ctx, bset, 90)
        t2, s2 = batch(L, ctx, hd, 50)
        t = time.perf_counter(); L.tic_destroy(ctx); t3 = (time.perf_counter() - t) * 1e3
        ref = ref if ref is not None else (s1, s2)
        assert (s1, s2) == ref, name
        if r:
            for l, v in zip(lines, (t0, t1, t2, t3)):
                res[(l, name)].append(v)
print("every library returned equal bytes on every first call (%s)" % ", ".join(libs))
med = {k: statistics.median(v) for k, v in res.items()}
for l in lines:
    for name in libs:
        v = res[(l, name)]
        print("%-22s %-10s median %8.3f ms  min %8.3f  max %8.3f  (%d rounds)" % (l, name, med[(l, name)], min(v), max(v), len(v)))
parents = [nm for nm in libs if nm.startswith("parent")]
if len(parents) == 2:
    for l in lines:
        a, b = med[(l, parents[0])], med[(l, parents[1])]
        own = min(med[(l, p)] - min(res[(l, p)]) for p in parents)
        margin, base = max(abs(a - b), own), (a + b) / 2
        over = med[(l, "product")] - base
        print("%-22s product    %+8.3f ms against the parent's median %8.3f (%8.3f / %8.3f: they differ by %.3f, median above minimum %.3f)  %s" % (l, over, base, a, b, abs(a - b), own, "inside" if over <= margin else "OUTSIDE the margin"))
