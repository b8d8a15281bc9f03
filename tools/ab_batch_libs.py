"""A/B of the batch entry points between builds of the library in one process, a context per library, rounds interleaved and the order rotated:
  1080p pageable     tic_compress_batch, threads = 0, 256 seeded 1080p frames (seeds 1234 + i, q = 50), pinned in place by the call
  1080p staged       the same with tic_set_auto_register(0): the staging threads' route
  set q90 / q5       tic_compress_batch on the 49 frames of tests/golden/benchmark_set.npz: one chunk, inline, zero copy
  set q90 / q5 dec   tic_decompress_batch of those streams
  1080p host coder   tic_compress_batch, threads = 4, 64 of the 1080p frames
Every library's bytes are compared with the first library's once, after the warm-up calls.  Then median, minimum and maximum per line and
library, and for every library that is not a parent build the verdict: its median may lie above the parent's (the mean of the two parent
builds' medians) by no more than identical code varies on that line - the larger of what the two parent builds (the same file twice) differ
by and of how far a parent build's own median lies above its own minimum (the smaller of the two builds' figures).
Usage: python tools/ab_batch_libs.py tools/bin/libparent_a.so tools/bin/libparent_b.so [--rounds 15] [--lines dec]   (--lines: only lines whose name holds one of the comma-separated words)"""
import argparse, ctypes as C, os, statistics, sys, time
sys.path.insert(0, '.')
import numpy as np
from tinyimgcodec_amd import _native as N
ap = argparse.ArgumentParser()
ap.add_argument("other", nargs="*")
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--lines", default="")
args = ap.parse_args()
assert args.rounds >= 7
names = ("tic_create", "tic_compress_batch", "tic_decompress_batch", "tic_compress_bound", "tic_set_auto_register", "tic_last_error")
def bind(path):
    L = C.CDLL(path)
    for name in names:
        res, a = N.SIGNATURES[name]
        fn = getattr(L, name); fn.restype = res; fn.argtypes = a
    return L
libs = {"product": bind(N.LIB_PATH)}
for pth in args.other:
    libs[os.path.basename(pth).replace("lib", "").replace(".so", "")] = bind(pth)
ctxs = {name: L.tic_create(0) for name, L in libs.items()}
assert all(ctxs.values())

class Job:
    """One timed call on buffers of its own; run(name) gives milliseconds, result() the bytes the last call left."""
    def __init__(self, frames, q, threads=0, auto_register=1):
        self.n, (self.h, self.w), self.q, self.threads, self.auto = len(frames), frames[0].shape, q, threads, auto_register
        self.frames = frames
        n, cap = self.n, libs["product"].tic_compress_bound(self.h, self.w)
        self.pool = np.zeros((n, cap), dtype=np.uint8)
        self.inp = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
        self.outp = (C.c_void_p * n)(*[self.pool[i].ctypes.data for i in range(n)])
        self.caps = (C.c_size_t * n)(*([cap] * n)); self.lens = (C.c_size_t * n)()
    def run(self, name):
        L, ctx = libs[name], ctxs[name]
        assert L.tic_set_auto_register(ctx, self.auto) == 0
        t = time.perf_counter()
        rc = L.tic_compress_batch(ctx, self.inp, self.n, self.h, self.w, self.w, self.q, self.outp, self.caps, self.lens, self.threads)
        t = (time.perf_counter() - t) * 1e3
        assert rc == 0, L.tic_last_error(ctx)
        assert L.tic_set_auto_register(ctx, 1) == 0
        return t
    def result(self):
        return [self.pool[i, : self.lens[i]].tobytes() for i in range(self.n)]

class DecJob:
    def __init__(self, streams, h, w):
        n = self.n = len(streams)
        self.keep = [np.frombuffer(s, dtype=np.uint8).copy() for s in streams]
        self.sp = (C.c_void_p * n)(*[s.ctypes.data for s in self.keep])
        self.sl = (C.c_size_t * n)(*[s.size for s in self.keep])
        self.pix = np.zeros((n, h, w), dtype=np.uint8)
        self.outp = (C.c_void_p * n)(*[self.pix[i].ctypes.data for i in range(n)])
        self.caps = (C.c_size_t * n)(*([h * w] * n))
    def run(self, name):
        L, ctx = libs[name], ctxs[name]
        t = time.perf_counter()
        rc = L.tic_decompress_batch(ctx, self.sp, self.sl, self.n, self.outp, self.caps, None, None)
        t = (time.perf_counter() - t) * 1e3
        assert rc == 0, L.tic_last_error(ctx)
        return t
    def result(self):
        return [self.pix.tobytes()]

wanted = lambda line: not args.lines or any(word in line for word in args.lines.split(","))
hd = [np.random.default_rng(1234 + i).integers(0, 256, (1080, 1920), dtype=np.uint8) for i in range(256 if any(map(wanted, ("1080p pageable", "1080p staged", "1080p host coder"))) else 64)]
px = np.load(os.path.join("tests", "golden", "benchmark_set.npz"))["pixels"]
bset = [np.ascontiguousarray(px[i]) for i in range(px.shape[0])]
jobs = {"1080p pageable": Job(hd, 50), "1080p staged": Job(hd, 50, auto_register=0), "set q90": Job(bset, 90), "set q5": Job(bset, 5),
        "1080p host coder": Job(hd[:64], 50, threads=4)}
for q in (90, 5):  # the decoder's input: the product's streams (every library's are compared with them below)
    jobs["set q%d" % q].run("product")
    jobs["set q%d dec" % q] = DecJob(jobs["set q%d" % q].result(), 512, 512)
jobs = {line: job for line, job in jobs.items() if wanted(line)}
# A line at a time: the batch slots belong to a context and are allocated anew when the frame size changes (tens of ms of pinned allocations),
# so every library first runs the line twice, untimed - its bytes are compared then - and the timed rounds follow on warm slots.  The
# libraries take turns at going first: the first call behind another library's is the slowest of a round, whichever library makes it.
res = {(line, name): [] for line in jobs for name in libs}
order = list(libs)
for line, job in jobs.items():
    ref = None
    for name in libs:
        job.run(name); job.run(name)
        got = job.result()
        ref = ref if ref is not None else got
        assert got == ref, (line, name)
    for r in range(args.rounds):
        for name in order[r % len(order):] + order[:r % len(order)]:
            res[(line, name)].append(job.run(name))
print("every library returned equal bytes on every line (%s)" % ", ".join(libs))
med = {k: statistics.median(v) for k, v in res.items()}
for line in jobs:
    for name in libs:
        v = res[(line, name)]
        print("%-18s %-10s median %7.3f ms  min %7.3f  max %7.3f  (%d rounds)" % (line, name, med[(line, name)], min(v), max(v), len(v)))
parents = [nm for nm in libs if nm.startswith("parent")]
if len(parents) == 2:
    bad = 0
    for line in jobs:
        a, b = med[(line, parents[0])], med[(line, parents[1])]
        own = min(med[(line, p)] - min(res[(line, p)]) for p in parents)
        margin, base = max(abs(a - b), own), (a + b) / 2
        for name in libs:
            if name in parents:
                continue
            over = med[(line, name)] - base
            ok = over <= margin
            bad += not ok
            print("%-18s %-10s %+7.3f ms against the parent's median %7.3f (%7.3f / %7.3f: they differ by %.3f, median above minimum %.3f)  %s" % (line, name, over, base, a, b, abs(a - b), own, "inside" if ok else "OUTSIDE the margin"))
    print("lines outside their margin: %d" % bad)
