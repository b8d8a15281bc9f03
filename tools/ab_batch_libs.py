"""A/B of the batch entry points between builds of the library in one process, a context per library, rounds interleaved and the order rotated:
  1080p pageable     tic_compress_batch, threads = 0, 256 seeded 1080p frames (seeds 1234 + i, q = 50), pinned in place by the call
  1080p staged       the same with tic_set_auto_register(0): the staging threads' route
  set q90 / q5       tic_compress_batch on the 49 frames of tests/golden/benchmark_set.npz: one chunk, inline, zero copy
  set q90 / q5 dec   tic_decompress_batch of those streams
  1080p host coder   tic_compress_batch, threads = 4, 64 of the 1080p frames
and, with --lines rate alone (they stay out of a run without --lines), the rate / rate-distortion family:
  rate sizes_v           tic_stream_sizes_v on the 49 frames at 6 qualities (5, 20, 35, 50, 75, 90)
  rate rd_points_v       tic_rd_points_v on the same input
  rate batch_to_size     tic_compress_batch_to_size on the 49 frames x 6 budgets (4 .. 128 KiB: 294 frames, the workload of tools/rate_batch_timing.py)
  rate batch_to_psnr     tic_compress_batch_to_psnr on the 49 frames, each at the error of 35 dB
  rate to_size 1080p     tic_compress_to_size on one 1080p noise frame, range 1..99, the budget its own size at q = 50
  rate to_psnr 1080p     tic_compress_to_psnr on the same frame, range 1..99, at the error of 30 dB
  rate adaptive_sizes_v  tic_adaptive_sizes_v on the 49 frames at 3 qualities (20, 50, 90)
Of these every library's return code, sizes or streams, lengths, qualities, errors, status[] and tic_last_rate_search / tic_last_rate_batch /
tic_last_rd_batch / tic_last_adaptive_rate counters are compared, not only bytes.
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
names = ("tic_create", "tic_compress_batch", "tic_decompress_batch", "tic_compress_bound", "tic_set_auto_register", "tic_last_error",
         "tic_stream_sizes", "tic_stream_sizes_v", "tic_rd_points_v", "tic_compress_batch_to_size", "tic_compress_batch_to_psnr", "tic_compress_to_size",
         "tic_compress_to_psnr", "tic_adaptive_sizes_v", "tic_last_rate_search", "tic_last_rate_batch", "tic_last_rd_batch", "tic_last_adaptive_rate")
def bind(path):
    L = C.CDLL(path)
    for name in names:
        res, a = N.SIGNATURES[name] if name in N.SIGNATURES else N.RATE_ADAPTIVE_SIGNATURES[name]
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

SENTINEL = 0xA5
class RateJob:
    """One timed call of the rate / rate-distortion family on `frames`; result() is everything the last call left: its return code (a frame
    over its budget fails its call by design), the call's output arrays and the twelve tic_last_* counters of the family."""
    def __init__(self, call, frames, qs=(), bounds=()):
        n = self.n = len(frames)
        self.call, self.frames, self.rc, nq = call, frames, None, len(qs)
        self.inp = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
        self.hs, self.ws = (C.c_int * n)(*[f.shape[0] for f in frames]), (C.c_int * n)(*[f.shape[1] for f in frames])
        self.strides = (C.c_ssize_t * n)(*[f.strides[0] for f in frames])
        self.qs = (C.c_int * nq)(*qs)
        self.sizes, self.sse, self.wrapped = (C.c_longlong * (n * nq))(), (C.c_uint64 * max(n * nq, n))(), (C.c_uint64 * (n * nq))()
        caps = [libs["product"].tic_compress_bound(f.shape[0], f.shape[1]) for f in frames]
        self.pool = [np.zeros(c, dtype=np.uint8) for c in caps] if bounds else []
        self.outp = (C.c_void_p * n)(*[b.ctypes.data for b in self.pool])
        self.caps, self.lens = (C.c_size_t * n)(*caps), (C.c_size_t * n)()
        self.budgets, self.max_sse = (C.c_size_t * n)(*bounds), (C.c_uint64 * n)(*bounds)
        self.quals, self.status = (C.c_int * n)(), (C.c_int * n)()
    def run(self, name):
        L, ctx, k = libs[name], ctxs[name], self.call
        a = (ctx, self.inp, self.n, self.hs, self.ws, self.strides)
        one = (ctx, self.inp[0], self.hs[0], self.ws[0], self.strides[0])
        for arr in (self.sizes, self.sse, self.wrapped, self.lens, self.quals, self.status):  # (nothing another library wrote is left to compare)
            C.memset(arr, SENTINEL, C.sizeof(arr))
        t = time.perf_counter()
        if k == "sizes_v": rc = L.tic_stream_sizes_v(*a, self.qs, len(self.qs), self.sizes)
        elif k == "rd_points_v": rc = L.tic_rd_points_v(*a, self.qs, len(self.qs), self.sizes, self.sse, self.wrapped)
        elif k == "adaptive_sizes_v": rc = L.tic_adaptive_sizes_v(*a, self.qs, len(self.qs), self.sizes)
        elif k == "batch_to_size": rc = L.tic_compress_batch_to_size(*a, self.budgets, 1, 99, self.outp, self.caps, self.lens, self.quals, self.status)
        elif k == "batch_to_psnr": rc = L.tic_compress_batch_to_psnr(*a, self.max_sse, 1, 99, self.outp, self.caps, self.lens, self.quals, self.sse, self.status)
        elif k == "to_size": rc = L.tic_compress_to_size(*one, self.budgets[0], 1, 99, self.outp[0], self.caps[0], self.lens, self.quals)
        else: rc = L.tic_compress_to_psnr(*one, self.max_sse[0], 1, 99, self.outp[0], self.caps[0], self.lens, self.quals, self.sse)
        t = (time.perf_counter() - t) * 1e3
        self.rc, self.lib = rc, name
        return t
    def result(self):
        L, ctx = libs[self.lib], ctxs[self.lib]
        v = [C.c_int(-1) for _ in range(12)]
        r = [C.byref(x) for x in v]
        assert L.tic_last_rate_search(ctx, *r[0:2]) == 0 and L.tic_last_rate_batch(ctx, *r[2:8]) == 0 and L.tic_last_rd_batch(ctx, r[8]) == 0
        assert L.tic_last_adaptive_rate(ctx, *r[9:12]) == 0
        ok = [self.rc == 0 if self.call.startswith("to_") else self.status[i] == 0 for i in range(self.n)]  # (a single call has no status[])
        streams = [self.pool[i][: self.lens[i]].tobytes() if ok[i] else None for i in range(len(self.pool))]
        return (self.rc, list(self.sizes), list(self.sse), list(self.wrapped), streams, list(self.lens), list(self.quals), list(self.status), [x.value for x in v])

wanted = lambda line: any(word in line for word in args.lines.split(",")) if args.lines else not line.startswith("rate ")
hd = [np.random.default_rng(1234 + i).integers(0, 256, (1080, 1920), dtype=np.uint8) for i in range(256 if any(map(wanted, ("1080p pageable", "1080p staged", "1080p host coder"))) else 64)]
px = np.load(os.path.join("tests", "golden", "benchmark_set.npz"))["pixels"]
bset = [np.ascontiguousarray(px[i]) for i in range(px.shape[0])]
jobs = {"1080p pageable": Job(hd, 50), "1080p staged": Job(hd, 50, auto_register=0), "set q90": Job(bset, 90), "set q5": Job(bset, 5),
        "1080p host coder": Job(hd[:64], 50, threads=4)}
for q in (90, 5):  # the decoder's input: the product's streams (every library's are compared with them below)
    jobs["set q%d" % q].run("product")
    jobs["set q%d dec" % q] = DecJob(jobs["set q%d" % q].result(), 512, 512)
if any(wanted("rate " + k) for k in ("sizes_v", "rd_points_v", "batch_to_size", "batch_to_psnr", "to_size 1080p", "to_psnr 1080p", "adaptive_sizes_v")):
    KIB, one = (4, 8, 16, 32, 64, 128), hd[:1]
    q50, sz = (C.c_int * 1)(50), (C.c_longlong * 1)()
    assert libs["product"].tic_stream_sizes(ctxs["product"], one[0].ctypes.data, 1080, 1920, 1920, q50, 1, sz) == 0 and sz[0] > 16
    db = lambda f, psnr: int(255 ** 2 * f.size / 10 ** (psnr / 10))  # the largest squared error at that PSNR
    jobs.update({"rate sizes_v": RateJob("sizes_v", bset, (5, 20, 35, 50, 75, 90)), "rate rd_points_v": RateJob("rd_points_v", bset, (5, 20, 35, 50, 75, 90)),
                 "rate batch_to_size": RateJob("batch_to_size", [f for f in bset for _ in KIB], bounds=[k << 10 for _ in bset for k in KIB]),
                 "rate batch_to_psnr": RateJob("batch_to_psnr", bset, bounds=[db(f, 35) for f in bset]),
                 "rate to_size 1080p": RateJob("to_size", one, bounds=[sz[0]]), "rate to_psnr 1080p": RateJob("to_psnr", one, bounds=[db(one[0], 30)]),
                 "rate adaptive_sizes_v": RateJob("adaptive_sizes_v", bset, (20, 50, 90))})
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
print("every library returned equal bytes%s on every line (%s)" % (" and side values" if any(isinstance(j, RateJob) for j in jobs.values()) else "", ", ".join(libs)))
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
