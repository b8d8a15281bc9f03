"""Rate-distortion for a whole list of frames, in one process on one GPU (it fails without one), against ANOTHER build of the library - the
parent commit's, which has no batch call - loaded side by side (the way of tools/ab_libs.py and tools/rate_batch_timing.py): a host clock
around calls that return their results - so the device has finished -, --rounds interleaved repetitions after two warm ones, the order rotated.
  1, 2. A PSNR bound per frame:
       (a) one call     ONE tic_compress_batch_to_psnr over the list (this build);
       (b) loop         tic_compress_to_psnr per frame on the other build;
       (b') the loop    on this build (the single call is untouched by the batch: the two loops should agree; their difference is the
                        loop's own spread).
     Workloads: (1) the 294-frame benchmark workload - the 49 benchmark images, each against its own round-trip error at the reference's six
     benchmark qualities (90, 80, 50, 20, 10, 5; the errors are taken from one tic_rd_points_v beforehand: the fixture records sizes, no
     PSNR) - and (2) 16 frames of 1080p noise, each against its own error at q = 50.  Every side's streams, qualities and errors are checked
     against the others'.
  3. The table: ONE tic_rd_points_v on 49 images x 6 qualities against 49 tic_rd_points on the other build, and on this one.
  4. One 4096^2 probe, kernels alone on resident coefficients (device events around --iters launches): tic_distortion_v_dev_timed
     (idct_sse_kernel_v, at most 1,024 atomics per sum) against tic_distortion_dev_timed (idct_sse_kernel, 8,192) and tic_idct_dev_timed
     (idct_kernel, which stores its pixels), all on this build, and the two single-frame timings on the other build.
Pass conditions, said in plain words by the tool: the one call (1 and 2) is not slower at the median than the other build's loop
by more than that loop's own spread; the new kernel on the 4096^2 probe is not slower than idct_sse_kernel beyond its spread.
  python tools/rd_batch_timing.py path/to/libparent.so [--rounds 7] [--iters 200]"""
import argparse, ctypes as C, os, statistics, sys, time
sys.path.insert(0, '.')
import numpy as np
import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

ap = argparse.ArgumentParser()
ap.add_argument("other")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=200)
args = ap.parse_args()
assert args.rounds >= 7
print("command line: python tools/rd_batch_timing.py %s --rounds %d --iters %d" % (args.other, args.rounds, args.iters))
L = N.load()
old = C.CDLL(args.other)
for name in ("tic_create", "tic_destroy", "tic_compress_to_psnr", "tic_rd_points", "tic_last_rate_search", "tic_compress_bound", "tic_dev_alloc", "tic_dev_free",
             "tic_memcpy_h2d", "tic_sync", "tic_dctq_dev", "tic_distortion_dev", "tic_distortion_dev_timed", "tic_idct_dev_timed"):
    res, a = N.SIGNATURES[name]
    fn = getattr(old, name); fn.restype = res; fn.argtypes = a
assert not hasattr(old, "tic_compress_batch_to_psnr"), "the other library is to be the parent's: it has no batch call"
ctx = T.Context(0)  # (raises without a GPU)
octx = old.tic_create(0)
assert octx
px = np.load(os.path.join("tests", "golden", "benchmark_set.npz"))["pixels"]
QS = (90, 80, 50, 20, 10, 5)
images = [np.ascontiguousarray(px[i]) for i in range(px.shape[0])]
table = T.rd_points_batch(images, QS, ctx=ctx)
bench = ([im for im in images for _ in QS], [int(v) for v in table[1].reshape(-1)])
noise_frames = [np.random.default_rng(3000 + k).integers(0, 256, (1080, 1920), dtype=np.uint8) for k in range(16)]
noise = (noise_frames, [int(v) for v in T.rd_points_batch(noise_frames, [50], ctx=ctx)[1][:, 0]])
verdicts = []


def frame_args(frames):
    n = len(frames)
    return ((C.c_void_p * n)(*[f.ctypes.data for f in frames]), (C.c_int * n)(*[f.shape[0] for f in frames]), (C.c_int * n)(*[f.shape[1] for f in frames]),
            (C.c_ssize_t * n)(*[f.shape[1] for f in frames]))


def timed_rounds(lines, check):
    """Two warm rounds with `check` on every side's result, then the interleaved rounds -> {label: [ms, ...]}."""
    for _ in range(2):
        results = [fn() for _, fn in lines]
        assert all(check(r, results[0]) for r in results[1:]), "the sides disagree"
    times = {label: [] for label, _ in lines}
    for r in range(args.rounds):
        for k in range(len(lines)):
            label, fn = lines[(k + r) % len(lines)]
            t = time.perf_counter()
            fn()
            times[label].append((time.perf_counter() - t) * 1e3)
    for label, _ in lines:
        t = times[label]
        print("  %-40s median %9.3f ms  min %9.3f  max %9.3f" % (label, statistics.median(t), min(t), max(t)))
    return times


def against_the_loop(what, times, lines):
    a, b, b2 = (statistics.median(times[label]) for label, _ in lines)
    own = max(times[lines[1][0]]) - min(times[lines[1][0]])
    spread = max(abs(b - b2), own)
    print("  the loop against itself: (b) - (b') = %+.3f ms at the median; (b)'s own range %.3f ms -> spread %.3f ms" % (b - b2, own, spread))
    verdict = "FASTER than" if b - a > spread else ("SLOWER than" if a - b > spread else "NOT DISTINGUISHABLE from")
    print("  (a) against (b): %+.3f ms (%.2f x)  ->  the one call is %s the other build's loop at the median (difference %s the loop's own spread)"
          % (a - b, b / a, verdict, "beyond" if abs(a - b) > spread else "within"))
    verdicts.append((what, not a - b > spread))


def search(title, work):
    frames, bounds = work
    n = len(frames)
    caps_l = [L.tic_compress_bound(f.shape[0], f.shape[1]) for f in frames]
    bufs = [np.empty(c, np.uint8) for c in caps_l]
    inp, hs, ws, strides = frame_args(frames)
    outp = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    caps = (C.c_size_t * n)(*caps_l)
    bnd = (C.c_uint64 * n)(*bounds)
    lens, quals, sse, status = (C.c_size_t * n)(), (C.c_int * n)(), (C.c_uint64 * n)(), (C.c_int * n)()
    counts = {}

    def result():
        return [(bufs[i][: lens[i]].tobytes(), quals[i], sse[i]) if status[i] == 0 else (None, status[i], lens[i], quals[i], sse[i]) for i in range(n)]

    def one_call():
        L.tic_compress_batch_to_psnr(ctx.handle, inp, n, hs, ws, strides, bnd, 1, 97, outp, caps, lens, quals, sse, status)
        return result()

    def loop_on(lib, handle):
        def run():
            ln, q, s = C.c_size_t(), C.c_int(), C.c_uint64()
            probes = waits = 0
            p, w = C.c_int(), C.c_int()
            for i in range(n):
                status[i] = lib.tic_compress_to_psnr(handle, inp[i], hs[i], ws[i], strides[i], bnd[i], 1, 97, outp[i], caps[i], C.byref(ln), C.byref(q), C.byref(s))
                lens[i], quals[i], sse[i] = ln.value, q.value, s.value
                lib.tic_last_rate_search(handle, C.byref(p), C.byref(w))
                probes, waits = probes + p.value, waits + w.value
            counts[run] = (probes, waits)
            return result()
        return run

    parent_loop, this_loop = loop_on(old, octx), loop_on(L, ctx.handle)
    lines = [("(a)  one tic_compress_batch_to_psnr", one_call), ("(b)  loop, the other build", parent_loop), ("(b') loop, this build", this_loop)]
    print("%s: %d frames, %.1f MB of pixels, qualities 1..97" % (title, n, sum(f.size for f in frames) / 1e6))
    times = timed_rounds(lines, lambda r, first: r == first)
    ok = sum(r[0] is not None for r in one_call())
    v = [C.c_int() for _ in range(6)]
    L.tic_last_rate_batch(ctx.handle, *[C.byref(x) for x in v])
    bf, sf, ch, pr, wa, la = [x.value for x in v]
    ml = C.c_int()
    L.tic_last_rd_batch(ctx.handle, C.byref(ml))
    print("  %d frames met their bound" % ok)
    print("  (a): %d batch frames, %d behind the batch, %d chunks, %d probes, %d search waits (+ the mixed batch's), %d size launches and %d measuring launches (one each per <= 64 probes)"
          % (bf, sf, ch, pr, wa, la, ml.value))
    for label, fn in (("(b) ", parent_loop), ("(b')", this_loop)):
        print("  %s: %d probes, %d host waits, as many size and measuring launches as probes" % (label, counts[fn][0], counts[fn][1]))
    against_the_loop(title, times, lines)


def rd_table():
    n, nq = len(images), len(QS)
    inp, hs, ws, strides = frame_args(images)
    qarr = (C.c_int * nq)(*QS)
    sizes, sse, wrapped = np.zeros((n, nq), np.int64), np.zeros((n, nq), np.uint64), np.zeros((n, nq), np.uint64)

    def result():
        return sizes.tolist(), sse.tolist(), wrapped.tolist()

    def one_call():
        assert L.tic_rd_points_v(ctx.handle, inp, n, hs, ws, strides, qarr, nq, sizes.ctypes.data, sse.ctypes.data, wrapped.ctypes.data) == 0
        return result()

    def loop_on(lib, handle):
        def run():
            for i in range(n):
                assert lib.tic_rd_points(handle, inp[i], hs[i], ws[i], strides[i], qarr, nq, sizes[i].ctypes.data, sse[i].ctypes.data, wrapped[i].ctypes.data) == 0
            return result()
        return run

    lines = [("(a)  one tic_rd_points_v", one_call), ("(b)  49 tic_rd_points, the other build", loop_on(old, octx)), ("(b') 49 tic_rd_points, this build", loop_on(L, ctx.handle))]
    print("(3) the benchmark table: 49 images x 6 qualities, sizes and both error sums")
    times = timed_rounds(lines, lambda r, first: r == first)
    against_the_loop("rd_points table", times, lines)


def kernels_alone():
    h = w = 4096
    img = np.random.default_rng(1234).integers(0, 256, (h, w), dtype=np.uint8)
    state = {}
    for name, lib, handle in (("this build", L, ctx.handle), ("the other build", old, octx)):
        d_img, d_zz, d_px = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert lib.tic_dev_alloc(handle, img.size, C.byref(d_img)) == 0 and lib.tic_dev_alloc(handle, img.size * 2, C.byref(d_zz)) == 0
        assert lib.tic_dev_alloc(handle, img.size, C.byref(d_px)) == 0
        assert lib.tic_memcpy_h2d(handle, d_img, img.ctypes.data, img.size) == 0
        assert lib.tic_dctq_dev(handle, d_img, h, w, w, 50, d_zz, 0) == 0 and lib.tic_sync(handle) == 0
        state[name] = (lib, handle, d_img, d_zz, d_px)
    ms = C.c_float()
    one_img, one_h, one_w, one_s, one_q = (C.c_void_p * 1)(state["this build"][2].value), (C.c_int * 1)(h), (C.c_int * 1)(w), (C.c_ssize_t * 1)(w), (C.c_int * 1)(50)

    def sse_v():
        lib, handle, d_img, d_zz, d_px = state["this build"]
        assert lib.tic_distortion_v_dev_timed(handle, d_zz, one_img, 1, one_h, one_w, one_s, one_q, 2, args.iters, C.byref(ms)) == 0
        return ms.value * 1e3 / args.iters

    def sse_on(name):
        def run():
            lib, handle, d_img, d_zz, d_px = state[name]
            assert lib.tic_distortion_dev_timed(handle, d_zz, d_img, h, w, w, 50, -1, 2, args.iters, C.byref(ms)) == 0
            return ms.value * 1e3 / args.iters
        return run

    def idct_on(name):
        def run():
            lib, handle, d_img, d_zz, d_px = state[name]
            assert lib.tic_idct_dev_timed(handle, d_zz, d_px, h, w, w, 50, -1, 2, args.iters, C.byref(ms)) == 0
            return ms.value * 1e3 / args.iters
        return run

    # the same sums from the three measuring paths
    a, b, c = (C.c_uint64 * 2)(), (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
    lib, handle, d_img, d_zz, d_px = state["this build"]
    assert lib.tic_distortion_v_dev(handle, d_zz, one_img, 1, one_h, one_w, one_s, one_q, a) == 0 and lib.tic_distortion_dev(handle, d_zz, d_img, h, w, w, 50, -1, b) == 0
    lib, handle, d_img, d_zz, d_px = state["the other build"]
    assert lib.tic_distortion_dev(handle, d_zz, d_img, h, w, w, 50, -1, c) == 0
    assert list(a) == list(b) == list(c) and a[0] > 0, "the kernels disagree"
    lines = [("idct_sse_kernel_v (descriptor form), this build", sse_v), ("idct_sse_kernel, this build", sse_on("this build")), ("idct_sse_kernel, the other build", sse_on("the other build")),
             ("idct_kernel, this build", idct_on("this build")), ("idct_kernel, the other build", idct_on("the other build"))]
    print("(4) one 4096^2 probe at q = 50, kernels alone on resident coefficients, %d launches per sample; sums %d / %d from all three" % (args.iters, a[0], a[1]))
    for _, fn in lines:
        fn()
    res = {label: [] for label, _ in lines}
    for r in range(args.rounds):
        for k in range(len(lines)):
            label, fn = lines[(k + r) % len(lines)]
            res[label].append(fn())
    for label, _ in lines:
        v = res[label]
        print("  %-48s median %8.2f us  min %8.2f  max %8.2f" % (label, statistics.median(v), min(v), max(v)))
    new, cur, par = (statistics.median(res[lines[k][0]]) for k in range(3))
    own = max(res[lines[1][0]]) - min(res[lines[1][0]])
    spread = max(abs(cur - par), own)
    verdict = "FASTER than" if cur - new > spread else ("SLOWER than" if new - cur > spread else "NOT DISTINGUISHABLE from")
    print("  idct_sse_kernel against itself: this build - the other build = %+.2f us at the median; its own range %.2f us -> spread %.2f us" % (cur - par, own, spread))
    print("  the descriptor form against idct_sse_kernel: %+.2f us (%.2f x)  ->  %s it (difference %s the spread)"
          % (new - cur, cur / new, verdict, "beyond" if abs(new - cur) > spread else "within"))
    verdicts.append(("the new kernel on one 4096^2 probe", not new - cur > spread))


print(ctx.arch, "rounds", args.rounds)
search("(1) benchmark images x six bounds", bench)
search("(2) 16 frames of 1080p noise, bound = own error at q = 50", noise)
rd_table()
kernels_alone()
for what, ok in verdicts:
    print("pass condition - %s: %s" % (what, "MET" if ok else "NOT MET"))
old.tic_destroy(octx)
ctx.close()
