"""The integer encoder's batch forms against the loops they replace, in one process on one GPU (it fails without one): a host clock around
calls that return their results - so the device has finished -, --rounds interleaved repetitions after two warm ones, the order rotated
(the way of tools/rate_batch_timing.py).  The loops run on ANOTHER build of the library too - the parent commit's, which has no batch call -
loaded side by side (tools/ab_libs.py): (b) the other build's loop, (b') this build's; their difference and (b)'s own range are the loop's
spread.
  (1) the 196-frame set - the 49 benchmark images x the four settings, image outer, setting inner (the reference's tests/cbenchmark.py) -
      as ONE tic_compress_batch_scaled_v against the loop of tic_compress_scaled;
  (2) 16 frames of 1088 x 1920 noise at med likewise;
  (3) the 49 x 4 table of lengths and round-trip errors as ONE tic_rd_points_scaled_v against the loop of tic_compress_scaled +
      tic_roundtrip_sse_scaled;
  (4) the transform alone on one mixed chunk, resident - 64 frames, four shapes x four settings x four frames -: ONE tic_dctq_scaled_v_dev
      (table upload, one launch of the descriptor form, wait) against the 16 tic_dctq_scaled_dev_frames launches of the same frames (a
      launch per run of four equal frames, then one wait).
Every side's results are checked against the others'.  No ratio is fixed in advance; the requirement, on (1), is that the one call is not
slower than the loop by more than the loop's own spread - the tool says in plain words whether that holds.  The lines go to stdout and to --out.
  python tools/scaled_batch_timing.py path/to/libparent.so [--rounds 7] [--out profiles/scaled_batch.txt]"""
import argparse, ctypes as C, os, statistics, sys, time
sys.path.insert(0, '.')
import numpy as np
import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

ap = argparse.ArgumentParser()
ap.add_argument("other")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=os.path.join("profiles", "scaled_batch.txt"))
args = ap.parse_args()
assert args.rounds >= 7
lines_out = []


def say(s):
    print(s, flush=True)
    lines_out.append(s)


say("command line: python tools/scaled_batch_timing.py <the parent commit's library> --rounds %d" % args.rounds)
L = N.load()
old = C.CDLL(args.other)
for name in ("tic_create", "tic_destroy", "tic_compress_scaled", "tic_roundtrip_sse_scaled", "tic_dctq_scaled_dev_frames", "tic_sync", "tic_dev_alloc",
             "tic_dev_free", "tic_memcpy_h2d", "tic_memcpy_d2h"):
    res, a = N.SIGNATURES[name]
    fn = getattr(old, name); fn.restype = res; fn.argtypes = a
assert not hasattr(old, "tic_compress_batch_scaled_v"), "the other library is to be the parent's: it has no batch call"
ctx = T.Context(0)  # (raises without a GPU)
octx = old.tic_create(0)
assert octx
px = np.load(os.path.join("tests", "golden", "benchmark_set.npz"))["pixels"]
bench = ([np.ascontiguousarray(px[i]) for i in range(px.shape[0]) for _ in range(4)], [q for _ in range(px.shape[0]) for q in range(4)])
noise = ([np.random.default_rng(3000 + k).integers(0, 256, (1088, 1920), dtype=np.uint8) for k in range(16)], [2] * 16)


def timed(lines, check):
    """Two warm rounds (the second one checked), then args.rounds timed ones, the order rotated -> {label: [ms]}."""
    for w in range(2):
        results = [fn() for _, fn in lines]
    check(results)
    times = {label: [] for label, _ in lines}
    for r in range(args.rounds):
        for k in range(len(lines)):
            label, fn = lines[(k + r) % len(lines)]
            t = time.perf_counter()
            fn()
            times[label].append((time.perf_counter() - t) * 1e3)
    return times


def report(lines, times, what):
    for label, _ in lines:
        t = times[label]
        say("  %-52s median %9.3f ms  min %9.3f  max %9.3f" % (label, statistics.median(t), min(t), max(t)))
    a, b, b2 = (statistics.median(times[label]) for label, _ in lines)
    rng_b = max(times[lines[1][0]]) - min(times[lines[1][0]])
    spread = max(abs(b - b2), rng_b)
    say("  the loop against itself: (b) - (b') = %+.3f ms at the median; (b)'s own range %.3f ms -> spread %.3f ms" % (b - b2, rng_b, spread))
    verdict = "FASTER than" if b - a > spread else ("SLOWER than" if a - b > spread else "NOT DISTINGUISHABLE from")
    say("  (a) against (b): %+.3f ms (%.2f x)  ->  %s is %s the parent's loop at the median (difference %s the loop's own spread)"
        % (a - b, b / a, what, verdict, "beyond" if abs(a - b) > spread else "within"))
    return a - b <= spread


def frame_args(frames):
    n = len(frames)
    return ((C.c_void_p * n)(*[f.ctypes.data for f in frames]), (C.c_int * n)(*[f.shape[0] for f in frames]), (C.c_int * n)(*[f.shape[1] for f in frames]),
            (C.c_ssize_t * n)(*[f.shape[1] for f in frames]))


def measure_compress(title, work):
    frames, qfs = work
    n = len(frames)
    caps_l = [L.tic_compress_scaled_bound(f.shape[0], f.shape[1]) for f in frames]
    bufs = [np.empty(c, np.uint8) for c in caps_l]
    inp, hs, ws, strides = frame_args(frames)
    qa = (C.c_int * n)(*qfs)
    outp = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    caps = (C.c_size_t * n)(*caps_l)
    lens = (C.c_size_t * n)()

    def result():
        return [bufs[i][: lens[i]].tobytes() for i in range(n)]

    def one_call():
        assert L.tic_compress_batch_scaled_v(ctx.handle, inp, n, hs, ws, strides, qa, outp, caps, lens) == 0
        return result()

    def loop_on(lib, handle):
        def run():
            ln = C.c_size_t()
            for i in range(n):
                assert lib.tic_compress_scaled(handle, inp[i], hs[i], ws[i], strides[i], qa[i], outp[i], caps[i], C.byref(ln)) == 0
                lens[i] = ln.value
            return result()
        return run

    lines = [("(a)  one tic_compress_batch_scaled_v", one_call), ("(b)  loop of tic_compress_scaled, the other build", loop_on(old, octx)),
             ("(b') loop of tic_compress_scaled, this build", loop_on(L, ctx.handle))]

    def check(results):
        assert results[0] == results[1] == results[2], "the sides disagree"

    times = timed(lines, check)
    one_call()
    v = [C.c_int() for _ in range(4)]
    L.tic_last_compress_batch_scaled(ctx.handle, *[C.byref(x) for x in v])
    say("%s: %d frames, %.1f MB of pixels, %.1f MB of streams" % (title, n, sum(f.size for f in frames) / 1e6, sum(lens) / 1e6))
    ok = report(lines, times, "the one call")
    say("  (a): %d batch frames, %d behind the batch, %d chunks, %d transform launches (one per chunk); (b), (b'): %d transform launches" % (*[x.value for x in v], n))
    return ok


def measure_rd():
    frames = [np.ascontiguousarray(px[i]) for i in range(px.shape[0])]
    n, nq = len(frames), 4
    inp, hs, ws, strides = frame_args(frames)
    qarr = np.arange(4, dtype=np.intc)
    cap = L.tic_compress_scaled_bound(512, 512)
    buf = np.empty(cap, np.uint8)

    def one_call():
        sizes, sse, wr = np.zeros((n, nq), np.int64), np.zeros((n, nq), np.uint64), np.zeros((n, nq), np.uint64)
        assert L.tic_rd_points_scaled_v(ctx.handle, inp, n, hs, ws, strides, qarr.ctypes.data, nq, sizes.ctypes.data, sse.ctypes.data, wr.ctypes.data) == 0
        return sizes.tolist(), sse.tolist(), wr.tolist()

    def loop_on(lib, handle):
        def run():
            sizes, sse, wr = np.zeros((n, nq), np.int64), np.zeros((n, nq), np.uint64), np.zeros((n, nq), np.uint64)
            ln, sums = C.c_size_t(), (C.c_uint64 * 2)()
            for i in range(n):
                for j in range(nq):
                    assert lib.tic_compress_scaled(handle, inp[i], 512, 512, 512, j, buf.ctypes.data, cap, C.byref(ln)) == 0
                    assert lib.tic_roundtrip_sse_scaled(handle, inp[i], 512, 512, 512, j, sums) == 0
                    sizes[i, j], sse[i, j], wr[i, j] = ln.value, sums[0], sums[1]
            return sizes.tolist(), sse.tolist(), wr.tolist()
        return run

    lines = [("(a)  one tic_rd_points_scaled_v", one_call), ("(b)  loop of compress + roundtrip_sse, the other build", loop_on(old, octx)),
             ("(b') loop of compress + roundtrip_sse, this build", loop_on(L, ctx.handle))]

    def check(results):
        assert results[0] == results[1] == results[2], "the sides disagree"

    times = timed(lines, check)
    one_call()
    v = [C.c_int() for _ in range(6)]
    L.tic_last_rd_scaled_batch(ctx.handle, *[C.byref(x) for x in v])
    say("(3) the 49 x 4 table of lengths and round-trip errors: %d probes" % (n * nq))
    report(lines, times, "the one call")
    say("  (a): %d batch frames, %d behind the batch, %d chunks, %d transform / %d size / %d measuring launches; (b), (b'): %d calls of each kind"
        % (*[x.value for x in v], n * nq))


def measure_transform():
    shapes = ((512, 512), (256, 384), (64, 96), (1088, 1920))
    runs = [(h, w, qf, np.random.default_rng(100 * k + qf).integers(0, 256, (4, h, w), dtype=np.uint8)) for k, (h, w) in enumerate(shapes) for qf in range(4)]
    nblk = sum(4 * (h // 8) * (w // 8) for h, w, _, _ in runs)

    def resident(lib, handle):
        ptrs = []
        for _, _, _, a in runs:
            p = C.c_void_p()
            assert lib.tic_dev_alloc(handle, a.nbytes, C.byref(p)) == 0 and lib.tic_memcpy_h2d(handle, p, a.ctypes.data, a.nbytes) == 0
            ptrs.append(p)
        z = C.c_void_p()
        assert lib.tic_dev_alloc(handle, nblk * 128, C.byref(z)) == 0
        return ptrs, z

    def fetch(lib, handle, z):
        out = np.empty(nblk * 64, np.int16)
        assert lib.tic_memcpy_d2h(handle, out.ctypes.data, z, out.nbytes) == 0
        return out.tobytes()

    mine, other = resident(L, ctx.handle), resident(old, octx)
    m = 4 * len(runs)
    dptr = (C.c_void_p * m)(*[mine[0][r].value + k * h * w for r, (h, w, _, _) in enumerate(runs) for k in range(4)])
    hs = (C.c_int * m)(*[h for h, _, _, _ in runs for _ in range(4)])
    ws = (C.c_int * m)(*[w for _, w, _, _ in runs for _ in range(4)])
    strides = (C.c_ssize_t * m)(*[w for _, w, _, _ in runs for _ in range(4)])
    qa = (C.c_int * m)(*[qf for _, _, qf, _ in runs for _ in range(4)])

    def one_launch():
        assert L.tic_dctq_scaled_v_dev(ctx.handle, dptr, m, hs, ws, strides, qa, mine[1]) == 0

    def launches_on(lib, handle, bufs):
        def run():
            off = 0
            for p, (h, w, qf, _) in zip(bufs[0], runs):
                assert lib.tic_dctq_scaled_dev_frames(handle, p, 4, h, w, w, h * w, qf, C.c_void_p(bufs[1].value + off), h * w * 2) == 0
                off += 4 * h * w * 2
            assert lib.tic_sync(handle) == 0
        return run

    lines = [("(a)  one tic_dctq_scaled_v_dev", one_launch), ("(b)  16 tic_dctq_scaled_dev_frames, the other build", launches_on(old, octx, other)),
             ("(b') 16 tic_dctq_scaled_dev_frames, this build", launches_on(L, ctx.handle, mine))]

    def check(_):
        one_launch()
        a = fetch(L, ctx.handle, mine[1])
        lines[2][1]()
        assert a == fetch(L, ctx.handle, mine[1]) == fetch(old, octx, other[1]), "the sides disagree"

    times = timed(lines, check)
    say("(4) the transform alone on one mixed chunk, resident: 64 frames (512x512, 256x384, 64x96, 1088x1920; four settings; four frames each), %.1f MB of pixels"
        % (nblk * 64 / 1e6))
    report(lines, times, "the one launch")
    for lib, handle, bufs in ((L, ctx.handle, mine), (old, octx, other)):
        for p in bufs[0] + [bufs[1]]:
            lib.tic_dev_free(handle, p)


say("%s rounds %d" % (ctx.arch, args.rounds))
ok = measure_compress("(1) benchmark images x four settings", bench)
measure_compress("(2) 16 frames of 1088 x 1920 noise at med", noise)
measure_rd()
measure_transform()
say("requirement, on (1): the one call is not slower than the loop by more than the loop's own spread -> %s" % ("MET" if ok else "NOT MET"))
old.tic_destroy(octx)
ctx.close()
os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines_out) + "\n")
