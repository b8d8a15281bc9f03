"""decompress_adaptive of this build against another build of the library (the parent commit's: host bit-serial decoder) in one process,
calls interleaved, median of --calls after 3 warm calls.  Rows: 4096^2 noise at q = 5 / 50 / 90, the 1080p fixture frame, benchmark
image 1 (512^2) at q = 5 / 50 / 90 and crops of it (the crossover below 16,384 blocks: those rows run on the hooks build with the
device decoder's lower bounds moved out of the way).  Per row: tic_decompress_adaptive host to host on both builds,
tic_decompress_adaptive_dev resident (this build only: the other has no such entry), and decompress() of the default-table stream of
the same frame and quality for orientation.  (The script loads the hooks build itself.)
Usage: python tools/ab_adaptive_dec.py path/to/libother.so [--calls 30]"""
import argparse, ctypes as C, os, statistics, sys, time
sys.path.insert(0, '.')
os.environ["TIC_TEST_HOOKS"] = "1"
import numpy as np
import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

ap = argparse.ArgumentParser()
ap.add_argument("other")
ap.add_argument("--calls", type=int, default=30)
args = ap.parse_args()


def bind(path, names):
    L = C.CDLL(path)
    for name in names:
        res, a = N.SIGNATURES[name]
        fn = getattr(L, name); fn.restype = res; fn.argtypes = a
    return L


base = ("tic_create", "tic_destroy", "tic_decompress_adaptive", "tic_last_decode_path", "tic_last_error")
new = N.load()  # the hooks build: TIC_DECODE_MIN_* below
assert new.tic_build_has_test_hooks() == 1
old = bind(args.other, base)
ctx = T.Context(0)
octx = old.tic_create(0)
assert octx


def row(name, img, q, calls, force_device=False):
    h, w = img.shape
    s = T.compress_adaptive(img, q, ctx=ctx)
    d = T.compress(img, q, ctx=ctx)
    buf = np.frombuffer(s, np.uint8)
    out_new, out_old = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    for k in ("TIC_DECODE_MIN_BLOCKS", "TIC_DECODE_MIN_BITS"):
        os.environ.pop(k, None)
    if force_device:
        os.environ["TIC_DECODE_MIN_BLOCKS"], os.environ["TIC_DECODE_MIN_BITS"] = "1", "0"
    d_s, d_o = C.c_void_p(), C.c_void_p()
    ctx.check(new.tic_dev_alloc(ctx.handle, len(s), C.byref(d_s))); ctx.check(new.tic_dev_alloc(ctx.handle, h * w, C.byref(d_o)))
    ctx.check(new.tic_memcpy_h2d(ctx.handle, d_s, buf.ctypes.data, buf.size))
    f_new = lambda: ctx.check(new.tic_decompress_adaptive(ctx.handle, buf.ctypes.data, buf.size, out_new.ctypes.data, out_new.size))
    f_old = lambda: old.tic_decompress_adaptive(octx, buf.ctypes.data, buf.size, out_old.ctypes.data, out_old.size)
    f_dev = lambda: ctx.check(new.tic_decompress_adaptive_dev(ctx.handle, d_s, len(s), d_o, w, h * w, None, None))
    f_def = lambda: T.decompress(d, ctx=ctx)
    f_new(); path = new.tic_last_decode_path(ctx.handle)
    assert f_old() == 0 and np.array_equal(out_new, out_old)
    f_dev(); back = np.zeros((h, w), np.uint8); ctx.check(new.tic_memcpy_d2h(ctx.handle, back.ctypes.data, d_o, back.size))
    assert np.array_equal(back, out_new)
    t = {"new": [], "old": [], "dev": [], "def": []}
    for f, k in ((f_new, "new"), (f_old, "old"), (f_dev, "dev"), (f_def, "def")):
        for _ in range(3):
            f()
    for _ in range(calls):  # interleaved
        for f, k in ((f_new, "new"), (f_old, "old"), (f_dev, "dev"), (f_def, "def")):
            t0 = time.perf_counter(); f(); t[k].append((time.perf_counter() - t0) * 1e6)
    m = {k: statistics.median(v) for k, v in t.items()}
    nb = ((h + 7) // 8) * ((w + 7) // 8)
    print("%-22s %7d blocks %9d bytes  path %d | host to host: this %10.1f us  other %10.1f us  ratio %6.1f | resident %9.1f us | decompress() default table %8.1f us"
          % (name, nb, len(s), path, m["new"], m["old"], m["old"] / m["new"], m["dev"], m["def"]), flush=True)
    ctx.check(new.tic_dev_free(ctx.handle, d_s)); ctx.check(new.tic_dev_free(ctx.handle, d_o))


golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
bench1 = np.load(os.path.join(golden, "benchmark_set.npz"))["pixels"][0]
for q in (5, 50, 90):
    row("noise 4096^2 q=%d" % q, np.random.default_rng(42).integers(0, 256, (4096, 4096), dtype=np.uint8), q, args.calls)
row("frame_1080p q=50", np.random.default_rng(1234).integers(0, 256, (1080, 1920), dtype=np.uint8), 50, args.calls)
for q in (5, 50, 90):
    row("benchmark 1 512^2 q=%d" % q, bench1, q, args.calls, force_device=True)
for side in (256, 128, 64):
    for q in (5, 50, 90):
        row("benchmark 1 %d^2 q=%d" % (side, q), np.ascontiguousarray(bench1[:side, :side]), q, args.calls, force_device=True)
old.tic_destroy(octx)
ctx.close()
