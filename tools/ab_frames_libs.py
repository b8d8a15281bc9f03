"""Config 4's kernel-only leg (256 resident 1920x1080 frames, one batched launch) across builds of the library in one process, rounds interleaved.
Usage: python tools/ab_frames_libs.py other.so [more.so ...]"""
import ctypes as C, os, statistics, sys
sys.path.insert(0, '.')
import numpy as np
from tinyimgcodec_amd import _native as N
def bind(path):
    L = C.CDLL(path)
    for name in ("tic_create", "tic_dev_alloc", "tic_memcpy_h2d", "tic_dctq_dev_frames_timed", "tic_num_blocks"):
        res, a = N.SIGNATURES[name]; fn = getattr(L, name); fn.restype = res; fn.argtypes = a
    return L
libs = {"product": bind(N.LIB_PATH)}
for p in sys.argv[1:]: libs[os.path.basename(p).replace(".so", "")] = bind(p)
h, w, n = 1080, 1920, 256
blk = np.random.default_rng(1).integers(0, 256, (16, h, w), dtype=np.uint8)
st = {}
for name, L in libs.items():
    ctx = L.tic_create(0); assert ctx
    img_bytes, coef_bytes = h * w, L.tic_num_blocks(h, w) * 128
    d_in, d_out = C.c_void_p(), C.c_void_p()
    assert L.tic_dev_alloc(ctx, img_bytes * n, C.byref(d_in)) == 0 and L.tic_dev_alloc(ctx, coef_bytes * n, C.byref(d_out)) == 0
    for i in range(0, n, 16):
        assert L.tic_memcpy_h2d(ctx, C.c_void_p(d_in.value + i * img_bytes), blk.ctypes.data, img_bytes * 16) == 0
    st[name] = (L, ctx, d_in, d_out, img_bytes, coef_bytes)
ms = C.c_float(); res = {k: [] for k in libs}
for rnd in range(8):
    for name, (L, ctx, d_in, d_out, ib, cb) in st.items():
        assert L.tic_dctq_dev_frames_timed(ctx, d_in, n, h, w, w, ib, 50, d_out, cb, 2, 20, C.byref(ms)) == 0
        if rnd: res[name].append(ms.value * 1e3 / 20)
for name, r in res.items():
    print("256 x 1080p %-10s median %8.2f us  min %8.2f  max %8.2f  (%s)" % (name, statistics.median(r), min(r), max(r), " ".join("%.1f" % x for x in r)))
