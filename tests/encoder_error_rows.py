"""The argument-error table of the encoder entry points: one named row per argument check, each a call through the C-ABI that must
fail.  tests/golden/gen/make_goldens_encoder_errors.py records (return code, tic_last_error text) of every row into
tests/golden/encoder_errors.json; tests/test_encoder_entry_gpu.py replays the rows and compares both fields."""
import ctypes as C

import numpy as np

from tinyimgcodec_amd import _native as N

ASYNC_SLOTS = 64  # kAsyncSlots of tic_api.hip
MARKER = "negative image size -7x-7"  # what tic_last_error holds when a row begins (a row that sets no text of its own keeps it)


class Env:
    """Buffers the rows share: a random 64 x 64 frame twice over (two frames for the multi-frame entries), on the host and the device."""

    def __init__(self, L, handle):
        self.L, self.h = L, handle
        self.img = np.random.default_rng(1234).integers(0, 256, (2, 64, 64), dtype=np.uint8)
        self.cap = L.tic_compress_bound(64, 64) + 64
        self.out = np.zeros(self.cap, np.uint8)
        self.zz = np.zeros((128, 64), np.int16)
        self.ptrs = []
        self.d_img = self.alloc(self.img.nbytes)
        assert L.tic_memcpy_h2d(handle, self.d_img, self.img.ctypes.data, self.img.nbytes) == 0
        self.d_zz = self.alloc(self.zz.nbytes + 16)  # the first frame's coefficients at quality 50: what tic_entropy_encode_dev's rows pack
        assert L.tic_dctq_dev(handle, self.d_img, 64, 64, 64, 50, self.d_zz, N.KERNEL_AUTO) == 0 and L.tic_sync(handle) == 0
        self.d_out = self.alloc(self.cap)
        self.n, self.q, self.ms, self.tk = C.c_size_t(0), C.c_int(0), C.c_float(0), C.c_longlong(0)
        self.per = (C.c_float * 8)()
        self.quals = np.array([50], np.int32)
        self.sizes = np.zeros(1, np.int64)

    def alloc(self, nbytes):
        p = C.c_void_p()
        assert self.L.tic_dev_alloc(self.h, nbytes, C.byref(p)) == 0
        self.ptrs.append(p)
        return p

    def close(self):
        for p in self.ptrs:
            self.L.tic_dev_free(self.h, p)
        self.ptrs = []


DEFAULTS = dict(h=64, w=64, stride=64, q=50, qf=2, cap=None, img=True, out=True, lenp=True, shift=0, nframes=2, fstride=4096, cstride=8192,
                variant=N.KERNEL_HYBRID, warm=0, iters=1, per=False, qmin=40, qmax=60, budget=10 ** 9, wait=1)


def _call(E, entry, kw):
    a = dict(DEFAULTS, **kw)
    L, c = E.L, E.h
    cap = E.cap if a["cap"] is None else a["cap"]
    himg = E.img.ctypes.data if a["img"] else None
    dimg = E.d_img if a["img"] else None
    hout = E.out.ctypes.data if a["out"] else None
    hzz = E.zz.ctypes.data if a["out"] else None
    dout = C.c_void_p(E.d_out.value + a["shift"]) if a["out"] else None
    dzz = E.d_zz if a["out"] else None
    n = C.byref(E.n) if a["lenp"] else None
    ms = C.byref(E.ms) if a["lenp"] else None
    per = E.per if a["per"] else None
    h, w, s, q, qf = a["h"], a["w"], a["stride"], a["q"], a["qf"]
    if entry == "tic_dctq":
        return L.tic_dctq(c, himg, h, w, s, q, hzz)
    if entry == "tic_compress":
        return L.tic_compress(c, himg, h, w, s, q, hout, cap, n)
    if entry == "tic_dctq_scaled":
        return L.tic_dctq_scaled(c, himg, h, w, s, qf, hzz)
    if entry == "tic_compress_scaled":
        return L.tic_compress_scaled(c, himg, h, w, s, qf, hout, cap, n)
    if entry == "tic_compress_adaptive":
        return L.tic_compress_adaptive(c, himg, h, w, s, q, hout, cap, n)
    if entry == "tic_stream_sizes":
        E.quals[0] = q
        return L.tic_stream_sizes(c, himg, h, w, s, E.quals.ctypes.data, 1, E.sizes.ctypes.data if a["out"] else None)
    if entry == "tic_compress_to_size":
        return L.tic_compress_to_size(c, himg, h, w, s, a["budget"], a["qmin"], a["qmax"], hout, cap, n, C.byref(E.q))
    if entry == "tic_compress_to_size_dev":
        return L.tic_compress_to_size_dev(c, dimg, h, w, s, a["budget"], a["qmin"], a["qmax"], dout, cap, n, C.byref(E.q))
    if entry == "tic_compress_dev":
        return L.tic_compress_dev(c, dimg, h, w, s, q, dout, cap, n)
    if entry == "tic_entropy_encode_dev":
        return L.tic_entropy_encode_dev(c, E.d_zz if a["img"] else None, h, w, q, dout, cap, n)
    if entry == "tic_compress_scaled_dev":
        return L.tic_compress_scaled_dev(c, dimg, h, w, s, qf, dout, cap, n)
    if entry == "tic_compress_dev_async":  # a ticket that opens is collected: the row's outcome is then the result's
        rc = L.tic_compress_dev_async(c, dimg, h, w, s, q, dout, cap, C.byref(E.tk) if a["lenp"] else None)
        return rc if rc != N.TIC_OK else L.tic_async_result(c, E.tk.value, a["wait"], C.byref(E.n))
    if entry == "tic_dctq_dev_frames":
        return L.tic_dctq_dev_frames(c, dimg, a["nframes"], h, w, s, a["fstride"], q, dzz, a["cstride"], a["variant"])
    if entry == "tic_dctq_dev_frames_timed":
        return L.tic_dctq_dev_frames_timed(c, dimg, a["nframes"], h, w, s, a["fstride"], q, dzz, a["cstride"], a["variant"], a["iters"], ms)
    if entry == "tic_dctq_scaled_dev_frames":
        return L.tic_dctq_scaled_dev_frames(c, dimg, a["nframes"], h, w, s, a["fstride"], qf, dzz, a["cstride"])
    if entry == "tic_dctq_dev_timed":
        return L.tic_dctq_dev_timed(c, dimg, h, w, s, q, dzz, a["variant"], a["iters"], ms)
    if entry == "tic_dctq_dev_timed_warm":
        return L.tic_dctq_dev_timed_warm(c, dimg, h, w, s, q, dzz, a["variant"], a["warm"], a["iters"], ms, per)
    if entry == "tic_dctq_dev_timed_rotating":
        imgs, outs = (C.c_void_p * 1)(dimg), (C.c_void_p * 1)(dzz)
        return L.tic_dctq_dev_timed_rotating(c, imgs, outs, 1, h, w, s, q, a["variant"], a["iters"], ms)
    if entry == "tic_dctq_scaled_dev_timed_warm":
        return L.tic_dctq_scaled_dev_timed_warm(c, dimg, h, w, s, qf, dzz, a["warm"], a["iters"], ms, per)
    if entry == "tic_entropy_size_dev_timed":
        return L.tic_entropy_size_dev_timed(c, E.d_zz if a["img"] else None, h, w, a["warm"], a["iters"], ms)
    raise KeyError(entry)


HOST = ("tic_dctq", "tic_compress", "tic_dctq_scaled", "tic_compress_scaled", "tic_compress_adaptive", "tic_stream_sizes", "tic_compress_to_size")
STREAM_DEV = ("tic_compress_dev", "tic_compress_dev_async", "tic_compress_scaled_dev", "tic_compress_to_size_dev")
FRAMES = ("tic_dctq_dev_frames", "tic_dctq_dev_frames_timed", "tic_dctq_scaled_dev_frames")
TIMED = ("tic_dctq_dev_timed", "tic_dctq_dev_timed_warm", "tic_dctq_dev_frames_timed", "tic_dctq_dev_timed_rotating",
         "tic_dctq_scaled_dev_timed_warm", "tic_entropy_size_dev_timed")
SCALED = ("tic_dctq_scaled", "tic_compress_scaled", "tic_compress_scaled_dev", "tic_dctq_scaled_dev_frames", "tic_dctq_scaled_dev_timed_warm")
NO_QUALITY = SCALED + ("tic_entropy_size_dev_timed",)
NO_STRIDE = ("tic_entropy_encode_dev", "tic_entropy_size_dev_timed")
ALL = tuple(dict.fromkeys(HOST + STREAM_DEV + ("tic_entropy_encode_dev",) + FRAMES + TIMED))
WRITES_STREAM = ("tic_compress", "tic_compress_scaled", "tic_compress_adaptive", "tic_compress_to_size", "tic_entropy_encode_dev") + STREAM_DEV


def rows():
    """[(row name, entry point, overrides)] in the order they are recorded and replayed."""
    r = []
    for e in ALL:
        r.append(("negative size", e, dict(h=-1)))
        if e not in NO_QUALITY:
            r.append(("quality 0 (TIC_QUALITY_CUSTOM)", e, dict(q=0, qmin=0)))
            r.append(("quality 100", e, dict(q=100, qmax=100)))
        if e not in NO_STRIDE:
            r.append(("stride less than width", e, dict(stride=63)))
        r.append(("null image", e, dict(img=False)))
        if e != "tic_entropy_size_dev_timed":  # (it writes nothing but the time)
            r.append(("null output", e, dict(out=False)))
        if e not in ("tic_dctq", "tic_dctq_scaled", "tic_stream_sizes") + tuple(x for x in FRAMES if x not in TIMED):
            r.append(("null length", e, dict(lenp=False)))
    for e in WRITES_STREAM:
        r.append(("cap 15", e, dict(cap=15)))
        r.append(("cap 64: TIC_E_SPACE", e, dict(cap=64)))
    for e in ("tic_compress_scaled", "tic_compress_scaled_dev"):
        r.append(("cap 16", e, dict(cap=16)))
    for e in ("tic_entropy_encode_dev", "tic_compress_dev", "tic_compress_dev_async", "tic_compress_scaled_dev"):
        r.append(("misaligned device output", e, dict(shift=8)))
    for e in FRAMES:
        r.append(("nframes -1", e, dict(nframes=-1)))
        r.append(("nframes 65536", e, dict(nframes=65536)))
        r.append(("frame stride one short", e, dict(fstride=4095)))
        r.append(("coefficient frame stride one short", e, dict(cstride=8191)))
    r.append(("coefficient frame stride 8 off", "tic_dctq_scaled_dev_frames", dict(cstride=8200)))
    for e in SCALED:
        r.append(("60x64", e, dict(h=60)))
        r.append(("setting 4", e, dict(qf=4)))
    for e in TIMED:
        r.append(("iters 0", e, dict(iters=0)))
    for e in ("tic_dctq_dev_timed_warm", "tic_dctq_scaled_dev_timed_warm", "tic_entropy_size_dev_timed"):
        r.append(("warm -1", e, dict(warm=-1)))
    for e in ("tic_dctq_dev_timed_warm", "tic_dctq_scaled_dev_timed_warm"):
        r.append(("per-launch times with iters 32769", e, dict(per=True, iters=32769)))
    for e in ("tic_dctq_dev_frames", "tic_dctq_dev_timed", "tic_dctq_dev_timed_warm", "tic_dctq_dev_frames_timed", "tic_dctq_dev_timed_rotating"):
        r.append(("unknown kernel variant", e, dict(variant=7)))
    r.append(("0x8 image", "tic_compress_adaptive", dict(h=0, w=8, stride=8)))
    for e in ("tic_compress_to_size", "tic_compress_to_size_dev"):
        r.append(("quality range 60..40", e, dict(qmin=60, qmax=40)))
        r.append(("budget 20: TIC_E_SPACE", e, dict(budget=20)))
    return r


def play(E):
    """{"entry: row": [return code, tic_last_error text]} of every row, and of the two ticket rows."""
    L, c = E.L, E.h
    out = {}

    def record(key, rc):
        assert key not in out, key
        out[key] = [int(rc), L.tic_last_error(c).decode()]

    def mark():
        assert L.tic_dctq_dev(c, None, -7, -7, 0, 50, None, N.KERNEL_AUTO) == N.TIC_E_ARG

    for name, entry, kw in rows():
        mark()
        record("%s: %s" % (entry, name), _call(E, entry, kw))
    # one ticket more than the context holds, and a ticket that is not open
    mark()
    tks = []
    for k in range(ASYNC_SLOTS):
        assert L.tic_compress_dev_async(c, E.d_img, 64, 64, 64, 50, E.d_out, E.cap, C.byref(E.tk)) == N.TIC_OK
        tks.append(E.tk.value)
    record("tic_compress_dev_async: ticket %d" % (ASYNC_SLOTS + 1), L.tic_compress_dev_async(c, E.d_img, 64, 64, 64, 50, E.d_out, E.cap, C.byref(E.tk)))
    for t in tks:
        assert L.tic_async_result(c, t, 1, C.byref(E.n)) == N.TIC_OK
    mark()
    record("tic_async_result: unopened ticket", L.tic_async_result(c, tks[-1] + 5, 1, C.byref(E.n)))
    return out
