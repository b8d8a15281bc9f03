"""Frames and the device driver of tests/test_strip_prologue_gpu.py, shared by the test process (test-hooks build) and the fresh process that
runs the shipped library.  Each frame is the smallest that reaches a branch of the strip kernel's start (csrc/tic_strip_plan.h); the same
list is walked on the CPU by tests/native/strip_plan_selftest.cpp."""
import ctypes as C

import numpy as np

# (name, width, height, row pitch)
SHAPES = [
    ("64x8: one strip, three idle waves", 64, 8, 64),
    ("72x16: a ninth block per row for the exact kernel", 72, 16, 72),
    ("72x16, rows not 8-aligned: no fast rectangle", 72, 16, 75),
    ("4096x8: one strip row", 4096, 8, 4096),
    ("1920x1080: 30 strips per row", 1920, 1080, 1920),
    ("64x1024: one strip per row", 64, 1024, 64),
    ("2048x1528: one block row below the team schedule", 2048, 1528, 2048),
    ("2048x1536: the smallest team schedule", 2048, 1536, 2048),
    ("2048x1544: one block row above", 2048, 1544, 2048),
    ("512x512", 512, 512, 512),
]
BATCH = ("3 x 1024x512, 4 KiB between frames", 1024, 512, 1024, 3, 4096)
QUALITY = 50


def frame(k, w, h):
    """Noise, with a band of posterised noise (rational ties and irrational trips: the rare paths find their strips through the schedule)."""
    img = np.random.default_rng(4200 + k).integers(0, 256, (h, w), dtype=np.uint8)
    if h >= 64:
        img[h // 2: h // 2 + 16] = img[h // 2: h // 2 + 16] // 8 * 8 + 1
    return img


class Dev:
    def __init__(self, ctx, L, imgs, pitch, gap=0):
        """imgs: frames of one size, laid out pitch bytes per row and `gap` bytes between frames."""
        self.ctx, self.L = ctx, L
        self.nf = len(imgs)
        self.h, self.w = imgs[0].shape
        self.pitch = pitch
        self.fstride = self.h * pitch + gap
        host = np.full(self.nf * self.fstride, 0xA5, dtype=np.uint8)
        for f, img in enumerate(imgs):
            host[f * self.fstride: f * self.fstride + self.h * pitch].reshape(self.h, pitch)[:, : self.w] = img
        self.n = L.tic_num_blocks(self.h, self.w)
        self.ostride = self.n * 128 + 256
        self.d_img, self.d_out = C.c_void_p(), C.c_void_p()
        ctx.check(L.tic_dev_alloc(ctx.handle, host.size, C.byref(self.d_img)))
        ctx.check(L.tic_dev_alloc(ctx.handle, self.nf * self.ostride, C.byref(self.d_out)))
        ctx.check(L.tic_memcpy_h2d(ctx.handle, self.d_img, host.ctypes.data, host.size))

    def run(self, variant, quality=QUALITY):
        """-> int16 [frames][blocks][64]"""
        ctx, L = self.ctx, self.L
        ctx.check(L.tic_memset_dev(ctx.handle, self.d_out, 0x5A, self.nf * self.ostride))
        if self.nf == 1:
            ctx.check(L.tic_dctq_dev(ctx.handle, self.d_img, self.h, self.w, self.pitch, quality, self.d_out, variant))
        else:
            ctx.check(L.tic_dctq_dev_frames(ctx.handle, self.d_img, self.nf, self.h, self.w, self.pitch, self.fstride, quality, self.d_out, self.ostride, variant))
        raw = np.empty(self.nf * self.ostride, dtype=np.uint8)
        ctx.check(L.tic_memcpy_d2h(ctx.handle, raw.ctypes.data, self.d_out, raw.size))
        rows = raw.reshape(self.nf, self.ostride)
        assert (rows[:, self.n * 128:] == 0x5A).all(), "bytes between the frames' coefficients were written"
        return np.ascontiguousarray(rows[:, : self.n * 128]).view(np.int16).reshape(self.nf, self.n, 64)

    def free(self):
        self.L.tic_dev_free(self.ctx.handle, self.d_img)
        self.L.tic_dev_free(self.ctx.handle, self.d_out)


def all_cases():
    """(name, frames, pitch, gap) for every shape and the batch."""
    out = [(name, [frame(k, w, h)], pitch, 0) for k, (name, w, h, pitch) in enumerate(SHAPES)]
    name, w, h, pitch, nf, gap = BATCH
    out.append((name, [frame(100 + f, w, h) for f in range(nf)], pitch, gap))
    return out


def check_all(ctx, L, N, oracle, label):
    """Every case: the strip kernel against the exact kernel and against the oracle, coefficient for coefficient.  Returns the number of cases."""
    n = 0
    for name, imgs, pitch, gap in all_cases():
        d = Dev(ctx, L, imgs, pitch, gap)
        try:
            want = np.stack([oracle(img) for img in imgs])
            exact = d.run(N.KERNEL_EXACT)
            hybrid = d.run(N.KERNEL_HYBRID)
            assert np.array_equal(exact, want), (label, name, "exact kernel against the oracle")
            assert np.array_equal(hybrid, exact), (label, name, "strip kernel against the exact kernel", int((hybrid != exact).any(axis=2).sum()), "blocks differ")
        finally:
            d.free()
        n += 1
    return n
