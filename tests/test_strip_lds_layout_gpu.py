"""The strip kernel's lane-linear LDS layouts (columns-first instantiation, csrc/tic_strip_lds.h: the dword transpose's planes and the
zig-zag staging's) on the smallest frames the kernel takes: one strip, two strips for one wave, all four waves of a workgroup.
Production kernel against exact kernel against the oracle, coefficient for coefficient, on the test-hooks build (columns first forced
through TIC_ORDER=1; grids this small take that order anyway) and on the shipped library, loaded beside it into this process.  The
content drives the tie patch (rational_quad reads its column sums from planes 0 and 4 and overwrites four halfwords of the staging), the
batch join (a copy of the gathered 16 bytes) and the batch overflow through the layouts."""
import ctypes as C

import numpy as np
import pytest

from conftest import rand_frame

from tinyimgcodec_amd import _native as N

pytestmark = pytest.mark.gpu

SHAPES = [(64, 8), (64, 16), (128, 8), (256, 72)]  # width x height
QUALITIES = (50, 90)
ABI = ("tic_build_has_test_hooks", "tic_create", "tic_destroy", "tic_num_blocks", "tic_dev_alloc", "tic_dev_free", "tic_memcpy_h2d",
       "tic_memcpy_d2h", "tic_memset_dev", "tic_dctq_dev", "tic_last_strip_launch")


def bind(path):
    L = C.CDLL(path)
    for name in ABI:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = N.SIGNATURES[name]
    return L


def tiled_blocks(img, w, h):
    """The 8x8 blocks of a golden image laid into a w x h frame, row by row, from the first block on (repeated when they run out)."""
    blocks = img.astype(np.uint8).reshape(img.shape[0] // 8, 8, img.shape[1] // 8, 8).swapaxes(1, 2).reshape(-1, 8, 8)
    n = (h // 8) * (w // 8)
    pick = blocks[np.arange(n) % len(blocks)]
    return np.ascontiguousarray(pick.reshape(h // 8, w // 8, 8, 8).swapaxes(1, 2).reshape(h, w))


def contents(golden, w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return {
        "noise": rand_frame(4000 + w + h, h, w),
        "flat odd grey": np.full((h, w), 129, np.uint8),
        "checkerboard 100/102": np.where((yy + xx) % 2 == 0, 100, 102).astype(np.uint8),
        "near_ties blocks": tiled_blocks(golden("near_ties")["img"], w, h),
        "tie_blocks blocks": tiled_blocks(golden("tie_blocks")["img"], w, h),
    }


class Frame:
    def __init__(self, L, ctx, img):
        self.L, self.ctx = L, ctx
        self.h, self.w = img.shape
        self.n = L.tic_num_blocks(self.h, self.w)
        self.d_img, self.d_out = C.c_void_p(), C.c_void_p()
        assert L.tic_dev_alloc(ctx, img.size, C.byref(self.d_img)) == 0 and L.tic_dev_alloc(ctx, self.n * 128, C.byref(self.d_out)) == 0
        assert L.tic_memcpy_h2d(ctx, self.d_img, img.ctypes.data, img.size) == 0

    def run(self, quality, variant):
        L, ctx = self.L, self.ctx
        assert L.tic_memset_dev(ctx, self.d_out, 0x5A, self.n * 128) == 0
        assert L.tic_dctq_dev(ctx, self.d_img, self.h, self.w, self.w, quality, self.d_out, variant) == 0
        zz = np.empty((self.n, 64), dtype=np.int16)
        assert L.tic_memcpy_d2h(ctx, zz.ctypes.data, self.d_out, self.n * 128) == 0
        return zz

    def free(self):
        self.L.tic_dev_free(self.ctx, self.d_img)
        self.L.tic_dev_free(self.ctx, self.d_out)


@pytest.fixture(scope="module")
def builds():
    """Both builds of the library in this process: the test-hooks build the suite runs on, and the product."""
    hooks, shipped = N.load(), bind(N.LIB_PATH)
    assert hooks.tic_build_has_test_hooks() == 1 and shipped.tic_build_has_test_hooks() == 0
    out = {}
    for name, L in (("hooks build", hooks), ("shipped library", shipped)):
        ctx = L.tic_create(0)
        assert ctx
        out[name] = (L, ctx)
    yield out
    for L, ctx in out.values():
        L.tic_destroy(ctx)


@pytest.fixture(scope="module")
def wanted(oracle, golden):
    """The oracle's coefficients of every frame, computed once."""
    out = {}
    for w, h in SHAPES:
        for name, img in contents(golden, w, h).items():
            out[(w, h, name)] = (img, {q: oracle.encode_zz16(img, q) for q in QUALITIES})
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_small_frames_through_the_plane_layout(builds, wanted, monkeypatch, shape):
    w, h = shape
    monkeypatch.setenv("TIC_TUNE", "1")  # the hooks build re-reads its knobs at every launch
    for (fw, fh, name), (img, want) in wanted.items():
        if (fw, fh) != (w, h):
            continue
        for build, (L, ctx) in builds.items():
            f = Frame(L, ctx, img)
            for q in QUALITIES:
                assert np.array_equal(f.run(q, N.KERNEL_EXACT), want[q]), (name, q, build, "exact kernel")
                monkeypatch.setenv("TIC_ORDER", "1")  # columns first (read by the hooks build only)
                got = f.run(q, N.KERNEL_HYBRID)
                monkeypatch.delenv("TIC_ORDER")
                # the launcher's report: columns first (forced on the hooks build, the grid's own choice on the product), one strided round of
                # ceil(strips / 4) workgroups over the whole frame
                info, wgs = (C.c_int * 8)(), ((w // 64) * (h // 8) + 3) // 4
                assert L.tic_last_strip_launch(ctx, info) == 0
                assert list(info) == [2, 0, 0, wgs, 1, 4 * wgs, w // 64, h // 8], (name, q, build, list(info))
                assert np.array_equal(got, want[q]), (name, q, build, "strip kernel", int((got != want[q]).any(axis=1).sum()), "blocks differ")
            f.free()
