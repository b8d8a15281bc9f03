"""The integer encoder's arithmetic at its edges on the MI355X: fdctq_scaled_kernel and fdctq_scaled_kernel_v (tic_scaled.hip) on the built
blocks of tests/golden/scaled_blocks.npz / .json (tests/scaled_blocks.py names the families; the generator pins them on the unmodified
reference).  Exact comparisons only, and every result is compared with the fixture - the reference's coefficients, streams and decoded
pixels, and for the one frame that has no code at `best` the model's coefficients, which tests/test_scaled_blocks_cpu.py licenses - never
with another GPU result.  The blocks expose every word of the quantiser table a lane can read wrongly, the top of the coefficient range,
the 1023 / 1024 line of the code table and the largest DC difference; the frames are 72 pixels wide, so blocks fall at every strip
position and every second strip holds one block."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

import scaled_blocks as S

pytestmark = pytest.mark.gpu

SETTINGS = S.SETTINGS


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(0)
    assert c.arch.startswith("gfx950"), c.arch
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return S.Fixture()


class Dev:
    """Device buffers through the C-ABI; freed by close()."""

    def __init__(self, ctx):
        self.ctx, self.L, self.ptrs = ctx, N.load(), []

    def alloc(self, nbytes, fill=None):
        p = C.c_void_p()
        self.ctx.check(self.L.tic_dev_alloc(self.ctx.handle, max(nbytes, 16), C.byref(p)))
        self.ptrs.append(p)
        if fill is not None:
            self.ctx.check(self.L.tic_memset_dev(self.ctx.handle, p, fill, max(nbytes, 16)))
        return p

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.alloc(arr.nbytes)
        self.ctx.check(self.L.tic_memcpy_h2d(self.ctx.handle, p, arr.ctypes.data, arr.nbytes))
        return p

    def download(self, p, nbytes):
        out = np.empty(nbytes, np.uint8)
        self.ctx.check(self.L.tic_memcpy_d2h(self.ctx.handle, out.ctypes.data, p, nbytes))
        return out

    def close(self):
        for p in self.ptrs:
            self.L.tic_dev_free(self.ctx.handle, p)
        self.ptrs = []


@pytest.fixture()
def dev(ctx):
    d = Dev(ctx)
    yield d
    d.close()


def test_single_frame_kernel_matches_the_fixture(ctx, fx):
    """dctq_scaled of every frame at every setting = the fixture's coefficients; compress_scaled = the fixture's stream (KeyError where the
    reference has none); decompress of the stream has the digest of the reference's decompress().  No frame here has the 1,024 blocks the
    device decoder asks for, so this decompress is the host decoder's; test_streams_through_the_device_decoder lowers that line."""
    L = N.load()
    for name, s in fx.cases():
        img, e = fx.pixels(name), fx.entry(name, s)
        zz = T.dctq_scaled(img, s, ctx=ctx)
        assert zz.dtype == np.int16 and np.array_equal(zz, fx.zz(name, s)), (name, s, int((zz != fx.zz(name, s)).sum()))
        if e["pinned_by"] == "model":
            with pytest.raises(KeyError):
                T.compress_scaled(img, s, ctx=ctx)
            continue
        bs = T.compress_scaled(img, s, ctx=ctx)
        assert bs == fx.stream(name, s), (name, s)
        dec = T.decompress(bs, ctx=ctx)
        assert dec.shape == img.shape and S.sha(dec) == e["dec_sha256"], (name, s)
        assert L.tic_last_decode_path(ctx.handle) == 2, (name, s)


def test_streams_through_the_device_decoder(ctx, fx, monkeypatch):
    """The reference's streams with the device decoder's block floor lowered to one block (TIC_DECODE_MIN_BLOCKS=1): every stream of
    at least 128 + 8,192 bits (1,040 bytes: the floor the kernel itself needs) is decoded on the device, without giving up, to the
    reference's pixels - among them peak_0 at best, which holds |AC| = 986 and the DC differences of +-1,020; the shorter ones stay on the
    host."""
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_DECODE_MIN_BLOCKS", "1")
    on_device = []
    for name, s in fx.cases():
        e, bs = fx.entry(name, s), fx.stream(name, s)
        if bs is None:
            continue
        dec = T.decompress(bs, ctx=ctx)
        assert dec.shape == fx.pixels(name).shape and S.sha(dec) == e["dec_sha256"], (name, s)
        if len(bs) >= 1040:
            assert L.tic_last_decode_path(ctx.handle) == 1 and L.tic_last_decode_giveup(ctx.handle) == 0, (name, s, len(bs))
            on_device.append((name, s))
        else:
            assert L.tic_last_decode_path(ctx.handle) == 2, (name, s, len(bs))
    assert ("peak_0", "best") in on_device and len(on_device) >= 4
    assert fx.entry("peak_0", "best")["max_abs_ac"] == 986 and fx.entry("peak_0", "best")["max_abs_dc_diff"] == 1020


def test_frames_launch(ctx, fx, dev):
    """tic_dctq_scaled_dev_frames: the corpus's full frames (64 x 72, one grid row each) in one launch per setting."""
    L = N.load()
    names = [n for n, e in fx.frames.items() if e["h"] == 64]
    assert len(names) >= 4
    px, zb = 64 * 72, 72 * 128
    d_img = dev.upload(np.stack([fx.pixels(n) for n in names]))
    for qf, s in enumerate(SETTINGS):
        d_zz = dev.alloc(len(names) * zb + 256, fill=0x5A)
        ctx.check(L.tic_dctq_scaled_dev_frames(ctx.handle, d_img, len(names), 64, 72, 72, px, qf, d_zz, zb))
        ctx.check(L.tic_sync(ctx.handle))
        raw = dev.download(d_zz, len(names) * zb + 256)
        assert (raw[len(names) * zb:] == 0x5A).all()
        got = raw[: len(names) * zb].view(np.int16).reshape(len(names), 72, 64)
        for k, n in enumerate(names):
            assert np.array_equal(got[k], fx.zz(n, s)), (n, s)


def test_unaligned_loads(ctx, fx, dev):
    """Every frame from a device buffer one byte past its allocation's start, rows 85 bytes apart: the byte-load path (aligned8 == 0)."""
    L = N.load()
    pitch, shift = S.FRAME_W + 13, 1
    for name in fx.frames:
        img = fx.pixels(name)
        h, w = img.shape
        host = np.full(h * pitch + shift + 16, 0x77, np.uint8)
        host[shift: shift + h * pitch].reshape(h, pitch)[:, :w] = img
        d_img = dev.upload(host)
        for qf, s in enumerate(SETTINGS):
            d_zz = dev.alloc(h * w * 2 + 256, fill=0x5A)
            ctx.check(L.tic_dctq_scaled_dev(ctx.handle, C.c_void_p(d_img.value + shift), h, w, pitch, qf, d_zz))
            ctx.check(L.tic_sync(ctx.handle))
            raw = dev.download(d_zz, h * w * 2 + 256)
            assert (raw[h * w * 2:] == 0x5A).all()
            assert np.array_equal(raw[: h * w * 2].view(np.int16).reshape(-1, 64), fx.zz(name, s)), (name, s)
        dev.close()


def dctq_v(ctx, dev, frames, qfs):
    """tic_dctq_scaled_v_dev: one launch -> [int16 [N_i, 64] per record]."""
    L = N.load()
    m = len(frames)
    ptrs = [dev.upload(f).value for f in frames]
    nblk = [f.size // 64 for f in frames]
    total = sum(nblk) * 128
    d_zz = dev.alloc(total + 256, fill=0x5A)
    ctx.check(L.tic_dctq_scaled_v_dev(ctx.handle, (C.c_void_p * m)(*ptrs), m, (C.c_int * m)(*[f.shape[0] for f in frames]),
                                      (C.c_int * m)(*[f.shape[1] for f in frames]), (C.c_ssize_t * m)(*[f.shape[1] for f in frames]),
                                      (C.c_int * m)(*qfs), d_zz))
    raw = dev.download(d_zz, total + 256)
    assert (raw[total:] == 0x5A).all()
    zz = raw[:total].view(np.int16).reshape(-1, 64)
    offs = np.concatenate(([0], np.cumsum(nblk)))
    return [zz[offs[i]: offs[i + 1]] for i in range(m)]


@pytest.mark.parametrize("groups", [None, "1"])
@pytest.mark.parametrize("order", ["alternating", "grouped"])
def test_descriptor_form_kernel(ctx, fx, dev, monkeypatch, order, groups):
    """All frames x four settings as the records of ONE tic_dctq_scaled_v_dev launch and ONE compress_batch_scaled call (without the record
    that has no code).  alternating: frame by frame, the settings inside; grouped: setting by setting.  The launch has 528 strips.  With
    one workgroup (TIC_SCALED_V_GROUPS=1) its four waves walk 132 strips each across every record, and a wave reloads its table words
    (rc.qf != tab_qf) at nearly every record it enters in the alternating order, three times in the grouped one.  The default grid has
    132 workgroups, a wave per strip: there the table is loaded once per wave in either order, and what the two orders vary is only which
    record and setting a wave finds through the descriptor table."""
    assert N.load().tic_build_has_test_hooks() == 1
    if groups:
        monkeypatch.setenv("TIC_SCALED_V_GROUPS", groups)
    cases = fx.cases() if order == "alternating" else sorted(fx.cases(), key=lambda c: SETTINGS.index(c[1]))
    qfs = [SETTINGS.index(s) for _, s in cases]
    assert len(cases) == 4 * len(fx.frames) <= 64
    assert sum(a != b for a, b in zip(qfs, qfs[1:])) == (len(cases) - 1 if order == "alternating" else 3)
    got = dctq_v(ctx, dev, [fx.pixels(n) for n, _ in cases], qfs)
    for (n, s), zz in zip(cases, got):
        assert np.array_equal(zz, fx.zz(n, s)), (n, s, int((zz != fx.zz(n, s)).sum()))
    coded = [(n, s) for n, s in cases if fx.entry(n, s)["pinned_by"] == "reference"]
    streams = T.compress_batch_scaled([fx.pixels(n) for n, _ in coded], [s for _, s in coded], ctx=ctx)
    for (n, s), bs in zip(coded, streams):
        assert bs == fx.stream(n, s), (n, s)
    with pytest.raises(KeyError):
        T.compress_batch_scaled([fx.pixels(n) for n, _ in cases], [s for _, s in cases], ctx=ctx)


def test_the_line_between_1023_and_1024(ctx, fx):
    """Blocks as frames of their own.  (1, 1) = +1023 and -1023 at best compress to what the host entropy stage - pinned on the reference
    by the CPU tests - makes of the fixture's coefficients, and the frame that holds them to the reference's stream; +1024, -1024 and the
    two (1, 1) peaks (1072, -1073) raise KeyError at best while dctq_scaled returns the model's coefficients, and compress at `high` to the
    reference's bytes.  rd_points_scaled_batch of all frames reports -1 for the no-code frame at best alone and the fixture's sizes
    everywhere else; its sums are roundtrip_sse_scaled's."""
    line = S.frame_blocks(fx.pixels("line1023_0"))
    line_zz = fx.zz("line1023_0", "best")
    for k, want in ((0, 1023), (1, -1023)):
        assert line_zz[k, 4] == want  # (1, 1) is scan position 4
        got = T.compress_scaled(line[k].reshape(8, 8), "best", ctx=ctx)
        assert got == T.entropy_encode_scaled(line_zz[k: k + 1], 8, 8, "best"), want
    assert T.compress_scaled(fx.pixels("line1023_0"), "best", ctx=ctx) == fx.stream("line1023_0", "best")
    nocode = S.frame_blocks(fx.pixels("nocode_0"))
    assert sorted(int(z[4]) for z in fx.zz("nocode_0", "best")[:4]) == [-1073, -1024, 1024, 1072]
    for k in range(4):
        blk = nocode[k].reshape(8, 8)
        with pytest.raises(KeyError):
            T.compress_scaled(blk, "best", ctx=ctx)
        assert np.array_equal(T.dctq_scaled(blk, "best", ctx=ctx), fx.zz("nocode_0", "best")[k: k + 1])
        assert T.compress_scaled(blk, "high", ctx=ctx) == T.entropy_encode_scaled(fx.zz("nocode_0", "high")[k: k + 1], 8, 8, "high")
    names = list(fx.frames)
    sizes, sse, wrapped = T.rd_points_scaled_batch([fx.pixels(n) for n in names], ctx=ctx)
    assert sizes.shape == (len(names), 4)
    for i, n in enumerate(names):
        for j, s in enumerate(SETTINGS):
            e = fx.entry(n, s)
            assert int(sizes[i, j]) == (e["bytes"] if e["pinned_by"] == "reference" else -1), (n, s)
            assert (int(sse[i, j]), int(wrapped[i, j])) == T.roundtrip_sse_scaled(fx.pixels(n), s, ctx=ctx), (n, s)
    assert int((sizes == -1).sum()) == 1


def test_single_calls_on_the_shipped_library(fx):
    """The single-frame checks once more in a fresh process that loads the library that ships (no test hooks, no TIC_* variable)."""
    code = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N
import scaled_blocks as S
assert N.load().tic_build_has_test_hooks() == 0 and N._lib_path() == N.LIB_PATH
fx = S.Fixture()
refused = 0
for name, s in fx.cases():
    img, e = fx.pixels(name), fx.entry(name, s)
    assert np.array_equal(T.dctq_scaled(img, s), fx.zz(name, s)), (name, s)
    if e["pinned_by"] == "model":
        try:
            T.compress_scaled(img, s)
        except KeyError:
            refused += 1
        continue
    bs = T.compress_scaled(img, s)
    assert bs == fx.stream(name, s), (name, s)
    assert S.sha(T.decompress(bs)) == e["dec_sha256"], (name, s)
assert refused == 1
print("scaled blocks on the shipped library ok")
'''
    env = {k: v for k, v in os.environ.items() if not k.startswith("TIC_")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "scaled blocks on the shipped library ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
