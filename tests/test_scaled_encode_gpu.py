"""The scaled-DCT encoder on the MI355X: the integer transform kernel (tic_scaled.hip) and the device entropy stage with the stream's
own header and flush byte, against the reference's streams and coefficients (tests/golden/scaled_encode.npz / .json: the unmodified
reference's C program, its output cut behind the last block and read back with the reference's own bit reader).  No result here is
compared with another GPU result only: every coefficient and every byte is pinned to the reference through the fixtures.

Not covered: 16384x16384 at `med` (4 M blocks through the reference's pure-Python bit reader were not generated); tic_compress_scaled_batch
does not exist."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

from conftest import rand_frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SETTINGS = ("best", "high", "med", "low")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(0)
    assert c.arch.startswith("gfx950"), c.arch
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(GOLDEN, "scaled_encode.json")) as f:
        man = json.load(f)
    return np.load(os.path.join(GOLDEN, "scaled_encode.npz")), man


def case_image(npz, key):
    if key.startswith("lenna512_"):
        return np.load(os.path.join(GOLDEN, "lenna.npz"))["img"]
    return npz[key + "_img"]


def check_array(npz, man, key, suffix, sha_key, got):
    """got == the fixture's array: by digest always, element by element where the fixture holds the whole array (else its head)."""
    assert sha(got) == man["cases"][key][sha_key], (key, suffix)
    name = "%s_%s" % (key, suffix)
    if name in npz.files:
        assert np.array_equal(got, npz[name]), (key, suffix)
    else:
        head = npz[name + "_head"]
        assert np.array_equal(got[: head.shape[0]], head), (key, suffix)


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
        if arr.nbytes:
            self.ctx.check(self.L.tic_memcpy_h2d(self.ctx.handle, p, arr.ctypes.data, arr.nbytes))
        return p

    def download(self, p, nbytes, dtype=np.uint8, offset=0):
        out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype)
        if nbytes:
            self.ctx.check(self.L.tic_memcpy_d2h(self.ctx.handle, out.ctypes.data, C.c_void_p(p.value + offset), nbytes))
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


def test_dctq_scaled_and_compress_scaled_match_the_reference(ctx, fx):
    """Every fixture case at every setting: coefficients and stream, byte for byte (the byte-boundary cases end in the extra 00, the
    flat frame is 6 bits + flush, the empty frame is 17 bytes)."""
    npz, man = fx
    for key, m in man["cases"].items():
        img = case_image(npz, key)
        zz = T.dctq_scaled(img, m["setting"], ctx=ctx)
        assert zz.shape == ((m["h"] // 8) * (m["w"] // 8), 64) and zz.dtype == np.int16
        check_array(npz, man, key, "zz", "zz_sha256", zz)
        bs = T.compress_scaled(img, m["setting"], ctx=ctx)
        assert len(bs) == m["bytes"] == 16 + m["payload_bits"] // 8 + 1, key
        check_array(npz, man, key, "bs", "sha256", np.frombuffer(bs, np.uint8))
        assert bs == T.compress_scaled(img, SETTINGS.index(m["setting"]), ctx=ctx)
    assert T.compress_scaled(case_image(npz, "noise64x96_med"), ctx=ctx) == npz["noise64x96_med_bs"].tobytes()  # default setting: med (encode.c:33)


def test_resident_entry_points_strides_and_frames(ctx, fx, dev):
    """tic_compress_scaled_dev (resident) and tic_compress_scaled (host buffers) give the reference's bytes; so do rows further apart than
    w (a multiple of 8, and one that is not: the byte-load path) and a misaligned first pixel; tic_dctq_scaled_dev_frames on 8 frames - the
    eight 64-row bands of Lenna, which are Lenna's coefficient rows - equals the reference, back to back and with padded frame strides."""
    npz, man = fx
    L = N.load()
    n = C.c_size_t()
    for key in ("noise64x96_best", "noise16x24_low", "ramp48x48_med", "aligned_med_med", "lenna512_high"):
        m = man["cases"][key]
        img, h, w, qf = case_image(npz, key), m["h"], m["w"], SETTINGS.index(m["setting"])
        cap = L.tic_compress_scaled_bound(h, w)
        out = np.empty(cap, np.uint8)
        ctx.check(L.tic_compress_scaled(ctx.handle, np.ascontiguousarray(img).ctypes.data, h, w, w, qf, out.ctypes.data, cap, C.byref(n)))
        check_array(npz, man, key, "bs", "sha256", out[: n.value])
        for pitch, shift in ((w, 0), (w + 40, 0), (w + 13, 0), (w + 24, 3)):
            host = np.full(h * pitch + shift + 16, 0x77, np.uint8)
            host[shift: shift + h * pitch].reshape(h, pitch)[:, :w] = img
            d_img = dev.upload(host)
            src = C.c_void_p(d_img.value + shift)
            d_zz = dev.alloc(m["h"] * m["w"] * 2, fill=0x5A)
            ctx.check(L.tic_dctq_scaled_dev(ctx.handle, src, h, w, pitch, qf, d_zz))
            ctx.check(L.tic_sync(ctx.handle))
            check_array(npz, man, key, "zz", "zz_sha256", dev.download(d_zz, h * w * 2, np.int16).reshape(-1, 64))
            d_out = dev.alloc(cap)
            ctx.check(L.tic_compress_scaled_dev(ctx.handle, src, h, w, pitch, qf, d_out, cap, C.byref(n)))
            assert n.value == m["bytes"]
            check_array(npz, man, key, "bs", "sha256", dev.download(d_out, n.value))
            dev.close()
    lenna = np.load(os.path.join(GOLDEN, "lenna.npz"))["img"]
    for setting in ("best", "low"):
        qf = SETTINGS.index(setting)
        want = man["cases"]["lenna512_" + setting]["zz_sha256"]
        band_px, band_zz = 64 * 512, 8 * 64 * 128
        for fs_in, fs_out in ((band_px, band_zz), (band_px + 4096, band_zz + 256)):
            host = np.zeros(8 * fs_in, np.uint8)
            for k in range(8):
                host[k * fs_in: k * fs_in + band_px] = lenna[64 * k: 64 * k + 64].reshape(-1)
            d_img = dev.upload(host)
            d_zz = dev.alloc(8 * fs_out, fill=0x5A)
            ctx.check(L.tic_dctq_scaled_dev_frames(ctx.handle, d_img, 8, 64, 512, 512, fs_in, qf, d_zz, fs_out))
            ctx.check(L.tic_sync(ctx.handle))
            raw = dev.download(d_zz, 8 * fs_out).reshape(8, fs_out)
            assert sha(raw[:, :band_zz]) == want, (setting, fs_in)
            assert (raw[:, band_zz:] == 0x5A).all()  # nothing between the frames' coefficients is written
            singles = []
            for k in range(8):  # ... and 8 single launches give the same
                d_one = dev.alloc(band_zz)
                ctx.check(L.tic_dctq_scaled_dev(ctx.handle, C.c_void_p(d_img.value + k * fs_in), 64, 512, 512, qf, d_one))
                ctx.check(L.tic_sync(ctx.handle))
                singles.append(dev.download(d_one, band_zz))
            assert sha(np.stack(singles)) == want
            dev.close()


def test_large_frames_match_the_reference_digests(ctx, fx, dev):
    """4096x4096 and 1080x1920 seeded noise at med and best: coefficients and stream against the digests the generator took from the
    reference (same three steps as the small cases)."""
    npz, man = fx
    L = N.load()
    large = man["large"]
    for key in ("rand4096_4096x4096_med", "rand4096_4096x4096_best", "rand1080_1080x1920_med", "rand1080_1080x1920_best"):
        assert key in large, "fixture digest missing: " + key
        m = large[key]
        img = rand_frame(m["seed"], m["h"], m["w"])
        zz = T.dctq_scaled(img, m["setting"], ctx=ctx)
        assert sha(zz) == m["zz_sha256"], key
        bs = T.compress_scaled(img, m["setting"], ctx=ctx)
        assert len(bs) == m["bytes"] == 16 + m["payload_bits"] // 8 + 1 and sha(np.frombuffer(bs, np.uint8)) == m["sha256"], key
        # resident: exactly the coefficient bytes are written, and the same stream comes out
        h, w, qf = m["h"], m["w"], SETTINGS.index(m["setting"])
        d_img = dev.upload(img)
        d_zz = dev.alloc(h * w * 2 + 4096, fill=0x5A)
        ctx.check(L.tic_dctq_scaled_dev(ctx.handle, d_img, h, w, w, qf, d_zz))
        ctx.check(L.tic_sync(ctx.handle))
        assert sha(dev.download(d_zz, h * w * 2)) == m["zz_sha256"] and (dev.download(d_zz, 4096, offset=h * w * 2) == 0x5A).all(), key
        cap = L.tic_compress_scaled_bound(h, w)
        d_out = dev.alloc(cap)
        n = C.c_size_t()
        ctx.check(L.tic_compress_scaled_dev(ctx.handle, d_img, h, w, w, qf, d_out, cap, C.byref(n)))
        assert n.value == m["bytes"] and sha(dev.download(d_out, n.value)) == m["sha256"], key
        dev.close()


def test_round_trip_through_the_existing_decoder(ctx, fx):
    """decompress(compress_scaled(img, q)) = what the reference's decompress() made of the reference's stream; decompress_batch of the four
    Lenna streams likewise: what is written is what is read."""
    npz, man = fx
    for key, m in man["cases"].items():
        if m["h"] == 0:
            continue
        dec = T.decompress(T.compress_scaled(case_image(npz, key), m["setting"], ctx=ctx), ctx=ctx)
        assert dec.shape == (m["h"], m["w"])
        check_array(npz, man, key, "dec", "dec_sha256", dec)
    lenna = case_image(npz, "lenna512_best")
    outs = T.decompress_batch([T.compress_scaled(lenna, s, ctx=ctx) for s in SETTINGS], ctx=ctx)
    for s, o in zip(SETTINGS, outs):
        check_array(npz, man, "lenna512_" + s, "dec", "dec_sha256", o)


def test_output_buffer_is_not_overrun(ctx, fx, dev):
    """A buffer of tic_compress_scaled_bound() bytes is not written past the stream's length rounded up to the packer's 16-byte unit; a
    smaller buffer receives exactly the stream; one that is too small - by one byte, the flush byte of a byte-aligned payload included -
    is not written at all (TIC_E_SPACE)."""
    npz, man = fx
    L = N.load()
    n = C.c_size_t()
    for key in ("noise64x96_best", "aligned_best_best", "aligned_low_low", "flat8x8_med", "lenna512_med"):
        m = man["cases"][key]
        img, h, w, qf = case_image(npz, key), m["h"], m["w"], SETTINGS.index(m["setting"])
        d_img = dev.upload(img)
        bound, length = L.tic_compress_scaled_bound(h, w), m["bytes"]
        d_out = dev.alloc(bound + 4096, fill=0xA5)
        ctx.check(L.tic_compress_scaled_dev(ctx.handle, d_img, h, w, w, qf, d_out, bound, C.byref(n)))
        raw = dev.download(d_out, bound + 4096)
        assert n.value == length
        check_array(npz, man, key, "bs", "sha256", raw[:length])
        assert (raw[(length + 15) // 16 * 16:] == 0xA5).all(), key
        for cap in (length, length + 5):  # smaller than the bound: exactly the stream
            ctx.check(L.tic_memset_dev(ctx.handle, d_out, 0xA5, bound + 4096))
            ctx.check(L.tic_compress_scaled_dev(ctx.handle, d_img, h, w, w, qf, d_out, cap, C.byref(n)))
            raw = dev.download(d_out, bound + 4096)
            assert n.value == length and (raw[length:] == 0xA5).all(), (key, cap)
            check_array(npz, man, key, "bs", "sha256", raw[:length])
        for cap in (length - 1, 17):
            if cap >= length:
                continue
            ctx.check(L.tic_memset_dev(ctx.handle, d_out, 0xA5, bound + 4096))
            assert L.tic_compress_scaled_dev(ctx.handle, d_img, h, w, w, qf, d_out, cap, C.byref(n)) == N.TIC_E_SPACE, (key, cap)
            assert (dev.download(d_out, bound + 4096) == 0xA5).all(), (key, cap)
        host = np.full(length + 64, 0xA5, np.uint8)  # host buffers: the same two rules
        assert L.tic_compress_scaled(ctx.handle, np.ascontiguousarray(img).ctypes.data, h, w, w, qf, host.ctypes.data, length - 1, C.byref(n)) == N.TIC_E_SPACE
        assert (host == 0xA5).all()
        ctx.check(L.tic_compress_scaled(ctx.handle, np.ascontiguousarray(img).ctypes.data, h, w, w, qf, host.ctypes.data, length, C.byref(n)))
        assert n.value == length and (host[length:] == 0xA5).all()
        dev.close()


def test_argument_errors(ctx, dev):
    L = N.load()
    img = np.zeros((16, 16), np.uint8)
    zz = np.zeros((4, 64), np.int16)
    out = np.zeros(4096, np.uint8)
    n = C.c_size_t()
    assert L.tic_dctq_scaled(ctx.handle, img.ctypes.data, 16, 12, 16, 2, zz.ctypes.data) == N.TIC_E_ARG
    assert L.tic_dctq_scaled(ctx.handle, img.ctypes.data, 9, 16, 16, 2, zz.ctypes.data) == N.TIC_E_ARG
    assert L.tic_dctq_scaled(ctx.handle, img.ctypes.data, -8, 16, 16, 2, zz.ctypes.data) == N.TIC_E_ARG
    assert L.tic_dctq_scaled(ctx.handle, img.ctypes.data, 16, 16, 8, 2, zz.ctypes.data) == N.TIC_E_ARG  # stride < w
    assert L.tic_dctq_scaled(ctx.handle, img.ctypes.data, 16, 16, 16, 4, zz.ctypes.data) == N.TIC_E_QUALITY
    assert L.tic_compress_scaled(ctx.handle, img.ctypes.data, 16, 16, 16, -1, out.ctypes.data, 4096, C.byref(n)) == N.TIC_E_QUALITY
    assert L.tic_compress_scaled(ctx.handle, img.ctypes.data, 16, 20, 20, 1, out.ctypes.data, 4096, C.byref(n)) == N.TIC_E_ARG
    d = dev.upload(img)
    d_out = dev.alloc(4096)
    assert L.tic_compress_scaled_dev(ctx.handle, d, 16, 16, 16, 7, d_out, 4096, C.byref(n)) == N.TIC_E_QUALITY
    assert L.tic_compress_scaled_dev(ctx.handle, d, 12, 16, 16, 0, d_out, 4096, C.byref(n)) == N.TIC_E_ARG
    ctx.check(L.tic_compress_scaled_dev(ctx.handle, None, 0, 0, 0, 3, d_out, 4096, C.byref(n)))
    assert n.value == 17 and dev.download(d_out, 17).tobytes().hex() == "00000000000000000300000000000040" + "00"
    for bad in (np.zeros((12, 16), np.uint8), np.zeros((16, 20), np.uint8), np.full((8, 8), 256, np.int32), np.full((8, 8), -1, np.int32)):
        with pytest.raises(ValueError):
            T.compress_scaled(bad, "med", ctx=ctx)
        with pytest.raises(ValueError):
            T.dctq_scaled(bad, "med", ctx=ctx)
    for q in ("good", 4, -1, 50, 2.0):
        with pytest.raises(ValueError):
            T.compress_scaled(img, q, ctx=ctx)
    assert T.compress_scaled(np.zeros((0, 0), np.uint8), "low", ctx=ctx).hex() == "00000000000000000300000000000040" + "00"
    assert T.compress(img, 50, ctx=ctx)[12:16] == b"\x00\x00\x00\x00"  # compress() is what it was


def test_coefficient_outside_the_tables_is_a_keyerror(ctx):
    """The sign pattern of basis function (1, 1) quantises to |AC| = 1072 / 1073 at best - category 11, where the C encoder reads past its
    table (undefined behaviour): KeyError here, as compress() raises it.  The same block compresses at high (536)."""
    yy, xx = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    f = np.cos((2 * yy + 1) * np.pi / 16) * np.cos((2 * xx + 1) * np.pi / 16)
    # (1072 for the pattern, 1073 for its inverse: the quantiser is symmetric, the >> 8 of the butterflies is not)
    for blk, top in ((np.where(f >= 0, 255, 0), 1072), (np.where(f >= 0, 0, 255), 1073)):
        img = np.tile(blk.astype(np.uint8), (2, 3))
        with pytest.raises(KeyError):
            T.compress_scaled(img, "best", ctx=ctx)
        assert np.abs(T.dctq_scaled(img, "best", ctx=ctx)[:, 1:]).max() == top
        bs = T.compress_scaled(img, "high", ctx=ctx)
        assert len(bs) > 17 and np.abs(T.dctq_scaled(img, "high", ctx=ctx)[:, 1:]).max() == 536
        assert bs == T.entropy_encode_scaled(T.dctq_scaled(img, "high", ctx=ctx), 16, 24, "high")


def test_cli_scaled(ctx, fx, tmp_path, capsys):
    """encode_cli --scaled med: the reference's stream for Lenna and the two lines encode.py prints."""
    npz, man = fx
    from tinyimgcodec_amd import encode_cli as cli

    src, dst = tmp_path / "lenna.npy", tmp_path / "out.img"
    np.save(src, np.load(os.path.join(GOLDEN, "lenna.npz"))["img"])
    assert cli.main([str(src), str(dst), "--scaled", "med"]) == 0
    out = capsys.readouterr().out.splitlines()
    n = man["cases"]["lenna512_med"]["bytes"]
    assert out[0] == f"{n} bytes" and out[1] == f"Compression Ratio: {512 * 512 / n}:1"
    assert dst.read_bytes() == npz["lenna512_med_bs"].tobytes()
