"""The device decoder of per-image Huffman table streams (tic_adaptive_dec_gpu.hip) behind decompress_adaptive() and
tic_decompress_adaptive_dev: which streams it takes (tic_last_decode_path), that its pixels are the fixtures' (the reference's
decode(encode()), tests/golden/adaptive_streams.json and benchmark_set.json), and that damaged streams end as they do in the host decoder."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

from adaptive_tables import longcode_coeffs  # the synthetic coefficients of make_goldens_adaptive.py (checked by the fixture's sha256)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
pytestmark = pytest.mark.gpu


def sha(b):
    return hashlib.sha256(b).hexdigest()


def px_sha(a):
    return sha(np.ascontiguousarray(a).tobytes())


def rand_frame(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def hard_frame(h, w):
    by, bx = np.indices(((h + 7) // 8, (w + 7) // 8))
    blocks = np.where((by + bx) % 2 == 0, 0, 255).astype(np.uint8)
    return np.kron(blocks, np.ones((8, 8), np.uint8))[:h, :w]


def case_image(name, h, w):
    """The frames of tests/golden/gen/make_goldens_adaptive.py (checked by the fixtures' stream sha256)."""
    if name.startswith("small_"):
        return rand_frame(7 * h + w, h, w)
    if name.startswith("ragged_"):
        return rand_frame(100 + int(name.split("_")[1]), h, w)
    if name == "flat":
        return np.full((h, w), 128, np.uint8)
    if name == "noise":
        return rand_frame(42, h, w)
    if name.startswith("hard_"):
        return hard_frame(h, w)
    if name == "frame_1080p":
        return rand_frame(1234, h, w)
    raise KeyError(name)


def table_counts(stream):
    """(DC entries, AC entries) of the embedded table, read from the stream itself (write_huffman_table, codec.py:73-84)."""
    bits = "".join(format(x, "08b") for x in stream[: 16 + 2700])
    p = 128
    ndc = int(bits[p : p + 16], 2)
    p += 16
    for _ in range(ndc):
        p += 8 + int(bits[p + 4 : p + 8], 2)
    return ndc, int(bits[p : p + 16], 2)


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(GOLDEN, "adaptive_streams.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(0)
    yield c
    c.close()


def path_of(ctx):
    L = N.load()
    return L.tic_last_decode_path(ctx.handle), L.tic_last_decode_giveup(ctx.handle)


def frame_1080p(fx, ctx):
    e = next(c for c in fx["cases"] if c["name"] == "frame_1080p")
    assert (e["height"] + 7) // 8 * ((e["width"] + 7) // 8) == 32400 and e["bytes"] == 865763  # 135 x 240 blocks
    s = T.compress_adaptive(case_image(e["name"], e["height"], e["width"]), e["quality"], ctx=ctx)
    assert len(s) == e["bytes"] and sha(s) == e["sha256"]
    return e, s


def test_frame_1080p_on_the_device(fx):
    """A stream of 32,400 blocks is decoded by the device decoder - in whichever build this process has loaded.  (The parent commit's
    host decoder leaves tic_last_decode_path at 0.)"""
    c = T.Context(0)  # fresh: no earlier call's path
    try:
        e, s = frame_1080p(fx, c)
        assert path_of(c)[0] == 0
        px = T.decompress_adaptive(s, ctx=c)
        print("path, giveup:", path_of(c))
        assert px_sha(px) == e["decoded_sha256"]
        assert path_of(c) == (1, 0)
    finally:
        c.close()


def test_frame_1080p_on_the_device_in_the_shipped_library():
    """... once more in a fresh process that loads the library that ships (TIC_TEST_HOOKS=0: no hooks compiled in)."""
    assert os.environ.get("TIC_TEST_HOOKS") == "1" and N.load().tic_build_has_test_hooks() == 1
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("TIC_")}
    env["TIC_TEST_HOOKS"] = "0"
    code = ("import sys; sys.path.insert(0, %r); import tinyimgcodec_amd._native as N; assert N.load().tic_build_has_test_hooks() == 0; "
            "import pytest; sys.exit(pytest.main([%r, '-m', 'gpu', '-q', '-x', '-s', '-p', 'no:cacheprovider', '-k', "
            "'test_frame_1080p_on_the_device and not shipped']))" % (root, os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=root)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0 and "1 passed" in r.stdout and "failed" not in r.stdout, tail


def test_long_codes_on_the_device(fx, ctx):
    """146,579 blocks, codes of 29 bits (44 with their value bits): far behind the 11-bit primary table, blocks longer than a range."""
    e = fx["longcode"]
    zz = longcode_coeffs()
    assert zz.shape[0] == 146579 and sha(np.ascontiguousarray(zz.astype("<i2")).tobytes()) == e["coeffs_sha256"]
    s = T.entropy_encode_adaptive(zz, e["height"], e["width"], e["quality"], ctx=ctx)
    assert len(s) == e["bytes"] and sha(s) == e["sha256"]
    px = T.decompress_adaptive(s, ctx=ctx)
    print("path, giveup:", path_of(ctx))
    assert path_of(ctx) == (1, 0)
    dc = zz[:, 0].astype(np.int32)
    dc[1:] = np.diff(dc)
    want = T.decode({"height": e["height"], "width": e["width"], "quality": e["quality"], "scaled_dct": False, "dc": dc,
                     "ac": zz[:, 1:].astype(np.int32)}, ctx=ctx)
    assert np.array_equal(px, want)


@pytest.mark.parametrize("q", [5, 50, 90])
@pytest.mark.parametrize("shape", [(4096, 4096), (1501, 1403)])
def test_large_frames(ctx, shape, q):
    """Noise at 4096^2 and a ragged frame of 188 x 176 = 33,088 blocks whose sides are no multiples of 8."""
    h, w = shape
    assert (h + 7) // 8 * ((w + 7) // 8) >= 16384
    img = rand_frame(h + q, h, w)
    s = T.compress_adaptive(img, q, ctx=ctx)
    px = T.decompress_adaptive(s, ctx=ctx)
    print("path, giveup:", path_of(ctx))
    assert path_of(ctx) == (1, 0)
    assert np.array_equal(px, T.decode(dict(T.encode(img, q, ctx=ctx), scaled_dct=False), ctx=ctx))


def test_small_streams_through_the_device_decoder(fx, ctx, monkeypatch):
    """Every stream of the fixtures with the device decoder's lower bounds moved out of the way: all 294 benchmark pairs and every
    case.  The device takes every stream whose table has at least two DC and two AC entries (counted in the stream itself); a
    one-entry table is a zero-length code - the one-block and the flat frames - and goes to the host."""
    assert N.load().tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_DECODE_MIN_BLOCKS", "1")
    monkeypatch.setenv("TIC_DECODE_MIN_BITS", "0")
    pixels = np.load(os.path.join(GOLDEN, "benchmark_set.npz"))["pixels"]
    with open(os.path.join(GOLDEN, "benchmark_set.json")) as f:
        decoded = {(e["image"], e["quality"]): e["decoded_sha256"] for e in json.load(f)["entries"]}
    assert len(fx["benchmark"]) == 294
    jobs = [((e["image"], e["quality"]), pixels[e["image"] - 1], e, decoded[(e["image"], e["quality"])]) for e in fx["benchmark"]]
    jobs += [(e["name"], case_image(e["name"], e["height"], e["width"]), e, e["decoded_sha256"]) for e in fx["cases"]]
    host = []
    for name, img, e, want in jobs:
        s = T.compress_adaptive(img, e["quality"], ctx=ctx)
        assert len(s) == e["bytes"] and sha(s) == e["sha256"], name
        px = T.decompress_adaptive(s, ctx=ctx)
        ndc, nac = table_counts(s)
        path, giveup = path_of(ctx)
        if path != 1:
            host.append((name, ndc, nac, path, giveup))
        assert px_sha(px) == want, name
        assert (path, giveup) == ((1, 0) if ndc >= 2 and nac >= 2 else (2, 0)), (name, ndc, nac, path, giveup)
    print("host decoder:", host)
    assert all(isinstance(name, str) for name, *_ in host)  # no benchmark stream is exempt


def damaged(s):
    """(label, stream) of the damage list: cuts, a bit flipped in the table, bits flipped in the payload, garbage behind the end."""
    out = [("cut %d" % c, s[:c]) for c in np.linspace(16, len(s) - 1, 10).astype(int)]
    ndc, nac = table_counts(s)
    assert ndc >= 2 and nac >= 2
    b = bytearray(s)
    b[40] ^= 0x10  # (the table of a noise frame is some hundred bytes long)
    out.append(("table bit", bytes(b)))
    rng = np.random.default_rng(2024)
    for _ in range(20):
        pos = int(rng.integers(len(s) * 8 // 4, len(s) * 8 * 3 // 4))
        b = bytearray(s)
        b[pos >> 3] ^= 0x80 >> (pos & 7)
        out.append(("payload bit %d" % pos, bytes(b)))
    out.append(("garbage", s + rng.integers(0, 256, 1000, dtype=np.uint8).tobytes()))
    return out


def outcome(stream, ctx):
    try:
        return px_sha(T.decompress_adaptive(stream, ctx=ctx))
    except ValueError:
        return "ValueError"


def test_strictness_is_the_host_decoders(fx, ctx, monkeypatch):
    """Damaged 1080p streams: pixels or ValueError exactly as under TIC_DECODE_HOST=1, the host's bit-serial decoder."""
    assert N.load().tic_build_has_test_hooks() == 1
    e, s = frame_1080p(fx, ctx)
    jobs = damaged(s)
    got, paths = [], []
    for label, d in jobs:
        got.append(outcome(d, ctx))
        paths.append(path_of(ctx))
        print(label, got[-1][:12], paths[-1])
    # both routes are taken: streams the device decoder decodes, and streams it gives up on (not only tables the host refuses)
    flips = [(g, p) for (label, _), g, p in zip(jobs, got, paths) if label.startswith("payload bit")]
    assert any(p == (1, 0) and g != "ValueError" for g, p in flips)
    cuts = [p for (label, _), p in zip(jobs, paths) if label.startswith("cut") and int(label.split()[1]) > 16 + 2700]
    assert cuts and all(p[0] == 2 and p[1] != 0 for p in cuts)
    monkeypatch.setenv("TIC_DECODE_HOST", "1")
    assert outcome(s, ctx) == e["decoded_sha256"] and path_of(ctx) == (2, 0)
    for (label, d), g in zip(jobs, got):
        assert outcome(d, ctx) == g, label
    monkeypatch.delenv("TIC_DECODE_HOST")
    assert got[-1] == e["decoded_sha256"]  # bits behind block N are ignored
    assert sum(g == "ValueError" for g in got) >= 10  # every cut at least
    with pytest.raises(ValueError):  # a default-table stream carries no table
        T.decompress_adaptive(T.compress(case_image("frame_1080p", 1080, 1920), 50, ctx=ctx), ctx=ctx)


def resident_window(ctx, s, h, w, want, stride, x0):
    L = N.load()
    rows, y0 = h + 9, 5
    d_s, d_o = C.c_void_p(), C.c_void_p()
    ctx.check(L.tic_dev_alloc(ctx.handle, len(s), C.byref(d_s)))
    ctx.check(L.tic_dev_alloc(ctx.handle, rows * stride, C.byref(d_o)))
    try:
        buf = np.frombuffer(s, np.uint8)
        ctx.check(L.tic_memcpy_h2d(ctx.handle, d_s, buf.ctypes.data, buf.size))
        win = C.c_void_p(d_o.value + y0 * stride + x0)
        cap = (h - 1) * stride + w
        surface = np.empty((rows, stride), np.uint8)
        for short in (1, 0):
            hh, ww = C.c_int(-1), C.c_int(-1)
            ctx.check(L.tic_memset_dev(ctx.handle, d_o, 0xA5, rows * stride))
            rc = L.tic_decompress_adaptive_dev(ctx.handle, d_s, len(s), win, stride, cap - short, C.byref(hh), C.byref(ww))
            ctx.check(L.tic_memcpy_d2h(ctx.handle, surface.ctypes.data, d_o, surface.size))
            assert (hh.value, ww.value) == (h, w)
            if short:
                assert rc == N.TIC_E_SPACE and (surface == 0xA5).all()
                continue
            ctx.check(rc)
            assert path_of(ctx) == (1, 0)
            assert np.array_equal(surface[y0 : y0 + h, x0 : x0 + w], want)
            surface[y0 : y0 + h, x0 : x0 + w] = 0xA5
            assert (surface == 0xA5).all()
    finally:
        ctx.check(L.tic_dev_free(ctx.handle, d_s))
        ctx.check(L.tic_dev_free(ctx.handle, d_o))


def test_resident_entry_point(fx, ctx):
    """tic_decompress_adaptive_dev into a window of a larger device surface with a stride above the width: the window is the image,
    every other byte keeps the sentinel, *h / *w are the header's, and a capacity one byte short gives TIC_E_SPACE with nothing
    written.  The 1080p fixture frame (the pixels of test_frame_1080p_on_the_device), and a frame whose width is no multiple of 8;
    rows the kernel stores directly (8-byte aligned) and rows that go through the pitched copy."""
    e, s = frame_1080p(fx, ctx)
    want = T.decompress_adaptive(s, ctx=ctx)
    assert px_sha(want) == e["decoded_sha256"]
    resident_window(ctx, s, e["height"], e["width"], want, 2048, 64)
    resident_window(ctx, s, e["height"], e["width"], want, 1923, 3)
    h, w = 1083, 1925  # 136 x 241 = 32,776 blocks
    img = rand_frame(77, h, w)
    s = T.compress_adaptive(img, 50, ctx=ctx)
    want = T.decode(dict(T.encode(img, 50, ctx=ctx), scaled_dct=False), ctx=ctx)
    resident_window(ctx, s, h, w, want, 2048, 64)
    resident_window(ctx, s, h, w, want, 1931, 3)
