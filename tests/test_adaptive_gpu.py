"""Per-image Huffman tables on the MI355X: compress_adaptive / entropy_encode_adaptive / decompress_adaptive against the unmodified
reference's compress(..., auto_generate_huffman_table=True) (tests/golden/adaptive_streams.json, made by
tests/golden/gen/make_goldens_adaptive.py; the frames are rebuilt here by the same recipes)."""
import ctypes as C
import hashlib
import json
import os
import struct

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


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(GOLDEN, "adaptive_streams.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(0)
    yield c
    c.close()


def check_stream(out, e):
    assert len(out) == e["bytes"]
    if "stream" in e:
        assert out.hex() == e["stream"]
    assert sha(out) == e["sha256"]


def test_cases_byte_exact_and_round_trip(fx, ctx):
    for e in fx["cases"]:
        img = case_image(e["name"], e["height"], e["width"])
        out = T.compress_adaptive(img, e["quality"], ctx=ctx)
        check_stream(out, e)
        assert px_sha(T.decompress_adaptive(out, ctx=ctx)) == e["decoded_sha256"], e["name"]
        assert px_sha(T.decompress(out, ctx=ctx)) == e["garbage_sha256"], e["name"]  # decompress() keeps the reference's misreading


def test_flat_frame_stream(ctx):
    out = T.compress_adaptive(np.full((32, 32), 128, np.uint8), 50, ctx=ctx)
    # header, flag 80 00 00 00, one DC and one AC entry of length 0 each, empty payload
    assert out.hex() == "20000000" "20000000" "32000000" "80000000" "0001" "00" "0001" "0000"


def test_hard_frames_beyond_the_default_table(fx, ctx):
    """DC categories 12-13: compress() has no code for them (KeyError), the adaptive stream does, and it decodes to decode(encode())."""
    for e in fx["cases"]:
        if not e["name"].startswith("hard_"):
            continue
        img = hard_frame(e["height"], e["width"])
        with pytest.raises(KeyError):
            T.compress(img, e["quality"], ctx=ctx)
        out = T.compress_adaptive(img, e["quality"], ctx=ctx)
        check_stream(out, e)
        px = T.decompress_adaptive(out, ctx=ctx)
        assert np.array_equal(px, T.decode(dict(T.encode(img, e["quality"], ctx=ctx), scaled_dct=False), ctx=ctx))


def test_benchmark_set(fx, ctx):
    pixels = np.load(os.path.join(GOLDEN, "benchmark_set.npz"))["pixels"]
    with open(os.path.join(GOLDEN, "benchmark_set.json")) as f:
        decoded = {(e["image"], e["quality"]): e["decoded_sha256"] for e in json.load(f)["entries"]}
    assert len(fx["benchmark"]) == 294
    for e in fx["benchmark"]:
        out = T.compress_adaptive(pixels[e["image"] - 1], e["quality"], ctx=ctx)
        check_stream(out, e)
        assert px_sha(T.decompress_adaptive(out, ctx=ctx)) == decoded[(e["image"], e["quality"])], (e["image"], e["quality"])
        assert px_sha(T.decompress(out, ctx=ctx)) == e["garbage_sha256"], (e["image"], e["quality"])


def test_long_codes(fx, ctx):
    """Codes of 29 bits, 44 with their value bits: the wide-code packing and the host decoder."""
    e = fx["longcode"]
    zz = longcode_coeffs()
    assert sha(np.ascontiguousarray(zz.astype("<i2")).tobytes()) == e["coeffs_sha256"]
    out = T.entropy_encode_adaptive(zz, e["height"], e["width"], e["quality"], ctx=ctx)
    assert len(out) == e["bytes"] and out[:64].hex() == e["head"] and sha(out) == e["sha256"]
    px = T.decompress_adaptive(out, ctx=ctx)
    dc = zz[:, 0].astype(np.int32)
    dc[1:] = np.diff(dc)
    want = T.decode({"height": e["height"], "width": e["width"], "quality": e["quality"], "scaled_dct": False, "dc": dc,
                     "ac": zz[:, 1:].astype(np.int32)}, ctx=ctx)
    assert np.array_equal(px, want)


def test_input_errors(ctx):
    img = rand_frame(3, 16, 16)
    for shape in ((0, 0), (0, 8), (8, 0)):
        with pytest.raises(IndexError):
            T.compress_adaptive(np.zeros(shape, np.uint8), 50, ctx=ctx)
    with pytest.raises(ZeroDivisionError):
        T.compress_adaptive(img, 0, ctx=ctx)
    with pytest.raises(KeyError):
        T.compress_adaptive(img, 100, ctx=ctx)
    with pytest.raises(ValueError):
        T.compress_adaptive(img, 101, ctx=ctx)
    with pytest.raises(struct.error):
        T.compress_adaptive(img, 50.0, ctx=ctx)
    with pytest.raises(struct.error):
        T.compress_adaptive(img, -5, ctx=ctx)
    with pytest.raises(ValueError):
        T.compress_adaptive(np.full((8, 8), 300, np.int32), 50, ctx=ctx)  # 8-bit pixels only
    with pytest.raises(ValueError):
        T.compress_adaptive(np.zeros((8, 8, 3), np.uint8), 50, ctx=ctx)
    with pytest.raises(NotImplementedError):
        T.compress(img, 50, auto_generate_huffman_table=True, ctx=ctx)
    zz = np.zeros((1, 64), np.int16)
    zz[0, 0] = -32768  # DC category 16: write_huffman_table has 4 bits for it
    with pytest.raises(OverflowError):
        T.entropy_encode_adaptive(zz, 8, 8, 50, ctx=ctx)


def test_cap_too_small_writes_nothing(ctx):
    L = N.load()
    img = rand_frame(9, 40, 56)
    want = T.compress_adaptive(img, 75, ctx=ctx)
    for cap in (0, 16, len(want) - 1, len(want)):
        buf = np.full(len(want) + 64, 0xAB, np.uint8)
        n = C.c_size_t(0)
        rc = L.tic_compress_adaptive(ctx.handle, img.ctypes.data, 40, 56, 56, 75, buf.ctypes.data, cap, C.byref(n))
        if cap < len(want):
            assert rc == N.TIC_E_SPACE and n.value == len(want)
            assert (buf == 0xAB).all()  # nothing written
        else:
            assert rc == N.TIC_OK and n.value == len(want)
            assert buf[: len(want)].tobytes() == want and (buf[len(want):] == 0xAB).all()


def test_decompress_adaptive_is_strict(ctx):
    img = rand_frame(11, 48, 40)
    s = T.compress_adaptive(img, 60, ctx=ctx)
    good = T.decompress_adaptive(s, ctx=ctx)
    assert np.array_equal(good, T.decompress_adaptive(bytearray(s), ctx=ctx))
    for cut in (0, 8, 15, 16, 17, 20, 40, len(s) // 2, len(s) - 1):
        with pytest.raises(ValueError):
            T.decompress_adaptive(s[:cut], ctx=ctx)
    with pytest.raises(ValueError):  # a default-table stream carries no table
        T.decompress_adaptive(T.compress(img, 60, ctx=ctx), ctx=ctx)
    bad = bytearray(s)
    bad[16:18] = b"\x00\x00"  # no DC entry
    with pytest.raises(ValueError):
        T.decompress_adaptive(bytes(bad), ctx=ctx)
    bad = bytearray(s)
    bad[16:18] = b"\x00\x11"  # 17 DC entries
    with pytest.raises(ValueError):
        T.decompress_adaptive(bytes(bad), ctx=ctx)
    # the second DC entry's codeword replaced by zeros of the same length: it then runs through the first entry's leaf (the tree's
    # leftmost, all zeros) or ends above it - a table that is no prefix code
    bits = "".join(format(x, "08b") for x in s)
    p1 = 128 + 16
    assert int(bits[p1 : p1 + 16], 2) >= 2
    len1 = int(bits[p1 + 20 : p1 + 24], 2)
    p2 = p1 + 16 + 8 + len1
    len2 = int(bits[p2 + 4 : p2 + 8], 2)
    assert "1" in bits[p2 + 8 : p2 + 8 + len2]
    bits = bits[: p2 + 8] + "0" * len2 + bits[p2 + 8 + len2 :]
    with pytest.raises(ValueError):
        T.decompress_adaptive(bytes(int(bits[i : i + 8], 2) for i in range(0, len(bits), 8)), ctx=ctx)
