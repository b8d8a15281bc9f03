"""encode() / compress() of integer images outside 0..255 on the MI355X: dctq_exact_wide_kernel and tic_encode_wide on the corpus of
tests/wide_blocks.py (its docstring names the families), the routing of tinyimgcodec_amd/codec.py in front of them and the host coder
behind them.  Every comparison is array_equal or a byte identity, and the expectation is always a fixture written by the unmodified
reference (tests/golden/wide_blocks.npz, and for 8-bit content transform_small / tie_blocks / near_ties / decode_small) - never another
GPU result; the oracle is not asked.  tests/test_wide_blocks_cpu.py shows that the corpus tells the mutants of the transform apart."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

import wide_blocks as WB

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A  # one block (64 values) of it behind each output array


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(0)
    assert c.arch.startswith("gfx950"), c.arch
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return WB.Fixture()


def encode_wide(ctx, img, quality, pad=0):
    """tic_encode_wide through ctypes -> (dc, ac).  pad: the rows lie w + pad elements apart, the padding full of INT32_MAX, so that a load
    past a row's end shows in the coefficients.  A non-integral quality goes through tic_set_custom_quality + TIC_QUALITY_CUSTOM.  Both
    output arrays have a block of SENTINEL behind them, which must be intact afterwards."""
    L = N.load()
    img = np.asarray(img)
    assert img.dtype == np.int32
    h, w = img.shape
    buf = np.full((h, w + pad), WB.I32_MAX, np.int32)
    buf[:, :w] = img
    n = L.tic_num_blocks(h, w)
    dc = np.full(n + 64, SENTINEL, np.int32)
    ac = np.full(n * 63 + 64, SENTINEL, np.int32)
    if isinstance(quality, float):
        ctx.check(L.tic_set_custom_quality(ctx.handle, quality))
        quality = N.QUALITY_CUSTOM
    ctx.check(L.tic_encode_wide(ctx.handle, buf.ctypes.data, h, w, w + pad, quality, dc.ctypes.data, ac.ctypes.data))
    assert (dc[n:] == SENTINEL).all() and (ac[n * 63:] == SENTINEL).all(), "a write behind the output arrays"
    assert (buf[:, w:] == WB.I32_MAX).all() and np.array_equal(buf[:, :w], img)
    return dc[:n].copy(), ac[: n * 63].reshape(n, 63).copy()


def check_frames(ctx, fx, names, pads=(0,)):
    bad = []
    for name in names:
        f = WB.frames()[name]
        for pad in pads:
            dc, ac = encode_wide(ctx, f.img, f.quality, pad)
            diff = WB.first_difference(dc, ac, fx.dc(name), fx.ac(name))
            if diff:
                bad.append("%s (row stride w + %d): %s" % (name, pad, diff))
    assert not bad, "%d of %d differ from the reference:\n%s" % (len(bad), len(names) * len(pads), "\n".join(bad[:40]))


@pytest.mark.parametrize("family", WB.FAMILIES)
def test_every_frame_contiguous_and_strided(ctx, fx, family):
    """Every frame of the family: contiguous, and with rows w + 3 and w + 8 elements apart."""
    names = fx.names(family)
    assert names
    check_frames(ctx, fx, names, pads=(0, 3, 8))


def test_an_integer_quality_after_a_float_quality(ctx, fx):
    """The custom slot and the integer slots are different constants: 33.3, then 50 (must not be 33.3's), then TIC_QUALITY_CUSTOM again
    without setting it anew (still 33.3), 98.5, 90, and 10 on another frame."""
    L = N.load()
    img = WB.frames()["geo_9x65_q50"].img
    for name in ("fq_geo_9x65_q33p3", "geo_9x65_q50"):
        dc, ac = encode_wide(ctx, img, WB.frames()[name].quality)
        assert WB.first_difference(dc, ac, fx.dc(name), fx.ac(name)) is None, name
    n = L.tic_num_blocks(*img.shape)
    dc, ac = np.zeros(n, np.int32), np.zeros((n, 63), np.int32)
    ctx.check(L.tic_encode_wide(ctx.handle, img.ctypes.data, img.shape[0], img.shape[1], img.shape[1], N.QUALITY_CUSTOM, dc.ctypes.data, ac.ctypes.data))
    assert WB.first_difference(dc, ac, fx.dc("fq_geo_9x65_q33p3"), fx.ac("fq_geo_9x65_q33p3")) is None
    check_frames(ctx, fx, ["fq_geo_9x65_q98p5", "geo_9x65_q90", "fq_mag_k16_sym_q1p5", "geo_72x136_q10", "fq_mag_k16_sym_q71p9", "geo_9x65_q50"])


def test_8bit_fixtures_through_the_wide_entry(ctx):
    """The images of transform_small, tie_blocks and near_ties, widened to int32, through tic_encode_wide: those fixtures' dc / ac - the
    exact-order kernel's int32 instance on the ties that pin the 8-bit kernels."""
    cases = []
    d = np.load(os.path.join(GOLDEN, "transform_small.npz"))
    for key in d["names"]:
        cases.append((str(key), d[key + "_img"], int(str(key).rsplit("_q", 1)[1]), d[key + "_dc"], d[key + "_ac"]))
    d = np.load(os.path.join(GOLDEN, "tie_blocks.npz"))
    cases.append(("tie_blocks", d["img"], 50, d["dc"], d["ac"]))
    d = np.load(os.path.join(GOLDEN, "near_ties.npz"))
    cases += [("near_ties q%d" % q, d["img"], q, d["q%d_dc" % q], d["q%d_ac" % q]) for q in (50, 90, 10, 37)]
    assert len(cases) >= 60
    bad = []
    for name, img, q, want_dc, want_ac in cases:
        for pad in (0, 5):
            dc, ac = encode_wide(ctx, img.astype(np.int32), q, pad)
            diff = WB.first_difference(dc, ac, want_dc, want_ac)
            if diff:
                bad.append("%s (w + %d): %s" % (name, pad, diff))
    assert not bad, "\n".join(bad[:40])


# ---- routing ------------------------------------------------------------------------------------------------------------------------

def check_encode(ctx, fx, name, image, quality=None):
    want_q = WB.frames()[name].quality if quality is None else quality
    info = T.encode(image, want_q, ctx=ctx)
    h, w = WB.frames()[name].img.shape
    assert (info["height"], info["width"]) == (h, w) and info["quality"] == want_q and type(info["quality"]) is type(want_q), name
    assert info["dc"].dtype == np.int32 and info["ac"].dtype == np.int32 and info["ac"].shape == (len(info["dc"]), 63), name
    diff = WB.first_difference(info["dc"], info["ac"], fx.dc(name), fx.ac(name))
    assert diff is None, "%s as %s: %s" % (name, getattr(image, "dtype", type(image).__name__), diff)


def with_fractions(img, seed):
    """float64 whose truncation toward zero is img: a fraction of the value's own sign (of either sign at 0) added to every pixel."""
    frac = np.random.default_rng(seed).uniform(0.01, 0.99, img.shape)
    sign = np.where(img > 0, 1.0, np.where(img < 0, -1.0, np.where(frac > 0.5, 1.0, -1.0)))
    out = img.astype(np.float64) + sign * frac
    assert np.array_equal(out.astype(np.int32), img) and (out != img).all()
    return out


def test_encode_routes_by_value_not_by_dtype(ctx, fx):
    """The same values as int8, int16, uint16, int32, int64, float64 with fractions of both signs (astype(int32) truncates toward zero) and
    a list of lists; F-ordered and strided views; the frame that is 0..255 but for its LAST pixel (256, -1: wide; 255, 0: the 8-bit path,
    whose result the reference's encode() of that frame pins as well)."""
    signed, unsigned = WB.frames()["rt_int8_q50"].img, WB.frames()["rt_uint16_q50"].img
    assert signed.min() < 0 and signed.min() >= -128 and signed.max() <= 127 and unsigned.min() >= 0 and unsigned.max() > 32767
    for dt in (np.int8, np.int16, np.int32, np.int64):
        check_encode(ctx, fx, "rt_int8_q50", signed.astype(dt))
    for dt in (np.uint16, np.int32, np.int64, np.uint32, np.uint64):
        check_encode(ctx, fx, "rt_uint16_q50", unsigned.astype(dt))
    for name, img in (("rt_int8_q50", signed), ("rt_uint16_q50", unsigned)):
        check_encode(ctx, fx, name, with_fractions(img, 1))
        check_encode(ctx, fx, name, with_fractions(img, 2).astype(np.float64).tolist())
        check_encode(ctx, fx, name, img.tolist())
        check_encode(ctx, fx, name, np.asfortranarray(img))
        check_encode(ctx, fx, name, np.asfortranarray(img.astype(np.int64)))
        big = np.full((img.shape[0] * 2 + 1, img.shape[1] * 3 + 2), WB.I32_MAX, np.int64)
        big[1::2, 2::3][: img.shape[0], : img.shape[1]] = img
        view = big[1::2, 2::3][: img.shape[0], : img.shape[1]]
        assert not view.flags.c_contiguous and np.array_equal(view, img)
        check_encode(ctx, fx, name, view)
        check_encode(ctx, fx, name, img[::-1, ::-1][::-1, ::-1])
        check_encode(ctx, fx, name, img.T.copy().T)
    check_encode(ctx, fx, "rt_int8_q50", signed, quality=50.0)  # an integral float: the integer's constants, the caller's number back
    check_encode(ctx, fx, "fq_geo_9x65_q33p3", WB.frames()["fq_geo_9x65_q33p3"].img.astype(np.int16))
    for tag in ("256", "m1", "255", "0"):
        name = "rt_last_%s_q50" % tag
        img = WB.frames()[name].img
        wide = tag in ("256", "m1")
        assert ((img[:-1].min() >= 0) and (img[:-1].max() <= 255) and ((img < 0) | (img > 255)).sum() == (1 if wide else 0))
        assert TC_as_image(img)[3] is wide, name
        for cast in (np.int32, np.int16, np.float64):
            check_encode(ctx, fx, name, img.astype(cast))
        if not wide:
            check_encode(ctx, fx, name, img.astype(np.uint8))


def TC_as_image(img):
    from tinyimgcodec_amd import codec

    return codec._as_image(img)


def test_the_8bit_helpers_keep_refusing_wide_input(ctx):
    img = WB.frames()["rt_last_256_q50"].img
    with pytest.raises(ValueError, match="outside 0..255"):
        T.dctq(img, 50, ctx=ctx)
    with pytest.raises(ValueError, match="outside 0..255"):
        T.compress_batch([img, img], 50, ctx=ctx)
    with pytest.raises(ValueError, match="outside 0..255"):
        T.compress_batch([WB.frames()["rt_last_255_q50"].img, img], [50, 60], ctx=ctx)
    assert T.dctq(WB.frames()["rt_last_255_q50"].img, 50, ctx=ctx).shape == (6, 64)


# ---- streams ------------------------------------------------------------------------------------------------------------------------

def test_compress_writes_the_reference_streams(ctx, fx):
    """compress() of the streams family: the reference's bytes whatever the running DC (the ramp reaches 46,000), KeyError where the
    reference raised it (a DC difference of +-2,048, an AC value of +-1,024); decompress() of every stream: the reference's pixels."""
    for name in fx.names("streams"):
        f, want = WB.frames()[name], fx.stream(name)
        if want == "KeyError":
            with pytest.raises(KeyError):
                T.compress(f.img, f.quality, ctx=ctx)
            continue
        got = T.compress(f.img, f.quality, ctx=ctx)
        assert got == want, "%s: %d bytes, want %d" % (name, len(got), len(want))
        assert got == T.compress(f.img.astype(np.int64), f.quality, ctx=ctx) == T.compress(f.img.tolist(), f.quality, ctx=ctx)
        dec = T.decompress(want, ctx=ctx)
        assert dec.dtype == np.uint8 and np.array_equal(dec, fx.decompressed(name)), name
    assert len(fx.stream("str_ramp_q50")) == 86
    # frames that have no stream for other reasons keep raising KeyError, with no word about int16
    for name in ("geo_9x65_q50", "mag_k31_sym_q10", WB.PAIR_FRAME):
        with pytest.raises(KeyError):
            T.compress(WB.frames()[name].img, WB.frames()[name].quality, ctx=ctx)


def test_decode_of_encode_equals_the_reference(ctx, fx):
    for name in WB.DECODE_FRAMES:
        f = WB.frames()[name]
        info = T.encode(f.img, f.quality, ctx=ctx)
        assert WB.first_difference(info["dc"], info["ac"], fx.dc(name), fx.ac(name)) is None, name
        info["scaled_dct"] = False
        pix = T.decode(info, ctx=ctx)
        assert pix.dtype == np.uint8 and np.array_equal(pix, fx.decoded(name)), name


# ---- one context as state -----------------------------------------------------------------------------------------------------------

def neighbours(ctx):
    """tic_compress, tic_dctq and tic_decompress calls of three other geometries, each against transform_small / decode_small."""
    s, d = np.load(os.path.join(GOLDEN, "transform_small.npz")), np.load(os.path.join(GOLDEN, "decode_small.npz"))
    for key in ("rand_24x40_q50", "rand_15x17_q90", "rand_64x7_q10"):
        img, q, bs = s[key + "_img"], int(key.rsplit("_q", 1)[1]), s[key + "_bs"].tobytes()
        yield key + " compress", lambda: T.compress(img, q, ctx=ctx) == bs
        zz_dc, zz_ac = s[key + "_dc"], s[key + "_ac"]

        def dctq_ok(img=img, q=q, zz_dc=zz_dc, zz_ac=zz_ac):
            zz = T.dctq(img, q, ctx=ctx).astype(np.int32)
            dc = zz[:, 0].copy()
            dc[1:] = np.diff(zz[:, 0])
            return np.array_equal(dc, zz_dc) and np.array_equal(zz[:, 1:], zz_ac)

        yield key + " dctq", dctq_ok
        yield key + " decompress", lambda: np.array_equal(T.decompress(bs, ctx=ctx), d[key])


WIDE_BETWEEN = ("geo_72x136_q50", "geo_2x3_q90", "ext_flat_min_q10", "geo_40x200_q10", "ref_3x4_q50", "mag_k31_sym_q10", "str_ramp_q50", "geo_264x8_q90",
                "tie_00_q50")


def interleave(ctx, fx):
    """A wide call (d_img as int32, d_coef as 256 bytes per block) between the 8-bit calls, which use the same two buffers as bytes and as
    128 bytes per block; sizes go up and down.  Every result stays exact."""
    wide = list(WIDE_BETWEEN)
    bad, k = [], 0
    for rounds in range(2):
        for what, ok in neighbours(ctx):
            if not ok():
                bad.append("%s (round %d)" % (what, rounds))
            name = wide[k % len(wide)]
            k += 1
            f = WB.frames()[name]
            dc, ac = encode_wide(ctx, f.img, f.quality, pad=k % 3)
            diff = WB.first_difference(dc, ac, fx.dc(name), fx.ac(name))
            if diff:
                bad.append("%s after %s: %s" % (name, what, diff))
    want = fx.stream("str_ramp_q50")
    if T.compress(WB.frames()["str_ramp_q50"].img, 50, ctx=ctx) != want:
        bad.append("compress of the ramp at the end")
    assert not bad, "\n".join(bad)
    assert k >= 2 * len(wide)


def test_wide_calls_between_other_calls_on_one_context(ctx, fx):
    interleave(ctx, fx)


@pytest.mark.parametrize("byte", (0x00, 0xA5, 0xFF), ids=lambda b: "0x%02X" % b)
def test_wide_calls_on_a_poisoned_context(fx, monkeypatch, byte):
    """The same on a fresh context under TIC_POISON: every buffer is first used, and grows, out of a poisoned allocation."""
    assert N.load().tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_POISON", "0x%02X" % byte)
    c = T.Context(0)
    try:
        interleave(c, fx)
    finally:
        c.close()


# ---- the library that ships -----------------------------------------------------------------------------------------------------------

def test_geometry_and_extremes_on_the_shipped_library():
    """The geometry and extremes families, the streams and the routing frames once more in a fresh process that loads the library that
    ships (no test hooks, no TIC_* variable), through the package's encode() / compress()."""
    code = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N
import wide_blocks as WB
assert N.load().tic_build_has_test_hooks() == 0 and N._lib_path() == N.LIB_PATH
fx = WB.Fixture()
bad, count = [], 0
for family in ("geometry", "extremes", "routing", "floatq"):
    for name in fx.names(family):
        f = WB.frames()[name]
        info = T.encode(f.img, f.quality)
        diff = WB.first_difference(info["dc"], info["ac"], fx.dc(name), fx.ac(name))
        count += 1
        if diff:
            bad.append("%s: %s" % (name, diff))
for name in fx.names("streams"):
    f, want = WB.frames()[name], fx.stream(name)
    try:
        got = T.compress(f.img, f.quality)
    except KeyError:
        got = "KeyError"
    count += 1
    if got != want:
        bad.append("%s: stream differs" % name)
assert not bad, "\n".join(bad)
print("wide blocks on the shipped library ok: %d frames" % count)
'''
    env = {k: v for k, v in os.environ.items() if not k.startswith("TIC_")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "wide blocks on the shipped library ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
