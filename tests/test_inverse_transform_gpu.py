"""Both inverse transforms - idct_kernel (tic_kernels.hip) and phase 2 of the fused decode kernel (tic_entropy_dec_gpu.hip, its four
instantiations and the batch form) - on BUILT coefficients: tests/golden/inverse_edges.npz (tests/golden/gen/make_goldens_inverse.py), frames
no encoder made - pixels whose truncating cast hangs on the operation order, the largest magnitudes the tables allow, pixels on the clip's
edges, scaled_dct exponents up to 62, and a running DC that leaves int16.

Bar: every route gives oracle.decompress of the same stream (tests/test_inverse_edges_cpu.py ties that to the unmodified reference), bit for
bit; no tolerance anywhere.  Run with `-m gpu` on an MI355X."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import inverse_edges as IE

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

pytestmark = pytest.mark.gpu

with open(os.path.join(IE.GOLDEN, "inverse_edges.json")) as _f:
    _FRAMES = json.load(_f)["frames"]
STREAM_NAMES = [n for n, e in _FRAMES.items() if e["stream_sha256"] is not None]
ALL_NAMES = list(_FRAMES)
GIVEUP_WIDE_DC = 512  # include/tinyimgcodec_hip.h, tic_last_decode_giveup: a running DC outside int16
GIVEUP_DOCUMENTED = 1 | 2 | 4 | 8 | 16 | 32 | 64 | 128 | 256 | 512


def check_wide_handover(name, path, giveup):
    """A wide-DC frame leaves the device decoder for the host route with documented give-up bits.  The frames of 63 equal AC per block are
    periodic bit patterns on which the speculative walks do not fall in step (bits 4 / 16 / 32, whatever the DC does: the sums of a broken
    chain say nothing); the "varied" frames are walked to the end, and the running DC is the one thing flagged."""
    assert path == 2 and giveup != 0 and giveup & ~GIVEUP_DOCUMENTED == 0, (describe(name), path, giveup)
    if "varied" in name:
        assert giveup == GIVEUP_WIDE_DC, (describe(name), giveup)


def is_wide(name):
    return _FRAMES[name]["family"] == "wide"


@pytest.fixture(scope="module")
def fx():
    return IE.Fixture()


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(0)
    assert c.arch.startswith("gfx950"), c.arch
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases(fx, oracle):
    """name -> (stream, oracle.decompress(stream)); computed once, never modified.  The digest ties every one to the reference's pixels."""
    out = {}
    for name in STREAM_NAMES:
        e = fx.frames[name]
        dc, ac = fx.coeffs(name)
        s = IE.stream_of(oracle, dc, ac, e["height"], e["width"], e["quality"], e["flag"])
        assert IE.sha(s) == e["stream_sha256"], name
        want = oracle.decompress(s)
        assert IE.px_sha(want) == e["pixels_sha256"], name
        want.setflags(write=False)
        out[name] = (s, want)
    return out


def describe(name, stream=None):
    e = _FRAMES[name]
    bpb = e["stream_bytes"] * 8 // e["blocks"] if e["stream_bytes"] else None
    return "%s: %d x %d, quality field %r, flag %#x, %s stream bits per block (fused kernel window: %s words, kScaled %s)" % (
        name, e["height"], e["width"], e["quality"], e["flag"], bpb, None if bpb is None else (2048 if bpb <= 240 else 4096), bool(e["flag"]))


def mismatch(got, want):
    bad = np.argwhere(got != want)
    return "%d pixels differ, first at %s: got %s, want %s" % (len(bad), bad[:4].tolist(), [int(got[tuple(i)]) for i in bad[:4]], [int(want[tuple(i)]) for i in bad[:4]])


def path_of(L, handle):
    return L.tic_last_decode_path(handle), L.tic_last_decode_giveup(handle)


def range_rule(nbytes, nblocks):
    """csrc/tic_entropy_dec_gpu.h dec_range_rule: the stream bits per lane a frame asks for."""
    floor_words = 33 if nbytes * 8 < 7 * nblocks else 9
    k = ((2 * nbytes * 8) // nblocks + 31) // 32 | 1
    return min(max(k, floor_words), 63) * 32


def decompress(L, handle, s, shape):
    buf = np.frombuffer(s, np.uint8)
    out = np.full(shape, 0xA5, np.uint8)
    rc = L.tic_decompress(handle, buf.ctypes.data, buf.size, out.ctypes.data, out.size)
    assert rc == N.TIC_OK, (rc, L.tic_last_error(handle).decode())
    return out


# ---- idct_kernel, called directly -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in ALL_NAMES if not is_wide(n)])
def test_idctq_on_the_coefficients(name, fx, ctx, oracle, cases):
    """tic_idctq / tic_idctq_scaled on the int16 coefficients (a non-integral quality through tic_set_custom_quality)."""
    L = N.load()
    e = fx.frames[name]
    h, w, q = e["height"], e["width"], e["quality"]
    zz = IE.zz_absolute(*fx.coeffs(name))
    assert np.abs(zz).max() <= 32768 and zz.max() <= 32767
    zz16 = np.ascontiguousarray(zz.astype(np.int16))
    out = np.full((h, w), 0xA5, np.uint8)
    if e["flag"] & IE.SCALED:
        rc = L.tic_idctq_scaled(ctx.handle, zz16.ctypes.data, h, w, int(q), out.ctypes.data, out.size)
    elif float(q) != int(q):
        assert L.tic_set_custom_quality(ctx.handle, float(q)) == N.TIC_OK
        rc = L.tic_idctq(ctx.handle, zz16.ctypes.data, h, w, N.QUALITY_CUSTOM, out.ctypes.data, out.size)
    else:
        rc = L.tic_idctq(ctx.handle, zz16.ctypes.data, h, w, int(q), out.ctypes.data, out.size)
    assert rc == N.TIC_OK, (rc, L.tic_last_error(ctx.handle).decode())
    if name in cases:
        assert np.array_equal(out, cases[name][1]), (describe(name), mismatch(out, cases[name][1]))
    else:  # (no stream can carry this quality: the reference's decode() of the dictionary, by digest and crops)
        assert fx.matches_reference(name, out), describe(name)
        assert np.array_equal(out, IE.pixels_block_idct(fx, oracle, zz, h, w, q, e["flag"]))


@pytest.mark.parametrize("name", [n for n in ALL_NAMES if is_wide(n)])
def test_decode_refuses_a_dc_outside_int16(name, fx):
    """The int16 layout of tic_idctq cannot carry a running DC outside int16: decode() says so instead of saturating it."""
    e = fx.frames[name]
    dc, ac = fx.coeffs(name)
    with pytest.raises(ValueError):
        T.decode({"height": e["height"], "width": e["width"], "quality": e["quality"], "scaled_dct": bool(e["flag"] & IE.SCALED), "dc": dc, "ac": ac})


# ---- tic_decompress: host Huffman decoder + idct_kernel; the device decoder's fused kernel --------------------------------------------
@pytest.mark.parametrize("name", STREAM_NAMES)
def test_decompress_host_route(name, ctx, cases, monkeypatch):
    """TIC_DECODE_HOST=1 (test-hooks build): the host decoder's coefficients through idct_kernel."""
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_DECODE_HOST", "1")
    s, want = cases[name]
    out = decompress(L, ctx.handle, s, want.shape)
    assert path_of(L, ctx.handle)[0] == 2
    assert np.array_equal(out, want), (describe(name), mismatch(out, want))


def check_default_route(L, handle, name, s, want):
    out = decompress(L, handle, s, want.shape)
    path, giveup = path_of(L, handle)
    r, tries = C.c_int(), C.c_int()
    assert L.tic_last_decode_range(handle, C.byref(r), C.byref(tries)) == N.TIC_OK
    print("%s -> path %d, giveup %d, range %d bits, tries %d" % (describe(name), path, giveup, r.value, tries.value))
    if is_wide(name):  # the device decoder hands it over; the host route's inverse stage gets the int32 DC
        check_wide_handover(name, path, giveup)
    else:
        assert (path, giveup) == (1, 0), describe(name)
        if tries.value == 1:
            assert r.value == range_rule(len(s), _FRAMES[name]["blocks"]), describe(name)
    assert np.array_equal(out, want), (describe(name), mismatch(out, want))


@pytest.mark.parametrize("name", STREAM_NAMES)
def test_decompress_default_route(name, ctx, cases):
    """What tic_decompress does on its own: every frame is one the device decoder takes (>= 1,024 blocks, >= 8,192 payload bits)."""
    check_default_route(N.load(), ctx.handle, name, *cases[name])


def test_the_frames_reach_all_four_fused_kernels():
    """By the size rule of entropy_decode_idct_gpu (stream bits / blocks <= 240: the 2,048-word window), with and without the scaled branch."""
    seen = {(e["stream_bytes"] * 8 // e["blocks"] <= 240, bool(e["flag"])) for n, e in _FRAMES.items() if e["stream_bytes"] and not is_wide(n)}
    assert seen == {(True, False), (False, False), (True, True), (False, True)}


# ---- tic_decompress_batch -------------------------------------------------------------------------------------------------------------
def run_batch(L, handle, streams, wants):
    n = len(streams)
    bufs = [np.frombuffer(s, np.uint8) for s in streams]
    outs = [np.full(w_.shape, 0xA5, np.uint8) for w_ in wants]
    rc = L.tic_decompress_batch(handle, (C.c_void_p * n)(*[b.ctypes.data for b in bufs]), (C.c_size_t * n)(*[b.size for b in bufs]), n,
                                (C.c_void_p * n)(*[o.ctypes.data for o in outs]), (C.c_size_t * n)(*[o.size for o in outs]), None, None)
    assert rc == N.TIC_OK, (rc, L.tic_last_error(handle).decode())
    v = [C.c_int() for _ in range(4)]
    assert L.tic_last_decompress_batch(handle, *[C.byref(x) for x in v]) == N.TIC_OK
    return outs, tuple(x.value for x in v)


def check_batch(L, handle, cases, names):
    outs, (batch_frames, single_frames, chunks, _) = run_batch(L, handle, [cases[n][0] for n in names], [cases[n][1] for n in names])
    print("batch of %d: batch_frames %d, single_frames %d, chunks %d" % (len(names), batch_frames, single_frames, chunks))
    for n, o in zip(names, outs):
        assert np.array_equal(o, cases[n][1]), (describe(n), mismatch(o, cases[n][1]))
    # the batch kernels decode every non-scaled frame whose DC stays inside int16; scaled_dct and wide-DC frames go behind the batch
    on_kernels = [n for n in names if not _FRAMES[n]["flag"] and not is_wide(n)]
    assert (batch_frames, single_frames) == (len(on_kernels), len(names) - len(on_kernels)), (batch_frames, single_frames)


def test_batch_small_window(ctx, cases):
    """sparse, ragged and clip frames, all under 240 bits per block: the batch form of the fused kernel with the 2,048-word window."""
    names = [n for n in STREAM_NAMES if _FRAMES[n]["family"] in ("sparse", "ragged", "clip")]
    assert len(names) >= 10 and all(_FRAMES[n]["stream_bytes"] * 8 // _FRAMES[n]["blocks"] <= 240 for n in names)
    check_batch(N.load(), ctx.handle, cases, names)


def test_batch_everything_in_one_call(ctx, cases):
    """Every frame in one call - sparse, ragged, dense and extremes mixed (one dense frame gives the chunk the 4,096-word window); the
    scaled_dct frames and the wide-DC frames are decoded behind the batch and are the oracle's all the same."""
    check_batch(N.load(), ctx.handle, cases, STREAM_NAMES)


# ---- tic_decompress_dev: rows out_stride apart, nothing outside h x w --------------------------------------------------------------------
@pytest.mark.parametrize("pad", [24, 13])  # (a stride that is a multiple of 8: the kernels store into the caller's buffer; one that is not: a strided copy)
def test_decompress_dev_keeps_its_window(pad, ctx, cases):
    L = N.load()
    hmax = max(w_.shape[0] for _, w_ in cases.values())
    smax = max(w_.shape[1] for _, w_ in cases.values()) + 64
    d_s, d_o = C.c_void_p(), C.c_void_p()
    ctx.check(L.tic_dev_alloc(ctx.handle, max(len(s) for s, _ in cases.values()) + 64, C.byref(d_s)))
    ctx.check(L.tic_dev_alloc(ctx.handle, hmax * smax + 64, C.byref(d_o)))
    try:
        for name in STREAM_NAMES:
            s, want = cases[name]
            h, w = want.shape
            stride = w + pad
            if pad % 8 == 0:
                stride = (stride + 7) // 8 * 8
            host = np.full(h * stride + 32, 0xCD, np.uint8)
            buf = np.frombuffer(s, np.uint8)
            ctx.check(L.tic_memcpy_h2d(ctx.handle, d_s, buf.ctypes.data, buf.size))
            ctx.check(L.tic_memcpy_h2d(ctx.handle, d_o, host.ctypes.data, host.size))
            hh, ww = C.c_int(), C.c_int()
            rc = L.tic_decompress_dev(ctx.handle, d_s, buf.size, d_o, stride, h * stride, C.byref(hh), C.byref(ww))
            assert rc == N.TIC_OK, (name, rc, L.tic_last_error(ctx.handle).decode())
            assert (hh.value, ww.value) == (h, w)
            path, giveup = path_of(L, ctx.handle)
            if is_wide(name):
                check_wide_handover(name, path, giveup)
            else:
                assert (path, giveup) == (1, 0), (describe(name), path, giveup)
            ctx.check(L.tic_memcpy_d2h(ctx.handle, host.ctypes.data, d_o, host.size))
            rows = host[: h * stride].reshape(h, stride)
            assert np.array_equal(rows[:, :w], want), (describe(name), mismatch(rows[:, :w], want))
            assert (rows[:, w:] == 0xCD).all() and (host[h * stride:] == 0xCD).all(), describe(name)
    finally:
        L.tic_dev_free(ctx.handle, d_s)
        L.tic_dev_free(ctx.handle, d_o)


# ---- the adaptive route: its own Huffman decoders, then idct_kernel ------------------------------------------------------------------------
def big_ac_coeffs():
    """1,024 blocks with |AC| of sizes 11 .. 15 (1,024 .. 32,767: only a stream with its own table holds them) and a DC inside int16."""
    rng = np.random.default_rng(77)
    n = 1024
    zz = np.zeros((n, 64), np.int64)
    zz[:, 0] = rng.integers(-16000, 16001, n)
    for size in range(11, 16):
        pos = rng.integers(1, 64, n)
        zz[np.arange(n), pos] = rng.integers(1 << (size - 1), 1 << size, n) * rng.choice((-1, 1), n)
    zz[0, 1], zz[1, 63] = 32767, -32767
    return zz


@pytest.mark.parametrize("name", ["sparse_q1", "sparse_q10", "sparse_q50", "sparse_q75", "sparse_q99", "big_ac_q50", "big_ac_q99"])
def test_adaptive_route(name, fx, ctx, oracle):
    """entropy_encode_adaptive -> decompress_adaptive of built coefficients against the oracle's divisors and block_idct in numpy."""
    if name.startswith("big_ac"):
        zz, h, w, q = big_ac_coeffs(), 256, 256, int(name.split("_q")[1])
        sizes = np.ceil(np.log2(np.abs(zz[:, 1:]) + 1)).astype(int)
        assert set(range(11, 16)) <= set(np.unique(sizes).tolist()) and np.abs(zz[:, 0]).max() <= 32767
    else:
        e = fx.frames[name]
        zz, h, w, q = IE.zz_absolute(*fx.coeffs(name)), e["height"], e["width"], e["quality"]
    s = T.entropy_encode_adaptive(zz.astype(np.int16), h, w, q, ctx=ctx)
    got = T.decompress_adaptive(s, ctx=ctx)
    want = IE.pixels_block_idct(fx, oracle, zz, h, w, q, 0)
    print(name, "adaptive stream %d bytes, path / giveup %s" % (len(s), path_of(N.load(), ctx.handle)))
    assert np.array_equal(got, want), (name, mismatch(got, want))
    if name in fx.frames:
        assert fx.matches_reference(name, got)  # (the same coefficients: the reference's pixels)


# ---- the library that ships ------------------------------------------------------------------------------------------------------------
def test_default_route_and_batch_on_the_shipped_library():
    """The default route, the batch and the device-resident form once more in a fresh process that loads the library that ships
    (TIC_TEST_HOOKS=0: no hooks compiled in)."""
    assert os.environ.get("TIC_TEST_HOOKS") == "1" and N.load().tic_build_has_test_hooks() == 1
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("TIC_")}
    env["TIC_TEST_HOOKS"] = "0"
    code = ("import sys; sys.path.insert(0, %r); import tinyimgcodec_amd._native as N; assert N.load().tic_build_has_test_hooks() == 0; "
            "import pytest; sys.exit(pytest.main([%r, '-m', 'gpu', '-q', '-x', '-p', 'no:cacheprovider', '-k', "
            "'test_decompress_default_route or test_batch or test_decompress_dev']))" % (root, os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=root)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, tail
