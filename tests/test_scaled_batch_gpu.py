"""The integer encoder's batch forms on the MI355X: compress_batch_scaled (tic_compress_batch_scaled_v), the transform's descriptor form alone
(tic_dctq_scaled_v_dev: fdctq_scaled_kernel_v, ONE launch for frames of any sizes and settings) and rd_points_scaled_batch
(tic_rd_points_scaled_v).  Every expected byte comes from the reference through fixtures - scaled_encode.npz / .json, scaled_batch.json (the
loop of the reference's tests/cbenchmark.py over the whole benchmark set), distortion.json - or from compress_scaled / dctq_scaled /
roundtrip_sse_scaled of the same frame, which tests/test_scaled_encode_gpu.py and tests/test_distortion_gpu.py pin on those fixtures."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

import mixed_batch_common as M

pytestmark = pytest.mark.gpu

SETTINGS = ("best", "high", "med", "low")
SENTINEL = 0xAB


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
    """(scaled_encode.npz, its manifest, Lenna, [(key, image, setting index)] of every fixture case in the fixture's order)."""
    with open(os.path.join(GOLDEN, "scaled_encode.json")) as f:
        man = json.load(f)
    npz = np.load(os.path.join(GOLDEN, "scaled_encode.npz"))
    lenna = np.load(os.path.join(GOLDEN, "lenna.npz"))["img"]
    cases = []
    for key in [str(k) for k in npz["names"]]:
        img = lenna if key.startswith("lenna512_") else npz[key + "_img"]
        cases.append((key, img, SETTINGS.index(man["cases"][key]["setting"])))
    assert len(cases) == 33 and sum(1 for c in cases if c[1].size == 0) == 4
    return npz, man, lenna, cases


def check_array(npz, man, key, suffix, sha_key, got):
    """got == the fixture's array: by digest always, element by element where the fixture holds the whole array (else its head)."""
    assert sha(got) == man["cases"][key][sha_key], (key, suffix)
    name = "%s_%s" % (key, suffix)
    if name in npz.files:
        assert np.array_equal(got, npz[name]), (key, suffix)
    else:
        head = npz[name + "_head"]
        assert np.array_equal(got[: head.shape[0]], head), (key, suffix)


class SCall:
    """One tic_compress_batch_scaled_v call.  outs[i] is a buffer of caps[i] bytes with 64 sentinel bytes behind it, all filled with the
    sentinel in front of the call; `null_images`: frames whose pixel pointer is null while their sizes stay; `caps`, `strides`, `hs`, `ws`
    override what the frames give; `null_arrays`: arguments passed as null pointers; `n`: the count passed, if not len(frames); `inputs`: (pointers, strides) of
    frames that lie elsewhere than in `frames` (batch_inputs_common.Arena.inputs(); a pointer of 0 is passed as null), which then only
    give the shapes."""

    def __init__(self, ctx, frames, qfs, null_images=(), caps=None, strides=None, hs=None, ws=None, null_arrays=(), n=None, inputs=None):
        L = N.load()
        self.frames = [np.ascontiguousarray(f) for f in frames]
        m = len(frames)
        hs = [f.shape[0] for f in frames] if hs is None else hs
        ws = [f.shape[1] for f in frames] if ws is None else ws
        self.caps = [L.tic_compress_scaled_bound(h, w) if h >= 0 and w >= 0 else 64 for h, w in zip(hs, ws)] if caps is None else list(caps)
        self.bufs = [np.full(c + 64, SENTINEL, np.uint8) for c in self.caps]
        if inputs is not None and strides is None:
            strides = inputs[1]
        arr = {"images": (C.c_void_p * m)(*([None if (i in null_images or f.size == 0) else f.ctypes.data for i, f in enumerate(self.frames)]
                                            if inputs is None else [p or None for p in inputs[0]])),
               "hs": (C.c_int * m)(*hs), "ws": (C.c_int * m)(*ws),
               "strides": (C.c_ssize_t * m)(*([max(w, 1) for w in ws] if strides is None else strides)), "quals": (C.c_int * m)(*qfs),
               "outs": (C.c_void_p * m)(*[b.ctypes.data for b in self.bufs]), "caps": (C.c_size_t * m)(*self.caps), "lens": (C.c_size_t * m)()}
        a = {k: (None if k in null_arrays else v) for k, v in arr.items()}
        self.lens = arr["lens"]
        self.rc = L.tic_compress_batch_scaled_v(ctx.handle, a["images"], m if n is None else n, a["hs"], a["ws"], a["strides"], a["quals"], a["outs"],
                                                a["caps"], a["lens"])
        self.error = L.tic_last_error(ctx.handle).decode() if self.rc else ""

    def streams(self):
        assert self.rc == 0, (self.rc, self.error)
        for b, c in zip(self.bufs, self.caps):
            assert (b[c:] == SENTINEL).all()  # nothing behind a caller's buffer
        return [b[: self.lens[i]].tobytes() for i, b in enumerate(self.bufs)]

    def untouched(self):
        return all((b == SENTINEL).all() for b in self.bufs)


def figures(ctx):
    """-> (batch_frames, single_frames, chunks, transform_launches) of the context's last tic_compress_batch_scaled_v."""
    v = [C.c_int(-1) for _ in range(4)]
    assert N.load().tic_last_compress_batch_scaled(ctx.handle, *[C.byref(x) for x in v]) == 0
    return tuple(x.value for x in v)


def rd_figures(ctx):
    """-> (batch_frames, single_frames, chunks, transform, size, sse launches) of the context's last tic_rd_points_scaled_v."""
    v = [C.c_int(-1) for _ in range(6)]
    assert N.load().tic_last_rd_scaled_batch(ctx.handle, *[C.byref(x) for x in v]) == 0
    return tuple(x.value for x in v)


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


def dctq_v(ctx, dev, frames, qfs, pitches=None, shifts=None):
    """tic_dctq_scaled_v_dev on frames uploaded one by one (rows pitches[i] apart, first pixel shifts[i] bytes into its allocation) ->
    (rc, [int16 [N_i, 64] per frame]); 256 sentinel bytes behind the coefficient area must stay."""
    L = N.load()
    m = len(frames)
    pitches = [max(f.shape[1], 1) for f in frames] if pitches is None else pitches
    shifts = [0] * m if shifts is None else shifts
    ptrs = []
    for f, pitch, shift in zip(frames, pitches, shifts):
        h, w = f.shape
        host = np.full(h * pitch + shift + 16, 0x77, np.uint8)
        if f.size:
            host[shift: shift + h * pitch].reshape(h, pitch)[:, :w] = f
        ptrs.append(dev.upload(host).value + shift)
    nblk = [(f.shape[0] // 8) * (f.shape[1] // 8) for f in frames]
    total = sum(nblk) * 128
    d_zz = dev.alloc(total + 256, fill=0x5A)
    rc = L.tic_dctq_scaled_v_dev(ctx.handle, (C.c_void_p * m)(*ptrs), m, (C.c_int * m)(*[f.shape[0] for f in frames]),
                                 (C.c_int * m)(*[f.shape[1] for f in frames]), (C.c_ssize_t * m)(*pitches), (C.c_int * m)(*qfs), d_zz)
    if rc:
        return rc, None
    raw = dev.download(d_zz, total + 256)
    assert (raw[total:] == 0x5A).all()  # nothing behind the coefficient area
    zz = raw[:total].view(np.int16).reshape(-1, 64)
    offs = np.concatenate(([0], np.cumsum(nblk)))
    return 0, [zz[offs[i]: offs[i + 1]] for i in range(m)]


def case_orders(cases):
    n = len(cases)  # (the fixture's order is case by case, the settings inside; the third one takes every fourth entry: setting by setting)
    return {"fixture": list(range(n)), "reversed": list(range(n))[::-1], "interleaved": sorted(range(n), key=lambda i: (i % 4, i))}


def check_fixture_cases(ctx, dev, fx, chunks_expected):
    npz, man, _, cases = fx
    with_blocks = sum(1 for c in cases if c[1].size)
    for name, order in case_orders(cases).items():
        call = SCall(ctx, [cases[i][1] for i in order], [cases[i][2] for i in order])
        got = call.streams()
        for k, i in enumerate(order):
            key = cases[i][0]
            assert len(got[k]) == man["cases"][key]["bytes"], (name, key)
            check_array(npz, man, key, "bs", "sha256", np.frombuffer(got[k], np.uint8))
        nb, ns, nc, nl = figures(ctx)
        assert (nb, ns) == (with_blocks, 0) and nl == nc and (chunks_expected is None or nc == chunks_expected), (name, nb, ns, nc, nl)
        rc, zz = dctq_v(ctx, dev, [cases[i][1] for i in order], [cases[i][2] for i in order])
        assert rc == 0
        for k, i in enumerate(order):
            check_array(npz, man, cases[i][0], "zz", "zz_sha256", zz[k])
        dev.close()


@pytest.mark.parametrize("hook", [None, ("TIC_BATCH_CHUNK", "3"), ("TIC_SCALED_V_GROUPS", "1")])
def test_every_fixture_case_in_one_call(ctx, dev, fx, monkeypatch, hook):
    """All 33 cases of scaled_encode.npz (29 with blocks, from 8 x 8 to Lenna, four settings, the byte-boundary cases, four empty frames) in
    ONE call, in the fixture's order, reversed and interleaved by setting: every stream and - through the kernel alone - every coefficient
    is the reference's; one transform launch per chunk, no frame behind the one-by-one fallback.  Again in chunks of three (ten chunks, every
    slot reused) and with ONE workgroup, whose four waves then walk strips across every frame and setting change."""
    assert N.load().tic_build_has_test_hooks() == 1
    if hook:
        monkeypatch.setenv(*hook)
    check_fixture_cases(ctx, dev, fx, 10 if hook and hook[0] == "TIC_BATCH_CHUNK" else 1)
    npz, man, _, cases = fx
    order = case_orders(cases)["interleaved"]
    got = T.compress_batch_scaled([cases[i][1] for i in order], [SETTINGS[cases[i][2]] for i in order], ctx=ctx)  # the Python mirror, settings by name
    assert [sha(np.frombuffer(s, np.uint8)) for s in got] == [man["cases"][cases[i][0]]["sha256"] for i in order]


def test_shapes_where_the_walk_can_go_wrong(ctx, dev, monkeypatch):
    """One block; 8 x 72 (two strips per block row, the second with one block); 24 x 8 (three one-block strips); two frames of equal width,
    different heights and settings, side by side; a frame whose last strip holds 7 blocks - each stream against compress_scaled of the same
    frame, each coefficient against dctq_scaled, with the default grid and with one workgroup.  Through the kernel alone also rows further
    apart than w (a multiple of 8 and one that is not: the byte-load path) and first pixels at odd addresses.  65 frames of 8 x 16 are two
    chunks and two launches."""
    rng = np.random.default_rng(20261019)
    shapes = [((8, 8), 2), ((8, 72), 0), ((24, 8), 3), ((16, 40), 0), ((32, 40), 3), ((16, 120), 1), ((8, 8), 0)]
    frames = [rng.integers(0, 256, s, dtype=np.uint8) for s, _ in shapes]
    qfs = [q for _, q in shapes]
    want = [T.compress_scaled(f, q, ctx=ctx) for f, q in zip(frames, qfs)]
    want_zz = [T.dctq_scaled(f, q, ctx=ctx) for f, q in zip(frames, qfs)]
    for groups in (None, "1"):
        if groups:
            monkeypatch.setenv("TIC_SCALED_V_GROUPS", groups)
        for order in (list(range(7)), list(range(7))[::-1]):
            assert SCall(ctx, [frames[i] for i in order], [qfs[i] for i in order]).streams() == [want[i] for i in order], (groups, order)
            assert figures(ctx) == (7, 0, 1, 1)
            for pitches, shifts in ((None, None), ([f.shape[1] + 40 for f in frames], [0] * 7), ([f.shape[1] + 13 for f in frames], [0] * 7),
                                    ([f.shape[1] + 24 for f in frames], [3, 0, 5, 1, 8, 7, 2])):
                rc, zz = dctq_v(ctx, dev, [frames[i] for i in order], [qfs[i] for i in order],
                                None if pitches is None else [pitches[i] for i in order], None if shifts is None else [shifts[i] for i in order])
                assert rc == 0
                for k, i in enumerate(order):
                    assert np.array_equal(zz[k], want_zz[i]), (groups, order, pitches, k, i)
                dev.close()
    monkeypatch.delenv("TIC_SCALED_V_GROUPS")
    many = [rng.integers(0, 256, (8, 16), dtype=np.uint8) for _ in range(65)]
    mq = [k % 4 for k in range(65)]
    assert SCall(ctx, many, mq).streams() == [T.compress_scaled(f, q, ctx=ctx) for f, q in zip(many, mq)]
    assert figures(ctx) == (65, 0, 2, 2)
    rc, zz = dctq_v(ctx, dev, many, mq)  # (two launches of the kernel alone)
    assert rc == 0 and all(np.array_equal(z, T.dctq_scaled(f, q, ctx=ctx)) for z, f, q in zip(zz, many, mq))


def test_dpcm_restarts_at_every_frame(ctx):
    """Two one-block frames whose DCs lie far apart (flat 0, flat 255), then noise: a previous DC that leaked from the frame in front changes
    the first symbol of the second (or third) stream."""
    frames = [np.zeros((8, 8), np.uint8), np.full((8, 8), 255, np.uint8), np.random.default_rng(77).integers(0, 256, (64, 64), dtype=np.uint8)]
    for qf in (2, 0):
        want = [T.compress_scaled(f, qf, ctx=ctx) for f in frames]
        assert want[0] != want[1] and all(w == T.entropy_encode_scaled(T.dctq_scaled(f, qf, ctx=ctx), *f.shape, qf) for w, f in zip(want, frames))
        for order in ([0, 1, 2], [1, 0, 2], [2, 1, 0]):
            assert SCall(ctx, [frames[i] for i in order], [qf] * 3).streams() == [want[i] for i in order], (qf, order)
            assert figures(ctx) == (3, 0, 1, 1)


def test_benchmark_loop_in_one_call(ctx, fx):
    """The loop of the reference's tests/cbenchmark.py - image outer, setting inner - over the whole benchmark set and Lenna as ONE compress
    call: every length and sha256 of tests/golden/scaled_batch.json; then ONE decompress_batch call - Lenna's four frames are the reference's
    decompress() of its streams."""
    npz, man, lenna, _ = fx
    with open(os.path.join(GOLDEN, "scaled_batch.json")) as f:
        doc = json.load(f)
    px = np.load(os.path.join(GOLDEN, "benchmark_set.npz"))["pixels"]
    idx = sorted(int(k) for k in doc["bench"])
    frames = [px[i] for i in idx for _ in SETTINGS] + [lenna] * 4
    settings = [s for _ in idx for s in SETTINGS] + list(SETTINGS)
    entries = [doc["bench"][str(i)][s] for i in idx for s in SETTINGS] + [doc["lenna"][s] for s in SETTINGS]
    assert len(frames) == 200
    streams = T.compress_batch_scaled(frames, settings, ctx=ctx)
    nb, ns, nc, nl = figures(ctx)
    print("cbenchmark's loop in one call: batch_frames %d single_frames %d chunks %d transform_launches %d" % (nb, ns, nc, nl))
    for k, (e, s) in enumerate(zip(entries, streams)):
        assert len(s) == e["bytes"] and hashlib.sha256(s).hexdigest() == e["sha256"], (k, settings[k])
    assert (nb, ns) == (200, 0) and nl == nc == 4, (nb, ns, nc, nl)
    images = T.decompress_batch(streams, ctx=ctx)
    assert all(im.shape == (512, 512) for im in images)
    for s, im in zip(SETTINGS, images[-4:]):
        check_array(npz, man, "lenna512_" + s, "dec", "dec_sha256", np.ascontiguousarray(im))


def test_rd_points_of_cbenchmarks_images(ctx, fx):
    """Lenna, data/1.gif and data/47.gif at the four settings (the table tests/cbenchmark.py prints): the sums are distortion.json's, the
    sizes scaled_batch.json's; twelve probes are one launch of each kernel."""
    _, _, lenna, _ = fx
    with open(os.path.join(GOLDEN, "distortion.json")) as f:
        dist = json.load(f)["scaled"]
    with open(os.path.join(GOLDEN, "scaled_batch.json")) as f:
        doc = json.load(f)
    px = np.load(os.path.join(GOLDEN, "benchmark_set.npz"))["pixels"]
    sizes, sse, wrapped = T.rd_points_scaled_batch([lenna, px[0], px[46]], ctx=ctx)
    assert sizes.shape == sse.shape == wrapped.shape == (3, 4)
    for i, (name, entry) in enumerate((("lenna", doc["lenna"]), ("bench01", doc["bench"]["0"]), ("bench47", doc["bench"]["46"]))):
        for j, s in enumerate(SETTINGS):
            print("%-8s %-5s size %7d sse %10d wrapped %9d" % (name, s, sizes[i, j], sse[i, j], wrapped[i, j]))
            assert int(sizes[i, j]) == entry[s]["bytes"], (name, s)
            assert (int(sse[i, j]), int(wrapped[i, j])) == (dist[name]["settings"][s]["sse"], dist[name]["settings"][s]["sse_wrapped"]), (name, s)
            assert T.psnr_from_sse(int(wrapped[i, j]), 512 * 512) == dist[name]["settings"][s]["psnr_ref"]
    assert rd_figures(ctx) == (3, 0, 1, 1, 1, 1)


def test_rd_points_of_small_frames_and_launch_counts(ctx, fx, monkeypatch):
    """The fixture's small frames and seven more of 8 x 16, every one at the four settings in another order: sizes are scaled_encode.json's
    `bytes` (compress_scaled's where the fixture has no such pair), sums roundtrip_sse_scaled's; 68 probes are two launches of each kernel.
    A 16 x 24 tile of the (1, 1) sign pattern has no code at best: size -1 there, its sums reported all the same, sizes at the other three.
    A frame without blocks: 17 / 0 / 0.  A frame beyond the chunk's byte budget goes through the single-frame calls."""
    npz, man, _, cases = fx
    rng = np.random.default_rng(5)
    seen, frames = set(), []
    for key, img, _ in cases:
        name = key.rsplit("_", 1)[0]
        if name not in seen and img.size and name != "lenna512":
            seen.add(name)
            frames.append((name, img))
    assert len(frames) == 10
    frames += [("extra%d" % k, rng.integers(0, 256, (8, 16), dtype=np.uint8)) for k in range(7)]
    quals = ["low", "best", "med", "high"]
    sizes, sse, wrapped = T.rd_points_scaled_batch([f for _, f in frames], quals, ctx=ctx)
    assert rd_figures(ctx) == (17, 0, 1, 2, 2, 2)
    for i, (name, img) in enumerate(frames):
        for j, s in enumerate(quals):
            m = man["cases"].get("%s_%s" % (name, s))
            assert int(sizes[i, j]) == (m["bytes"] if m else len(T.compress_scaled(img, s, ctx=ctx))), (name, s)
            assert (int(sse[i, j]), int(wrapped[i, j])) == T.roundtrip_sse_scaled(img, s, ctx=ctx), (name, s)
    yy, xx = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    f11 = np.cos((2 * yy + 1) * np.pi / 16) * np.cos((2 * xx + 1) * np.pi / 16)
    tile = np.tile(np.where(f11 >= 0, 255, 0).astype(np.uint8), (2, 3))
    empty = np.zeros((0, 16), np.uint8)
    big = rng.integers(0, 256, (128, 128), dtype=np.uint8)
    for budget in (None, str(8 << 10)):
        if budget:
            monkeypatch.setenv("TIC_BATCH_CHUNK_BYTES", budget)
        sizes, sse, wrapped = T.rd_points_scaled_batch([frames[1][1], tile, empty, big], ctx=ctx)
        assert rd_figures(ctx)[:3] == ((2, 1, 1) if budget else (3, 0, 1))
        assert sizes[1, 0] == -1 and [int(v) for v in sizes[1, 1:]] == [len(T.compress_scaled(tile, s, ctx=ctx)) for s in SETTINGS[1:]]
        assert [int(v) for v in sizes[2]] == [17] * 4 and not sse[2].any() and not wrapped[2].any()
        for i, img in ((0, frames[1][1]), (1, tile), (3, big)):
            for j, s in enumerate(SETTINGS):
                assert (int(sse[i, j]), int(wrapped[i, j])) == T.roundtrip_sse_scaled(img, s, ctx=ctx), (budget, i, s)
                if (i, j) != (1, 0):
                    assert int(sizes[i, j]) == len(T.compress_scaled(img, s, ctx=ctx)), (budget, i, s)


def test_fallback_frames(ctx, fx, monkeypatch):
    """A frame without blocks (the host's 17-byte stream) and a 256 x 256 frame beyond the chunk's byte budget - lowered to 16 KiB - among
    small frames: the large one goes through tic_compress_scaled behind the batch and counts as a single frame."""
    npz, man, _, cases = fx
    rng = np.random.default_rng(99)
    frames = [npz["noise16x24_med_img"], np.zeros((0, 16), np.uint8), rng.integers(0, 256, (256, 256), dtype=np.uint8), npz["ramp48x48_low_img"]]
    qfs = [2, 1, 0, 3]
    want = [npz["noise16x24_med_bs"].tobytes(), None, T.compress_scaled(frames[2], 0, ctx=ctx), npz["ramp48x48_low_bs"].tobytes()]
    monkeypatch.setenv("TIC_BATCH_CHUNK_BYTES", str(16 << 10))
    got = SCall(ctx, frames, qfs).streams()
    assert got[1].hex() == "00000000100000000100000000000040" + "00" and [got[0], got[2], got[3]] == [want[0], want[2], want[3]]
    assert figures(ctx) == (2, 1, 1, 1)
    monkeypatch.delenv("TIC_BATCH_CHUNK_BYTES")
    assert SCall(ctx, frames, qfs).streams() == got and figures(ctx) == (3, 0, 1, 1)


def test_errors(ctx, fx):
    """Argument checks run before any work and name the first offending frame: nothing is written to any output buffer.  A stream that does
    not fit its buffer and a coefficient without a Huffman code fail the call once the device has found them."""
    npz, man, _, cases = fx
    L = N.load()
    pick = [c for c in cases if c[1].size and not c[0].startswith("lenna")][:12]
    frames, qfs = [c[1] for c in pick], [c[2] for c in pick]
    want = [npz[c[0] + "_bs"].tobytes() for c in pick]
    bad = list(qfs)
    bad[5], bad[8] = 4, -1  # (the FIRST offender is reported)
    call = SCall(ctx, frames, bad)
    assert call.rc == N.TIC_E_QUALITY and call.error.startswith("frame 5: ") and call.untouched(), (call.rc, call.error)
    call = SCall(ctx, frames, qfs, null_images=(6, 9))
    assert call.rc == N.TIC_E_ARG and call.error.startswith("frame 6: ") and call.untouched(), (call.rc, call.error)
    for name in ("images", "hs", "ws", "strides", "quals", "outs", "caps", "lens"):
        call = SCall(ctx, frames, qfs, null_arrays=(name,))
        assert call.rc == N.TIC_E_ARG and call.untouched(), (name, call.rc, call.error)
    call = SCall(ctx, frames, qfs, n=-1)
    assert call.rc == N.TIC_E_ARG and call.untouched(), (call.rc, call.error)
    assert L.tic_compress_batch_scaled_v(ctx.handle, None, 0, None, None, None, None, None, None, None) == N.TIC_OK
    call = SCall(ctx, frames, qfs, strides=[f.shape[1] - (1 if i == 9 else 0) for i, f in enumerate(frames)])
    assert call.rc == N.TIC_E_ARG and call.error.startswith("frame 9: ") and call.untouched(), (call.rc, call.error)
    for which, (dh, dw) in (("hs", (4, 0)), ("ws", (0, -4))):  # a size that is no multiple of 8
        hs = [f.shape[0] + (dh if i == 3 else 0) for i, f in enumerate(frames)]
        ws = [f.shape[1] + (dw if i == 3 else 0) for i, f in enumerate(frames)]
        call = SCall(ctx, frames, qfs, hs=hs, ws=ws, caps=[4096 + f.size for f in frames])
        assert call.rc == N.TIC_E_ARG and call.error.startswith("frame 3: ") and "multiples of 8" in call.error and call.untouched(), (which, call.rc, call.error)
    # the kernel alone: the same checks
    scratch = Dev(ctx)
    rc, _ = dctq_v(ctx, scratch, frames[:3], [0, 7, 0])
    scratch.close()
    assert rc == N.TIC_E_QUALITY and L.tic_last_error(ctx.handle).decode().startswith("frame 1: ")
    # caps[i] one byte short: TIC_E_SPACE naming frame i; the scaled bound always suffices (SCall's default)
    for i in (7, 0):
        caps_l = [L.tic_compress_scaled_bound(*f.shape) for f in frames]
        caps_l[i] = len(want[i]) - 1
        call = SCall(ctx, frames, qfs, caps=caps_l)
        assert call.rc == N.TIC_E_SPACE and "frame %d " % i in call.error, (i, call.rc, call.error)
    # the (1, 1) sign pattern has no code at best: a late frame fails the call (KeyError in the mirror), and is fine at high
    yy, xx = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    f11 = np.cos((2 * yy + 1) * np.pi / 16) * np.cos((2 * xx + 1) * np.pi / 16)
    tile = np.tile(np.where(f11 >= 0, 255, 0).astype(np.uint8), (2, 3))
    call = SCall(ctx, frames + [tile], qfs + [0])
    assert call.rc == N.TIC_E_RANGE, (call.rc, call.error)
    with pytest.raises(KeyError):
        T.compress_batch_scaled(frames + [tile], qfs + [0], ctx=ctx)
    assert SCall(ctx, frames + [tile], qfs + [1]).streams() == want + [T.compress_scaled(tile, "high", ctx=ctx)]
    # rd: the same argument checks
    sz = np.zeros((2, 2), np.int64)
    m = 2
    args = [(C.c_void_p * m)(frames[0].ctypes.data, frames[1].ctypes.data), m, (C.c_int * m)(frames[0].shape[0], 12), (C.c_int * m)(frames[0].shape[1], 16),
            (C.c_ssize_t * m)(frames[0].shape[1], 16)]
    assert L.tic_rd_points_scaled_v(ctx.handle, *args, (C.c_int * 2)(0, 3), 2, sz.ctypes.data, None, None) == N.TIC_E_ARG
    assert L.tic_last_error(ctx.handle).decode().startswith("frame 1: ") and not sz.any()
    args[2] = (C.c_int * m)(frames[0].shape[0], 16)
    assert L.tic_rd_points_scaled_v(ctx.handle, *args, (C.c_int * 2)(0, 5), 2, sz.ctypes.data, None, None) == N.TIC_E_QUALITY and not sz.any()
    # and the context still works
    assert SCall(ctx, frames, qfs).streams() == want


def test_nothing_learnt_nothing_changed(ctx, fx, oracle):
    """After scaled batches on the same context - with the lane-per-block kernel allowed for the float route, which a scaled call must
    neither use nor switch off - the uniform call of tests/golden/uniform_batch.json gives its recorded bytes and figures, a small mixed
    compress_batch the oracle's bytes, compress_scaled a fixture case's bytes."""
    npz, man, _, cases = fx
    L = N.load()
    with open(os.path.join(GOLDEN, "uniform_batch.json")) as f:
        gold = json.load(f)
    uniform = [np.random.default_rng(gold["seed"] + i).integers(0, 256, (gold["h"], gold["w"]), dtype=np.uint8) for i in range(gold["n"])]
    mixed, qs = M.small_frames()
    want_mixed = [oracle.compress(f, q) for f, q in zip(mixed, qs)]
    pick = [c for c in cases if c[1].size]
    try:
        for lane in (0, 99):
            ctx.check(L.tic_set_entropy_lane_kernel(ctx.handle, lane))
            got = T.compress_batch_scaled([c[1] for c in pick], [c[2] for c in pick], ctx=ctx)
            assert [sha(np.frombuffer(s, np.uint8)) for s in got] == [man["cases"][c[0]]["sha256"] for c in pick]
            T.rd_points_scaled_batch([c[1] for c in pick[:6]], ctx=ctx)
            out = T.compress_batch(uniform, gold["quality"], ctx=ctx)
            d, s, z = C.c_int(-1), C.c_int(-1), C.c_int(-1)
            ctx.check(L.tic_last_batch_input_path(ctx.handle, C.byref(d), C.byref(s)))
            ctx.check(L.tic_last_batch_zero_copy(ctx.handle, C.byref(z)))
            assert [hashlib.sha256(b).hexdigest() for b in out] == gold["sha256"], lane
            assert (d.value, s.value, z.value) == (gold["direct_frames"], gold["staged_frames"], gold["zero_copy"]), (lane, d.value, s.value, z.value)
            assert T.compress_batch(mixed, qs, ctx=ctx) == want_mixed, lane
            assert M.figures(ctx)[:2] == (len(mixed), 0)
            assert T.compress_scaled(npz["noise64x96_best_img"], "best", ctx=ctx) == npz["noise64x96_best_bs"].tobytes()
    finally:
        ctx.check(L.tic_set_entropy_lane_kernel(ctx.handle, 0))


def test_fixture_cases_on_the_shipped_library(fx):
    """Every fixture case in one call, three orders, in a fresh process that loads the library that ships (no test hooks, no TIC_* variable)."""
    code = r'''
import hashlib, json, os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N
assert N.load().tic_build_has_test_hooks() == 0 and N._lib_path() == N.LIB_PATH
G = os.path.join(os.getcwd(), "tests", "golden")
man = json.load(open(os.path.join(G, "scaled_encode.json")))["cases"]
npz = np.load(os.path.join(G, "scaled_encode.npz"))
lenna = np.load(os.path.join(G, "lenna.npz"))["img"]
keys = [str(k) for k in npz["names"]]
imgs = [lenna if k.startswith("lenna512_") else npz[k + "_img"] for k in keys]
n = len(keys)
for order in (list(range(n)), list(range(n))[::-1], sorted(range(n), key=lambda i: (i % 4, i))):
    got = T.compress_batch_scaled([imgs[i] for i in order], [man[keys[i]]["setting"] for i in order])
    for k, i in enumerate(order):
        assert len(got[k]) == man[keys[i]]["bytes"] and hashlib.sha256(got[k]).hexdigest() == man[keys[i]]["sha256"], (k, keys[i])
sizes, sse, wrapped = T.rd_points_scaled_batch([npz["noise64x96_med_img"]])
assert [int(v) for v in sizes[0]] == [man["noise64x96_" + s]["bytes"] for s in ("best", "high", "med", "low")]
assert all((int(sse[0, j]), int(wrapped[0, j])) == T.roundtrip_sse_scaled(npz["noise64x96_med_img"], j) for j in range(4))
print("scaled batch on the shipped library ok")
'''
    env = {k: v for k, v in os.environ.items() if not k.startswith("TIC_")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "scaled batch on the shipped library ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_cli_scaled_writes_several_files_in_one_call(ctx, fx, tmp_path, capsys):
    """encode_cli --scaled med INPUT OUTPUT --also INPUT OUTPUT --also ...: images of different sizes, one compress_batch_scaled() call, a
    file and two lines each."""
    from tinyimgcodec_amd import encode_cli

    npz, man, _, _ = fx
    keys = ["noise64x96_med", "ramp48x48_med", "noise16x24_med"]
    argv = []
    for k, key in enumerate(keys):
        np.save(tmp_path / ("in%d.npy" % k), npz[key + "_img"])
        argv += ([] if k == 0 else ["--also"]) + [str(tmp_path / ("in%d.npy" % k)), str(tmp_path / ("out%d.img" % k))]
    assert encode_cli.main(argv + ["--scaled", "med"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 6
    for k, key in enumerate(keys):
        got = (tmp_path / ("out%d.img" % k)).read_bytes()
        h, w = man["cases"][key]["h"], man["cases"][key]["w"]
        assert got == npz[key + "_bs"].tobytes() == T.compress_scaled(npz[key + "_img"], "med", ctx=ctx), key
        assert lines[2 * k] == "%d bytes" % len(got) and lines[2 * k + 1] == f"Compression Ratio: {w * h / len(got)}:1", key
