"""The batch forms of rate-distortion control on the GPU: rd_points_batch / compress_batch_to_psnr and the C calls under them
(tic_rd_points_v, tic_compress_batch_to_psnr, tic_distortion_v_dev, tic_last_rd_batch) against the round-trip errors and stream lengths
recorded from the unmodified reference (tests/golden/distortion.json, rate_control.json), the oracle's round trip and streams, the
single-frame calls, closed-form sums of built coefficients, and the Python replay of the bisection that is the search's contract.  Every
comparison is an integer equality or a byte identity."""
import ctypes as C
import math
import random

import numpy as np
import pytest

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

import rate_batch_common as R
import rd_batch_common as RD
from distortion_common import load_distortion, oracle_sums
from test_distortion_gpu import bisect_psnr
from test_rate_control_cpu import IMAGES, fixture_image, load_fixture
from test_rate_control_gpu import Dev

pytestmark = pytest.mark.gpu

CAPS = ("1", "2", "3")  # TIC_SSE_MAX_GROUPS: one group walks a whole probe, two and three share it


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(0)
    assert c.arch.startswith("gfx950"), c.arch
    yield c
    c.close()


@pytest.fixture(scope="module")
def shipped():
    """(library, context handle) of the build that ships (no test hooks compiled in), bound beside the test-hooks build this process runs."""
    assert N.load().tic_build_has_test_hooks() == 1
    L = RD.bind(N.LIB_PATH)
    assert L.tic_build_has_test_hooks() == 0
    handle = L.tic_create(0)
    assert handle, L.tic_last_error(None)
    yield L, handle
    L.tic_destroy(handle)


@pytest.fixture(scope="module")
def fx():
    return load_distortion()["images"]


@pytest.fixture(scope="module")
def rate():
    return load_fixture()["images"]


@pytest.fixture(scope="module")
def streams(oracle):
    return R.Streams(oracle)


@pytest.fixture(scope="module")
def small(ctx, oracle):
    """Test 2's frames with, per frame and quality, (size, sse, wrapped) of the single call (unchanged by this feature) and the oracle's sums,
    computed once."""
    frames = RD.frames()
    L = N.load()
    single = [RD.rd_single(L, ctx.handle, f, RD.QUALITIES) for f in frames]
    want = [[oracle_sums(oracle, f, q) if f.size else (0, 0) for q in RD.QUALITIES] for f in frames]
    return frames, single, want


def rows(sizes, sse, wrapped):
    return [(a.tolist(), b.tolist(), c.tolist()) for a, b, c in zip(sizes, sse, wrapped)]


def test_fixture_table_in_one_call(ctx, shipped, fx, rate):
    """1. The six fixture images (512^2, 256^2, the ragged 203 x 317 crop) at q = 1, 5, 20, 50, 75, 90, 97, 99 in ONE tic_rd_points_v: the
    reference's recorded sums and stream lengths wherever they are not null; where null, size -1 and the sums of the single tic_rd_points.
    On the test-hooks build and on the build that ships."""
    qs = [1, 5, 20, 50, 75, 90, 97, 99]
    imgs = [fixture_image(n) for n in IMAGES]
    nulls = 0
    for L, handle in ((N.load(), ctx.handle), shipped):
        rc, sizes, sse, wrapped = RD.rd_v(L, handle, imgs, qs)
        assert rc == N.TIC_OK, L.tic_last_error(handle)
        assert R.figures(L, handle)[:5] == (6, 0, 1, 48, 1) and RD.sse_launches(L, handle) == R.figures(L, handle)[5] == 1
        for i, name in enumerate(IMAGES):
            for j, q in enumerate(qs):
                got = (int(sizes[i, j]), int(sse[i, j]), int(wrapped[i, j]))
                if fx[name]["sse"][q - 1] is not None:
                    assert got == (rate[name]["sizes"][q - 1], fx[name]["sse"][q - 1], fx[name]["sse_wrapped"][q - 1]), (name, q, got)
                else:
                    one = RD.rd_single(L, handle, imgs[i], [q])
                    assert rate[name]["sizes"][q - 1] is None and got == (-1, one[1][0], one[2][0]) and one[0] == [-1] and got[1] > 0, (name, q, got)
                    nulls += 1
    assert nulls >= 2  # (q = 99 has no code on the photographs)


def test_smallest_shapes(ctx, shipped, small):
    """2. 1x1, 8x8, 7x9, 15x17, 24x8, 72x8, 128x8, 136x8, 40x52, 203x317, 0x8, 8x0, 8x264 (33 blocks: a second workgroup) and 72x136 (27
    tiles: no multiple of a workgroup's 4) in one call at [5, 50, 90], forward and reversed: every row is the oracle's round trip and the
    single call's; frames without blocks give 16 / 0 / 0."""
    frames, single, want = small
    for f, s, w in zip(frames, single, want):
        assert list(zip(s[1], s[2])) == w, f.shape
    for L, handle in ((N.load(), ctx.handle), shipped):
        for order in (list(range(len(frames))), list(range(len(frames)))[::-1]):
            rc, sizes, sse, wrapped = RD.rd_v(L, handle, [frames[i] for i in order], RD.QUALITIES)
            assert rc == N.TIC_OK, L.tic_last_error(handle)
            assert rows(sizes, sse, wrapped) == [tuple(single[i]) for i in order], order
            for k, i in enumerate(order):
                if frames[i].size == 0:
                    assert (sizes[k].tolist(), sse[k].tolist(), wrapped[k].tolist()) == ([16] * 3, [0] * 3, [0] * 3)
        assert R.figures(L, handle)[:5] == (12, 0, 1, 36, 1) and RD.sse_launches(L, handle) == 1


def test_the_walk(ctx, small, monkeypatch):
    """3. Test 2's list with TIC_SSE_MAX_GROUPS = 1, 2, 3 (test-hooks build): one, two and three workgroups walk every probe - 203 x 317 is
    130 tiles, 33 steps at cap 1 - with results identical to the default cap's and the same number of launches."""
    frames, single, want = small
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    rc, s0, a0, b0 = RD.rd_v(L, ctx.handle, frames, RD.QUALITIES)
    assert rc == N.TIC_OK and rows(s0, a0, b0) == [tuple(s) for s in single]
    launches = (R.figures(L, ctx.handle)[5], RD.sse_launches(L, ctx.handle))
    for cap in CAPS:
        monkeypatch.setenv("TIC_SSE_MAX_GROUPS", cap)
        rc, s1, a1, b1 = RD.rd_v(L, ctx.handle, frames, RD.QUALITIES)
        assert rc == N.TIC_OK, L.tic_last_error(ctx.handle)
        assert (s1 == s0).all() and (a1 == a0).all() and (b1 == b0).all(), cap
        assert (R.figures(L, ctx.handle)[5], RD.sse_launches(L, ctx.handle)) == launches == (1, 1)
    monkeypatch.delenv("TIC_SSE_MAX_GROUPS")


def built_specs(n, seed):
    """n probes, shuffled: 264 x 256 once (33 workgroup-tiles), a 33-block row, several block rows, ragged ones (unaligned image, odd
    pitch) between aligned ones; decoded 0 or 255 against a constant of the probe's own - the two exact extremes among them."""
    shapes = [(264, 256), (8, 264), (8, 8), (16, 24), (7, 9), (24, 40), (1, 1), (72, 136), (13, 21), (40, 8)]
    specs = []
    for i in range(n):
        h, w = shapes[i % len(shapes)] if i else shapes[0]
        if i and (h, w) == (264, 256):
            h, w = 32, 32
        dec = 255 if i % 2 == 0 else 0
        const = (0 if dec == 255 else 255) if i < 4 else (3 * i + 1) % 255 if dec == 255 else 255 - (3 * i + 1) % 255
        specs.append((h, w, (5, 50, 90)[i % 3], dec, const, (h, w) not in ((7, 9), (13, 21))))
    random.Random(seed).shuffle(specs)
    return specs


def test_built_coefficients_through_the_kernel_alone(ctx, shipped, monkeypatch):
    """4. tic_distortion_v_dev on coefficients that decode to all 0 or all 255 against constant images: exactly h * w * d^2 and
    h * w * (d^2 & 255) per probe (h * w * 65025 and h * w * 1 at the extremes; 65025 & 255 = 1).  64 probes in one launch and 65 in two,
    every probe a sum of its own (asserted), sizes shuffled, a ragged probe between aligned ones - a probe that took a neighbour's record,
    alignment, constants or result entry, or an entry added to twice, shows.  264 x 256 (1,056 blocks, 33 workgroup-tiles) at cap 1 is one
    workgroup's sum of 264 * 256 * 65025 > 2^32: a 32-bit workgroup sum would wrap."""
    L = N.load()
    for n, seed, launches in ((64, 1, 1), (65, 2, 2)):
        p = RD.BuiltProbes(built_specs(n, seed))
        assert len(set(p.want)) == n and (264 * 256 * 65025, 264 * 256) in p.want and 264 * 256 * 65025 > 2 ** 32
        assert any(s[0] * s[1] * 65025 == w[0] and w[1] == s[0] * s[1] for s, w in zip(p.specs, p.want) if s[3] == 0)
        ragged = [k for k, s in enumerate(p.specs) if not s[5]]
        assert any(0 < k < n - 1 and p.specs[k - 1][5] and p.specs[k + 1][5] for k in ragged)
        for cap in (None,) + CAPS[:1]:
            if cap is not None:
                monkeypatch.setenv("TIC_SSE_MAX_GROUPS", cap)
            d = Dev(L, ctx.handle)
            try:
                rc, got, nl = p.run(L, ctx.handle, d)
            finally:
                d.close()
            assert rc == N.TIC_OK, L.tic_last_error(ctx.handle)
            assert got == p.want, [(k, p.specs[k], g, w) for k, (g, w) in enumerate(zip(got, p.want)) if g != w][:4]
            assert nl == launches
        monkeypatch.delenv("TIC_SSE_MAX_GROUPS")
    Ls, hs = shipped
    p = RD.BuiltProbes(built_specs(9, 3))
    d = Dev(Ls, hs)
    try:
        rc, got, nl = p.run(Ls, hs, d)
        assert rc == N.TIC_OK and got == p.want and nl == 1
        # arguments: per probe, before any work
        buf = d.alloc(4096)
        one = (C.c_void_p * 2)(buf.value, buf.value)
        h8, s8, q50 = (C.c_int * 2)(8, 8), (C.c_ssize_t * 2)(8, 8), (C.c_int * 2)(50, 50)
        out = np.full((2, 2), 7, np.uint64)
        assert Ls.tic_distortion_v_dev(hs, buf, one, 2, h8, h8, s8, (C.c_int * 2)(50, 100), out.ctypes.data) == N.TIC_E_QUALITY
        assert Ls.tic_last_error(hs).decode().startswith("probe 1: ") and (out == 7).all()
        assert Ls.tic_distortion_v_dev(hs, buf, one, 2, h8, h8, (C.c_ssize_t * 2)(8, 7), q50, out.ctypes.data) == N.TIC_E_ARG
        assert Ls.tic_distortion_v_dev(hs, None, one, 2, h8, h8, s8, q50, out.ctypes.data) == N.TIC_E_ARG
        assert Ls.tic_distortion_v_dev(hs, buf, (C.c_void_p * 2)(buf.value, None), 2, h8, h8, s8, q50, out.ctypes.data) == N.TIC_E_ARG
        assert Ls.tic_distortion_v_dev(hs, buf, one, 2, h8, h8, s8, q50, None) == N.TIC_E_ARG
        assert Ls.tic_distortion_v_dev(hs, buf, one, -1, h8, h8, s8, q50, out.ctypes.data) == N.TIC_E_ARG and (out == 7).all()
        assert Ls.tic_distortion_v_dev(hs, None, None, 0, None, None, None, None, None) == N.TIC_OK
        assert Ls.tic_distortion_v_dev(hs, None, (C.c_void_p * 2)(), 2, (C.c_int * 2)(0, 8), (C.c_int * 2)(8, 0), s8, q50, out.ctypes.data) == N.TIC_OK
        assert (out == 0).all()  # (no blocks: both sums 0)
    finally:
        d.close()


SEARCH_IMAGES = ("lenna", "bench06_crop203x317", "noise256_seed7")


def search_list(fx):
    """Test 5's 24 frames: per image the bounds sse(q) for q in (1, 20, 50, 90, 97), sse(50) - 1, 0 and 2^63 -> [(name, max_sse), ...]."""
    out = []
    for name in SEARCH_IMAGES:
        s = fx[name]["sse"]
        out += [(name, b) for b in [s[q - 1] for q in (1, 20, 50, 90, 97)] + [s[49] - 1, 0, 2 ** 63]]
    return out


def check_search(L, handle, fx, rate, streams):
    lst = search_list(fx)
    imgs = [streams.image(n) for n, _ in lst]
    want = [bisect_psnr(fx[n]["sse"], b, 1, 97) for n, b in lst]
    assert sum(w is ValueError for w in want) == 3 and KeyError not in want and len({w for w in want if w is not ValueError}) >= 5
    call = RD.PsnrCall(L, handle, imgs, [b for _, b in lst], 1, 97)
    rc = call.run()
    fig = R.figures(L, handle)
    print("search 1..97 figures (batch, single, chunks, probes, waits, size launches):", fig, "measuring launches:", RD.sse_launches(L, handle))
    first_bad = next(i for i, w in enumerate(want) if w is ValueError)
    assert rc == N.TIC_E_SPACE and L.tic_last_error(handle).decode().startswith("frame %d: squared error %d at quality 97" % (first_bad, fx[lst[first_bad][0]]["sse"][96]))
    for i, (n, b) in enumerate(lst):
        sse, sizes = fx[n]["sse"], rate[n]["sizes"]
        if want[i] is ValueError:  # out of reach: quality and error of qmax, no length, nothing written
            assert (call.status[i], call.lens[i], call.quals[i], call.sse[i]) == (N.TIC_E_SPACE, 0, 97, sse[96]) and call.tail_intact(i), i
        else:
            q = want[i]
            assert (call.status[i], call.quals[i], call.sse[i], call.lens[i]) == (N.TIC_OK, q, sse[q - 1], sizes[q - 1]), (i, n, b)
            assert sse[q - 1] <= b and call.stream(i) == streams.get(n, q) and call.tail_intact(i), (i, n, b)
    # one chunk; its depth is the plan's for its blocks; every round one wait, no (frame, quality) pair probed twice
    depth = RD.rate_depth(sum(((im.shape[0] + 7) // 8) * ((im.shape[1] + 7) // 8) for im in imgs))
    replay = [RD.lockstep_probes(fx[n]["sse"], b, 1, 97, depth) for n, b in lst]
    assert fig[:3] == (24, 0, 1) and depth == 3
    assert fig[4] == max(r for r, _ in replay) <= 1 + math.ceil(7 / depth)
    assert fig[3] == sum(p for _, p in replay)
    assert fig[5] == RD.sse_launches(L, handle) >= fig[4]


def test_the_search_is_the_bisection(ctx, shipped, fx, rate, streams):
    """5. Lenna, the ragged crop and the noise frame, eight bounds each, 24 frames in one call over 1..97: the quality is the bisection
    replayed on the RECORDED errors, the stream the oracle's compress() at that quality byte for byte, sse[i] the recorded error; bounds
    out of reach give TIC_E_SPACE with out_lens[i] = 0, quality 97 and its recorded error.  Search waits and probes are those of the
    lockstep search replayed in Python: at most 1 + ceil(7 / depth) rounds, no pair probed twice.  Lenna over 1..99, whose upper end has no
    code: TIC_E_RANGE."""
    L = N.load()
    check_search(L, ctx.handle, fx, rate, streams)
    check_search(*shipped, fx, rate, streams)
    assert fx["lenna"]["sse"][98] is None
    img = streams.image("lenna")
    call = RD.PsnrCall(L, ctx.handle, [np.full((8, 8), 128, np.uint8), img], [2 ** 63, 2 ** 63], 1, 99)
    one = RD.rd_single(L, ctx.handle, img, [99])
    assert call.run() == N.TIC_E_RANGE and L.tic_last_error(ctx.handle).decode().startswith("frame 1: coefficient without a Huffman code at quality 99")
    assert (call.status[1], call.quals[1], call.sse[1], call.lens[1]) == (N.TIC_E_RANGE, 99, one[1][0], 0) and call.tail_intact(1)
    assert call.status[0] == N.TIC_OK and call.quals[0] == 1 and call.tail_intact(0)
    assert R.figures(L, ctx.handle)[4] == 3  # (the settled frame asks for nothing more; the other one ends after three rounds)


def test_equal_to_the_loop(ctx, shipped, small):
    """6. Test 2's frames with mixed bounds - the error at q = 50, one less than the error at q = 90 or at q = 5, 0, 2^63 - and the
    capacities of frames 2, 9 and 12 one byte short of the stream they end at: status, length, quality, error and bytes are those of
    tic_compress_to_psnr per frame; sentinel tails intact, failed frames' buffers wholly intact; the call returns the first failing frame's
    status and its message starts "frame i:"."""
    frames, single, want = small
    bounds = []
    for i, s in enumerate(single):
        bounds.append([s[1][1], max(s[1][2], 1) - 1, max(s[1][0], 1) - 1, 0, 2 ** 63][i % 5])
    for L, handle in ((N.load(), ctx.handle), shipped):
        full = [L.tic_compress_bound(f.shape[0], f.shape[1]) for f in frames]
        loop = [RD.psnr_single(L, handle, f, b, 1, 97, c) for f, b, c in zip(frames, bounds, full)]
        caps = list(full)
        for i in (2, 9, 12):
            assert loop[i][0] == N.TIC_OK and loop[i][1] > 16
            caps[i] = loop[i][1] - 1
            loop[i] = RD.psnr_single(L, handle, frames[i], bounds[i], 1, 97, caps[i])
            assert loop[i][0] == N.TIC_E_SPACE and loop[i][1] == caps[i] + 1
        codes = [r[0] for r in loop]
        assert N.TIC_OK in codes and codes.count(N.TIC_E_SPACE) >= 4 and any(r[0] == N.TIC_E_SPACE and r[1] == 0 for r in loop)
        call = RD.PsnrCall(L, handle, frames, bounds, 1, 97, caps)
        rc = call.run()
        first_bad = next(i for i, c in enumerate(codes) if c != N.TIC_OK)
        assert rc == codes[first_bad] and L.tic_last_error(handle).decode().startswith("frame %d: " % first_bad)
        for i, (c, n, q, s, buf) in enumerate(loop):
            assert (call.status[i], call.lens[i], call.quals[i], call.sse[i]) == (c, n, q, s), (i, frames[i].shape, bounds[i])
            assert np.array_equal(call.bufs[i][: caps[i] + 8], buf[: caps[i] + 8]) and call.tail_intact(i), i


def test_neighbours_unchanged(ctx, fx, rate, oracle, small):
    """7. tic_compress_to_psnr, tic_compress_to_size, tic_rd_points and tic_compress_batch_to_size give after a batch call in the same
    context what they gave before it: they share the rate buffers, the scratch image and the workspace."""
    frames, single, want = small
    img = fixture_image("bench40")
    sizes, sse = rate["bench40"]["sizes"], fx["bench40"]["sse"]

    def neighbours():
        return (T.compress_to_psnr(img, 35.0, 1, 97, ctx=ctx), T.compress_to_size(img, sizes[39], 20, 60, ctx=ctx),
                [a.tolist() for a in T.rd_points(img, [20, 50, 98], ctx=ctx)], T.compress_batch_to_size(frames[:10], [s[0][1] for s in single[:10]], ctx=ctx))

    before = neighbours()
    assert before[2][0][:2] == [sizes[19], sizes[49]] and before[2][1][:2] == [sse[19], sse[49]]
    assert before[0][1] == bisect_psnr(sse, T.max_sse_for_psnr(35.0, img.size), 1, 97) and before[0][0] == oracle.compress(img, before[0][1])
    T.rd_points_batch(frames + [img], [5, 90], ctx=ctx)
    assert neighbours() == before
    T.compress_batch_to_psnr(frames[:10] + [img], 30.0, 1, 97, ctx=ctx)
    assert neighbours() == before


def test_python_mirrors(ctx, small):
    """8. compress_batch_to_psnr equals [compress_to_psnr(im, t) ...] with one target and with one per frame; rd_points_batch equals the
    stacked rd_points; a failing frame raises what compress_to_psnr raises for it, prefixed "frame i: "."""
    frames, single, want = small
    got = T.rd_points_batch(frames, RD.QUALITIES, ctx=ctx)
    one = [T.rd_points(f, RD.QUALITIES, ctx=ctx) for f in frames]
    for k in range(3):
        assert got[k].dtype == one[0][k].dtype and got[k].shape == (len(frames), 3) and (got[k] == np.stack([o[k] for o in one])).all()
    assert T.compress_batch_to_psnr(frames, 30.0, 1, 97, ctx=ctx) == [T.compress_to_psnr(f, 30.0, 1, 97, ctx=ctx) for f in frames]
    targets = [25.0 + 1.5 * i for i in range(len(frames))]
    reach = [T.psnr_from_sse(T.rd_points(f, [97], ctx=ctx)[1][0], f.size) if f.size else math.inf for f in frames]
    targets = [min(t, r) for t, r in zip(targets, reach)]  # (every target within reach of quality 97)
    assert T.compress_batch_to_psnr(frames, targets, 1, 97, ctx=ctx) == [T.compress_to_psnr(f, t, 1, 97, ctx=ctx) for f, t in zip(frames, targets)]
    short = next(i for i, r in enumerate(reach) if r < 200.0)
    with pytest.raises(ValueError, match=r"frame %d: %s dB at quality 97 fall short of min_psnr = 200\.0" % (short, repr(reach[short]).replace(".", r"\."))):
        T.compress_batch_to_psnr(frames, 200.0, 1, 97, ctx=ctx)
    with pytest.raises(ValueError, match="dB at quality 97 fall short of min_psnr = 200"):
        T.compress_to_psnr(frames[short], 200.0, 1, 97, ctx=ctx)
    noise = fixture_image("noise256_seed7")
    with pytest.raises(KeyError, match="frame 1: "):
        T.compress_batch_to_psnr([np.full((8, 8), 128, np.uint8), noise], 20.0, 1, 99, ctx=ctx)  # (the noise frame has no code at 99)
