"""The batch forms of rate control on the GPU: compressed_sizes_batch / compress_batch_to_size and the C calls under them
(tic_stream_sizes_v, tic_compress_batch_to_size, tic_last_rate_batch) against stream lengths recorded from the unmodified reference
(tests/golden/rate_control.json, benchmark_set.json), the oracle's streams, the single-frame calls, and the Python replay of the bisection
that is the search's contract."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

import rate_batch_common as R
from conftest import rand_frame
from test_rate_control_cpu import GOLDEN, IMAGES, fixture_image, load_fixture
from test_rate_control_gpu import bisect

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(0)
    assert c.arch.startswith("gfx950"), c.arch
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return load_fixture()["images"]


@pytest.fixture(scope="module")
def streams(oracle):
    return R.Streams(oracle)


@pytest.fixture(scope="module")
def small(ctx, oracle):
    """Test 3's frames with, per frame, the sizes of the single path (unchanged by this feature) and of the oracle's streams."""
    frames = R.small_frames()
    single = [T.compressed_sizes(f, R.SMALL_QUALITIES, ctx=ctx).tolist() for f in frames]
    want = [[len(oracle.compress(f, q)) for q in R.SMALL_QUALITIES] for f in frames]
    return frames, single, want


def test_reference_sizes_in_one_call(ctx, fx):
    """1. The six fixture images (512^2, 203 x 317, 256^2) at q = 1..99 in ONE call: the 594 recorded reference sizes, -1 where the record
    is null; any order of frames gives the same rows."""
    imgs = [fixture_image(n) for n in IMAGES]
    want = np.array([[-1 if v is None else v for v in fx[n]["sizes"]] for n in IMAGES], np.int64)
    got = T.compressed_sizes_batch(imgs, range(1, 100), ctx=ctx)
    print("figures (batch, single, chunks, probes, waits, size launches):", R.figures(N.load(), ctx.handle))
    assert got.dtype == np.int64 and got.shape == (6, 99)
    assert (got == want).all(), np.argwhere(got != want)[:5]
    assert R.figures(N.load(), ctx.handle)[:5] == (6, 0, 1, 594, 1)
    for order in ([5, 4, 3, 2, 1, 0], [2, 5, 0, 4, 1, 3]):
        got = T.compressed_sizes_batch([imgs[i] for i in order], range(1, 100), ctx=ctx)
        assert (got == want[order]).all(), order


def test_benchmark_table_in_one_call(ctx):
    """2. The reference's benchmark table: 49 images x qualities [90, 80, 50, 20, 10, 5] in one call == the 294 `bytes` of benchmark_set.json."""
    with open(os.path.join(GOLDEN, "benchmark_set.json")) as f:
        entries = json.load(f)["entries"]
    px = np.load(os.path.join(GOLDEN, "benchmark_set.npz"))["pixels"]
    qs = [90, 80, 50, 20, 10, 5]
    assert len(entries) == 294 and [(e["image"], e["quality"]) for e in entries[:7]] == [(1, q) for q in qs] + [(2, 90)]
    got = T.compressed_sizes_batch(list(px), qs, ctx=ctx)
    print("figures:", R.figures(N.load(), ctx.handle))
    assert got.reshape(-1).tolist() == [e["bytes"] for e in entries]
    assert R.figures(N.load(), ctx.handle)[:5] == (49, 0, 1, 294, 1)


def test_smallest_shapes(ctx, small):
    """3. 1x1, 8x8, 7x9, 15x17, 24x8, 72x8, 128x8, 136x8, 40x52, 203x317, 0x8 and 8x0 in one call at [5, 50, 90], forward and reversed:
    every row is compressed_sizes(img, qs) of the single path and len(oracle.compress(img, q))."""
    frames, single, want = small
    assert single == want
    assert want[-1] == want[-2] == [16, 16, 16]
    for order in (list(range(len(frames))), list(range(len(frames)))[::-1]):
        got = T.compressed_sizes_batch([frames[i] for i in order], R.SMALL_QUALITIES, ctx=ctx)
        assert got.tolist() == [want[i] for i in order], order


def test_dpcm_restart_and_probe_local_flags(ctx):
    """4. Flat 8x8 and 16x8 frames of 0 and 255 in turn (a frame that kept its neighbour's DC would code another difference; the middle
    frames start inside a launch, off a multiple of 8 blocks), and the noise frame that has no code at q = 99 between two encodable
    probes of the same frame: -1 for that probe alone."""
    flat = lambda h, v: np.full((h, 8), v, np.uint8)
    frames = [flat(8, 0), flat(16, 255), flat(8, 255), flat(16, 0), flat(8, 0), flat(16, 255), rand_frame(7, 256, 256), flat(8, 255)]
    qs = [50, 99, 90]
    want = [T.compressed_sizes(f, qs, ctx=ctx).tolist() for f in frames]
    assert want[6][1] == -1 and want[6][0] > 16 and want[6][2] > want[6][0]
    print("flat frames and the noise frame at 50, 99, 90:", want)
    for order in (list(range(8)), [7, 6, 5, 4, 3, 2, 1, 0], [6, 0, 1, 2, 3, 4, 5, 7]):
        got = T.compressed_sizes_batch([frames[i] for i in order], qs, ctx=ctx)
        assert got.tolist() == [want[i] for i in order], order


def test_group_cap(ctx):
    """5. A 4096^2 frame (262,144 blocks: its groups are capped at 1,024 and the strided loop runs) at [20, 50] among three small frames."""
    frames = [rand_frame(3, 24, 40), rand_frame(1234, 4096, 4096), rand_frame(4, 8, 8), rand_frame(5, 72, 8)]
    got = T.compressed_sizes_batch(frames, [20, 50], ctx=ctx)
    print("4096^2 at 20, 50:", got[1].tolist(), "figures:", R.figures(N.load(), ctx.handle))
    for f, row in zip(frames, got.tolist()):
        assert row == T.compressed_sizes(f, [20, 50], ctx=ctx).tolist(), f.shape
    assert R.figures(N.load(), ctx.handle)[:3] == (4, 0, 1)


def test_chunk_hooks(ctx, small, monkeypatch):
    """6. Test 3's list with TIC_BATCH_CHUNK=5 and with TIC_BATCH_CHUNK_BYTES = 512 KiB: identical results; tic_last_rate_batch shows the
    chunks, and - at 64 KiB per chunk - the frame set aside (203 x 317 is staged at 104 KB)."""
    frames, single, want = small
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_BATCH_CHUNK", "5")
    assert T.compressed_sizes_batch(frames, R.SMALL_QUALITIES, ctx=ctx).tolist() == want
    assert R.figures(L, ctx.handle) == (10, 0, 2, 30, 2, 2)
    monkeypatch.delenv("TIC_BATCH_CHUNK")
    monkeypatch.setenv("TIC_BATCH_CHUNK_BYTES", str(512 << 10))
    assert T.compressed_sizes_batch(frames, R.SMALL_QUALITIES, ctx=ctx).tolist() == want
    assert R.figures(L, ctx.handle)[:5] == (10, 0, 1, 30, 1)
    monkeypatch.setenv("TIC_BATCH_CHUNK_BYTES", str(64 << 10))
    assert T.compressed_sizes_batch(frames, R.SMALL_QUALITIES, ctx=ctx).tolist() == want
    assert R.figures(L, ctx.handle)[:4] == (9, 1, 1, 27)
    # ... and the search, with several chunks and a frame behind the batch
    monkeypatch.setenv("TIC_BATCH_CHUNK", "4")
    budgets = [row[1] for row in want]
    got = T.compress_batch_to_size(frames, budgets, ctx=ctx)
    assert R.figures(L, ctx.handle)[:3] == (9, 1, 3)
    monkeypatch.delenv("TIC_BATCH_CHUNK")
    monkeypatch.delenv("TIC_BATCH_CHUNK_BYTES")
    assert got == T.compress_batch_to_size(frames, budgets, ctx=ctx)


def check_search_1_99(L, handle, fx, streams):
    """Test 7, range (1, 99), through library L: qualities of the replayed bisection, the oracle's streams, lengths within budget,
    sentinels intact behind every stream, search_waits <= 7 x chunks."""
    lst = R.search_list(fx)
    assert len(lst) == 66 and sum(streams.image(n).size for n, _ in lst) == 12963093
    want_q = [bisect(fx[n]["sizes"], b, 1, 99) for n, b in lst]
    assert len(set(want_q)) == 11
    for n in IMAGES:
        enc = [v for v in fx[n]["sizes"] if v is not None]
        assert all(a < b for a, b in zip(enc, enc[1:])), n
    call = R.SearchCall(L, handle, [streams.image(n) for n, _ in lst], [b for _, b in lst])
    assert call.run() == N.TIC_OK, L.tic_last_error(handle)
    fig = R.figures(L, handle)
    print("search 1..99 figures (batch, single, chunks, probes, waits, size launches):", fig)
    assert list(call.status) == [N.TIC_OK] * 66
    assert list(call.quals) == want_q
    for i, (n, b) in enumerate(lst):
        assert call.lens[i] <= b and call.stream(i) == streams.get(n, want_q[i]), (i, n, b)
        assert call.tail_intact(i), i
    assert fig[0] == 66 and fig[1] == 0 and fig[2] >= 2 and fig[4] <= 7 * fig[2]


def test_search_against_the_recorded_sizes(ctx, fx, streams):
    """7. The 66-frame list (11 distinct expected qualities, 13 MB of pixels, two chunks).  Range (1, 99): see check_search_1_99.
    Range (20, 60): the C call returns TIC_E_SPACE, status[] and out_lens[] are exact for the 18 frames whose q = 20 size exceeds the budget
    (their buffers untouched), the other 48 streams are right; the Python call raises ValueError naming frame 0 and its size at quality 20."""
    L = N.load()
    check_search_1_99(L, ctx.handle, fx, streams)
    lst = R.search_list(fx)
    want = [bisect(fx[n]["sizes"], b, 20, 60) for n, b in lst]
    assert sum(w is ValueError for w in want) == 18 and KeyError not in want and want[0] is ValueError
    call = R.SearchCall(L, ctx.handle, [streams.image(n) for n, _ in lst], [b for _, b in lst], 20, 60)
    assert call.run() == N.TIC_E_SPACE
    assert L.tic_last_error(ctx.handle).decode().startswith("frame 0: %d bytes at quality 20" % fx[lst[0][0]]["sizes"][19])
    for i, (n, b) in enumerate(lst):
        if want[i] is ValueError:
            assert call.status[i] == N.TIC_E_SPACE and call.lens[i] == fx[n]["sizes"][19] and call.tail_intact(i), i
        else:
            assert call.status[i] == N.TIC_OK and call.quals[i] == want[i] and call.stream(i) == streams.get(n, want[i]) and call.tail_intact(i), i
    with pytest.raises(ValueError, match="frame 0: %d bytes at quality 20 exceed" % fx[lst[0][0]]["sizes"][19]):
        T.compress_batch_to_size([streams.image(n) for n, _ in lst], [b for _, b in lst], 20, 60, ctx=ctx)
    # the Python call on the whole range: the same streams and qualities
    got = T.compress_batch_to_size([streams.image(n) for n, _ in lst[:12]], [b for _, b in lst[:12]], ctx=ctx)
    assert got == [(streams.get(n, q), q) for (n, b), q in zip(lst[:12], [bisect(fx[n]["sizes"], b, 1, 99) for n, b in lst[:12]])]
    # a frame without a code at min_quality: KeyError naming it
    with pytest.raises(KeyError, match="frame 1"):
        T.compress_batch_to_size([streams.image("bench40"), streams.image("lenna")], 10 ** 9, 98, 98, ctx=ctx)  # (Lenna has no code from 98 on)


def test_small_searches(ctx, small):
    """8. Test 3's frames, each with its own q = 50 size as the budget: what compress_to_size gives per frame.  Empty frames: budget 16
    gives the header at max_quality, budget 15 a failing status."""
    frames, single, want = small
    budgets = [row[1] for row in want]
    got = T.compress_batch_to_size(frames, budgets, ctx=ctx)
    assert got == [T.compress_to_size(f, b, ctx=ctx) for f, b in zip(frames, budgets)]
    assert all(len(bs) <= b for (bs, q), b in zip(got, budgets))
    got = T.compress_batch_to_size(frames[::-1], budgets[::-1], 5, 80, ctx=ctx)
    assert got == [T.compress_to_size(f, b, 5, 80, ctx=ctx) for f, b in zip(frames[::-1], budgets[::-1])]
    empty = [np.zeros((0, 8), np.uint8), np.zeros((8, 0), np.uint8)]
    assert T.compress_batch_to_size(empty, 16, 5, 80, ctx=ctx) == [(T.compress(e, 80, ctx=ctx), 80) for e in empty]
    call = R.SearchCall(N.load(), ctx.handle, empty + [frames[1]], [15, 16, budgets[1]], 5, 80)
    assert call.run() == N.TIC_E_SPACE
    assert list(call.status) == [N.TIC_E_SPACE, N.TIC_OK, N.TIC_OK] and list(call.lens)[:2] == [16, 16] and call.quals[1] == 80
    assert call.tail_intact(0) and call.tail_intact(1) and call.stream(2) == T.compress_to_size(frames[1], budgets[1], 5, 80, ctx=ctx)[0]
    with pytest.raises(ValueError, match="frame 0: 16 bytes"):
        T.compress_batch_to_size(empty, 15, ctx=ctx)


def test_nothing_written_that_should_not_be(ctx, small):
    """9. caps[i] = the exact length: the sentinel behind every stream is intact.  caps[i] one byte short: TIC_E_SPACE for that frame,
    out_lens[i] = the needed length, its buffer untouched, the other frames delivered."""
    frames, single, want = small
    L = N.load()
    budgets = [row[1] for row in want]
    ref = R.SearchCall(L, ctx.handle, frames, budgets)
    assert ref.run() == N.TIC_OK
    lens = list(ref.lens)
    exact = R.SearchCall(L, ctx.handle, frames, budgets, caps=lens)
    assert exact.run() == N.TIC_OK
    for i in range(len(frames)):
        assert exact.stream(i) == ref.stream(i) and exact.quals[i] == ref.quals[i] and exact.tail_intact(i), i
    short_caps = list(lens)
    for i in (2, 9, 10):  # a ragged frame, the largest one, a frame without blocks
        short_caps[i] -= 1
    short = R.SearchCall(L, ctx.handle, frames, budgets, caps=short_caps)
    assert short.run() == N.TIC_E_SPACE
    assert L.tic_last_error(ctx.handle).decode().startswith("frame 2: output buffer too small")
    for i in range(len(frames)):
        if i in (2, 9, 10):
            assert short.status[i] == N.TIC_E_SPACE and short.lens[i] == lens[i] and short.tail_intact(i), i
        else:
            assert short.status[i] == N.TIC_OK and short.stream(i) == ref.stream(i) and short.tail_intact(i), i


def test_argument_checks_of_the_c_calls(ctx, small):
    """Every argument is checked before any work: "frame i: ..." for the first offender, nothing written."""
    frames, single, want = small
    L = N.load()
    keep, inp, hs, ws, strides = R.frame_arrays(frames[:3])
    out = np.full((3, 2), -7, np.int64)
    bad_q = (C.c_int * 2)(50, 100)
    assert L.tic_stream_sizes_v(ctx.handle, inp, 3, hs, ws, strides, bad_q, 2, out.ctypes.data) == N.TIC_E_QUALITY
    assert L.tic_last_error(ctx.handle).decode().startswith("frame 0: ") and (out == -7).all()
    ok_q = (C.c_int * 2)(50, 60)
    bad_strides = (C.c_ssize_t * 3)(1, 8, 3)
    assert L.tic_stream_sizes_v(ctx.handle, inp, 3, hs, ws, bad_strides, ok_q, 2, out.ctypes.data) == N.TIC_E_ARG
    assert L.tic_last_error(ctx.handle).decode().startswith("frame 2: ") and (out == -7).all()
    assert L.tic_stream_sizes_v(ctx.handle, inp, -1, hs, ws, strides, ok_q, 2, out.ctypes.data) == N.TIC_E_ARG
    assert L.tic_stream_sizes_v(ctx.handle, None, 3, hs, ws, strides, ok_q, 2, out.ctypes.data) == N.TIC_E_ARG
    assert L.tic_stream_sizes_v(ctx.handle, inp, 0, hs, ws, strides, ok_q, 2, out.ctypes.data) == N.TIC_OK
    call = R.SearchCall(L, ctx.handle, frames[:3], [1000] * 3, 60, 20)
    assert call.run() == N.TIC_E_QUALITY and list(call.status) == [-99] * 3
    assert all((b == R.SENTINEL).all() for b in call.bufs)
    call = R.SearchCall(L, ctx.handle, frames[:3], [1000] * 3)
    call.inp[1] = None
    assert call.run() == N.TIC_E_ARG and L.tic_last_error(ctx.handle).decode().startswith("frame 1: null image")
    assert all((b == R.SENTINEL).all() for b in call.bufs) and list(call.status) == [-99] * 3


def test_shipped_library(fx, streams):
    """10. Tests 1 (two images) and 7 (range 1..99) through the library that ships (no test hooks compiled in), bound here beside the
    test-hooks build this process runs."""
    assert N.load().tic_build_has_test_hooks() == 1
    L = C.CDLL(N.LIB_PATH)
    for fn, (res, args) in N.SIGNATURES.items():
        f = getattr(L, fn)
        f.restype, f.argtypes = res, args
    assert L.tic_build_has_test_hooks() == 0
    handle = L.tic_create(0)
    assert handle, L.tic_last_error(None)
    try:
        names = ("lenna", "noise256_seed7")
        rc, got = R.sizes_v(L, handle, [streams.image(n) for n in names], list(range(1, 100)))
        assert rc == 0 and got.tolist() == [[-1 if v is None else v for v in fx[n]["sizes"]] for n in names]
        check_search_1_99(L, handle, fx, streams)
    finally:
        L.tic_destroy(handle)
