"""tic_decompress_batch at its edges: the work buffer's bound (a batch must decode whatever the context decoded before), destinations laid out
as an arena (bytes between two frames are the caller's) and a chunk the batch launcher refuses (its frames fall back, the call does not fail).

Bar: every frame equals oracle.decompress of the same stream, bit for bit.  Run with `-m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest

from conftest import rand_frame
from test_gpu_parity import mixed_batch_streams

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(0)
    assert c.arch.startswith("gfx950"), c.arch
    yield c
    c.close()


def run_batch(L, handle, streams, out_ptrs, caps):
    """tic_decompress_batch through the C-ABI -> (return code, geometries)."""
    n = len(streams)
    bufs = [np.frombuffer(s, np.uint8) for s in streams]
    hs, ws = (C.c_int * n)(), (C.c_int * n)()
    rc = L.tic_decompress_batch(handle, (C.c_void_p * n)(*[b.ctypes.data for b in bufs]), (C.c_size_t * n)(*[b.size for b in bufs]), n,
                                (C.c_void_p * n)(*out_ptrs), (C.c_size_t * n)(*caps), hs, ws)
    return rc, list(zip(hs, ws))


def counts(L, handle):
    """(batch_frames, single_frames, chunks, direct_frames) of the last tic_decompress_batch."""
    v = [C.c_int() for _ in range(4)]
    assert L.tic_last_decompress_batch(handle, *[C.byref(x) for x in v]) == N.TIC_OK
    return tuple(x.value for x in v)


def work(L, handle):
    """(range_bits, work_used, work_held) of the last chunk handed to the batch launcher."""
    r, used, held = C.c_int(), C.c_size_t(), C.c_size_t()
    assert L.tic_last_decompress_batch_work(handle, C.byref(r), C.byref(used), C.byref(held)) == N.TIC_OK
    return r.value, used.value, held.value


def range_rule(nbytes, nblocks):
    """csrc/tic_entropy_dec_gpu.h dec_range_rule: the stream bits per lane a frame asks for (a chunk takes the largest of its frames')."""
    floor_words = 33 if nbytes * 8 < 7 * nblocks else 9
    k = ((2 * nbytes * 8) // nblocks + 31) // 32 | 1
    return min(max(k, floor_words), 63) * 32


def ranges_of(nbytes, r):
    return -(-(nbytes * 8 - 128) // r)


@pytest.fixture(scope="module")
def flat(oracle):
    """The flat 192 x 472 frame at pixel value 128: 1,416 blocks of 6 bits (2-bit DC code, end-of-block), the sparsest stream there is."""
    img = np.full((192, 472), 128, np.uint8)
    s = oracle.compress(img, 50)
    assert len(s) == 1078 and range_rule(len(s), 1416) == 1056
    return s, oracle.decompress(s)


def decode_copies(L, handle, s, want, n):
    """n copies of one stream in one batch, each into its own part of one block (the frame is a whole number of 256 bytes: back to back)."""
    out = np.full((n, want.size), 0xCD, np.uint8)
    rc, geo = run_batch(L, handle, [s] * n, [out.ctypes.data + k * want.size for k in range(n)], [want.size] * n)
    print("batch of %d: rc %d, counts %s, range / work used / held %s" % (n, rc, counts(L, handle), work(L, handle)))
    assert rc == N.TIC_OK, (n, rc, L.tic_last_error(handle).decode(), work(L, handle))
    assert geo == [want.shape] * n
    assert (out == want.reshape(1, -1)).all(), (n, np.flatnonzero((out != want.reshape(1, -1)).any(1))[:8])
    assert counts(L, handle)[0] == n and counts(L, handle)[1] == 0, (n, counts(L, handle))


def history_sequence(L, handle, flat, sizes):
    s, want = flat
    # alone in a batch of two the frame is a batch frame: nothing below can pass by falling to the single-frame call or the host decoder
    decode_copies(L, handle, s, want, 2)
    assert work(L, handle)[0] == 1056
    for n in sizes:
        decode_copies(L, handle, s, want, n)
        r, used, held = work(L, handle)
        assert r == 1056 and used == L.tic_decode_work_bytes(n, n * 9, n * 1416, 1056) and used <= held, (n, r, used, held)


def test_a_batch_decodes_whatever_the_context_decoded_before(flat):
    """The work buffer is sized from the stream lengths at 288 bits per range and carved up at the chunk's range.  The flat frame takes 1,056-bit
    ranges: 9 ranges of 178 trace entries where (8,624 / 288 + 2) x 50 were provided, 208 bytes short per frame, and a context whose buffer had
    grown (by a quarter more than asked) for 160 of them refused 200 - the whole call failed with TIC_E_HIP; likewise 100, then 125.  Now
    every one of these batches returns TIC_OK with every frame on the batch kernels and equal to the oracle's, and the chunk's carve-up
    (tic_last_decompress_batch_work) is the header's figure and fits what the context holds."""
    L = N.load()
    c = T.Context(0)
    try:
        history_sequence(L, c.handle, flat, (160, 200, 100, 125))
    finally:
        c.close()


def test_the_same_on_the_shipped_library(flat):
    """160, then 200 copies on the library that ships (no test hooks compiled in), bound beside the test-hooks build this process runs."""
    assert N.load().tic_build_has_test_hooks() == 1
    L = C.CDLL(N.LIB_PATH)
    for fn, (res, args) in N.SIGNATURES.items():
        f = getattr(L, fn)
        f.restype, f.argtypes = res, args
    assert L.tic_build_has_test_hooks() == 0
    handle = L.tic_create(0)
    assert handle, L.tic_last_error(None)
    try:
        history_sequence(L, handle, flat, (160, 200))
    finally:
        L.tic_destroy(handle)


def sparse_stream(oracle, rng, h, w, nbytes):
    """A stream of exactly `nbytes` bytes for an h x w frame of flat 8 x 8 blocks: value 128 (6 bits a block), `t` isolated blocks of 130 (a DC step
    of +1 and one of -1 at q = 50: 4 bits more).  None when the geometry cannot give that length."""
    n = (h // 8) * (w // 8)
    t = (8 * (nbytes - 16) - 6 * n) // 4
    if t < 0 or t > (n - 1) // 2:
        return None
    blocks = np.full(n, 128, np.uint8)
    blocks[2 * rng.choice((n - 1) // 2, t, replace=False)] = 130  # (even indices, never the last block: every step is followed by its way back)
    img = np.kron(blocks.reshape(h // 8, w // 8), np.ones((8, 8), np.uint8))
    s = oracle.compress(img, 50)
    assert len(s) == nbytes, (h, w, nbytes, len(s))
    return s


def test_sparse_frames_behind_a_dense_one(ctx, oracle):
    """The mixed form: 120 short sparse streams - 1,089 .. 1,500 blocks at 6 .. 8.7 bits per block, lengths at which a frame's trace entries at the
    chunk's range exceed its share of the 288-bit figure (checked for each with the header's carve-up, tic_decode_work_bytes) - and behind them
    one 512 x 512 frame of noise at q = 90, whose own choice is 864 bits.  The chunk's range is the largest of its frames' choices
    (tic_last_decompress_batch_work): 1,056 bits, from the sparse frames below 7 bits per block.  (The dense frame's own share of the 288-bit figure
    is some 30 KB more than it needs at that range, which is why this batch was not refused before the bound was fixed; the equal batches above
    were.)  One chunk, every frame on the batch kernels, every frame the oracle's."""
    L = N.load()
    rng = np.random.default_rng(20)
    geos = [(264, 264), (192, 472), (200, 480), (256, 320), (240, 328), (208, 400), (224, 392)]
    noise = T.compress(rand_frame(41, 512, 512), 90, ctx=ctx)
    assert range_rule(len(noise), 4096) >= 864
    R = 1056
    lens = [nb for nb in range(1040, 1900) if 4 * ranges_of(nb, R) * (R // 6 + 2) - (nb * 8 // 288 + 2) * 200 >= 100]  # the parent's per-frame figure, >= 100 bytes short
    assert lens[0] == 1073 and len(lens) >= 30
    streams = []
    for i in range(4 * len(lens) * len(geos)):
        h, w = geos[i % len(geos)]
        s = sparse_stream(oracle, rng, h, w, lens[(i // len(geos)) % len(lens)])
        if s is not None:
            streams.append(s)
        if len(streams) == 120:
            break
    assert len(streams) == 120 and len(set(streams)) >= 100
    nblk = [L.tic_num_blocks(hd["height"], hd["width"]) for hd in map(T.parse_header, streams)]
    for s, n in zip(streams, nblk):
        assert 1024 <= n <= 1500 and 6 * n <= (len(s) - 16) * 8 <= 10 * n and len(s) >= 1040, (n, len(s))
        # the header's carve-up, rounding taken out (128 frames' ranges make every piece a whole number of 256 B): this frame's two traces
        traces = (L.tic_decode_work_bytes(1, 128 * ranges_of(len(s), R), 0, R) - 256) // 128
        assert traces > (len(s) * 8 // 288 + 2) * 200, (len(s), traces)
    assert any(len(s) * 8 < 7 * n for s, n in zip(streams, nblk))
    streams.append(noise)
    nblk.append(4096)
    assert max(range_rule(len(s), n) for s, n in zip(streams, nblk)) == R
    want = [oracle.decompress(s) for s in streams]
    outs = [np.full(w_.size + 64, 0xCD, np.uint8) for w_ in want]
    for _ in range(2):  # (the second time on the buffers the first left)
        rc, geo = run_batch(L, ctx.handle, streams, [o.ctypes.data for o in outs], [w_.size for w_ in want])
        assert rc == N.TIC_OK, L.tic_last_error(ctx.handle).decode()
        print("mixed: counts %s, range / work used / held %s" % (counts(L, ctx.handle), work(L, ctx.handle)))
        assert counts(L, ctx.handle)[:3] == (121, 0, 1)
        r, used, held = work(L, ctx.handle)
        assert r == R and used <= held
        assert used == L.tic_decode_work_bytes(121, sum(ranges_of(len(s), R) for s in streams), sum(nblk), R)
        for k, (o, w_) in enumerate(zip(outs, want)):
            assert geo[k] == w_.shape and np.array_equal(o[: w_.size].reshape(w_.shape), w_) and (o[w_.size:] == 0xCD).all(), k
            o[:] = 0xCD


class PinnedBlock:
    """tic_host_alloc_pinned memory as a numpy array."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.p = ctx, C.c_void_p()
        ctx.check(N.load().tic_host_alloc_pinned(ctx.handle, nbytes, C.byref(self.p)))
        self.a = np.frombuffer((C.c_uint8 * nbytes).from_address(self.p.value), np.uint8)

    def free(self):
        self.a = None
        self.ctx.check(N.load().tic_host_free_pinned(self.ctx.handle, self.p))


def test_an_arena_keeps_the_bytes_between_its_frames(oracle):
    """8 frames of noise, 264 x 264 at q = 50 (1,089 blocks; h * w = 272 x 256 + 64), into ONE host block at distances of align_up(h * w, 256) with
    caps[k] = h * w: the device pixel buffer has the same distances, and the single copy that brought such a block down (557 KB: the registering
    route) wrote the device buffer's padding over the 192 bytes between two frames - bytes the caller never gave away.  Every frame is the
    oracle's and every byte outside the frames keeps the fill, with two fills on one context (a stale byte of the device buffer cannot match
    both), in pageable memory and in pinned memory of tic_host_alloc_pinned.  Frames of a whole number of 256 bytes laid back to back (8 of
    512 x 512) still come down in one copy: direct_frames == 8."""
    L = N.load()
    c = T.Context(0)
    pin = None
    try:
        h = w = 264
        hw, pad = h * w, (h * w + 255) // 256 * 256
        assert hw % 256 == 64 and L.tic_num_blocks(h, w) == 1089
        streams = [T.compress(rand_frame(50 + k, h, w), 50, ctx=c) for k in range(8)]
        want = [oracle.decompress(s) for s in streams]
        size = 8 * pad + 256
        pin = PinnedBlock(c, size)
        for name, arena in (("pageable", np.empty(size, np.uint8)), ("pinned", pin.a)):
            for fill in (0xCD, 0x32):
                arena[:] = fill
                rc, geo = run_batch(L, c.handle, streams, [arena.ctypes.data + k * pad for k in range(8)], [hw] * 8)
                assert rc == N.TIC_OK, L.tic_last_error(c.handle).decode()
                nb, ns, nc, nd = counts(L, c.handle)
                print("arena (%s, fill 0x%02X): batch_frames %d, single_frames %d, chunks %d, direct_frames %d" % (name, fill, nb, ns, nc, nd))
                assert (nb, ns, nc) == (8, 0, 1) and geo == [(h, w)] * 8
                for k in range(8):
                    assert np.array_equal(arena[k * pad: k * pad + hw].reshape(h, w), want[k]), (name, fill, k)
                    gap = arena[k * pad + hw: (k + 1) * pad]
                    assert gap.size == 192 and (gap == fill).all(), (name, fill, k, np.flatnonzero(gap != fill)[:8], gap[gap != fill][:8])
                assert (arena[8 * pad:] == fill).all(), (name, fill)
        # caps that reach to the next frame give the gaps away: such an arena may take the single copy, and the frames are the oracle's either way
        arena = np.full(size, 0xCD, np.uint8)
        rc, _ = run_batch(L, c.handle, streams, [arena.ctypes.data + k * pad for k in range(8)], [pad] * 7 + [hw])
        assert rc == N.TIC_OK and counts(L, c.handle)[:3] == (8, 0, 1)
        print("arena with padded caps: direct_frames %d" % counts(L, c.handle)[3])
        for k in range(8):
            assert np.array_equal(arena[k * pad: k * pad + hw].reshape(h, w), want[k]), k
        assert (arena[7 * pad + hw:] == 0xCD).all()
        # the fast path stays: whole numbers of 256 bytes, back to back
        streams = [T.compress(rand_frame(60 + k, 512, 512), 50, ctx=c) for k in range(8)]
        want = [oracle.decompress(s) for s in streams]
        block = np.full(8 * 512 * 512 + 256, 0xCD, np.uint8)
        rc, _ = run_batch(L, c.handle, streams, [block.ctypes.data + k * 512 * 512 for k in range(8)], [512 * 512] * 8)
        assert rc == N.TIC_OK and counts(L, c.handle) == (8, 0, 1, 8), counts(L, c.handle)
        for k in range(8):
            assert np.array_equal(block[k * 512 * 512: (k + 1) * 512 * 512].reshape(512, 512), want[k]), k
        assert (block[8 * 512 * 512:] == 0xCD).all()
    finally:
        if pin is not None:
            pin.free()
        c.close()


def test_a_refused_chunk_falls_back(ctx, oracle, golden, monkeypatch):
    """TIC_DBATCH_WORK_CAP=4096 (test-hooks build only) caps the work buffer handed to the batch launcher: it refuses the chunk of the 14-stream mix
    of test_decompress_batch_mixed_streams, and every frame takes the single-frame call - TIC_OK, every frame the oracle's, batch_frames == 0,
    single_frames == the non-empty frames.  Before, the refusal was the whole call's TIC_E_HIP and no frame was decoded.
    The refusal is entropy_decode_idct_gpu_batch's host-side size check ('cv.end > work_bytes' -> hipErrorInvalidValue), which stands in front of
    both hipLaunchKernelGGL calls of that function: no kernel runs on the too-small buffer.  That is read off the code, not measured here."""
    L = N.load()
    streams = mixed_batch_streams(ctx, golden)
    assert len(streams) == 14
    want = [oracle.decompress(s) for s in streams]
    nonempty = sum(1 for w_ in want if w_.size)
    assert nonempty == 13
    outs = [np.full(max(w_.size, 1) + 64, 0xCD, np.uint8) for w_ in want]
    monkeypatch.setenv("TIC_DBATCH_WORK_CAP", "4096")
    rc, geo = run_batch(L, ctx.handle, streams, [o.ctypes.data for o in outs], [w_.size for w_ in want])
    assert rc == N.TIC_OK, L.tic_last_error(ctx.handle).decode()
    nb, ns, nc, nd = counts(L, ctx.handle)
    r, used, held = work(L, ctx.handle)
    print("refused chunk: counts %s, range %d, work used %d, held %d" % ((nb, ns, nc, nd), r, used, held))
    assert held == 4096 and used > held
    assert (nb, ns, nd) == (0, nonempty, 0)
    for k, (o, w_) in enumerate(zip(outs, want)):
        assert geo[k] == w_.shape and np.array_equal(o[: w_.size].reshape(w_.shape), w_) and (o[w_.size:] == 0xCD).all(), k
    # without the cap the same call is the batch kernels' again
    monkeypatch.delenv("TIC_DBATCH_WORK_CAP")
    rc, _ = run_batch(L, ctx.handle, streams, [o.ctypes.data for o in outs], [w_.size for w_ in want])
    assert rc == N.TIC_OK and counts(L, ctx.handle)[0] >= 8
    for k, (o, w_) in enumerate(zip(outs, want)):
        assert np.array_equal(o[: w_.size].reshape(w_.shape), w_), k


def device_decoder_takes(nblocks, nbytes):
    """csrc/tic_api.hip device_decoder_takes at its defaults: at least 1,024 blocks and 8,192 stream bits behind the 16-byte header."""
    return nblocks >= 1024 and nbytes * 8 >= 128 + 8192


@pytest.fixture(scope="module")
def ten_streams(ctx, oracle):
    """Ten streams for chunks of three: four 256 x 256 frames of noise (1,024 blocks: the smallest frame the device decoder takes) at q = 50, 90,
    50, 10, a 264 x 260 one (row pitch 264 in the device buffer), 203 x 517 at q = 90, 64 x 64 (too short: single-frame), an empty image, the first
    stream cut at two thirds (taken, then flagged: single-frame), one more 256 x 256 -> (streams, the oracle's images, E = how many the batch takes)."""
    L = N.load()
    imgs = [(rand_frame(71, 256, 256), 50), (rand_frame(72, 256, 256), 90), (rand_frame(73, 256, 256), 50), (rand_frame(74, 256, 256), 10),
            (rand_frame(75, 264, 260), 50), (rand_frame(76, 203, 517), 90), (rand_frame(77, 64, 64), 50), (np.zeros((0, 8), np.uint8), 50)]
    streams = [T.compress(im, q, ctx=ctx) for im, q in imgs]
    streams.append(streams[0][: len(streams[0]) * 2 // 3])
    streams.append(T.compress(rand_frame(78, 256, 256), 50, ctx=ctx))
    want = [oracle.decompress(s) for s in streams]
    takes = [device_decoder_takes(L.tic_num_blocks(hd["height"], hd["width"]), len(s)) for hd, s in zip(map(T.parse_header, streams), streams)]
    assert takes == [True] * 6 + [False, False, True, True] and sum(1 for w_ in want if w_.size) == 9
    return streams, want, sum(takes)


def decode_scattered(L, handle, streams, want):
    """One tic_decompress_batch into scattered destinations, each 64 bytes longer than its frame and pre-filled with 0xCD: every frame the oracle's,
    hs / ws right, the guard bytes untouched -> the call's counts."""
    outs = [np.full(w_.size + 64, 0xCD, np.uint8) for w_ in want]
    rc, geo = run_batch(L, handle, streams, [o.ctypes.data for o in outs], [w_.size for w_ in want])
    assert rc == N.TIC_OK, L.tic_last_error(handle).decode()
    for k, (o, w_) in enumerate(zip(outs, want)):
        assert geo[k] == w_.shape, (k, geo[k])
        assert np.array_equal(o[: w_.size].reshape(w_.shape), w_), k
        assert o[w_.size:].size == 64 and (o[w_.size:] == 0xCD).all(), k
    return counts(L, handle)


def test_several_chunks(ctx, ten_streams, monkeypatch):
    """TIC_DBATCH_CHUNK (test-hooks build only) sets the frames per chunk: with 3 the ten streams are ceil(E / 3) chunks - the second and third packed
    into the upload buffer the first left, descriptors, ranges, tiles and workgroups starting over, the single-frame list collecting over chunks
    (the cut stream is flagged in the third) - and with 1 a chunk per frame; without the hook one chunk.  Every time every frame is the oracle's."""
    L = N.load()
    if not L.tic_build_has_test_hooks():
        pytest.skip("needs chunks of 3 frames (TIC_DBATCH_CHUNK, a test hook)")
    streams, want, E = ten_streams
    assert E == 8
    monkeypatch.setenv("TIC_DBATCH_CHUNK", "3")
    nb, ns, nc, nd = decode_scattered(L, ctx.handle, streams, want)
    print("chunks of 3: batch_frames %d, single_frames %d, chunks %d, direct_frames %d" % (nb, ns, nc, nd))
    assert nc == (E + 2) // 3 and nb + ns == 9 and ns >= 2 and nb >= E - 1
    monkeypatch.setenv("TIC_DBATCH_CHUNK", "1")
    nb, ns, nc, nd = decode_scattered(L, ctx.handle, streams, want)
    print("chunks of 1: batch_frames %d, single_frames %d, chunks %d, direct_frames %d" % (nb, ns, nc, nd))
    assert nc == E and nb + ns == 9 and ns >= 2 and nb >= E - 1
    monkeypatch.delenv("TIC_DBATCH_CHUNK")
    nb, ns, nc, nd = decode_scattered(L, ctx.handle, streams, want)
    print("no hook: batch_frames %d, single_frames %d, chunks %d, direct_frames %d" % (nb, ns, nc, nd))
    assert nc == 1 and nb + ns == 9 and ns >= 2 and nb >= E - 1


def test_every_chunk_refused(ctx, ten_streams, monkeypatch):
    """The same streams in chunks of 3 with TIC_DBATCH_WORK_CAP=4096: the launcher refuses all three chunks, each refusal drains the stream before the
    next chunk is packed into the same pinned upload buffer, and every frame takes the single-frame call.  The call behind it, without the two
    hooks, decodes in chunks again."""
    L = N.load()
    if not L.tic_build_has_test_hooks():
        pytest.skip("needs TIC_DBATCH_CHUNK and TIC_DBATCH_WORK_CAP (test hooks)")
    streams, want, E = ten_streams
    monkeypatch.setenv("TIC_DBATCH_CHUNK", "3")
    monkeypatch.setenv("TIC_DBATCH_WORK_CAP", "4096")
    nb, ns, nc, nd = decode_scattered(L, ctx.handle, streams, want)
    print("every chunk refused: batch_frames %d, single_frames %d, chunks %d, direct_frames %d" % (nb, ns, nc, nd))
    assert (nb, ns, nc) == (0, 9, 0)
    monkeypatch.delenv("TIC_DBATCH_CHUNK")
    monkeypatch.delenv("TIC_DBATCH_WORK_CAP")
    nb, ns, nc, nd = decode_scattered(L, ctx.handle, streams, want)
    assert nc == 1 and nb >= E - 1 and nb + ns == 9
