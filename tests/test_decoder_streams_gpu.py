"""The device decoder's Huffman walk (tinyimgcodec_amd/csrc/tic_entropy_dec_gpu.hip: the measure walk's chain tables mdc / mac / mlong, the
stitch from range to range, the fused kernel's phase 1 with the pair table ac2 and the long-codeword table long32) on BUILT streams:
tests/decoder_streams.py builds the frames, tests/golden/decoder_streams.json holds what the unmodified reference wrote for them and the
pixels it read back.  Every fused pair at its extreme values at every word alignment, every long codeword behind and in front of every
kind of neighbour, 600- to 1,662-bit blocks among 6-bit ones under the 288- and 1,056-bit ranges, ranges filled with block starts, a
running DC on the int16 boundary.  tests/test_decoder_streams_cpu.py shows on the CPU that the frames reach these states and that a
wrong coefficient in the value-bearing frames would change a pixel.

The fixture is the expectation (pixel digests); the oracle only names the first differing pixel in a failure message.  Besides the
pixels every test asserts the PATH: a walk that goes wrong quietly raises a give-up bit and the host decodes the stream again - right
pixels, and a device decoder that does not work.  Run with `-m gpu` on an MI355X."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import decoder_streams as DS
import entropy_blocks as EB
import inverse_edges as IE

import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N

pytestmark = pytest.mark.gpu

FX = DS.load_fixture()["frames"]
NAMES = list(FX)
TAIL = 64                      # sentinel bytes behind every output buffer
GIVEUP_WIDE_DC = 512           # include/tinyimgcodec_hip.h, tic_last_decode_giveup: a running DC outside int16
GIVEUP_DOCUMENTED = 1 | 2 | 4 | 8 | 16 | 32 | 64 | 128 | 256 | 512
# The one frame that may leave the device decoder although it is well formed: 2,145 equal 6-bit blocks, an exactly periodic bit pattern in
# which a speculative walk that starts out of step never falls in step (tic_api.hip decode_range_bits: "nearly flat content ... is
# periodic bit patterns in which a walk can stay out of step for tens of ranges"); cap is its twin with a seeded, aperiodic tail.
MAY_HAND_OVER = ("zeros",)
# A well-formed, aperiodic frame whose FIRST run gives up, a finding of these tests: spikes_sparse at 288 bits per lane, the range its
# average asks for.  Its spikes sit in three neighbouring blocks around every multiple of 256 (3,362 .. 4,424 bits: 11 .. 15 ranges of 288
# bits with two block starts among them); a walk that starts inside a 1,662-bit block of 26-bit symbols does not fall in step before the
# block ends, so more ranges in a row stay without a synchronisation point than the stitch hands an exit over (stitch_rounds() = 8,
# tic_entropy_dec_gpu.hip: "more ranges in a row than rounds without a synchronisation point" - give-up bit 4).  The documented rule for
# that: tic_decompress runs once more at 2,016 bits (tic_api.hip decode_on_device) and stays on the device decoder; a chunk of
# tic_decompress_batch runs once, so there the frame is flagged and decoded by tic_decompress behind the batch.  From 544 bits on one run
# is enough (test_forced_ranges).  name -> the ranges at which the first run gives up.
# dense_max (1,662 bits in every block) is the same case when 288 bits are forced on it; its own rule gives 2,016.
SECOND_RUN = {"spikes_sparse": (288,), "dense_max": (288,)}
FORCED = ("spikes_flat_one", "spikes_flat_two", "spikes_sparse", "dense_max", "cap", "long_codes", "pairs")


def plain_key(name):
    """The plain variant a test takes where it takes one: the finest quality of the frame."""
    return "q%d" % max(q for flag, q in FX[name]["variants"] if not flag)


def scaled(key):
    return key.startswith("s")


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(0)
    assert c.arch.startswith("gfx950"), c.arch
    yield c
    c.close()


@pytest.fixture(scope="module")
def streams(oracle):
    """(name, variant key) -> stream bytes, built once: the oracle's payload under every header variant, tied to the fixture's digests."""
    frames = DS.build_frames(EB.Lengths(oracle.dump_tables()))
    assert sorted(frames) == sorted(NAMES)
    out = {}
    for name, fr in frames.items():
        payload = DS.payload_stream(oracle, fr)
        for variant in fr["variants"]:
            s = DS.with_header(payload, fr, variant)
            rec = FX[name]["streams"][DS.key(variant)]
            assert (len(s), EB.sha(s)) == (rec["bytes"], rec["sha256"]), (name, variant)
            out[name, DS.key(variant)] = s
    return out


def check_pixels(name, key, px, s, oracle, what):
    if px.shape != (DS.H, DS.W) or IE.px_sha(px) != FX[name]["streams"][key]["pixels_sha256"]:
        want = oracle.decompress(s)  # (diagnosis only)
        pytest.fail("%s, %s %s: %s" % (what, name, key, DS.first_difference(px, want)))


def check_path(name, path, giveup, what=""):
    """(1, 0) - the device decoder, nothing flagged - for every frame but the twins (the running DC leaves int16: host route, bit 512
    alone) and the exactly periodic frame (either, with documented bits)."""
    if DS.is_twin(name):
        assert (path, giveup) == (2, GIVEUP_WIDE_DC), (what, name, path, giveup)
    elif name in MAY_HAND_OVER and path != 1:
        assert path == 2 and giveup != 0 and giveup & ~GIVEUP_DOCUMENTED == 0, (what, name, path, giveup)
    else:
        assert (path, giveup) == (1, 0), (what, name, path, giveup)


def decompress(L, handle, s):
    buf = np.frombuffer(s, np.uint8)
    out = np.full(DS.H * DS.W + TAIL, 0xA5, np.uint8)
    rc = L.tic_decompress(handle, buf.ctypes.data, buf.size, out.ctypes.data, DS.H * DS.W)
    assert rc == N.TIC_OK, (rc, L.tic_last_error(handle).decode())
    assert (out[DS.H * DS.W:] == 0xA5).all(), "bytes behind the caller's buffer were written"
    return out[: DS.H * DS.W].reshape(DS.H, DS.W)


def state(L, handle):
    r, tries = C.c_int(), C.c_int()
    assert L.tic_last_decode_range(handle, C.byref(r), C.byref(tries)) == N.TIC_OK
    return L.tic_last_decode_path(handle), L.tic_last_decode_giveup(handle), r.value, tries.value


# ---- tic_decompress ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_default_route(name, ctx, streams, oracle):
    """What tic_decompress does on its own, every variant: the fixture's pixels from the device decoder, in one run at the range the rule
    gives or in two with the longest."""
    L = N.load()
    rule = FX[name]["census"]["range_rule"]
    for flag, q in FX[name]["variants"]:
        key = DS.key((flag, q))
        px = decompress(L, ctx.handle, streams[name, key])
        path, giveup, r, tries = state(L, ctx.handle)
        print("%-22s %-4s -> path %d, giveup %d, range %d bits (rule %d), tries %d" % (name, key, path, giveup, r, rule, tries))
        check_pixels(name, key, px, streams[name, key], oracle, "default route")
        check_path(name, path, giveup)
        if path == 1:  # one run at the range the rule gives - or, for the frame named in SECOND_RUN, two
            assert (r, tries) == ((2016, 2) if rule in SECOND_RUN.get(name, ()) else (rule, 1)), (name, key, r, tries)


@pytest.mark.parametrize("name", NAMES)
def test_host_route(name, ctx, streams, oracle, monkeypatch):
    """TIC_DECODE_HOST=1 (test-hooks build): the host decoder's coefficients through idct_kernel."""
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_DECODE_HOST", "1")
    for flag, q in FX[name]["variants"]:
        key = DS.key((flag, q))
        px = decompress(L, ctx.handle, streams[name, key])
        assert L.tic_last_decode_path(ctx.handle) == 2, (name, key)
        check_pixels(name, key, px, streams[name, key], oracle, "host route")


def forced_set(L, handle, streams, oracle, forced, what):
    for name in FORCED:
        key = plain_key(name)
        px = decompress(L, handle, streams[name, key])
        path, giveup, r, tries = state(L, handle)
        print("%s: %-16s -> path %d, giveup %d, range %d bits, tries %d" % (what, name, path, giveup, r, tries))
        check_pixels(name, key, px, streams[name, key], oracle, what)
        assert (path, giveup) == (1, 0), (what, name, path, giveup)
        first = forced if forced else FX[name]["census"]["range_rule"]
        assert (r, tries) in ((first, 1), (2016, 2)), (what, name, r, tries)
        assert (tries == 2) == (first in SECOND_RUN.get(name, ())), (what, name, r, tries)  # the second run where SECOND_RUN names it, nowhere else


@pytest.mark.parametrize("forced", [288, 544, 1056, 2016])
def test_forced_ranges(forced, ctx, streams, oracle, monkeypatch):
    """TIC_DECODE_RANGE: the spikes frames, dense_max, cap, long_codes and pairs with every lane walking `forced` stream bits - a 1,662-bit
    block passes over five ranges of 288 bits, a range of 2,016 holds 336 block starts.  The device decoder all the same, at the forced
    range or, where a range holds no block start, in a second run at the longest."""
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_DECODE_RANGE", str(forced))
    forced_set(L, ctx.handle, streams, oracle, forced, "forced range %d" % forced)


def test_flat_grid(ctx, streams, oracle, monkeypatch):
    """TIC_DECODE_FLAT_GRID=0: the same set with the sums in front of a workgroup taken by look-back (the form launches beyond 4,096
    workgroups use)."""
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_DECODE_FLAT_GRID", "0")
    forced_set(L, ctx.handle, streams, oracle, 0, "look-back sums")


def test_the_frames_reach_all_four_fused_kernels():
    """By the size rule of entropy_decode_idct_gpu (stream bits / blocks <= 240: the 2,048-word window), with and without the scaled branch."""
    seen = {(e["census"]["bits_per_block"] <= 240, bool(flag)) for n, e in FX.items() if not DS.is_twin(n) for flag, q in e["variants"]}
    assert seen == {(True, False), (False, False), (True, True), (False, True)}


# ---- tic_decompress_batch ---------------------------------------------------------------------------------------------------------------
def expected_singles(jobs, per_chunk):
    """The frames of a call that the single-frame call decodes behind the batch, in the caller's order, by the code's own rules:
    scaled_dct frames are in no chunk; the twins are in one, flagged by the kernels (bit 512); a chunk runs ONCE, at the largest
    dec_range_rule of its frames (tic_decode_plan.h dec_plan_close_chunk) - a frame that gives up at that range (SECOND_RUN) is flagged
    with bit 4 and decoded again by tic_decompress, which alone has the second run.  Chunks: the frames taken, in order, `per_chunk` at
    a time (streams and pixels of these calls stay far inside a chunk's byte limits)."""
    taken = [j for j in jobs if not scaled(j[1])]
    out = [j for j in jobs if scaled(j[1])]
    for i in range(0, len(taken), per_chunk):
        chunk = taken[i:i + per_chunk]
        chunk_range = max(FX[n]["census"]["range_rule"] for n, k in chunk)
        out += [j for j in chunk if DS.is_twin(j[0]) or chunk_range in SECOND_RUN.get(j[0], ())]
    return sorted(out, key=jobs.index), (len(taken) + per_chunk - 1) // per_chunk


def single_state(name):
    """(path, giveup, range, tries) tic_decompress leaves behind a frame that went single."""
    if DS.is_twin(name):
        return (2, GIVEUP_WIDE_DC, FX[name]["census"]["range_rule"], 1)
    rule = FX[name]["census"]["range_rule"]
    return (1, 0, 2016, 2) if rule in SECOND_RUN.get(name, ()) else (1, 0, rule, 1)


def run_batch(L, handle, jobs, streams, oracle, what, per_chunk=1024):
    n = len(jobs)
    bufs = [np.frombuffer(streams[j], np.uint8) for j in jobs]
    outs = [np.full(DS.H * DS.W + TAIL, 0xA5, np.uint8) for _ in jobs]
    rc = L.tic_decompress_batch(handle, (C.c_void_p * n)(*[b.ctypes.data for b in bufs]), (C.c_size_t * n)(*[b.size for b in bufs]), n,
                                (C.c_void_p * n)(*[o.ctypes.data for o in outs]), (C.c_size_t * n)(*[DS.H * DS.W] * n), None, None)
    assert rc == N.TIC_OK, (rc, L.tic_last_error(handle).decode())
    v = [C.c_int() for _ in range(4)]
    assert L.tic_last_decompress_batch(handle, *[C.byref(x) for x in v]) == N.TIC_OK
    batch_frames, single_frames, chunks, _ = (x.value for x in v)
    last = state(L, handle)
    singles, want_chunks = expected_singles(jobs, per_chunk)
    print("%s: %d frames -> batch_frames %d, single_frames %d, chunks %d; expected behind the batch %s; last single-frame decode: path %d, giveup %d, "
          "range %d, tries %d" % ((what, n, batch_frames, single_frames, chunks, [j[0] for j in singles]) + last))
    for (name, key), o in zip(jobs, outs):
        assert (o[DS.H * DS.W:] == 0xA5).all(), (what, name, key)
        check_pixels(name, key, o[: DS.H * DS.W].reshape(DS.H, DS.W), streams[name, key], oracle, what)
    assert chunks == want_chunks, (what, chunks, want_chunks)
    # The single-frame calls run in the caller's order, so the decoder's last state is that of the last frame behind the batch.  The one
    # named exception to the expected set is the exactly periodic frame (MAY_HAND_OVER): if the batch kernels flag it, it is one more
    # single frame - and, the last name of the fixture, the last one decoded: its state shows that, not a count with slack.
    extra = []
    if singles and last != single_state(singles[-1][0]) or not singles and single_frames:
        extra = [j for j in jobs if j[0] in MAY_HAND_OVER and not scaled(j[1]) and (not singles or jobs.index(j) > jobs.index(singles[-1]))][-1:]
        assert extra and (last[0] == 2 and last[1] & ~GIVEUP_DOCUMENTED == 0 and last[1] != 0 or last == single_state(extra[0][0])), (what, last, singles)
        print("%s: %s was flagged by the batch kernels and decoded behind the batch" % (what, extra[0][0]))
    assert (batch_frames, single_frames) == (n - len(singles) - len(extra), len(singles) + len(extra)), (what, batch_frames, single_frames, singles, extra)


def every_frame():
    return [(n, plain_key(n)) for n in NAMES]


def small_window():
    return [(n, plain_key(n)) for n in NAMES if FX[n]["census"]["bits_per_block"] <= 240]


def test_batch_every_frame(ctx, streams, oracle):
    """One plain variant of every frame in one call (dense_max gives the chunk the 4,096-word window and the longest range); the twins
    are decoded behind the batch."""
    run_batch(N.load(), ctx.handle, every_frame(), streams, oracle, "every frame")


def test_batch_small_window(ctx, streams, oracle):
    """Only frames of at most 240 stream bits per block: the batch form of the fused kernel with the 2,048-word window."""
    jobs = small_window()
    assert len(jobs) >= 20 and ("dense_max", plain_key("dense_max")) not in jobs
    run_batch(N.load(), ctx.handle, jobs, streams, oracle, "small window")


def test_batch_in_chunks_of_three(ctx, streams, oracle, monkeypatch):
    """Both calls once more with TIC_DBATCH_CHUNK=3 (test-hooks build): every chunk its own range and window - and no second run."""
    L = N.load()
    assert L.tic_build_has_test_hooks() == 1
    monkeypatch.setenv("TIC_DBATCH_CHUNK", "3")
    run_batch(L, ctx.handle, every_frame(), streams, oracle, "every frame, chunks of 3", 3)
    jobs = small_window()
    run_batch(L, ctx.handle, jobs, streams, oracle, "small window, chunks of 3", 3)
    # here spikes_sparse shares its chunk with frames whose rule is 288 as well: the chunk runs at 288, and it is decoded behind the batch
    assert ("spikes_sparse", plain_key("spikes_sparse")) in expected_singles(jobs, 3)[0]
    assert ("spikes_sparse", plain_key("spikes_sparse")) not in expected_singles(every_frame(), 3)[0]


def test_batch_one_payload_eight_headers(ctx, streams, oracle):
    """The eight plain variants of the pairs payload in one call: the same bits under eight sets of constants."""
    jobs = [("pairs", "q%d" % q) for q in DS.VALUE_QUALITIES]
    run_batch(N.load(), ctx.handle, jobs, streams, oracle, "pairs, eight qualities")


# ---- tic_decompress_dev and its asynchronous form ----------------------------------------------------------------------------------------
class Surface:
    """A stream buffer and a pixel buffer in device memory; rows `stride` apart, 0xCD everywhere the decoder must not write."""

    def __init__(self, ctx, L, max_stream, stride):
        self.ctx, self.L, self.stride = ctx, L, stride
        self.d_s, self.d_o = C.c_void_p(), C.c_void_p()
        self.bytes = DS.H * stride + TAIL
        ctx.check(L.tic_dev_alloc(ctx.handle, max_stream + 64, C.byref(self.d_s)))
        ctx.check(L.tic_dev_alloc(ctx.handle, self.bytes, C.byref(self.d_o)))

    def load(self, s):
        buf = np.frombuffer(s, np.uint8)
        self.ctx.check(self.L.tic_memcpy_h2d(self.ctx.handle, self.d_s, buf.ctypes.data, buf.size))
        self.ctx.check(self.L.tic_memset_dev(self.ctx.handle, self.d_o, 0xCD, self.bytes))
        return buf.size

    def pixels(self, what):
        host = np.empty(self.bytes, np.uint8)
        self.ctx.check(self.L.tic_memcpy_d2h(self.ctx.handle, host.ctypes.data, self.d_o, host.size))
        rows = host[: DS.H * self.stride].reshape(DS.H, self.stride)
        assert (rows[:, DS.W:] == 0xCD).all() and (host[DS.H * self.stride:] == 0xCD).all(), ("bytes outside the window were written", what)
        return np.ascontiguousarray(rows[:, :DS.W])

    def free(self):
        self.L.tic_dev_free(self.ctx.handle, self.d_s)
        self.L.tic_dev_free(self.ctx.handle, self.d_o)


@pytest.mark.parametrize("stride", [DS.W + 24, DS.W + 13])  # (a multiple of 8: the kernels store into the caller's buffer; not one: a strided copy)
def test_decompress_dev_keeps_its_window(stride, ctx, streams, oracle):
    """tic_decompress_dev of every frame, the variants in turn: rows `stride` apart, nothing outside 264 x 520 written, the path as on
    the default route."""
    L = N.load()
    assert (stride % 8 == 0) == (stride == DS.W + 24)
    sf = Surface(ctx, L, max(len(s) for s in streams.values()), stride)
    try:
        for i, name in enumerate(NAMES):
            keys = [DS.key(v) for v in FX[name]["variants"]]
            key = keys[i % len(keys)]
            n = sf.load(streams[name, key])
            hh, ww = C.c_int(), C.c_int()
            rc = L.tic_decompress_dev(ctx.handle, sf.d_s, n, sf.d_o, stride, DS.H * stride, C.byref(hh), C.byref(ww))
            assert rc == N.TIC_OK, (name, key, rc, L.tic_last_error(ctx.handle).decode())
            assert (hh.value, ww.value) == (DS.H, DS.W)
            check_path(name, L.tic_last_decode_path(ctx.handle), L.tic_last_decode_giveup(ctx.handle), "tic_decompress_dev")
            check_pixels(name, key, sf.pixels((name, key)), streams[name, key], oracle, "tic_decompress_dev, stride %d" % stride)
    finally:
        sf.free()


def test_decompress_dev_async_four_tickets(streams, oracle):
    """tic_decompress_dev_async with four tickets open: pairs, long_codes and the spikes frames on streams of their own, launched on the
    guess of their header where two equal headers came before.  Every ticket: the fixture's pixels inside its window, (1, 0)."""
    L = N.load()
    ctx2 = T.Context(0)
    # (a launch on the guess needs two equal headers in a row before it: runs of one header, so that four launched frames are in flight)
    jobs = [("pairs", "q50"), ("long_codes", "q50"), ("spikes_flat_one", "q50"), ("spikes_flat_two", "q50"), ("pairs", "q50"), ("long_codes", "q50"),
            ("spikes_sparse", "q50"), ("pairs", "q50"), ("pairs", "q99"), ("long_codes", "q99"), ("pairs", "q99"), ("long_codes", "q99"),
            ("pairs", "s0"), ("long_codes", "s0"), ("pairs", "s0"), ("pairs", "q5")]
    stride = DS.W + 24
    surfaces = [Surface(ctx2, L, len(streams[j]), stride) for j in jobs]
    try:
        def collect(k, ticket):
            hh, ww = C.c_int(), C.c_int()
            rc = L.tic_decompress_async_result(ctx2.handle, ticket, 1, C.byref(hh), C.byref(ww))
            assert rc == N.TIC_OK and (hh.value, ww.value) == (DS.H, DS.W), (jobs[k], rc, L.tic_last_error(ctx2.handle))
            print("ticket %d %s: path %d, giveup %d, guess %d" % (k, jobs[k], L.tic_last_decode_path(ctx2.handle), L.tic_last_decode_giveup(ctx2.handle),
                                                                 L.tic_last_decode_guess(ctx2.handle)))
            assert (L.tic_last_decode_path(ctx2.handle), L.tic_last_decode_giveup(ctx2.handle)) == (1, 0), jobs[k]
            held.append(L.tic_last_decode_guess(ctx2.handle) == 1)
            check_pixels(jobs[k][0], jobs[k][1], surfaces[k].pixels(jobs[k]), streams[jobs[k]], oracle, "tic_decompress_dev_async")

        open_tickets, held = [], []
        for k, j in enumerate(jobs):
            n = surfaces[k].load(streams[j])
            t = C.c_longlong(-1)
            ctx2.check(L.tic_decompress_dev_async(ctx2.handle, surfaces[k].d_s, n, surfaces[k].d_o, stride, DS.H * stride, C.byref(t)))
            open_tickets.append((k, t.value))
            if len(open_tickets) == 4:
                collect(*open_tickets.pop(0))
        while open_tickets:
            collect(*open_tickets.pop(0))
        # jobs 2 .. 5 come behind two equal headers and decode in one run at the range the rule gives: launched, and the launch stands
        assert all(held[2:6]), held
    finally:
        for sf in surfaces:
            sf.free()
        ctx2.close()


# ---- the library that ships ------------------------------------------------------------------------------------------------------------
def test_on_the_shipped_library():
    """The default route, the batch calls without a hook and the device-resident forms once more in a fresh process that loads the library
    that ships (TIC_TEST_HOOKS=0: no hooks compiled in)."""
    assert os.environ.get("TIC_TEST_HOOKS") == "1" and N.load().tic_build_has_test_hooks() == 1
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("TIC_")}
    env["TIC_TEST_HOOKS"] = "0"
    code = ("import sys; sys.path.insert(0, %r); import tinyimgcodec_amd._native as N; assert N.load().tic_build_has_test_hooks() == 0; "
            "import pytest; sys.exit(pytest.main([%r, '-m', 'gpu', '-q', '-x', '-p', 'no:cacheprovider', '-k', "
            "'test_default_route or test_batch_every or test_batch_small or test_batch_one or test_decompress_dev']))" % (root, os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=root)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, tail
