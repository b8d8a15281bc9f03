"""How the eight batch entry points that take a pointer and a row stride per frame read their input, on the MI355X: tic_compress_batch_v,
tic_compress_batch_scaled_v, tic_compress_batch_adaptive_v, tic_stream_sizes_v, tic_compress_batch_to_size, tic_rd_points_v,
tic_compress_batch_to_psnr and tic_rd_points_scaled_v on frames whose rows lie further apart than w, at odd addresses, as windows of one
picture, and in registered (pinned) memory - packed in the plan's order, scattered, partly registered, ragged rows that end with the
registration (tests/batch_inputs_common.py builds the memory; every byte that is no pixel is a poison, 0x00 in one run and 0xFF in the next).
Every expected value is pinned on the reference by something else than the call under test: oracle.compress / oracle.decompress of the frame,
the fixtures scaled_encode.npz / .json and adaptive_batch.json, and the replayed bisections of the rate tests.  For every call, layout and
poison: the results in the caller's order, the arena bit-identical behind the call, equal results for both poisons, the route
tic_last_batch_input_path reports for the three compress families, and the family's figures equal to those of dense frames.
What no test here can see: a staging copy that takes more than w bytes of a row.  No kernel reads a row's padding, so the bytes taken along
change no result; only a read outside mapped memory would show it, and the arenas are built so that there is none."""
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

import adaptive_batch_common as A
import batch_inputs_common as B
import mixed_batch_common as M
import rate_batch_common as R
import rd_batch_common as RD
from distortion_common import sums
from test_adaptive_batch_gpu import caps_of, streams_of
from test_distortion_gpu import bisect_psnr
from test_rate_control_gpu import bisect
from test_scaled_batch_gpu import SCall, SETTINGS
from test_scaled_batch_gpu import figures as scaled_figures
from test_scaled_batch_gpu import rd_figures as rd_scaled_figures

pytestmark = pytest.mark.gpu

POISONS = (0x00, 0xFF)
FAMILIES = ("v", "scaled", "adaptive", "sizes", "to_size", "rd", "to_psnr", "rd_scaled")
COMPRESS = ("v", "scaled", "adaptive")  # the families whose chunks go through upload_chunk_v
QS = (20, 50, 85)        # tic_stream_sizes_v, tic_rd_points_v
RANGE = (20, 60)         # the searches' quality range; budgets are the sizes at 50, bounds the errors at 40 (Data.budget, Data.bound)
SCALED_QS = (3, 0, 2, 1)  # tic_rd_points_scaled_v's settings

# (layout, variant, TIC_BATCH_CHUNK).  Chunks of three: several chunks, every slot used again, a later and smaller frame's padding where an
# earlier chunk's pixels lay in the slot's pinned buffer.  ragged_at_256 in chunks of one: the frame that crosses the registration's end has
# a chunk of its own.
CASES = [("dense", 0, None), ("wide_odd", 0, None), ("wide_odd", 0, "3"), ("wide_8", 0, None), ("mosaic", 0, None), ("mosaic", 1, None),
         ("packed_in_plan_order", 0, None), ("packed_in_plan_order", 0, "3"), ("packed_reversed_with_gaps", 0, None), ("registered_wide", 0, None),
         ("half_registered", 0, None), ("half_registered", 0, "3"), ("half_registered", 1, "3"), ("ragged_at_256", 0, None), ("ragged_at_256", 0, "1")]


def expected_path(layout, variant, chunk, nb):
    """(direct, staged) of tic_last_batch_input_path for nb frames that go through the batch, by upload_chunk_v's rule: a chunk is copied from
    where it lies when EVERY frame of it is registered from its first byte to the last of its staged image and its rows are the staged pitch
    apart; else all of the chunk is staged.  Frames without blocks and single frames count in neither."""
    return {
        ("dense", None): (0, nb), ("wide_odd", None): (0, nb), ("wide_odd", "3"): (0, nb), ("wide_8", None): (0, nb), ("mosaic", None): (0, nb),
        ("packed_in_plan_order", None): (nb, 0), ("packed_in_plan_order", "3"): (nb, 0), ("packed_reversed_with_gaps", None): (nb, 0),
        ("registered_wide", None): (0, nb),      # registered, but rows 24 bytes further apart than the staged pitch
        ("half_registered", None): (0, nb),      # one chunk, and it holds frames outside the registration
        # chunks of three, the registration ends at plan position 4 - between positions 3 and 4 (variant 0) or inside the frame at position 4
        # (variant 1: its first byte is registered, its last is not): the first chunk (positions 0..2) is direct, the second holds position 4
        # and is staged as a whole, position 3 with it; everything behind is unregistered
        ("half_registered", "3"): (3, nb - 3),
        ("ragged_at_256", None): (0, nb),        # one chunk, and it holds the frame that crosses the registration's end
        ("ragged_at_256", "1"): (nb - 1, 1),     # the frame whose last row's padding ends WITH the registration is direct, the one 16 bytes on is not
    }[(layout, chunk)]


def sha(b):
    return hashlib.sha256(b).hexdigest()


class PerQuality:
    """A value per quality, computed when asked for; indexed q - 1, as the recorded tables the bisections replay are."""

    def __init__(self, fn):
        self.fn, self.cache = fn, {}

    def __getitem__(self, i):
        if i not in self.cache:
            self.cache[i] = self.fn(i + 1)
        return self.cache[i]


def input_path(ctx):
    d, s = C.c_int(-1), C.c_int(-1)
    ctx.check(N.load().tic_last_batch_input_path(ctx.handle, C.byref(d), C.byref(s)))
    return d.value, s.value


class Registered:
    """The arena's range registered around a call; unregistered whatever happens, and then registered once more: nothing was left pinned."""

    def __init__(self, ctx, arena):
        self.ctx, self.range = ctx, arena.register_range()

    def __enter__(self):
        if self.range:
            self.ctx.check(N.load().tic_host_register(self.ctx.handle, *self.range))

    def __exit__(self, *exc):
        if self.range:
            L = N.load()
            self.ctx.check(L.tic_host_unregister(self.ctx.handle, self.range[0]))
            self.ctx.check(L.tic_host_register(self.ctx.handle, *self.range))
            self.ctx.check(L.tic_host_unregister(self.ctx.handle, self.range[0]))


class FrameSet:
    """frames and the qualities (settings) that order them in the plan; ragged: (indices, last, cross) for ragged_at_256 or None."""

    def __init__(self, frames, quals, ragged=None):
        self.frames, self.quals, self.ragged = frames, quals, ragged
        self.all = list(range(len(frames)))

    def nb(self, idx):
        return sum(1 for i in idx if self.frames[i].size)


class Data:
    """The frame sets and everything expected of them, computed once."""

    def __init__(self, oracle):
        self.oracle = oracle
        small, _ = M.small_frames()
        rng = np.random.default_rng(20261020)
        noise = lambda h, w: rng.integers(0, 256, (h, w), dtype=np.uint8)
        # one block; a block row of nine; three one-block rows; 16 x 40 and 32 x 40 of one quality (one transform run); a last strip of 7 blocks;
        # 13 x 21 and 5 x 3 (ragged both ways, pitch 256); 0 x 16 with a null pointer; five of mixed_batch_common's; the fixture's largest size
        frames = [noise(8, 8), noise(8, 72), noise(24, 8), noise(16, 40), noise(13, 21), np.zeros((0, 16), np.uint8), noise(32, 40), noise(16, 120),
                  noise(5, 3), small[0], small[2], small[3], small[4], small[10], noise(64, 96)]
        quals = [50, 20, 85, 35, 60, 45, 35, 10, 90, 55, 70, 25, 65, 65, 30]
        assert [f.shape for f in frames[9:14]] == [(1, 1), (7, 9), (15, 17), (40, 52), (24, 52)]
        ragged = [i for i, f in enumerate(frames) if f.shape[1] % 8 != 0 or f.size == 0]
        self.float = FrameSet(frames, quals, (ragged, ragged.index(8), ragged.index(4)))
        self.streams = [oracle.compress(f, q) for f, q in zip(frames, quals)]
        self.sizes = [PerQuality(lambda q, f=f: len(oracle.compress(f, q))) for f in frames]
        self.sums = [PerQuality(lambda q, f=f: sums(f, oracle.decompress(oracle.compress(f, q)))) for f in frames]
        self.at = {}  # (frame, quality) -> the oracle's stream

        with open(os.path.join(GOLDEN, "scaled_encode.json")) as f:
            self.man = json.load(f)["cases"]
        self.npz = np.load(os.path.join(GOLDEN, "scaled_encode.npz"))
        keys = ["noise16x24_med", "noise64x96_best", "ramp48x48_low", "highfreq8x16_high", "flat8x8_med", "aligned_best_best", "empty0x0_med",
                "aligned_high_high", "aligned_med_med", "aligned_low_low", "noise16x24_low", "ramp48x48_best"]
        self.scaled_keys = keys
        self.scaled = FrameSet([self.npz[k + "_img"] for k in keys], [SETTINGS.index(self.man[k]["setting"]) for k in keys])
        names = ["noise16x24", "noise64x96", "empty0x0", "ramp48x48", "highfreq8x16", "flat8x8"]
        self.rd_scaled_names = names
        self.rd_scaled = FrameSet([self.npz[k + "_best_img"] for k in names], [0] * len(names))

        self.entries, aframes, aquals = A.load_fixture()
        aragged = [i for i, f in enumerate(aframes) if f.shape[1] % 8 != 0]
        assert [aframes[i].shape for i in aragged] == [(1, 1), (13, 21), (7, 4100)]
        self.adaptive = FrameSet(aframes, aquals, (aragged, 0, 1))

    def stream_at(self, i, q):
        if (i, q) not in self.at:
            self.at[(i, q)] = self.oracle.compress(self.float.frames[i], q)
        return self.at[(i, q)]

    def budget(self, i):
        """tic_compress_batch_to_size's budget of frame i: its size at q = 50 (and no less than at the range's lower end: every frame fits)."""
        return max(self.sizes[i][49], self.sizes[i][RANGE[0] - 1])

    def bound(self, i):
        """tic_compress_batch_to_psnr's bound of frame i: its error at q = 40 (and no less than at the range's upper end: every frame meets it)."""
        return max(self.sums[i][39][0], self.sums[i][RANGE[1] - 1][0])

    def frame_set(self, family):
        return {"scaled": self.scaled, "rd_scaled": self.rd_scaled, "adaptive": self.adaptive}.get(family, self.float)


def run(family, ctx, data, idx, inputs):
    """One call of `family` on the frames idx of its set, read through `inputs` -> (what it returned, in a form two runs can be compared by;
    the family's figures).  Sentinels behind every stream are checked here."""
    L, S = N.load(), data.frame_set(family)
    frames, quals = [S.frames[i] for i in idx], [S.quals[i] for i in idx]
    if family == "v":
        call = M.VCall(ctx, frames, quals, inputs=inputs)
        got = call.streams()
        assert all((call.outs[k][len(s):] == 0xAB).all() for k, s in enumerate(got))
        return got, M.figures(ctx)
    if family == "scaled":
        return SCall(ctx, frames, quals, inputs=inputs).streams(), scaled_figures(ctx)
    if family == "adaptive":
        return streams_of(A.ACall(ctx, frames, quals, caps_of(frames), inputs=inputs)), A.figures(ctx)
    if family == "sizes":
        rc, sizes = R.sizes_v(L, ctx.handle, frames, QS, inputs=inputs)
        assert rc == N.TIC_OK, L.tic_last_error(ctx.handle)
        return sizes.tolist(), R.figures(L, ctx.handle)
    if family in ("rd", "rd_scaled"):
        rc, sizes, sse, wrapped = RD.rd_v(L, ctx.handle, frames, SCALED_QS if family == "rd_scaled" else QS, inputs=inputs, scaled=family == "rd_scaled")
        assert rc == N.TIC_OK, L.tic_last_error(ctx.handle)
        fig = rd_scaled_figures(ctx) if family == "rd_scaled" else R.figures(L, ctx.handle) + (RD.sse_launches(L, ctx.handle),)
        return (sizes.tolist(), sse.tolist(), wrapped.tolist()), fig
    if family == "to_size":
        call = R.SearchCall(L, ctx.handle, frames, [data.budget(i) for i in idx], *RANGE, inputs=inputs)
        assert call.run() == N.TIC_OK, L.tic_last_error(ctx.handle)
        assert all(call.tail_intact(k) for k in range(len(idx)))
        return [(call.status[k], call.quals[k], call.stream(k)) for k in range(len(idx))], R.figures(L, ctx.handle)
    assert family == "to_psnr"
    call = RD.PsnrCall(L, ctx.handle, frames, [data.bound(i) for i in idx], *RANGE, inputs=inputs)
    assert call.run() == N.TIC_OK, L.tic_last_error(ctx.handle)
    assert all(call.tail_intact(k) for k in range(len(idx)))
    return [(call.status[k], call.quals[k], call.sse[k], call.stream(k)) for k in range(len(idx))], R.figures(L, ctx.handle) + (RD.sse_launches(L, ctx.handle),)


def check(family, data, idx, got):
    """`got` of run() against what is pinned on the reference, frame by frame in the caller's order."""
    if family == "v":
        assert got == [data.streams[i] for i in idx]
    elif family == "scaled":
        for k, i in enumerate(idx):
            key = data.scaled_keys[i]
            assert len(got[k]) == data.man[key]["bytes"] and sha(got[k]) == data.man[key]["sha256"] and got[k] == data.npz[key + "_bs"].tobytes(), key
    elif family == "adaptive":
        for k, i in enumerate(idx):
            A.check_stream(got[k], data.entries[i])
    elif family == "sizes":
        assert got == [[data.sizes[i][q - 1] for q in QS] for i in idx]
    elif family == "rd":
        assert got[0] == [[data.sizes[i][q - 1] for q in QS] for i in idx]
        assert got[1] == [[data.sums[i][q - 1][0] for q in QS] for i in idx] and got[2] == [[data.sums[i][q - 1][1] for q in QS] for i in idx]
    elif family == "rd_scaled":
        for k, i in enumerate(idx):
            name = data.rd_scaled_names[i]
            img = data.rd_scaled.frames[i]
            for j, qf in enumerate(SCALED_QS):
                key = "%s_%s" % (name, SETTINGS[qf])
                want = sums(img, data.oracle.decompress(data.npz[key + "_bs"].tobytes()))  # int64 numpy; the wrapped sum as the reference's tests/psnr.py forms it
                assert (got[0][k][j], got[1][k][j], got[2][k][j]) == (data.man[key]["bytes"],) + want, key
    elif family == "to_size":
        for k, i in enumerate(idx):
            q = bisect(data.sizes[i], data.budget(i), *RANGE)
            assert got[k] == (N.TIC_OK, q, data.stream_at(i, q)) and len(got[k][2]) <= data.budget(i), (k, i)
    else:
        for k, i in enumerate(idx):
            sse = PerQuality(lambda q, i=i: data.sums[i][q - 1][0])
            q = bisect_psnr(sse, data.bound(i), *RANGE)
            assert got[k] == (N.TIC_OK, q, data.sums[i][q - 1][0], data.stream_at(i, q)), (k, i)


def run_on_arena(family, ctx, data, idx, arena):
    """run() on an arena: registered around the call where the layout says so, bit-identical behind it -> (got, figures, (direct, staged))."""
    before = arena.raw.copy()
    with Registered(ctx, arena):
        got, fig = run(family, ctx, data, idx, arena.inputs())
        path = input_path(ctx)
    assert np.array_equal(arena.raw, before), "the call wrote to its input"
    return got, fig, path


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(0)
    assert c.arch.startswith("gfx950"), c.arch
    yield c
    c.close()


@pytest.fixture(scope="module")
def data(oracle):
    return Data(oracle)


@pytest.mark.parametrize("family", FAMILIES)
def test_every_layout(ctx, data, monkeypatch, family):
    """Every layout that applies to the call (ragged_at_256: the float families, on their frames with w % 8 != 0), each with both poisons,
    mosaic with two arrangements of the windows as well."""
    assert N.load().tic_build_has_test_hooks() == 1
    S = data.frame_set(family)
    dense_fig, mosaic = {}, []
    for layout, variant, chunk in CASES:
        if layout == "ragged_at_256" and S.ragged is None:
            continue
        idx, last, cross = S.ragged if layout == "ragged_at_256" else (S.all, None, None)
        frames, quals = [S.frames[i] for i in idx], [S.quals[i] for i in idx]
        if chunk:
            monkeypatch.setenv("TIC_BATCH_CHUNK", chunk)
        else:
            monkeypatch.delenv("TIC_BATCH_CHUNK", raising=False)
        if (tuple(idx), chunk) not in dense_fig:  # the figures' reference values: dense frames, same chunking
            got, fig, _ = run_on_arena(family, ctx, data, idx, B.build(frames, "dense", 0x5A, quals))
            check(family, data, idx, got)
            dense_fig[(tuple(idx), chunk)] = fig
        runs = []
        for poison in POISONS:
            arena = B.build(frames, layout, poison, quals, variant=variant, last=last, cross=cross)
            got, fig, path = run_on_arena(family, ctx, data, idx, arena)
            where = (family, layout, variant, chunk, poison)
            check(family, data, idx, got)
            assert fig == dense_fig[(tuple(idx), chunk)], where
            if family in COMPRESS:
                assert path == expected_path(layout, variant, chunk, S.nb(idx)), where
            elif family in ("to_size", "to_psnr") and chunk is None:
                # (the streams come from tic_compress_batch_v on the same pointers: every frame gets one here)
                assert path == ((S.nb(idx), 0) if layout.startswith("packed_") else (0, S.nb(idx))), where
            runs.append(got)
        assert runs[0] == runs[1], (family, layout, variant, chunk)
        if layout == "mosaic":
            mosaic += runs
    assert all(m == mosaic[0] for m in mosaic) and len(mosaic) == 4  # two poisons below the short windows, two sets of neighbours


@pytest.mark.parametrize("family", ["v", "scaled", "sizes", "rd", "rd_scaled"])
def test_single_frame_behind_the_batch(ctx, data, monkeypatch, family):
    """With the chunk's byte budget lowered, one frame held wide_odd goes through the one-by-one call behind the batch, which is handed its
    row stride: 128 x 128 under 8 KiB for the float calls; for the integer encoder's calls the largest fixture frame below Lenna, 64 x 96
    under 4 KiB (the expected bytes of a scaled stream come from the fixture alone)."""
    oracle = data.oracle
    if family in ("scaled", "rd_scaled"):
        budget = 4 << 10
        names = ["noise16x24", "noise64x96", "flat8x8"]
        sets = [2, 1, 3]
        frames = [data.npz["%s_%s_img" % (n, SETTINGS[s])] for n, s in zip(names, sets)]
    else:
        budget = 8 << 10
        frames = [data.float.frames[0], np.random.default_rng(128).integers(0, 256, (128, 128), dtype=np.uint8), data.float.frames[3]]
        quals = [50, 40, 35]
    monkeypatch.setenv("TIC_BATCH_CHUNK_BYTES", str(budget))
    L = N.load()
    runs = []
    for poison in POISONS:
        arena = B.build(frames, "wide_odd", poison)
        before = arena.raw.copy()
        inputs = arena.inputs()
        if family == "v":
            got = M.VCall(ctx, frames, quals, inputs=inputs).streams()
            assert got == [oracle.compress(f, q) for f, q in zip(frames, quals)]
            fig = M.figures(ctx)
        elif family == "scaled":
            got = SCall(ctx, frames, sets, inputs=inputs).streams()
            assert got == [data.npz["%s_%s_bs" % (n, SETTINGS[s])].tobytes() for n, s in zip(names, sets)]
            fig = scaled_figures(ctx)
        elif family == "sizes":
            rc, sizes = R.sizes_v(L, ctx.handle, frames, QS[:2], inputs=inputs)
            assert rc == N.TIC_OK
            got = sizes.tolist()
            assert got == [[len(oracle.compress(f, q)) for q in QS[:2]] for f in frames]
            fig = R.figures(L, ctx.handle)
        elif family == "rd":
            rc, sizes, sse, wrapped = RD.rd_v(L, ctx.handle, frames, QS[:2], inputs=inputs)
            assert rc == N.TIC_OK
            got = (sizes.tolist(), sse.tolist(), wrapped.tolist())
            want = [[sums(f, oracle.decompress(oracle.compress(f, q))) for q in QS[:2]] for f in frames]
            assert got[0] == [[len(oracle.compress(f, q)) for q in QS[:2]] for f in frames]
            assert got[1] == [[s[0] for s in row] for row in want] and got[2] == [[s[1] for s in row] for row in want]
            fig = R.figures(L, ctx.handle)
        else:
            rc, sizes, sse, wrapped = RD.rd_v(L, ctx.handle, frames, SCALED_QS, inputs=inputs, scaled=True)
            assert rc == N.TIC_OK
            got = (sizes.tolist(), sse.tolist(), wrapped.tolist())
            for k, n in enumerate(names):
                for j, qf in enumerate(SCALED_QS):
                    key = "%s_%s" % (n, SETTINGS[qf])
                    want = sums(frames[k], oracle.decompress(data.npz[key + "_bs"].tobytes()))
                    assert (got[0][k][j], got[1][k][j], got[2][k][j]) == (data.man[key]["bytes"],) + want, key
            fig = rd_scaled_figures(ctx)
        assert fig[:2] == (2, 1), (family, fig)
        assert np.array_equal(arena.raw, before)
        runs.append(got)
    assert runs[0] == runs[1]


@pytest.mark.parametrize("family", COMPRESS)
def test_neighbours_in_memory_and_neighbours_in_the_plan(ctx, data, family):
    """Registered frames packed in the plan order of OTHER qualities than the call's: frames that follow each other in memory without being
    neighbours in the call's plan, and neighbours in the plan that lie apart in memory.  Every frame is pinned and dense, so every chunk is
    copied from where it lies, stretch by stretch; a merged copy that trusts the plan alone or the addresses alone lands a frame's pixels
    in another frame's place.  tic_compress_batch_v also on overlapping row windows of one strip: the third window starts where the second
    would end if it were as long as the first - a stretch that grows by a frame's own length instead of the stretch's would take it in."""
    S = data.frame_set(family)
    n = len(S.all)
    for laid in ([S.quals[(i + 1) % n] for i in range(n)], [-q for q in S.quals], [0] * n):  # rotated, reversed, the caller's order by size
        mem = B.plan_order([f.shape for f in S.frames], laid)
        plan = B.plan_order([f.shape for f in S.frames], S.quals)
        follows = lambda order: {(a, b) for a, b in zip(order, order[1:])}
        assert follows(mem) - follows(plan) and follows(plan) - follows(mem)
        runs = []
        for poison in POISONS:
            got, fig, path = run_on_arena(family, ctx, data, S.all, B.build(S.frames, "packed_in_plan_order", poison, laid))
            check(family, data, S.all, got)
            assert path == (S.nb(S.all), 0), (family, path)
            runs.append(got)
        assert runs[0] == runs[1]
    if family == "v":
        pic = np.random.default_rng(40).integers(0, 256, (48, 40), dtype=np.uint8)
        windows, quals = [(0, 16), (16, 32), (32, 16)], [30, 40, 50]
        for poison in POISONS:
            arena = B.crops_of_a_strip(pic, windows, poison)
            before = arena.raw.copy()
            with Registered(ctx, arena):
                got = M.VCall(ctx, arena.frames, quals, inputs=arena.inputs()).streams()
                assert input_path(ctx) == (3, 0)
            assert got == [data.oracle.compress(pic[r: r + m], q) for (r, m), q in zip(windows, quals)]
            assert np.array_equal(arena.raw, before)


def test_route_figures_of_a_call_that_runs_twice(ctx, oracle):
    """With the lane-per-block packing kernel allowed up to q = 99, mixed_batch_common's set (noise at q = 90 and 99 does not fit that kernel's
    strings) makes tic_compress_batch_v lower the bound and run its chunks again: every frame is uploaded twice, and tic_last_batch_input_path
    still counts each frame once - staged when the frames are pageable and held wide_odd, direct when they are registered and packed.  The
    second call of each pair runs once (the bound stays lowered) and reports the same."""
    L = N.load()
    frames, quals = M.small_frames()
    want = [oracle.compress(f, q) for f, q in zip(frames, quals)]
    try:
        for layout, path in (("wide_odd", (0, len(frames))), ("packed_in_plan_order", (len(frames), 0))):
            arena = B.build(frames, layout, 0xFF, quals)
            before = arena.raw.copy()
            with Registered(ctx, arena):
                ctx.check(L.tic_set_entropy_lane_kernel(ctx.handle, 99))
                for rep in range(2):
                    assert M.VCall(ctx, frames, quals, inputs=arena.inputs()).streams() == want, (layout, rep)
                    assert input_path(ctx) == path and M.figures(ctx)[:2] == (len(frames), 0), (layout, rep, input_path(ctx))
            assert np.array_equal(arena.raw, before)
    finally:
        ctx.check(L.tic_set_entropy_lane_kernel(ctx.handle, 0))


def test_strided_and_registered_frames_on_the_shipped_library(data, tmp_path):
    """wide_odd and registered packed_in_plan_order through tic_compress_batch_v and tic_compress_batch_scaled_v in a fresh process that loads
    the library that ships (no test hooks, no TIC_* variable); the expected digests are handed in."""
    doc = {"v": {"quals": data.float.quals, "sha256": [sha(s) for s in data.streams]},
           "scaled": {"quals": data.scaled.quals, "sha256": [data.man[k]["sha256"] for k in data.scaled_keys]}}
    np.savez(tmp_path / "frames.npz", **{"v%d" % i: f for i, f in enumerate(data.float.frames)}, **{"scaled%d" % i: f for i, f in enumerate(data.scaled.frames)})
    with open(tmp_path / "want.json", "w") as f:
        json.dump(doc, f)
    code = r'''
import ctypes as C, hashlib, json, os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
import tinyimgcodec_amd as T
from tinyimgcodec_amd import _native as N
L = N.load()
assert L.tic_build_has_test_hooks() == 0 and N._lib_path() == N.LIB_PATH
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import batch_inputs_common as B
import mixed_batch_common as M
from test_scaled_batch_gpu import SCall
assert N.load() is L and L.tic_build_has_test_hooks() == 0
z = np.load(sys.argv[1])
want = json.load(open(sys.argv[2]))
ctx = T.Context(0)
for family in ("v", "scaled"):
    quals = want[family]["quals"]
    frames = [z["%s%d" % (family, i)] for i in range(len(quals))]
    nb = sum(1 for f in frames if f.size)
    for layout, path in (("wide_odd", (0, nb)), ("packed_in_plan_order", (nb, 0))):
        for poison in (0x00, 0xFF):
            arena = B.build(frames, layout, poison, quals)
            before = arena.raw.copy()
            reg = arena.register_range()
            if reg:
                ctx.check(L.tic_host_register(ctx.handle, *reg))
            try:
                call = (M.VCall if family == "v" else SCall)(ctx, frames, quals, inputs=arena.inputs())
                got = call.streams()
                d, s = C.c_int(-1), C.c_int(-1)
                ctx.check(L.tic_last_batch_input_path(ctx.handle, C.byref(d), C.byref(s)))
            finally:
                if reg:
                    ctx.check(L.tic_host_unregister(ctx.handle, reg[0]))
            assert [hashlib.sha256(b).hexdigest() for b in got] == want[family]["sha256"], (family, layout, poison)
            assert (d.value, s.value) == path, (family, layout, d.value, s.value)
            assert np.array_equal(arena.raw, before)
ctx.close()
print("strided and registered frames on the shipped library ok")
'''
    env = {k: v for k, v in os.environ.items() if not k.startswith("TIC_")}
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "frames.npz"), str(tmp_path / "want.json")], capture_output=True, text=True, timeout=300,
                       env=env, cwd=ROOT)
    assert r.returncode == 0 and "strided and registered frames on the shipped library ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
